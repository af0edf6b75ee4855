"""CPU tests of the boundary: the C-ABI library loads and exports every symbol
include/gpusort.h declares; host-only entry points behave; no compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared, "ctypes binding and header disagree"


def test_library_exports_nothing_the_header_does_not_declare():
    """The boundary is exactly include/gpusort.h: no stray gs_* entry points in the dynamic symbol table."""
    import shutil
    import subprocess
    from gpusorting_amd import _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        import pytest
        pytest.skip("no nm on this box")
    exported = sorted({ln.split()[-1] for ln in out.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("gs_")})
    assert exported == _declared_symbols()


def test_library_reads_no_environment():
    """SURVEY 5.6 / VERDICT r3 item 8: configuration is gs_onesweep_options / gs_mgpu_options, not GPUSORT_* variables read
    inside the library.  getenv must not even be imported by the product library; the Python harness translates the
    environment (tests, tools/) into the options structs."""
    import shutil
    import subprocess
    from gpusorting_amd import _lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("no nm on this box")
    assert "getenv" not in out.stdout
    csrc = os.path.join(ROOT, "gpusorting_amd", "csrc")
    sources = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")))
    assert "gpusort_capi.hip" in sources and len(sources) >= 6
    for f in sources:
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_options_structs_match_the_header_defaults(monkeypatch):
    from gpusorting_amd import _lib
    lib = _lib.load()
    o = _lib.OneSweepOptions()
    lib.gs_onesweep_options_default(C.byref(o))
    assert o.struct_size == C.sizeof(_lib.OneSweepOptions)
    assert (o.rank_mode, o.small_path, o.mid_path, o.skip_passes, o.position_chains, o.position_chains_min_log2, o.key64_sweeps,
            o.plan, o.first_pass_big, o.hist_blocks, o.debug_flags) == (-1, 1, 1, 1, 1, 25, 1, 0, 1, 0, 0)
    m = _lib.MgpuOptions()
    lib.gs_mgpu_options_default(C.byref(m))
    assert m.struct_size == C.sizeof(_lib.MgpuOptions) and (m.force_exchange, m.overlap, m.alltoallv, m.by_bin) == (0, 1, 0, 1)
    # the harness' translation of the environment
    monkeypatch.setenv("GPUSORT_MID_PATH", "0")
    monkeypatch.setenv("GPUSORT_POS", "2")
    monkeypatch.setenv("GPUSORT_SHAPE", "512x16")
    e = _lib.onesweep_options_from_env(plan=1)
    assert (e.mid_path, e.position_chains, e.shape_threads, e.shape_keys_per_thread, e.plan) == (0, 2, 512, 16, 1)
    h = C.c_void_p()
    bad = _lib.OneSweepOptions()
    lib.gs_onesweep_options_default(C.byref(bad))
    bad.struct_size = 12
    assert lib.gs_onesweep_create_ex(C.byref(h), 1024, 0, 0, C.byref(bad)) == _lib.GS_ERR_ARG
    lib.gs_onesweep_options_default(C.byref(bad))
    bad.position_chains = 7
    assert lib.gs_onesweep_create_ex(C.byref(h), 1024, 0, 0, C.byref(bad)) == _lib.GS_ERR_ARG
    lib.gs_onesweep_options_default(C.byref(bad))
    bad.shape_threads, bad.shape_keys_per_thread = 333, 7
    assert lib.gs_onesweep_create_ex(C.byref(h), 1024, 0, 0, C.byref(bad)) == _lib.GS_ERR_ARG


def test_version_and_status_strings():
    from gpusorting_amd import _lib
    lib = _lib.load()
    assert b"gfx950" in lib.gs_version()
    assert lib.gs_status_string(0) == b"ok"
    assert b"timeout" in lib.gs_status_string(_lib.GS_ERR_TIMEOUT)


def test_argument_errors_without_touching_the_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gs_onesweep_create(None, 1024, 0, 0) == _lib.GS_ERR_ARG
    assert lib.gs_onesweep_create(C.byref(h), 0, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_onesweep_create(C.byref(h), 1 << 30, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_onesweep_create(C.byref(h), 1024, 0, 4) == _lib.GS_ERR_MODE   # keys-only with values
    assert lib.gs_onesweep_create(C.byref(h), 1024, 1, 2) == _lib.GS_ERR_MODE   # 2-byte values
    assert lib.gs_onesweep_sort_keys(None, None, None, 4, 0, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_onesweep_destroy(None) == _lib.GS_ERR_ARG
    assert lib.gs_onesweep_temp_bytes(1 << 28) > 0
    assert lib.gs_onesweep_partition_size(0, 0) % 64 == 0


def test_null_handle_is_an_argument_error_in_every_handle_entry():
    """A null handle is refused with GS_ERR_ARG before anything else is looked at (every other argument is plausible)."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint32 * 4096)()
    p, u32p = C.addressof(buf), C.cast(buf, C.POINTER(C.c_uint32))
    calls = {
        "gs_onesweep_global_histogram": (None, p, 1024, 0, u32p, None),
        "gs_onesweep_scan": (None, p, 1024, 0, u32p, None),
        "gs_onesweep_digit_pass": (None, p, p, None, None, 1024, 0, 0, 0, None),
        "gs_onesweep_msd_prepare": (None, p, 1024, 0, u32p, None),
        "gs_onesweep_msd_partition": (None, p, p, None, None, 1024, None),
        "gs_onesweep_msd_fine_histogram": (None, p, 1024, 0, u32p, None),
        "gs_onesweep_last_plan": (None, u32p, u32p, None),
        "gs_onesweep_set_plan": (None, 1),
        "gs_segsort_sort_keys": (None, p, p, 1024, p, 1, 0, 0, 0, None),
        "gs_segsort_check": (None, None),
        "gs_segsort_last_classes": (None, u32p, 4096, None),
        "gs_topk_select_keys": (None, p, 1024, 8, p + 8192, 0, 0, None),
        "gs_topk_check": (None, None),
        "gs_topk_last": (None, u32p, 4096, None),
        "gs_debug_sort_route": (None, 1024, 0, u32p),
        "gs_debug_set_hy_class": (None, 0),
        "gs_debug_set_pos_grid": (None, 0),
        "gs_debug_pass_flags": (None, u32p, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == _lib.GS_ERR_ARG, name
    # the entries that hand out a borrowed engine answer NULL, as gs_mgpu_sorter does
    for name in ("gs_segsort_engine", "gs_topk_engine", "gs_mgpu_sorter"):
        assert getattr(lib, name)(None) is None, name


def test_msd_splitters_match_oracle(oracle):
    from gpusorting_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    for world in (1, 2, 3, 4, 8):
        for hist in (np.full(256, 12345, dtype=np.uint64), rng.integers(0, 10**6, 256).astype(np.uint64),
                     np.concatenate([np.full(8, 10**7), np.zeros(248)]).astype(np.uint64)):
            fb = (C.c_uint32 * (world + 1))()
            st = lib.gs_msd_splitters(hist.ctypes.data_as(C.POINTER(C.c_uint64)), world, fb)
            assert st == 0
            assert list(fb) == oracle.msd_splitters(hist, world).tolist()
    assert lib.gs_msd_splitters(None, 2, None) == _lib.GS_ERR_ARG


def test_product_does_not_import_the_oracle():
    """The product path must never route through oracle/ (prompt rule 3)."""
    pkg = os.path.join(ROOT, "gpusorting_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "gs_oracle" not in src and "oracle_lib" not in src and "gso_" not in src, f
    for f in os.listdir(os.path.join(ROOT, "include")):
        p = os.path.join(ROOT, "include", f)
        if os.path.isfile(p):
            assert "gso_" not in open(p).read()


def _numpy_plan(table, rank, capacity):
    """Independent restatement of the exchange plan: equal-count splitters at bin granularity
    (first bin whose exclusive prefix reaches ceil(r * total / world)), then [source, destination] counts."""
    world, nbins = table.shape
    g = table.astype(np.uint64).sum(axis=0)
    excl = np.concatenate([[0], np.cumsum(g)[:-1]]).astype(np.uint64)
    total = int(g.sum())
    first = [0]
    for r in range(1, world):
        target = (total * r + world - 1) // world
        first.append(int(np.count_nonzero(excl < target)))
    first.append(nbins)
    csum = np.concatenate([np.zeros((world, 1), np.int64), np.cumsum(table.astype(np.int64), axis=1)], axis=1)
    per = csum[:, first[1:]] - csum[:, first[:-1]]          # [source, destination]
    return {"send": per[rank].tolist(), "recv": per[:, rank].tolist(), "n_recv": int(per[:, rank].sum()),
            "max_bucket": int(per.sum(axis=0).max()), "overflow": bool(per.sum(axis=0).max() > capacity), "first_bin": first}


def _tables(rng):
    for world, nbins in ((1, 256), (2, 256), (3, 256), (8, 256), (8, 4096), (5, 4096), (256, 256)):
        t = rng.integers(0, 5000, size=(world, nbins), dtype=np.uint32)
        yield t
        t2 = t.copy()
        t2[:, rng.integers(0, nbins)] += 3_000_000          # one heavy bin
        yield t2
        t3 = np.zeros_like(t)
        t3[0, nbins - 1] = 7                                 # almost empty
        yield t3
        yield np.zeros_like(t)                               # empty


def test_msd_plan_host_function():
    """gs_msd_plan (host twin of the device plan kernel of the multi-GPU split) against a numpy restatement."""
    from gpusorting_amd.sharded import msd_plan
    rng = np.random.default_rng(5)
    for t in _tables(rng):
        world = t.shape[0]
        for rank in sorted({0, world - 1, world // 2}):
            cap = int(t.sum() // world * 1.2) + 1
            got, ref = msd_plan(t, rank, cap), _numpy_plan(t, rank, cap)
            assert got["send"] == ref["send"] and got["recv"] == ref["recv"], (t.shape, rank)
            assert got["n_recv"] == ref["n_recv"] and got["max_bucket"] == ref["max_bucket"] and got["overflow"] == ref["overflow"]
            assert got["first_bin"].tolist() == ref["first_bin"]


@pytest.mark.gpu
def test_msd_plan_device_kernel_equals_host(gpu):
    """The device plan kernel (splitters + counts + overflow from the gathered histograms, no host round trip
    besides the final counts) gives the host function's plan word for word."""
    import ctypes as C
    from gpusorting_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(6)
    for t in _tables(rng):
        world, nbins = t.shape
        t = np.ascontiguousarray(t)
        for rank in sorted({0, world - 1, world // 2}):
            cap = int(t.sum() // world * 1.2) + 1
            words = 4 + 3 * world + 1
            host, dev = np.zeros(words, np.uint32), np.zeros(words, np.uint32)
            p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
            assert lib.gs_msd_plan(p(t), nbins, world, rank, cap, p(host)) == 0
            assert lib.gs_debug_msd_plan_device(p(t), nbins, world, rank, cap, p(dev), None) == 0
            np.testing.assert_array_equal(dev, host, err_msg=f"world={world} nbins={nbins} rank={rank}")


def test_bench_headline_line_is_small_and_complete():
    """bench.py's LAST stdout line is what the driver parses (contract: one JSON line with `roofline` and `cpu_baseline`); round 5's
    28 KB line outgrew the driver's stdout tail and was recorded as unparsed.  The formatter is run on a canned full record (a real
    round-5 run, tests/golden/bench_full_record_r05.json): the line stays under 4 KiB whatever the `more` block holds, parses, and
    carries every field the contract names."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    full = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_full_record_r05.json")))
    full["roofline"]["traffic"] = 2219491840   # (that run's line had no counters attached; the formatter must carry them when present)
    full["roofline"]["traffic_provenance"] = {"source": "profiles/r05_pmc_traffic.json (x; commit y)", "sources_match": True}
    line = bench.headline_line(full)
    assert "\n" not in line and len(line) <= bench.HEADLINE_MAX_BYTES < 6000
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"]
    assert d["config"]["workload"].startswith("2^28 uniform-random uint32 keys-only OneSweep")
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and rf["traffic"] == 2219491840
    assert rf["algorithmic_bytes_per_launch"] == 8 << 28 and rf["avg_launch_ms"] > 0
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["sample"]
    assert len(d["more_digest"]["entropy_pairs_u64"]) == 5
    # a record whose digest would not fit loses the digest, never the contract's fields
    full["more"]["entropy_sweep"]["keys"] = full["more"]["entropy_sweep"]["keys"] * 400
    d2 = json.loads(bench.headline_line(full))
    assert "more_digest" not in d2 and d2["roofline"]["frac"] == rf["frac"] and d2["cpu_baseline"]["value"] == cb["value"]
    # the counters file the line borrows `traffic` from exists and names the sources it was measured on
    path = bench.pmc_traffic_file()
    assert path and "kernel_sources_sha256" in json.load(open(path))
    # a plain run (no --full) measures none of the blocks: its line is the contract's fields + config, nothing borrowed
    plain = {k: v for k, v in full.items() if k not in ("roofline", "box_floor", "more", "cpu_baseline", "full_record")}
    d3 = json.loads(bench.headline_line(plain))
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert d3[k] == d[k], k
    assert not {"roofline", "cpu_baseline", "more_digest", "full_record"} & set(d3)


def test_bench_dump_outputs_is_a_fixed_exact_sample(tmp_path):
    """bench.py --dump-outputs on (CPU) tensors standing in for the last step's output: float64, exact for every 32-bit word (u64 values
    as two uint32 columns), the same positions every time, in order, within 64 MB for the largest output the bench can produce."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_SAMPLE * 3 + 12345
    keys = np.sort(np.random.default_rng(1).integers(0, 1 << 32, n, dtype=np.uint64)).astype(np.uint32)
    kt = torch.from_numpy(keys.view(np.int32))
    vt = torch.from_numpy((keys.astype(np.int64) << 32) | 5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), kt, vt, n)
    k, v = np.load(tmp_path / "a" / "keys.npy"), np.load(tmp_path / "a" / "values.npy")
    assert k.dtype == v.dtype == np.float64 and k.shape == (bench.DUMP_SAMPLE,) and v.shape == (bench.DUMP_SAMPLE, 2)
    assert np.array_equal(k, np.load(tmp_path / "b" / "keys.npy")) and np.array_equal(v, np.load(tmp_path / "b" / "values.npy"))
    assert np.all(np.diff(k) >= 0) and np.isin(k, keys).all() and k[0] >= keys[0] and k[-1] <= keys[-1]
    assert np.array_equal(v[:, 1], k) and (v[:, 0] == 5).all()
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64e6
    bench.dump_outputs(str(tmp_path / "small"), kt, None, 1000)   # below the sample size: the whole output
    assert np.array_equal(np.load(tmp_path / "small" / "keys.npy"), keys[:1000].astype(np.float64))


@pytest.mark.parametrize("world,bin_major", [(2, 1), (3, 1), (8, 1), (8, 0), (5, 1)])
def test_bucket_exchange_rounds_land_the_stable_top_byte_partition(world, bin_major):
    """Round 6, multi-GPU (no GPU needed): the per-(peer, top byte) exchange rounds of gs_onesweep_sort_sharded — the host function the
    pipeline itself calls (gs_msd_exchange_round) — replayed over numpy shards.  Every rank's shard is grouped by top byte (what the
    split pass leaves); the rounds' messages are delivered; a bin-major landing must hold EXACTLY the stable top-byte partition of the
    concatenated sources restricted to the rank's byte range (so that the local sort can start at its second pass), a source-major
    landing the sources one after another; uneven splitters, empty bytes and an empty shard included."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(600 + world)
    # shards: (key, id) with id = global index; rank 1 of a 3-rank world brings nothing
    shards = []
    gid = 0
    for r in range(world):
        n = 0 if (world == 3 and r == 1) else int(rng.integers(2000, 5000))
        top = (rng.integers(0, 256, size=n) if r % 2 else np.minimum(rng.integers(0, 256, size=n), rng.integers(0, 300, size=n)).clip(0, 255)).astype(np.uint32)
        top[(top > 40) & (top < 60)] = 41                     # some empty bytes
        keys = (top << 24) | rng.integers(0, 1 << 24, size=n).astype(np.uint32)
        ids = np.arange(gid, gid + n, dtype=np.uint32)
        gid += n
        order = np.argsort(keys >> 24, kind="stable")         # the split pass: stable by top byte
        shards.append((keys[order], ids[order]))
    table = np.zeros((world, 256), dtype=np.uint32)
    for r, (k, _) in enumerate(shards):
        table[r] = np.bincount(k >> 24, minlength=256)
    plan = np.zeros(4 + 3 * world + 1, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.gs_msd_plan(table.ctypes.data_as(u32p), 256, world, 0, 1 << 30, plan.ctypes.data_as(u32p)) == _lib.GS_OK
    first = np.ascontiguousarray(plan[4 + 2 * world:4 + 3 * world + 1])
    assert first[0] == 0 and first[-1] == 256
    n_recv = [int(table[:, first[r]:first[r + 1]].sum()) for r in range(world)]
    land_k = [np.full(n, 0xFFFFFFFF, dtype=np.uint32) for n in n_recv]
    land_i = [np.full(n, 0xFFFFFFFF, dtype=np.uint32) for n in n_recv]
    rounds = C.c_uint32(0)
    sc, sd, rc, rd = (np.zeros(world, dtype=np.uint32) for _ in range(4))
    per_rank = {}
    for r in range(world):
        assert lib.gs_msd_exchange_round(table.ctypes.data_as(u32p), world, r, first.ctypes.data_as(u32p), bin_major, 0, sc.ctypes.data_as(u32p),
                                         sd.ctypes.data_as(u32p), rc.ctypes.data_as(u32p), rd.ctypes.data_as(u32p), C.byref(rounds)) == _lib.GS_OK
        assert rounds.value == int((first[1:] - first[:-1]).max())
    for j in range(rounds.value):
        for r in range(world):
            assert lib.gs_msd_exchange_round(table.ctypes.data_as(u32p), world, r, first.ctypes.data_as(u32p), bin_major, j, sc.ctypes.data_as(u32p),
                                             sd.ctypes.data_as(u32p), rc.ctypes.data_as(u32p), rd.ctypes.data_as(u32p), None) == _lib.GS_OK
            per_rank[r] = (sc.copy(), sd.copy(), rc.copy(), rd.copy())
        for src in range(world):                              # deliver: what src sends to dst is what dst expects from src
            for dst in range(world):
                cnt, off = int(per_rank[src][0][dst]), int(per_rank[src][1][dst])
                assert cnt == int(per_rank[dst][2][src])
                at = int(per_rank[dst][3][src])
                land_k[dst][at:at + cnt] = shards[src][0][off:off + cnt]
                land_i[dst][at:at + cnt] = shards[src][1][off:off + cnt]
    all_k = np.concatenate([s[0] for s in shards])
    all_i = np.concatenate([s[1] for s in shards])
    for r in range(world):
        mine = ((all_k >> 24) >= first[r]) & ((all_k >> 24) < first[r + 1])
        k, i = all_k[mine], all_i[mine]                       # sources in rank order, each grouped by top byte
        if bin_major:
            o = np.argsort(k >> 24, kind="stable")            # the stable top-byte partition of the concatenated sources
            k, i = k[o], i[o]
        np.testing.assert_array_equal(land_k[r], k)
        np.testing.assert_array_equal(land_i[r], i)
