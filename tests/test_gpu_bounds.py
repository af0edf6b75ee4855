"""The buffer contract of include/gpusort.h on the GPU (-m gpu): 16 bytes of alignment and no more; nothing outside [0, n) written,
no element outside it counted; const inputs not written.

Every buffer of every case is a view into one guard arena (tests/guard_arena.py): 16-byte but not 32-byte aligned, each buffer on a
skew of its own, count > n elements long, 128 KiB of guard on both sides, handles created with max_keys > n.  After the call: check(),
the n results bit for bit against the reference the other GPU tests use, arena.verify(), and — where the route leaves scan state —
every pass accounts for exactly n keys.  Constant fills are legal keys (0x00.. the smallest, 0xFF.. the largest), so both patterns
are cleared out of the inputs: a guard word pulled into a sort then changes a compared element instead of hiding among equals.
Scratch buffers are left holding the fill.  Every (route, value width) cell runs all classes of n mod 4, a multiple of the route's
tile and that multiple +- 1, under both constant fills; the hash fill runs once per cell; key types and orders rotate over the cases."""
import ctypes as C
import os

import numpy as np
import pytest

from guard_arena import Arena

pytestmark = pytest.mark.gpu

VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
T20 = 1 << 20
SLACK = 37          # count = n + SLACK: [n, count) is guard inside the view
ROOM = 4099         # max_keys = n + ROOM
SINGLE_TILE = {0: 32768, 4: 16384, 8: 8192}


def _skews(i, count):
    """`count` different odd skews, rotated by the case index."""
    return [2 * ((i + 3 * j) % 8) + 1 for j in range(count)]


def _clear_fill_patterns(keys):
    """All-zero and all-one words are what the constant fills look like as keys: none of them in the input."""
    ones = np.array(~np.zeros(1, dtype=keys.dtype))[0]
    keys[keys == 0] = 1
    keys[keys == ones] = ones - keys.dtype.type(1)
    return keys


def _keys32(oracle, n, seed, preset=0):
    return _clear_fill_patterns(oracle.init_random(n, seed, preset))


def _keys64(oracle, n, seed, preset=0):
    hi = oracle.init_random(n, seed, preset).astype(np.uint64)
    lo = oracle.init_random(n, seed + 0x5151, preset).astype(np.uint64)
    return _clear_fill_patterns((hi << np.uint64(32)) | lo)


def _values(n, vb):
    """Distinct, position-derived, never a fill pattern: stability and a value taken from the guard both show."""
    if vb == 4:
        return (np.arange(n, dtype=np.uint32) + np.uint32(1)) | np.uint32(0x40000000)
    return ((np.arange(n, dtype=np.uint64) + np.uint64(1)) << np.uint64(20)) | np.uint64(0x4000000000000001)


def _fill_id(fill):
    return {0x00: "00", 0xFF: "ff", "hash": "hash"}[fill]


def _assert_chains(r):
    assert (r["rows_not_inclusive"], r["rows_not_monotone"], r["chains_short_of_tickets"], r["hist_words_nonzero"]) == (0, 0, 0, 0), r


# ---- gs_onesweep_sort_keys / _sort_pairs: every route ------------------------------------------------------------------
# name -> (options of OneSweep, value widths, n by width, entropy preset, what check_state / last_plan must show)
def _single_tile_ns(vb):
    ns = [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 8190, 8191, 8192]  # tiles of 1024, 2048 and 8192 slots
    if vb != 8:
        ns += [16382, 16383, 16384]
    if vb == 0:
        ns += [32766, 32767, 32768]
    return ns


def _mid_ns(vb):
    ns = [8193, 24575, 24576, 24577, 100002, T20 - 1, T20]          # class 0: tiles of 8192, buckets up to 8192
    if vb != 8:
        ns += [T20 + 16383, T20 + 16384, T20 + 16385]               # class 1: tiles of 16 384
    if vb == 0:
        ns += [(1 << 21) + 16385, (1 << 22) + 32767]                # classes 2 and 3 (keys only)
    if vb == 4:
        ns += [(1 << 21) + 16386]                                   # class 4 (4-byte values)
    return ns


# (the two-level plan's descriptor rows — 256 chains in its second pass — need a handle of a few million keys: max_keys = 2^22 there)
ROUTES = {
    # one workgroup, one launch.  Above 8192 keys the two-launch route comes first while it is on: mid_path = 0 there.
    "single-tile": dict(options=lambda n: {} if n <= 8192 else {"mid_path": 0}, widths=(0, 4, 8), ns=_single_tile_ns, proof="no-scan-state"),
    "tiled-small": dict(options=lambda n: {"small_path": 0, "mid_path": 0}, widths=(0, 4, 8),
                        ns=lambda vb: [1, 2, 3, 6, 8191, 8192, 8193, 16383, 16384, 16385], proof="all-n"),
    "mid": dict(options=lambda n: {}, widths=(0, 4, 8), ns=_mid_ns, proof="no-scan-state"),
    "general": dict(options=lambda n: {"mid_path": 0}, widths=(0, 4, 8),
                    ns=lambda vb: [T20 + 2, T20 + 8191, T20 + 8192, T20 + 8193, T20 + 16389], proof="all-n"),
    "first-pass-16384": dict(options=lambda n: {"mid_path": 0}, widths=(0,),
                             ns=lambda vb: [(1 << 22) + 2, (1 << 22) + 16383, (1 << 22) + 16384, (1 << 22) + 16385], proof="all-n"),
    "position-chains": dict(options=lambda n: {"position_chains": 2, "position_chains_min_log2": 20, "mid_path": 0}, widths=(0, 4, 8),
                            ns=lambda vb: [T20, T20 + 2, T20 + 16383, T20 + 16384, T20 + 16385], proof="0-or-n"),
    "two-level": dict(options=lambda n: {"plan": 2, "position_chains_min_log2": 20, "small_path": 0, "mid_path": 0}, widths=(0, 4, 8),
                      ns=lambda vb: [T20 + 1, T20 + 2, T20 + 16383, T20 + 16384, T20 + 16385], proof="two-level", max_keys=1 << 22),
    "two-level-voided": dict(options=lambda n: {"plan": 2, "position_chains_min_log2": 20, "small_path": 0, "mid_path": 0}, widths=(0, 4, 8),
                             ns=lambda vb: [T20 + 1, T20 + 2, T20 + 16383, T20 + 16384, T20 + 16385], preset=3, proof="voided", max_keys=1 << 22),
}


def _sort_cases():
    cases = []
    for route, spec in ROUTES.items():
        for vb in spec["widths"]:
            ns = spec["ns"](vb)
            assert {n % 4 for n in ns} == {0, 1, 2, 3}, (route, vb)
            for i, n in enumerate(ns):
                for fill in (0x00, 0xFF):
                    cases.append(pytest.param(route, vb, n, fill, i, id=f"{route}-v{vb}-n{n}-{_fill_id(fill)}"))
            cases.append(pytest.param(route, vb, ns[len(ns) // 2], "hash", len(ns), id=f"{route}-v{vb}-n{ns[len(ns) // 2]}-hash"))
    return cases


def _run_sort(gpu, oracle, n, vb, fill, i, options, key64=False, preset=0, proof="0-or-n", fold_nans=False, max_keys=None):
    """One sort with every buffer in the arena; returns nothing, asserts everything."""
    kt, order = i % 3, i % 2
    kdt = np.uint64 if key64 else np.uint32
    count = n + SLACK
    specs = [(count, kdt), (count, kdt)] + ([(count, VALUE_DTYPE[vb])] * 2 if vb else [])
    arena = Arena.for_views(specs, "cuda", fill)
    sk = _skews(i, 4)
    dk = arena.carve(count, kdt, sk[0], "keys")
    da = arena.carve(count, kdt, sk[1], "alt_keys")
    dv = dav = None
    if vb:
        dv = arena.carve(count, VALUE_DTYPE[vb], sk[2], "values")
        dav = arena.carve(count, VALUE_DTYPE[vb], sk[3], "alt_values")
    keys = (_keys64 if key64 else _keys32)(oracle, n, 1000 + n + i, preset)
    if fold_nans and kt == 2:  # (as tests/test_gpu_twolevel.py: NaN patterns folded onto finite exponents)
        keys = np.where((keys & 0x7F800000) == 0x7F800000, keys & ~np.uint32(0x00800000), keys).astype(np.uint32)
    vals = _values(n, vb) if vb else None
    arena.write(dk, keys)
    arena.live(dk, n)
    arena.live(da, n)
    if vb:
        arena.write(dv, vals)
        arena.live(dv, n)
        arena.live(dav, n)
    s = gpu.OneSweep(max_keys or n + ROOM, order, kt + (3 if key64 else 0), gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb, **options)
    try:
        s.sort(dk, dv, n=n, alt_keys=da, alt_values=dav)
        s.check()
        r = s.check_state()
        plan = s.last_plan() if proof in ("two-level", "voided") else None
    finally:
        s.close()
    ref = (oracle.std_sort64 if key64 else oracle.std_sort)(keys, kt, order, vals)
    rk, rv = ref if vb else (ref, None)
    where = f"n={n} vb={vb} kt={kt} order={order} fill={fill!r} {options}"
    np.testing.assert_array_equal(arena.read(dk, kdt, n), rk, err_msg=where)
    if vb:
        np.testing.assert_array_equal(arena.read(dv, VALUE_DTYPE[vb], n), rv, err_msg="values " + where)
    arena.verify()
    _assert_chains(r)
    kpp = r["keys_per_pass"]
    if proof == "all-n" and n < 64:  # a handful of keys may agree in a byte: that pass is an identity and is dropped
        proof = "0-or-n"
    if proof == "no-scan-state":
        assert kpp == [0, 0, 0, 0], (where, r)
    elif proof == "all-n":
        assert kpp == [n, n, n, n], (where, r)
    elif proof == "key64-all":      # one plan for eight passes: entry q sums passes q and q + 4; two sweeps: the last round's four
        assert kpp == [2 * n if options.get("key64_sweeps", 1) == 1 else n] * 4, (where, r)
    else:
        assert all(k in (0, n) for k in kpp), (where, r)
    if proof == "two-level":
        assert plan["two_level"], (where, plan)
        if not vb:  # pass A, pass B; LSD passes 2 and 3 did not run
            assert kpp[:2] == [n, n] and sum(kpp) == 2 * n, (where, r)
    if proof == "voided":
        assert not plan["two_level"] and plan["largest_bucket"] > 0, (where, plan)  # offered, and found void on the device
        assert sum(kpp) > 0, (where, r)


@pytest.mark.parametrize("route,vb,n,fill,i", _sort_cases())
def test_sort_routes(gpu, oracle, route, vb, n, fill, i):
    spec = ROUTES[route]
    _run_sort(gpu, oracle, n, vb, fill, i, spec["options"](n), preset=spec.get("preset", 0), proof=spec["proof"],
              fold_nans=route == "two-level", max_keys=spec.get("max_keys"))


def _key64_cases():
    single = [1, 2, 3, 1023, 1024, 1025, 8190, 8191, 8192]   # one workgroup (64-bit keys: the classes up to 8192 slots)
    tiled = [8191, 8192, 8193, 16383, 16384, 16385, 20002]   # 8192-key tiles; the first two with the single-tile kernel off
    cases = []
    for sweeps in (1, 2):
        for vb in (0, 4, 8):
            for name, ns in (("single-tile", single), ("tiled", tiled)):
                assert {n % 4 for n in ns} == {0, 1, 2, 3} and {n % 2 for n in ns} == {0, 1}
                for i, n in enumerate(ns):
                    for fill in (0x00, 0xFF):
                        cases.append(pytest.param(name, sweeps, vb, n, fill, i, id=f"key64-{name}-s{sweeps}-v{vb}-n{n}-{_fill_id(fill)}"))
                cases.append(pytest.param(name, sweeps, vb, ns[4], "hash", len(ns), id=f"key64-{name}-s{sweeps}-v{vb}-n{ns[4]}-hash"))
    return cases


@pytest.mark.parametrize("route,sweeps,vb,n,fill,i", _key64_cases())
def test_sort_routes_64_bit_keys(gpu, oracle, route, sweeps, vb, n, fill, i):
    options = {"key64_sweeps": sweeps}
    if route == "tiled":
        options["small_path"] = 0
    _run_sort(gpu, oracle, n, vb, fill, i, options, key64=True, proof="no-scan-state" if route == "single-tile" else "key64-all")


# ---- structural and fixture entry points -------------------------------------------------------------------------------
def _in_out(fill, i, n, kdt, vb):
    """Read-only inputs and outputs live on [0, n), all of count = n + SLACK elements."""
    count = n + SLACK
    specs = [(count, kdt)] * 2 + ([(count, VALUE_DTYPE[vb])] * 2 if vb else [])
    arena = Arena.for_views(specs, "cuda", fill)
    sk = _skews(i, 4)
    kin = arena.carve(count, kdt, sk[0], "keys_in")
    kout = arena.carve(count, kdt, sk[1], "keys_out")
    vin = vout = None
    if vb:
        vin = arena.carve(count, VALUE_DTYPE[vb], sk[2], "values_in")
        vout = arena.carve(count, VALUE_DTYPE[vb], sk[3], "values_out")
    arena.live(kout, n)
    if vb:
        arena.live(vout, n)
    return arena, kin, kout, vin, vout


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("n", [8191, 8192, 8193, T20 + 2])
def test_digit_pass(gpu, oracle, n, vb, fill):
    """32-bit passes 0-3, reverse_index both ways: inputs read-only, outputs live on [0, n)."""
    i = n % 7 + vb
    arena, kin, kout, vin, vout = _in_out(fill, i, n, np.uint32, vb)
    keys = _keys32(oracle, n, n + vb, 1)
    vals = _values(n, vb) if vb else None
    arena.write(kin, keys)
    if vb:
        arena.write(vin, vals)
    s = gpu.OneSweep(n + ROOM, mode=gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, value_bytes=vb)
    for p in range(4):
        for rev in (False, True):
            s.digit_pass(kin, kout, p, n=n, values_in=vin, values_out=vout, reverse_index=rev)
            s.check()
            r = s.check_state()
            ref = oracle.digit_pass(keys, 8 * p, 0, vals, rev)
            rk, rv = ref if vb else (ref, None)
            np.testing.assert_array_equal(arena.read(kout, np.uint32, n), rk, err_msg=f"pass {p} rev {rev}")
            if vb:
                np.testing.assert_array_equal(arena.read(vout, VALUE_DTYPE[vb], n), rv, err_msg=f"values pass {p} rev {rev}")
            arena.verify()
            _assert_chains(r)
            assert all(k in (0, n) for k in r["keys_per_pass"]) and sum(r["keys_per_pass"]) == n, (p, rev, r)
    s.close()


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("n", [8191, 8192, 8193, 100002])
def test_digit_pass_64_bit_keys(gpu, oracle, n, vb, fill):
    i = n % 5 + vb
    arena, kin, kout, vin, vout = _in_out(fill, i, n, np.uint64, vb)
    keys = _keys64(oracle, n, n + vb, 0)
    vals = _values(n, vb) if vb else None
    arena.write(kin, keys)
    if vb:
        arena.write(vin, vals)
    s = gpu.OneSweep(n + ROOM, key_type=gpu.KEY_UINT64, mode=gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, value_bytes=vb)
    for p in range(8):
        for rev in (False, True):
            s.digit_pass(kin, kout, p, n=n, values_in=vin, values_out=vout, reverse_index=rev)
            s.check()
            ref = oracle.digit_pass64(keys, 8 * p, 0, vals, rev)
            rk, rv = ref if vb else (ref, None)
            np.testing.assert_array_equal(arena.read(kout, np.uint64, n), rk, err_msg=f"pass {p} rev {rev}")
            if vb:
                np.testing.assert_array_equal(arena.read(vout, VALUE_DTYPE[vb], n), rv, err_msg=f"values pass {p} rev {rev}")
            arena.verify()
    s.close()


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("n", [8191, 8192, 8193, T20 + 2])
def test_msd_prepare_and_partition(gpu, oracle, n, vb, fill):
    kt = n % 3
    arena, kin, kout, vin, vout = _in_out(fill, n % 7 + vb + 1, n, np.uint32, vb)
    keys = _keys32(oracle, n, 3 * n + vb, 0)
    vals = _values(n, vb) if vb else None
    arena.write(kin, keys)
    if vb:
        arena.write(vin, vals)
    s = gpu.OneSweep(n + ROOM, key_type=kt, mode=gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, value_bytes=vb)
    top = s.msd_prepare(kin, n)
    np.testing.assert_array_equal(top, oracle.global_histogram(keys, kt)[3])
    s.msd_partition(kin, kout, n, values_in=vin, values_out=vout)
    s.check()
    s.close()
    ref = oracle.digit_pass(keys, 24, kt, vals)
    rk, rv = ref if vb else (ref, None)
    np.testing.assert_array_equal(arena.read(kout, np.uint32, n), rk)
    if vb:
        np.testing.assert_array_equal(arena.read(vout, VALUE_DTYPE[vb], n), rv)
    arena.verify()


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1023, 8190, 8191, 8192, 8193, 65539, T20 + 2, (1 << 22) + 5])
def test_histograms_count_exactly_n_keys(gpu, oracle, n, fill):
    """global_histogram, scan_rows, msd_fine_histogram: the input is read-only and a key behind n is not counted — under a constant
    fill such a key lands in bin 0x00 / 0xFF of every table."""
    from gpusorting_amd.segsort import sortable_bits
    kt = n % 3
    count = n + SLACK
    arena = Arena.for_views([(count, np.uint32)], "cuda", fill)
    kin = arena.carve(count, np.uint32, _skews(n, 1)[0], "keys")
    keys = _keys32(oracle, n, 5 * n + 1, n % 2)
    arena.write(kin, keys)
    s = gpu.OneSweep(n + ROOM, key_type=kt)
    want = oracle.global_histogram(keys, kt)
    assert int(want[0].sum()) == n
    np.testing.assert_array_equal(s.global_histogram(kin, n), want)
    rows = s.scan_rows(kin, n)
    assert ((rows & 3) == 2).all()
    np.testing.assert_array_equal(rows >> 2, oracle.scan(want).reshape(4, 256))
    fine = s.msd_fine_histogram(kin, n)
    np.testing.assert_array_equal(fine, np.bincount(sortable_bits(keys, kt) >> np.uint32(20), minlength=4096).astype(np.uint32))
    s.check()
    s.close()
    arena.verify()


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 65536, 65537, 200002])
def test_init_random_fills_exactly_n(gpu, oracle, n, vb, fill):
    import torch
    count = n + SLACK
    arena = Arena.for_views([(count, np.uint32)] + ([(count, VALUE_DTYPE[vb])] if vb else []), "cuda", fill)
    sk = _skews(n + vb, 2)
    dk = arena.carve(count, np.uint32, sk[0], "keys")
    dv = arena.carve(count, VALUE_DTYPE[vb], sk[1], "values") if vb else None
    arena.live(dk, n)
    if vb:
        arena.live(dv, n)
    gpu.init_random(dk, 17 + n, n % 5, dv, n=n)
    torch.cuda.synchronize()
    ref = oracle.init_random(n, 17 + n, n % 5, vb)
    rk, rv = ref if vb else (ref, None)
    np.testing.assert_array_equal(arena.read(dk, np.uint32, n), rk)
    if vb:
        np.testing.assert_array_equal(arena.read(dv, VALUE_DTYPE[vb], n), rv)
    arena.verify()


@pytest.mark.parametrize("fill,order", [(0x00, 0), (0xFF, 1)], ids=["00-ascending", "ff-descending"])
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 65536, 65537, 300002])
def test_validate_stops_at_n(gpu, oracle, n, pairs, fill, order):
    """Behind a sorted [0, n) lies a fill that would be an inversion: the smallest key behind ascending keys, the largest behind
    descending ones.  Keys (and values = keys) are read-only."""
    count = n + SLACK
    arena = Arena.for_views([(count, np.uint32)] * 2, "cuda", fill)
    dk = arena.carve(count, np.uint32, 5, "keys")
    dv = arena.carve(count, np.uint32, 11, "values") if pairs else None
    keys = oracle.std_sort(_keys32(oracle, n, n, 0), 0, order)
    arena.write(dk, keys)
    if pairs:
        arena.write(dv, keys)
    assert gpu.validate(dk, dv, n=n, order=order) == 0
    assert gpu.validate(dk, dv, n=n + 1, order=order) >= 1, "the test's own premise: the guard word IS an inversion"
    arena.verify()


# ---- segmented sort through the raw C-ABI: the caller owns the alternates ----------------------------------------------
def _segsort_mix(vb, rng):
    """As test_heavy_tailed_mix of tests/test_gpu_segsort.py: every class filled, three long segments."""
    limit = SINGLE_TILE[vb]
    bounds = [b for b in (1, 32, 256, 1024, 2048, 8192, 16384, 32768) if b <= limit]
    parts = [rng.integers(0, 16, size=6000), rng.integers(900, 1100, size=60), [limit] * 2, [limit + 1, 40005 + limit, T20 + 6]]
    parts += [[b] for b in bounds] + [[40, 200, 1500, 5000]] + ([[12000]] if vb != 8 else []) + ([[20000]] if vb == 0 else [])
    lengths = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    rng.shuffle(lengths)
    mid = lengths.size // 2
    return np.concatenate([np.zeros(3, dtype=np.int64), lengths[:mid], np.zeros(50, dtype=np.int64), lengths[mid:], np.zeros(4, dtype=np.int64)])


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("promise", [False, True], ids=["long-segments", "promise-no-alternates"])
def test_segmented_sort_raw_abi(gpu, vb, fill, promise):
    """gs_segsort_sort_keys / _sort_pairs with d_alt* from the arena: offsets read-only, alternates live on [0, n), keys and values on
    [offsets[0], offsets[-1]) only.  With a promise (max_segment_len <= the LDS limit) d_alt* = NULL."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    i = vb // 4 + (3 if promise else 0) + {0x00: 0, 0xFF: 1, "hash": 2}[fill]
    kt, descending = i % 3, bool(i % 2)
    rng = np.random.default_rng(50 + vb)
    lengths = _segsort_mix(vb, rng)
    if promise:
        lengths = lengths[lengths <= SINGLE_TILE[vb]]
    head, tail = 5, 3
    offsets = (head + np.concatenate([[0], np.cumsum(lengths)])).astype(np.uint32)
    n = int(offsets[-1]) + tail
    count = n + SLACK
    num_segments = offsets.size - 1
    specs = [(count, np.uint32)] * 2 + [(offsets.size + SLACK, np.uint32)] + ([(count, VALUE_DTYPE[vb])] * 2 if vb else [])
    arena = Arena.for_views(specs, "cuda", fill)
    sk = _skews(i, 5)
    dk = arena.carve(count, np.uint32, sk[0], "keys")
    da = arena.carve(count, np.uint32, sk[1], "alt_keys")
    do = arena.carve(offsets.size + SLACK, np.uint32, sk[2], "offsets")
    dv = dav = None
    if vb:
        dv = arena.carve(count, VALUE_DTYPE[vb], sk[3], "values")
        dav = arena.carve(count, VALUE_DTYPE[vb], sk[4], "alt_values")
    keys = _clear_fill_patterns(_host_init_random(gpu, n, 77 + i, gpu.ENTROPY_PRESET_1))
    vals = _values(n, vb) if vb else None
    arena.write(dk, keys)
    arena.write(do, offsets)
    arena.live(dk, int(offsets[-1]), first=int(offsets[0]))
    if vb:
        arena.write(dv, vals)
        arena.live(dv, int(offsets[-1]), first=int(offsets[0]))
    if not promise:
        arena.live(da, n)
        if vb:
            arena.live(dav, n)
    h = C.c_void_p()
    mode = gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY
    assert lib.gs_segsort_create(C.byref(h), n + ROOM, num_segments + 9, mode, vb) == _lib.GS_OK
    try:
        max_len = SINGLE_TILE[vb] if promise else 0
        alt_k = None if promise else da.data_ptr()
        alt_v = None if promise or not vb else dav.data_ptr()
        if vb:
            st = lib.gs_segsort_sort_pairs(h, dk.data_ptr(), dv.data_ptr(), alt_k, alt_v, n, do.data_ptr(), num_segments, max_len, kt, int(descending), None)
        else:
            st = lib.gs_segsort_sort_keys(h, dk.data_ptr(), alt_k, n, do.data_ptr(), num_segments, max_len, kt, int(descending), None)
        assert st == _lib.GS_OK
        assert lib.gs_segsort_check(h, None) == _lib.GS_OK
        counts = (C.c_uint32 * (_lib.GS_SEGSORT_CLASSES + 1))()
        assert lib.gs_segsort_last_classes(h, counts, _lib.GS_SEGSORT_CLASSES + 1, None) == _lib.GS_OK
    finally:
        lib.gs_segsort_destroy(h)
    assert sum(counts[c] for c in range(9)) == num_segments and counts[8] == (0 if promise else 3)
    classes = sum(1 for b in (1, 32, 256, 1024, 2048, 8192, 16384, 32768) if b <= SINGLE_TILE[vb])
    assert all(counts[c] > 0 for c in range(classes)), list(counts)
    ref = gpu.segmented_sort_reference(keys, offsets, vals, kt, descending)
    rk, rv = ref if vb else (ref, None)
    np.testing.assert_array_equal(arena.read(dk, np.uint32, n), rk)
    if vb:
        np.testing.assert_array_equal(arena.read(dv, VALUE_DTYPE[vb], n), rv)
    arena.verify()


def _host_init_random(gpu, n, seed, preset):
    import torch
    t = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.init_random(t, seed, preset)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).copy()


# ---- top-k: inputs carved, skewed and read-only; outputs with a front guard as well ------------------------------------
@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"], ids=_fill_id)
@pytest.mark.parametrize("mode", ["keys", "v4", "v8", "pos"])
@pytest.mark.parametrize("n", [8191, 8192, 16384, 32768, 32769, 100003])
def test_topk(gpu, n, mode, fill):
    """Both routes (single tile up to 32 768 / 16 384 / 8192 keys by value width, the radix select above), k from _ks of
    tests/test_gpu_topk.py, reference and report checks by that file's helpers."""
    import test_gpu_topk as tk
    vb = tk._vb(mode)
    i = n % 11 + vb + {0x00: 0, 0xFF: 1, "hash": 2}[fill]
    key_type, descending = i % 3, bool(i % 2)
    keys = _clear_fill_patterns(_host_init_random(gpu, n, 7 * n + i, (gpu.ENTROPY_PRESET_1, gpu.ENTROPY_PRESET_3, gpu.ENTROPY_PRESET_5)[i % 3]))
    vals = tk._values(n, mode)
    count = n + SLACK
    h = tk._handle(gpu, n + ROOM, n, mode, key_type, descending)
    for j, k in enumerate(tk._ks(n)):
        specs = [(count, np.uint32), (k + SLACK, np.uint32)] + ([(count, VALUE_DTYPE[vb])] if vals is not None else []) + ([(k + SLACK, VALUE_DTYPE[vb])] if vb else [])
        arena = Arena.for_views(specs, "cuda", fill)
        sk = _skews(i + j, 4)
        dk = arena.carve(count, np.uint32, sk[0], "keys")
        ok = arena.carve(k + SLACK, np.uint32, sk[1], "out_keys")
        dv = arena.carve(count, VALUE_DTYPE[vb], sk[2], "values") if vals is not None else None
        ov = arena.carve(k + SLACK, VALUE_DTYPE[vb], sk[3], "out_values") if vb else None
        arena.write(dk, keys)
        arena.live(ok, k)
        if dv is not None:
            arena.write(dv, vals)
        if vb:
            arena.live(ov, k)
        h.select(dk, k, ok, dv, ov, n=n)
        h.check()
        rep = h.last()
        rk, rv = tk._reference(gpu, keys, k, vals, key_type, descending)
        np.testing.assert_array_equal(arena.read(ok, np.uint32, k), rk, err_msg=f"n={n} k={k} {mode}")
        if vb:
            np.testing.assert_array_equal(arena.read(ov, VALUE_DTYPE[vb], k), rv.astype(VALUE_DTYPE[vb]), err_msg=f"values n={n} k={k} {mode}")
        arena.verify()
        assert rep["route"] == (tk.SINGLE if n <= tk.SINGLE_TILE[vb] else tk.SELECT)
        tk._check_report(gpu, rep, keys, k, key_type, descending, vb)
    h.close()


# ---- sharded pipeline, one rank, exchange forced: the input shard is unchanged on return -------------------------------
@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=_fill_id)
@pytest.mark.parametrize("pairs", [False, True])
def test_sharded_single_rank_leaves_its_input(gpu, oracle, pairs, fill):
    import torch
    import torch.distributed as dist
    from gpusorting_amd.sharded import ShardedOneSweep
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        n = T20 + 77
        count = n + SLACK
        arena = Arena.for_views([(count, np.uint32)] * 2, "cuda", fill)
        dk = arena.carve(count, np.uint32, 7, "shard_keys")
        dv = arena.carve(count, np.uint32, 13, "shard_values") if pairs else None
        keys = _keys32(oracle, n, 99, 1)
        vals = _values(n, 4) if pairs else None
        arena.write(dk, keys)
        if pairs:
            arena.write(dv, vals)
        s = ShardedOneSweep(n + ROOM, pairs=pairs, value_bytes=4, always_exchange=True)
        bk, bv, nb = s.sort(dk, n, values=dv)
        s.engine.sorter.check()
        s.check()
        assert nb == n
        ref = oracle.std_sort(keys, vals=vals)
        rk, rv = ref if pairs else (ref, None)
        np.testing.assert_array_equal(bk.cpu().numpy().view(np.uint32), rk)
        if pairs:
            np.testing.assert_array_equal(bv.cpu().numpy().view(np.uint32), rv)
        arena.verify()
        s.close()
    finally:
        if created:
            dist.destroy_process_group()


# ---- sensitivity: the checker sees a one-element overrun on the real device path ---------------------------------------
def test_a_call_with_n_plus_one_is_seen(gpu, oracle):
    """Legal calls on memory the test owns: views prepared with live(view, n) are handed to the library with n + 1.  The element at n
    holds a key that the sort must move (the largest, ascending -> it stays; so the smallest: it goes to the front), and init_random
    overwrites it: verify() must raise and name it."""
    import torch
    n = 5000
    count = n + SLACK
    arena = Arena.for_views([(count, np.uint32)] * 2, "cuda", 0x00)   # the guard word behind n is the smallest key: an ascending sort moves it
    dk = arena.carve(count, np.uint32, 3, "keys")
    da = arena.carve(count, np.uint32, 9, "alt_keys")
    keys = _keys32(oracle, n, 4, 0)
    arena.write(dk, keys)
    arena.live(dk, n)
    arena.live(da, n)
    s = gpu.OneSweep(n + ROOM)
    s.sort(dk, n=n, alt_keys=da)
    s.check()
    arena.verify()                       # the same call with n: clean
    s.sort(dk, n=n + 1, alt_keys=da)     # sorted keys + the zero behind them
    s.check()
    s.close()
    with pytest.raises(AssertionError, match=r"keys \("):
        arena.verify()
    (name, first, last, damaged), = arena.damage()
    assert name == "keys" and 4 * n <= first <= last < 4 * n + 4 and damaged <= 4, "exactly the element behind n"
    assert int(arena.read(dk, np.uint32, n + 1)[0]) == 0, "the guard word was pulled into the result"

    arena = Arena.for_views([(count, np.uint32), (count, np.uint64)], "cuda", 0xFF)
    dk = arena.carve(count, np.uint32, 1, "keys")
    dv = arena.carve(count, np.uint64, 15, "values")
    arena.live(dk, n)
    arena.live(dv, n)
    gpu.init_random(dk, 12, 0, dv, n=n)
    torch.cuda.synchronize()
    arena.verify()
    gpu.init_random(dk, 12, 0, dv, n=n + 1)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"keys \((.|\n)*values \("):
        arena.verify()
    (kname, kfirst, klast, _), (vname, vfirst, vlast, _) = arena.damage()
    assert kname == "keys" and 4 * n <= kfirst <= klast < 4 * n + 4, "exactly the key behind n"
    assert vname == "values" and 8 * n <= vfirst <= vlast < 8 * n + 8, "exactly the value behind n"
