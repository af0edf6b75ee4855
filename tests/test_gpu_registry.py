"""Every compiled kernel instantiation runs once, with proof that it ran (-m gpu).  The cases come from the ledger,
tests/registry_cases.py: one per cell (or small group of cells that share a call) of the kernel registry.  Each case
  1. asks the host which way the call will go (gs_debug_sort_route, gs_segsort_class_of, the row-length classes) and asserts that it
     names the intended cell,
  2. runs the call and check(),
  3. compares keys and values bit for bit with the CPU reference the other GPU tests use (oracle.std_sort / std_sort64,
     segmented_sort_reference, topk_reference / topk_rows_reference),
  4. asserts the evidence after the call: the passes' flag words (gs_debug_pass_flags: which form of a pass worked, which passes were
     dropped, from which buffer each read), gs_onesweep_last_plan, the chained-scan state, last_classes, gs_topk_rows_last.
The bucket-local sorts of the two-level plan's classes 1 .. 3 (n > 2^27 in production) run with their class forced
(gs_debug_set_hy_class) on buckets of exactly the class's capacity: largest_bucket == cap is the proof.
Both orders everywhere.  Planted into the random keys: -0, +0, +-inf, NaN patterns of both signs, the integer minimum, -1, 0 and the
maximum, at the key's width.  Values are distinct and derived from the position; 8-byte values differ in their high words
((i << 33) | 0x1F), so a pass that moves a value in two halves shows."""
import numpy as np
import pytest

import registry_cases as rc

pytestmark = pytest.mark.gpu

SKEW, SKIP, SRC_ALT, LAST, POS = 1, 2, 4, 8, 16
WAVE, TILE, STREAM = 1, 2, 3
SPECIAL = {
    2: [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0xFFFF, 0x7FFF],
    4: [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0xFFFFFFFF, 0x7FFFFFFF],
    8: [0, 1 << 63, 0x7FF0 << 48, 0xFFF0 << 48, 0x7FF8 << 48, 0xFFF8 << 48, (1 << 64) - 1, (1 << 63) - 1],
}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
BIG_REF = 1 << 18   # above: the descending reference is the reversed ascending one (its definition), to keep the cases quick


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def plant(k, seed):
    """The exact keys of the issue, twice each (ties: stability shows in the values), spread over the array."""
    sp = SPECIAL[k.dtype.itemsize] * 2
    if k.size >= 4 * len(sp):
        pos = (np.arange(len(sp), dtype=np.int64) * k.size) // len(sp) + (seed % 3)
        k[pos] = np.array(sp, dtype=k.dtype)
    return k


def make_keys(oracle, n, kt, kind, seed):
    """n keys of key type kt (0 .. 2: uint32 words, 3 .. 5: uint64 words) of an input kind of the ledger."""
    wide = kt >= 3
    draw = (lambda s, a=0: oracle.init_random(n, s, a, 0))
    k = draw(seed, 4 if kind == rc.AND4 else 0)
    if wide:
        k = (draw(seed + 1000, 4 if kind == rc.AND4 else 0).astype(np.uint64) << np.uint64(32)) | k.astype(np.uint64)
    dt, bits = k.dtype.type, 64 if wide else 32
    if kind == rc.SKEW90:    # 90 % one key: every byte of it holds more than 1/16 of the keys, PF_SKEW in every pass
        heavy = np.random.default_rng(seed).random(n) < 0.9
        k[heavy] = dt(0x1010101010101010 if wide else 0x10101010)
    k = plant(k, seed)
    if kind == rc.LOW16:     # the low 16 bits constant: two identity passes.  Floats: one sign, a negative key's sortable form is inverted
        k = (k & dt(((1 << bits) - 1) ^ 0xFFFF)) | dt(0x1234)
        if kt in (2, 5):
            k &= dt((1 << (bits - 1)) - 1)
    if kind == rc.TOPBYTE:   # one top byte: the mid-size route's first kernel runs the LSD passes itself
        k = (k & dt((1 << (bits - 8)) - 1)) | dt(0x5A << (bits - 8))
    return k


def make_values(n, vb):
    if vb == 4:
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    if vb == 8:
        return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x1F)
    return None


def reference(oracle, k, kt, v):
    """[ascending, descending] -> (keys, values or None)"""
    f = oracle.std_sort64 if kt >= 3 else oracle.std_sort
    out = []
    for order in (0, 1):
        if order == 1 and k.size > BIG_REF:
            out.append(tuple(None if a is None else a[::-1].copy() for a in out[0]))
            continue
        r = f(k, kt % 3, order, v)
        out.append((r, None) if v is None else r)
    return out


@pytest.fixture(scope="module")
def handles(gpu):
    """Handles shared by the cases of one family x value width x key type (and across families where the options agree)."""
    made = {}

    def onesweep(max_keys, vb, kt, **options):
        key = ("onesweep", max_keys, vb, kt, tuple(sorted(options.items())))
        if key not in made:
            made[key] = gpu.OneSweep(max_keys, 0, kt, gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb, **options)
        return made[key]

    def segsort(max_keys, max_segments, vb, kt):
        key = ("segsort", max_keys, max_segments, vb, kt)
        if key not in made:
            made[key] = gpu.SegmentedSort(max_keys, max_segments, 0, kt, gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)
        return made[key]

    def topk(vb):
        key = ("topk", vb)
        if key not in made:
            made[key] = gpu.TopK(8 * 32776 + 64, 32768, 0, 0, gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)
        return made[key]

    class H:
        pass
    H.onesweep, H.segsort, H.topk = staticmethod(onesweep), staticmethod(segsort), staticmethod(topk)
    yield H
    for h in made.values():
        h.close()


def _clean(state):
    return (state["rows_not_inclusive"], state["rows_not_monotone"], state["chains_short_of_tickets"], state["hist_words_nonzero"]) == (0, 0, 0, 0)


def _sort_and_compare(s, k, v, ref, order, what):
    s.order = order
    dk, dv = _dev(k), (None if v is None else _dev(v))
    s.sort(dk, dv)
    s.check()
    np.testing.assert_array_equal(_host(dk, k.dtype), ref[order][0], err_msg=f"keys {what}")
    if v is not None:
        np.testing.assert_array_equal(_host(dv, v.dtype), ref[order][1], err_msg=f"values {what}")


def expected_flags(kind, passes, pos=False):
    """(flag word without PF_SKEW, PF_SKEW expected or None where the pass did not run) of every pass, as the Scan kernel plans them:
    identity passes are dropped in pairs, every pass that runs behind an odd number of passes reads the alternate buffers."""
    dropped = {0, 1} if kind == rc.LOW16 else set()
    last = max(q for q in range(passes) if q not in dropped)
    out, ran = [], 0
    for q in range(passes):
        if q in dropped:
            out.append((SKIP, None))
            continue
        out.append(((SRC_ALT if ran & 1 else 0) | (LAST if q == last else 0) | (POS if pos else 0), kind in (rc.SKEW90, rc.AND4)))
        ran += 1
    return out


def _assert_flags(s, kind, passes, n, what, pos=False):
    flags = s.pass_flags()
    want = expected_flags(kind, passes, pos)
    for q, (struct, skew) in enumerate(want):
        assert flags[q] & ~SKEW == struct, (what, q, flags, want)
        if skew is not None and not pos:   # (position chains: the passes behind the first derive their own skew, in LDS)
            assert bool(flags[q] & SKEW) == skew, (what, q, flags, want)
    assert flags[passes:] == [0] * (8 - passes), (what, flags)
    state = s.check_state()
    assert _clean(state), (what, state)
    ran = [0 if want[q][0] & SKIP else n for q in range(passes)]
    assert state["keys_per_pass"] == [sum(ran[q::4]) for q in range(4)], (what, state)   # (64-bit keys: passes q and q + 4 share a slot)


# ---- the runners, one per case kind ------------------------------------------------------------------------------------------------
def run_small(c, gpu, oracle, handles):
    vb, kt, cls = c["vb"], c["kt"], c["cls"]
    s = handles.onesweep(32768, vb, kt, **c["options"])
    for n in c["sizes"]:
        assert rc.SMALL_LOWER[cls] < n <= rc.SMALL_UPPER[cls]
        k, v = make_keys(oracle, n, kt, c["inputs"][0], 11 + n), make_values(n, vb)
        ref = reference(oracle, k, kt, v)
        for rank in c["ranks"]:
            s.set_rank_mode(rank)
            route = s.sort_route(n)
            assert (route["small"], route["mid"], route["rank_mode"]) == (cls, None, rank), route
            for order in (0, 1):
                _sort_and_compare(s, k, v, ref, order, (n, rank, order))
                assert s.check_state()["keys_per_pass"] == [0, 0, 0, 0] and s.pass_flags() == [0] * 8   # one launch, no scan state


def run_bin(c, gpu, oracle, handles):
    vb, kt, (threads, kpt) = c["vb"], c["kt"], c["shape"]
    (n,) = c["sizes"]
    s = handles.onesweep(1 << 17, vb, kt, **c["options"])
    s.set_shape(threads, kpt)
    passes = 8 if kt >= 3 else 4
    v = make_values(n, vb)
    for kind in c["inputs"]:
        k = make_keys(oracle, n, kt, kind, 23)
        ref = reference(oracle, k, kt, v)
        for rank in c["ranks"]:
            s.set_rank_mode(rank)
            route = s.sort_route(n)
            assert (route["small"], route["mid"], route["shape"], route["shape0"], route["dyn"], route["pos"], route["hy"], route["rank_mode"]) == \
                   (None, None, c["shape_index"], c["shape_index"], 2, 0, False, rank), route
            for order in (0, 1):
                _sort_and_compare(s, k, v, ref, order, (kind, rank, order))
                # 8-byte values on 512 x 32: both forms of every pass were launched, PF_SKEW says which one worked — VR 1 on the uniform
                # keys, VR 2 where a digit holds more than 1/16 of the keys
                _assert_flags(s, kind, passes, n, (kind, rank, order))
            if c["two_forms"] and kind == rc.SKEW90:
                # ... and the one-round form on skewed keys: without the device's plan there is one form per pass
                s.set_skip_passes(False)
                assert s.sort_route(n)["dyn"] == 0
                _sort_and_compare(s, k, v, ref, 0, (kind, rank, "fixed ping-pong"))
                assert all(f & SKEW for f in s.pass_flags()[:passes])
                s.set_skip_passes(True)


def run_pos(c, gpu, oracle, handles):
    vb, kt = c["vb"], c["kt"]
    (n,) = c["sizes"]
    s = handles.onesweep(n + 4091, vb, kt, **c["options"])
    assert s.rank_mode == 1, "the position-chain forms rank with LDS atomics: the probe must have passed on this device"
    route = s.sort_route(n)
    assert route["small"] is None and route["mid"] is None and route["pos"] & 0x7FFFFFFF in (16384, 12288) and not route["hy"], route
    assert route["shape"] == (1 if vb == 4 else 0), route
    k, v = make_keys(oracle, n, kt, c["inputs"][0], 31), make_values(n, vb)
    ref = reference(oracle, k, kt, v)
    for order in (0, 1):
        _sort_and_compare(s, k, v, ref, order, order)
        _assert_flags(s, c["inputs"][0], 4, n, order, pos=True)   # GS_PF_POS in every pass: both LAST forms worked
        assert not s.last_plan()["two_level"]


def run_hy(c, gpu, oracle, handles):
    vb, kt = c["vb"], c["kt"]
    (n,) = c["sizes"]
    s = handles.onesweep(c["max_keys"], vb, kt, **c["options"])
    assert s.rank_mode == 1
    route = s.sort_route(n)
    assert route["hy"] and route["pos"] and route["small"] is None and route["mid"] is None, route
    k = make_keys(oracle, n, kt, c["inputs"][0], n & 0xFFFF | 1)
    if kt == 2:   # as tests/test_gpu_twolevel.py builds its typed cases: the random NaN patterns folded onto finite exponents
        k = np.where((k & 0x7F800000) == 0x7F800000, k & ~np.uint32(0x00800000), k).astype(np.uint32)
        k = plant(k, 1)
    v = make_values(n, vb)
    ref = reference(oracle, k, kt, v)
    for order in (0, 1):
        _sort_and_compare(s, k, v, ref, order, order)
        assert s.last_plan()["two_level"], s.last_plan()
        state = s.check_state()
        assert _clean(state) and state["keys_per_pass"] == [n, n, 0, 0], state   # pass A, pass B; the LSD passes behind them did not run


def run_hy_class(c, gpu, oracle, handles):
    """Classes 1 .. 3 of the bucket-local sorts: the class is forced, the input holds buckets of exactly the class's cap (the first and
    the last prefix among them) and of every keys-per-thread value at its edges (tests/hy_bucket_inputs.py).  That the forced class
    ran: the plan is valid with a largest bucket of cap, which the class n implies (class 0: 3072 keys) would have refused."""
    import hy_bucket_inputs as hb
    vb, kt, cls, n = c["vb"], c["kt"], c["hy_class"], hb.N
    assert hb.cap(cls) == c["cap"] > hb.cap(0)
    s = handles.onesweep(c["max_keys"], vb, kt, **c["options"])
    assert s.rank_mode == 1
    k = hb.ladder_input(cls, kt)
    assert hb.prefix_histogram(k, kt).max() == c["cap"]
    v = make_values(n, vb)
    ref = reference(oracle, k, kt, v)
    s.set_hy_class(cls)
    try:
        route = s.sort_route(n)
        assert route["hy"] and route["pos"] and route["small"] is None and route["mid"] is None, route
        for order in (0, 1):
            _sort_and_compare(s, k, v, ref, order, order)
            lp = s.last_plan()
            assert lp["two_level"] and lp["largest_bucket"] == c["cap"], lp
            state = s.check_state()
            assert _clean(state) and state["keys_per_pass"] == [n, n, 0, 0], state
    finally:
        s.set_hy_class(-1)   # the handle is shared with the class-0 cases


def run_mid(c, gpu, oracle, handles):
    vb, kt, cls = c["vb"], c["kt"], c["cls"]
    (n,) = c["sizes"]
    s = handles.onesweep((1 << 22) + 1, vb, kt)
    v = make_values(n, vb)
    if cls > 0:
        assert s.sort_route(n - 1)["mid"] == (1 if cls == 4 else cls - 1)   # the smallest n of the class
    for kind in c["inputs"]:
        k = make_keys(oracle, n, kt, kind, 41 + cls)
        ref = reference(oracle, k, kt, v)
        for rank in c["ranks"]:
            s.set_rank_mode(rank)
            route = s.sort_route(n)
            assert (route["small"], route["mid"], route["rank_mode"]) == (None, cls, rank), route
            for order in (0, 1):
                _sort_and_compare(s, k, v, ref, order, (kind, rank, order))
                assert s.check_state()["keys_per_pass"] == [0, 0, 0, 0] and s.pass_flags() == [0] * 8   # two launches, no scan state


def _duplicate_every_second(k, starts, ends):
    """Ties in every second segment / row: 16 K distinct keys of both signs (position order among equal keys shows in the values)."""
    mask = k.dtype.type(0xC03F if k.dtype.itemsize == 2 else 0xC0000FFF)
    for a, b in list(zip(starts, ends))[::2]:
        k[a:b] &= mask
    return k


def run_seg_wg(c, gpu, oracle, handles):
    from gpusorting_amd import segmented_sort_reference
    vb, kt = c["vb"], c["kt"]
    rng = np.random.default_rng(50 + vb + kt)
    lens = []
    for cls in c["classes"]:
        lens += [rc.SMALL_UPPER[cls]] * 3 + [int(x) for x in rng.integers(0, 200, 12)] + [max(rc.SMALL_LOWER[cls], 256) + 1] * 3
    offsets = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.uint32)   # (three elements in front of the first segment: not touched)
    n = int(offsets[-1]) + 5
    h = handles.segsort(n, len(lens), vb, kt)
    for cls in c["classes"]:
        assert h.class_of(rc.SMALL_UPPER[cls]) == 3 + cls == h.class_of(max(rc.SMALL_LOWER[cls], 256) + 1)
    k = _duplicate_every_second(make_keys(oracle, n, kt, rc.UNIFORM, 61), offsets[:-1], offsets[1:])
    v = make_values(n, vb)
    d_off = _dev(offsets)
    for order in (0, 1):
        ref = segmented_sort_reference(k, offsets, v, kt, bool(order))
        rk, rv = (ref, None) if v is None else ref
        for rank in c["ranks"]:
            h.engine.set_rank_mode(rank)
            assert h.engine.rank_mode == rank
            h.order = order
            dk, dv = _dev(k), (None if v is None else _dev(v))
            h.sort(dk, d_off, dv, max_segment_len=h.max_lds_segment)
            h.check()
            np.testing.assert_array_equal(_host(dk, np.uint32), rk, err_msg=f"keys rank {rank} order {order}")
            if v is not None:
                np.testing.assert_array_equal(_host(dv, v.dtype), rv, err_msg=f"values rank {rank} order {order}")
            counts = h.last_classes()["counts"]
            assert [counts[3 + cls] for cls in range(5)] == [6 if cls in c["classes"] else 0 for cls in range(5)] and counts[8] == 0, counts
            assert h.engine.rank_mode == rank


def run_seg_vb(c, gpu, oracle, handles):
    from gpusorting_amd import segmented_sort_reference
    vb = c["vb"]
    rng = np.random.default_rng(70 + vb)
    long_len = {0: 32768, 4: 16384, 8: 8192}[vb] + 5
    lens = [int(x) for x in rng.integers(0, 33, 70)] + [int(x) for x in rng.integers(33, 257, 20)] + [2, 32, 33, 256, 0, 1]
    rng.shuffle(lens)
    lens = lens[:40] + [1] + [long_len] + lens[40:]     # the long segment starts off a 16-byte boundary: the head merge runs
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    if offsets[41] % 4 == 0:
        offsets[1:] += 1
    assert offsets[41] % 4 != 0 and offsets[42] - offsets[41] == long_len
    n = int(offsets[-1]) + 2
    v = make_values(n, vb)
    d_off = _dev(offsets)
    for kt in c["kts"]:
        h = handles.segsort(n, len(lens), vb, kt)
        assert h.max_lds_segment == long_len - 5 and h.class_of(long_len) == 8 and h.class_of(32) == 1 and h.class_of(33) == 2 == h.class_of(256)
        k = _duplicate_every_second(make_keys(oracle, n, kt, rc.UNIFORM, 71 + kt), offsets[:-1], offsets[1:])
        for order in (0, 1):
            ref = segmented_sort_reference(k, offsets, v, kt, bool(order))
            rk, rv = (ref, None) if v is None else ref
            h.order = order
            dk, dv = _dev(k), (None if v is None else _dev(v))
            h.sort(dk, d_off, dv)
            h.check()
            np.testing.assert_array_equal(_host(dk, np.uint32), rk, err_msg=f"keys kt {kt} order {order}")
            if v is not None:
                np.testing.assert_array_equal(_host(dv, v.dtype), rv, err_msg=f"values kt {kt} order {order}")
            counts = h.last_classes()
            assert counts["counts"][1] >= 50 and counts["counts"][2] >= 20 and counts["counts"][8] == 1 and counts["longest"] == long_len, counts


def _rows_keys(oracle, extent, kt, seed):
    if kt in rc.KEY16:
        k = plant(oracle.init_random((extent + 1) // 2, seed, 0, 0).view(np.uint16)[:extent].copy(), seed)
    else:
        k = make_keys(oracle, extent, kt, rc.UNIFORM, seed)
    return k


def _view2d(flat, rows, row_len, stride):
    return np.lib.stride_tricks.as_strided(flat, (rows, row_len), (stride * flat.itemsize, flat.itemsize), writeable=False)


def _rows_case(gpu, oracle, h, c, kt, rows, row_len, ks, route, seed):
    """One matrix (odd row stride), its full per-row reference once per order, every k of ks on the device."""
    from gpusorting_amd import topk_rows_reference
    vm, vb = c["vm"], c["vb"]
    stride = row_len + 3 if row_len % 2 == 0 else row_len + 4
    extent = (rows - 1) * stride + row_len
    starts = np.arange(rows) * stride
    k = _duplicate_every_second(_rows_keys(oracle, extent, kt, seed), starts, starts + row_len)
    v = make_values(extent, vb) if vm in (4, 8) else None
    dk, dv = _dev(k), (None if v is None else _dev(v))
    torch = _torch()
    fill = 0x5EED
    for order in (0, 1):
        rk, rv = topk_rows_reference(_view2d(k, rows, row_len, stride), row_len, None if v is None else _view2d(v, rows, row_len, stride), kt, bool(order))
        h.key_type, h.order = kt, order
        for kk in ks:
            kk = row_len if kk == "row_len" else min(kk, row_len)
            m = rows * kk
            ok = torch.full((m + 5,), fill, dtype=torch.int16 if k.dtype.itemsize == 2 else torch.int32, device="cuda")
            ov = torch.full((m + 5,), fill, dtype=torch.int32 if vb == 4 else torch.int64, device="cuda") if vb else None
            h.select_rows(dk, rows, row_len, stride, kk, ok, dv, ov)
            h.check()
            rep = h.rows_last()
            assert (rep["route"], rep["rows"], rep["row_len"], rep["k"], rep["status"]) == (route, rows, row_len, kk, 0), rep
            hk = _host(ok, k.dtype)
            np.testing.assert_array_equal(hk[:m].reshape(rows, kk), rk[:, :kk].view(k.dtype), err_msg=f"keys kt {kt} order {order} row_len {row_len} k {kk}")
            assert np.all(hk[m:] == fill)
            if vb:
                hv = _host(ov, UINT[vb])
                np.testing.assert_array_equal(hv[:m].reshape(rows, kk), rv[:, :kk].astype(UINT[vb]), err_msg=f"values kt {kt} order {order} row_len {row_len} k {kk}")
                assert np.all(hv[m:] == fill)


def run_tkr_tile(c, gpu, oracle, handles):
    vb, cls = c["vb"], c["cls"]
    h = handles.topk(vb)
    mode = gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY
    lib = h._lib
    for row_len in c["row_lens"]:
        assert lib.gs_segsort_class_of(row_len, mode, vb) - 3 == cls and row_len > 256, row_len   # the workgroup class the TILE route takes
        for rank in c["ranks"]:
            h.engine.set_rank_mode(rank)
            for kt in c["kts"]:
                _rows_case(gpu, oracle, h, c, kt, c["rows"], row_len, c["ks"], TILE, 80 + cls)
            assert h.engine.rank_mode == rank


def run_tkr_vm(c, gpu, oracle, handles):
    from gpusorting_amd.topk import rows_max_k
    vb = c["vb"]
    h = handles.topk(vb)
    mode = gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY
    long_len = h._lib.gs_segsort_max_lds_segment(mode, vb) + c["stream_extra"]
    max_k = rows_max_k(mode, vb)
    assert 1 < max_k <= 32768
    for kt in c["kts"]:
        for row_len in c["wave_row_lens"]:
            _rows_case(gpu, oracle, h, c, kt, 9, row_len, (1, 7, "row_len"), WAVE, 90)
        _rows_case(gpu, oracle, h, c, kt, 3, long_len, (1, max_k), STREAM, 91)


def run_topk1d(c, gpu, oracle, handles):
    from gpusorting_amd import topk_reference
    vm, vb = c["vm"], c["vb"]
    h = handles.topk(vb)
    torch = _torch()
    for (n, kk), route in ((c["single"], 3), (c["select"], 1)):
        v = make_values(n, vb) if vm in (4, 8) else None
        for kt in (0, 1, 2):
            k = make_keys(oracle, n, kt, rc.UNIFORM, 95 + kt)
            k[::2] &= np.uint32(0xC0000FFF)
            dk, dv = _dev(k), (None if v is None else _dev(v))
            for order in (0, 1):
                rk, rv = topk_reference(k, kk, v, kt, bool(order))
                for rank in c["ranks"]:
                    h.engine.set_rank_mode(rank)
                    h.key_type, h.order = kt, order
                    ok = torch.empty(kk, dtype=torch.int32, device="cuda")
                    ov = torch.empty(kk, dtype=torch.int32 if vb == 4 else torch.int64, device="cuda") if vb else None
                    h.select(dk, kk, ok, dv, ov)
                    h.check()
                    assert h.last()["route"] == route and h.engine.rank_mode == rank
                    # the final sort of k (select route) / the sort of the copy (single-tile route) ran on the engine's single-tile kernel
                    assert h.engine.sort_route(kk if route == 1 else n, kt)["small"] is not None
                    np.testing.assert_array_equal(_host(ok, np.uint32), rk, err_msg=f"keys n {n} kt {kt} order {order} rank {rank}")
                    if vb:
                        np.testing.assert_array_equal(_host(ov, UINT[vb]), rv.astype(UINT[vb]), err_msg=f"values n {n} kt {kt} order {order} rank {rank}")


def run_hist(c, gpu, oracle, handles):
    kt = c["kt"]
    (n,) = c["sizes"]
    s = handles.onesweep(1 << 17, 0, kt, small_path=0, mid_path=0, position_chains=0)
    k = make_keys(oracle, n, kt, rc.UNIFORM, 99)
    np.testing.assert_array_equal(s.global_histogram(_dev(k)), oracle.global_histogram(k, kt))


RUNNERS = {"small": run_small, "bin": run_bin, "pos": run_pos, "hy": run_hy, "hy_class": run_hy_class, "mid": run_mid, "seg_wg": run_seg_wg, "seg_vb": run_seg_vb,
           "tkr_tile": run_tkr_tile, "tkr_vm": run_tkr_vm, "topk1d": run_topk1d, "hist": run_hist}


@pytest.mark.parametrize("cid", sorted(rc.CASES))
def test_registry_cell(gpu, oracle, handles, cid):
    c = rc.CASES[cid]
    RUNNERS[c["kind"]](c, gpu, oracle, handles)
