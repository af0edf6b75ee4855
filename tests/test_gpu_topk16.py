"""The 1-D top-k on 16-bit keys (gs_topk16_* of include/gpusort.h, gpusorting_amd/csrc/topk16_kernels.hpp, gpusorting_amd/topk16.py) on
the GPU.  Every case compares keys AND values bit for bit with gpusorting_amd.topk_reference (tests/test_topk16_cpu.py holds it against
the head of sort16_reference), calls status(), asks last() for the route and the report, checks the fill behind element k of both
outputs and that the inputs are unchanged.  No counterpart in the reference project.

The constants of the plan (topk16_kernels.hpp): a chunk is 8 keys x 1024 threads = 8192 keys, a tile 4 chunks = 32 768 keys, a range a
multiple of a chunk and at least one tile, at most 256 ranges."""
import numpy as np
import pytest

from test_gpu_topk_rows16 import FLOAT_SALT, INT_SALT, _dev, _torch, _values, _vb  # the row-wise 16-bit tests' helpers and float patterns

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
KEY_TYPES = (U16, I16, F16, BF16)
VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
LDS = {0: 32768, 4: 16384, 8: 8192}  # gs_segsort_max_lds_segment: up to here the TILE route
NONE, TILE, COUNT, SELECT = 0, 1, 2, 3
HIST_AUTO, HIST_SLICES, HIST_GLOBAL = 0, 1, 2
SLICES_MIN = 1 << 27  # GS_TOPK16_COUNT_SLICES_MIN: HIST_AUTO takes the slices from here on
MODES = ("keys", "v4", "v8", "pos")
FILL16, FILL = 0x5EED, 0x5EEDBEEF
CHUNK, MIN_RANGE, MAX_RANGES = 8192, 32768, 256


def _handle(gpu, max_keys, max_k, mode, key_type=U16, descending=False):
    vb = _vb(mode)
    return gpu.TopK16(max_keys, max_k, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type,
                      gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _plan(n, hist=HIST_SLICES):
    """(ranges, elements per range) of the histogram: the slices' plan, or gs_sort16_plan's for keys only (HIST_GLOBAL)."""
    if hist == HIST_GLOBAL:
        per = -(-(-(-n // 128)) // CHUNK) * CHUNK
    else:
        per = max(MIN_RANGE, -(-(-(-n // MAX_RANGES)) // CHUNK) * CHUNK)
    return -(-n // per), per


def _route(n, mode):
    return TILE if n <= LDS[_vb(mode)] else COUNT if mode == "keys" else SELECT


def _bits16(u, kt):
    """The 16-bit pattern whose unsigned order is the key order."""
    u = u.astype(np.uint32)
    if kt == U16:
        return u
    if kt == I16:
        return u ^ 0x8000
    return np.where(u & 0x8000, u ^ 0xFFFF, u ^ 0x8000)


class _Case:
    """One array of 2-byte keys on the device and its full reference (k = n), computed once: the reference for a smaller k is its head,
    by the definition of topk_reference."""

    def __init__(self, gpu, keys, mode, key_type=U16, descending=False):
        assert keys.dtype == np.uint16 and keys.ndim == 1
        self.gpu, self.keys, self.mode, self.key_type, self.descending = gpu, keys, mode, key_type, descending
        self.n = keys.size
        self.vals = _values(self.n, mode)
        self.dk = _dev(keys)
        self.dv = _dev(self.vals) if self.vals is not None else None
        self.rk, self.rv = gpu.topk_reference(keys, self.n, self.vals, key_type, descending)
        flip = 0xFFFF if descending else 0
        self.bins = np.sort(_bits16(keys, key_type) ^ flip)  # selection space: both orders look for the k smallest
        self.flip = flip

    def expected_report(self, k, hist):
        t = int(self.bins[k - 1])
        front, behind = int(np.searchsorted(self.bins, t, "left")), int(np.searchsorted(self.bins, t, "right"))
        ranges, per = _plan(self.n, hist)
        return {"threshold": t ^ self.flip, "in_front": front, "equal": behind - front, "taken": k - front, "ranges": ranges, "per_range": per,
                "hist": hist}

    def run(self, h, k, pad=5):
        """A COUNT call runs three times: with each of the two histograms forced, then as the handle chooses (by n)."""
        if _route(self.n, self.mode) != COUNT:
            return self._run(h, k, pad, HIST_SLICES)
        for hist in (HIST_SLICES, HIST_GLOBAL):
            h.set_count_histogram(hist)
            self._run(h, k, pad, hist)
        h.set_count_histogram(HIST_AUTO)
        return self._run(h, k, pad, HIST_SLICES if self.n >= SLICES_MIN else HIST_GLOBAL)

    def _run(self, h, k, pad, hist):
        torch, vb = _torch(), _vb(self.mode)
        ok = torch.full((k + pad,), FILL16, dtype=torch.int16, device="cuda")
        ov = torch.full((k + pad,), FILL, dtype=torch.int32 if vb == 4 else torch.int64, device="cuda") if vb else None
        h.select(self.dk, k, ok, self.dv, ov, n=self.n)
        assert h.status() == 0
        rep = h.last()
        route = _route(self.n, self.mode)
        assert rep["route"] == route and rep["status"] == 0, rep
        if route != TILE:
            want = self.expected_report(k, hist)
            assert {name: rep[name] for name in want} == want, (rep, want)
        hk = ok.cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(hk[:k], self.rk[:k])
        assert np.all(hk[k:] == FILL16), "nothing at or behind element k of the output keys is written"
        if vb:
            hv = ov.cpu().numpy().view(VALUE_DTYPE[vb])
            np.testing.assert_array_equal(hv[:k], self.rv[:k].astype(VALUE_DTYPE[vb]))
            assert np.all(hv[k:] == FILL), "nothing at or behind element k of the output values is written"
        return rep

    def inputs_unchanged(self):
        np.testing.assert_array_equal(self.dk.cpu().numpy().view(np.uint16), self.keys)
        if self.dv is not None:
            np.testing.assert_array_equal(self.dv.cpu().numpy().view(self.vals.dtype), self.vals)


def _random16(n, seed, distinct=1 << 16):
    return np.random.default_rng(seed).integers(0, distinct, n).astype(np.uint16)


def _salted(n, seed, key_type):
    keys = _random16(n, seed)
    salt = np.array(FLOAT_SALT.get(key_type, INT_SALT), dtype=np.uint16)
    at = np.arange(0, n, 5)
    keys[at] = salt[(at // 5) % salt.size]  # every fifth element one of 13 or 6 values: ties
    return keys


# ---- types and modes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_types_and_modes(gpu, key_type, descending, mode):
    n = 70001  # COUNT / SELECT for every mode: three ranges, the last one partial, n no multiple of 8
    h = _handle(gpu, n, n, mode, key_type, descending)
    case = _Case(gpu, _salted(n, 40 + key_type, key_type), mode, key_type, descending)
    for k in (1, 50, 5001):
        case.run(h, k)
    case.inputs_unchanged()
    h.close()


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
def _sizes(vb):
    L = LDS[vb]
    return sorted({1, 2, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1, CHUNK - 1, CHUNK, CHUNK + 1, MIN_RANGE - 1, MIN_RANGE, MIN_RANGE + 1,
                   2 * MIN_RANGE + 3, (1 << 20) - 1})


@pytest.mark.parametrize("mode,n", [(mode, n) for mode in MODES for n in _sizes(_vb(mode))])
def test_sizes(gpu, mode, n):
    """Around a wave, the TILE | COUNT / SELECT border L (the route is asserted on both sides; L is the minimum range keys only and a
    chunk with 8-byte values), a chunk, the minimum range, two ranges + 3 (the last range partial, n no multiple of 8) and 2^20 - 1;
    every k of the list that fits."""
    size_index = _sizes(_vb(mode)).index(n)
    case = _Case(gpu, _random16(n, 100 + size_index, 1 << 12), mode, BF16, size_index % 2 == 1)  # (4096 patterns: ties at the larger sizes)
    h = _handle(gpu, n, n, mode, BF16, case.descending)
    for k in sorted({k for k in (1, 2, 63, 64, 65, 1000, 4097, n - 1, n) if 1 <= k <= n}):
        case.run(h, k)
    case.inputs_unchanged()
    h.close()


@pytest.mark.parametrize("mode", ["keys", "pos", "v8"])
def test_odd_k_on_a_guard_arena(gpu, mode):
    """Bases with 16 bytes of alignment and no more, guard bands around the input and both outputs, an odd k: the 2-byte element behind
    the k-th is untouched, and the input is unchanged.  One TILE-sized and one COUNT / SELECT-sized array."""
    from guard_arena import Arena
    torch = _torch()
    vb = _vb(mode)
    for n, k in ((3001, 65), (2 * MIN_RANGE + 3, 4097)):
        keys = _random16(n, 23 + n, 1 << 10)
        vals = _values(n, mode)
        spare = 11
        vt = VALUE_DTYPE.get(vb, np.uint32)
        specs = [(2 * n, np.uint8), (2 * (k + spare), np.uint8), (k + spare, vt)] + ([(n, vt)] if vals is not None else [])
        arena = Arena.for_views(specs, "cuda", fill="hash")
        dk = arena.carve(2 * n, np.uint8, 1, "keys")
        ok = arena.carve(2 * (k + spare), np.uint8, 3, "out_keys")
        ov = arena.carve(k + spare, vt, 5, "out_values")
        dv = None
        if vals is not None:
            dv = arena.carve(n, vt, 7, "values")
            arena.write(dv, vals)
        arena.write(dk, keys.view(np.uint8))
        arena.live(ok, 2 * k)
        if vb:
            arena.live(ov, k)
        h = _handle(gpu, n, k, mode, I16, True)
        h.select(dk.view(torch.int16), k, ok.view(torch.int16), dv, ov if vb else None, n=n)
        assert h.status() == 0
        assert h.last()["route"] == _route(n, mode)
        h.close()
        arena.verify()
        rk, rv = gpu.topk_reference(keys, k, vals, I16, True)
        np.testing.assert_array_equal(arena.read(ok, np.uint16, 2 * k), rk)
        if vb:
            np.testing.assert_array_equal(arena.read(ov, vt, k), rv.astype(vt))


# ---- structure ---------------------------------------------------------------------------------------------------------------------
N_BIG = (1 << 20) + 5


def _structure_keys(name, descending):
    """(keys, key type, [k, ...]); the patterns are stated for the ascending order and mirrored for the descending one, so that the
    k-th element lies where the name says in both."""
    n = N_BIG
    mirror = (lambda a: ~a) if descending else (lambda a: a)
    if name == "all_equal":
        return np.full(n, 0x1234, dtype=np.uint16), U16, [1, 1000, n]
    if name in ("half_one_pattern", "run_end"):
        keys = (_random16(n, 3) >> np.uint16(1)) | np.uint16(0x8000)  # behind the run
        keys[np.random.default_rng(4).permutation(n)[: n // 2]] = 0x4000  # half of the array, everywhere
        keys[7::4099] = 0x0007  # a few in front
        front = int(np.count_nonzero(keys == 0x0007))
        run = int(np.count_nonzero(keys == 0x4000))
        return mirror(keys), U16, ([front + run // 3, front + 1] if name == "half_one_pattern" else [front + run, front])
    if name == "bin_0_and_bin_65535":
        keys = _random16(n, 5)
        where = np.random.default_rng(6).permutation(n)
        keys[where[: n // 4]] = 0x0000
        keys[where[n // 4: n // 2]] = 0xFFFF
        return keys, U16, [n // 8, n - n // 8]  # (its own mirror image)
    if name == "sorted":
        return mirror(np.sort(_random16(n, 7))), U16, [1, 777, 70001]
    if name == "reverse_sorted":
        return mirror(np.sort(_random16(n, 8))[::-1].copy()), U16, [1, 777, 70001]
    assert name == "float_specials"
    return _salted(n, 9, F16), F16, [3, 100000, n - 100000]


@pytest.mark.parametrize("name", ["all_equal", "half_one_pattern", "run_end", "bin_0_and_bin_65535", "sorted", "reverse_sorted", "float_specials"])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("mode", ["pos", "v8", "keys"])
def test_structure(gpu, name, descending, mode):
    keys, key_type, ks = _structure_keys(name, descending)
    n = keys.size
    h = _handle(gpu, n, n, mode, key_type, descending)
    case = _Case(gpu, keys, mode, key_type, descending)
    reps = [case.run(h, k) for k in ks]
    if name == "all_equal":
        assert all((r["in_front"], r["equal"], r["taken"]) == (0, n, k) for r, k in zip(reps, ks))
        if mode == "pos":  # ascending the lowest positions rising, descending the highest falling
            want = n - 1 - np.arange(1000) if descending else np.arange(1000)
            np.testing.assert_array_equal(case.rv[:1000], want)
    if name == "half_one_pattern":
        assert 0 < reps[0]["taken"] < reps[0]["equal"], reps[0]
        assert reps[0]["threshold"] == (0xBFFF if descending else 0x4000)
    if name == "run_end":
        assert reps[0]["taken"] == reps[0]["equal"] > 1000, reps[0]
        assert reps[1]["taken"] == reps[1]["equal"], reps[1]
    if name == "bin_0_and_bin_65535":
        assert [r["threshold"] for r in reps] == ([0xFFFF, 0x0000] if descending else [0x0000, 0xFFFF])
        assert all(0 < r["taken"] < r["equal"] for r in reps)
    case.inputs_unchanged()
    h.close()


# ---- counter wrap -------------------------------------------------------------------------------------------------------------------
WRAP_PER = 16 * CHUNK                       # 131 072: the smallest range that holds two patterns of 65 536 keys each
WRAP_N = (WRAP_PER - CHUNK) * MAX_RANGES + 1  # 31 457 281: the smallest n whose ranges are that long (ceil(n / 256) > 15 chunks)


def _wrap_case(descending):
    keys = (_random16(WRAP_N, 12) | np.uint16(0x0400))
    keys[:65536] = 0x0100          # range 0: two patterns of 65 536 keys each and nothing else
    keys[65536:WRAP_PER] = 0x0200
    keys[WRAP_PER + 5::300007] = 0x0001  # a few keys in front of the heavy runs, in later ranges
    if descending:
        keys = ~keys
    bits = np.sort(keys ^ np.uint16(0xFFFF if descending else 0))[:70000]
    return keys, _dev(keys), bits


@pytest.mark.parametrize("descending", [False, True])
def test_counter_wrap_is_recounted(gpu, descending):
    """The histogram's table holds 16-bit counters, two to a word: a pattern with 65 536 keys in one range wraps its counter to 0.
    The smallest case follows from the constants: a range must hold 2 x 65 536 keys, so 16 chunks of 8192 = 131 072 keys, and the
    ranges are that long from n = 15 x 8192 x 256 + 1 = 31 457 281 on.  Range 0 holds 65 536 keys of one pattern and 65 536 of another
    and nothing else: the vote makes one of them the hot bin (counted in registers, exact), the other one's counter wraps, the
    overflow test (table sum + hot count != keys of the range) sees it, the range is recounted on 32-bit counters and its per-range
    counts come from the keys.  pos mode; k below the heavy runs and inside the second of them.  Only the head of the reference is
    made (by position within equal keys), not an argsort of 31 M keys per k."""
    assert _plan(WRAP_N) == (241, WRAP_PER) and _plan(WRAP_N - 1)[1] == WRAP_PER - CHUNK
    torch = _torch()
    keys, dk, bits = _wrap_case(descending)
    few = int(np.count_nonzero(bits == 0x0001))
    assert few > 50 and np.count_nonzero(bits == 0x0100) == 65536 and bits[-1] == 0x0200
    h = _handle(gpu, WRAP_N, 70000, "pos", U16, descending)
    for k in (few // 2, few + 65536 + 1000):
        ok = torch.full((k + 4,), FILL16, dtype=torch.int16, device="cuda")
        ov = torch.full((k + 4,), FILL, dtype=torch.int32, device="cuda")
        h.select(dk, k, ok, None, ov, n=WRAP_N)
        assert h.status() == 0
        rep = h.last()
        t = int(bits[k - 1])
        assert (rep["route"], rep["status"], rep["ranges"], rep["per_range"]) == (SELECT, 0, 241, WRAP_PER), rep
        assert (rep["threshold"], rep["in_front"], rep["taken"]) == (t ^ (0xFFFF if descending else 0), int(np.searchsorted(bits, t)),
                                                                     k - int(np.searchsorted(bits, t))), rep
        # the reference's head: the candidates are the keys up to the threshold, few enough for a stable argsort
        sel = keys ^ np.uint16(0xFFFF if descending else 0)
        cand = np.flatnonzero(sel <= t)
        order = cand[np.argsort(sel[cand], kind="stable")]
        if descending:  # the exact reverse of the stable ascending order of the keys: equal keys in falling position
            order = cand[::-1][np.argsort(sel[cand[::-1]], kind="stable")]
        order = order[:k]
        hk, hv = ok.cpu().numpy().view(np.uint16), ov.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(hk[:k], keys[order])
        np.testing.assert_array_equal(hv[:k], order.astype(np.uint32))
        assert np.all(hk[k:] == FILL16) and np.all(hv[k:] == FILL)
    h.close()


# ---- the histogram HIST_AUTO takes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SLICES_MIN - 1, SLICES_MIN])
def test_count_histogram_by_n(gpu, n):
    """Keys only on both sides of GS_TOPK16_COUNT_SLICES_MIN: the global histogram below it, the slices from it on, the same result.
    uint16 keys, so that the reference's head is numpy's sort of the keys (no argsort of 2^27 elements)."""
    torch = _torch()
    keys = _random16(n, 77, 5000)
    keys[::3] |= np.uint16(0x8000)
    dk = _dev(keys)
    ordered = np.sort(keys)
    k = 100001
    want_hist = HIST_SLICES if n >= SLICES_MIN else HIST_GLOBAL
    for descending in (False, True):
        h = _handle(gpu, n, k, "keys", U16, descending)
        ok = torch.full((k + 3,), FILL16, dtype=torch.int16, device="cuda")
        h.select(dk, k, ok, n=n)
        assert h.status() == 0
        rep = h.last()
        assert (rep["route"], rep["hist"], rep["ranges"], rep["per_range"]) == (COUNT, want_hist) + _plan(n, want_hist), rep
        hk = ok.cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(hk[:k], ordered[::-1][:k] if descending else ordered[:k])
        assert np.all(hk[k:] == FILL16)
        h.close()


# ---- handle reuse ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["keys", "pos"])
def test_handle_reuse(gpu, mode):
    """Two calls of different n and k on one handle (the larger first, so that the scratch holds the leftovers of a longer call), and
    a TILE call between them: the same results as on fresh handles — every run is compared with the reference."""
    big, small, tile = _Case(gpu, _random16(300007, 61, 300), mode, F16, True), _Case(gpu, _random16(70001, 62, 5), mode, F16, True), \
        _Case(gpu, _random16(5000, 63), mode, F16, True)
    h = _handle(gpu, 300007, 300007, mode, F16, True)
    for case, k in ((big, 100000), (small, 333), (tile, 77), (big, 9), (small, 70001)):
        case.run(h, k)
        fresh = _handle(gpu, case.n, k, mode, F16, True)
        case.run(fresh, k)
        fresh.close()
    h.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,hist", [("keys", HIST_SLICES), ("keys", HIST_GLOBAL), ("pos", HIST_SLICES)])
def test_captured_graph_replayed_on_new_data(gpu, mode, hist):
    """A COUNT call on either histogram and a SELECT call, each a single-stream, linear capture, replayed after the input was
    overwritten."""
    torch = _torch()
    n, k = 100003, 257
    h = _handle(gpu, n, k, mode, BF16, True)
    h.set_count_histogram(hist)
    dk = _dev(_random16(n, 31))
    ok = torch.empty(k, dtype=torch.int16, device="cuda")
    ov = torch.empty(k, dtype=torch.int32, device="cuda") if mode == "pos" else None
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        h.select(dk, k, ok, None, ov)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.select(dk, k, ok, None, ov)
    for seed in (32, 33):
        keys = _random16(n, seed, 1 << 16 if seed == 32 else 40)
        dk.copy_(_dev(keys))
        ok.zero_()
        if ov is not None:
            ov.zero_()
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        assert (h.last()["route"], h.last()["hist"]) == (COUNT if mode == "keys" else SELECT, hist)
        rk, rv = gpu.topk_reference(keys, k, None, BF16, True)
        np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint16), rk)
        if ov is not None:
            np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), rv)
    h.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    OK, A, S, M = _lib.GS_OK, _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    n = 100000
    keys = torch.zeros(n, dtype=torch.int16, device="cuda")
    vals = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = torch.full((n,), FILL16, dtype=torch.int16, device="cuda")
    outv = torch.full((n,), FILL, dtype=torch.int64, device="cuda")
    p, v, o, ov = keys.data_ptr(), vals.data_ptr(), out.data_ptr(), outv.data_ptr()
    max_k = 5000
    hk = gpu.TopK16(n, max_k)
    h4 = gpu.TopK16(n, max_k, mode=gpu.MODE_PAIRS, value_bytes=4)
    h8 = gpu.TopK16(n, max_k, mode=gpu.MODE_PAIRS, value_bytes=8)

    def sk(h, keys_p, n_, k, out_p, kt=U16, order=0):
        return lib.gs_topk16_select_keys(h._h if h else None, keys_p, n_, k, out_p, kt, order, None)

    def sp(h, keys_p, vals_p, n_, k, out_p, outv_p, kt=U16, order=0):
        return lib.gs_topk16_select_pairs(h._h if h else None, keys_p, vals_p, n_, k, out_p, outv_p, kt, order, None)

    # 1. GS_ERR_ARG: the null handle first of all; pointers, key type, order — before the mode and the sizes are looked at
    assert sk(None, None, 0, 0, None, 99, 7) == A and sp(None, None, None, 0, 0, None, None, 99, 7) == A
    assert sk(hk, None, n, 8, o) == A and sk(hk, p, n, 8, None) == A
    assert sk(hk, p + 2, n, 8, o) == A and sk(hk, p + 8, n, 8, o) == A and sk(hk, p, n, 8, o + 4) == A
    for kt in (0, 1, 2, 3, 4, 5, 10, -1):  # the 32-bit and 64-bit key types are refused
        assert sk(hk, p, n, 8, o, kt) == A and sp(h4, p, None, n, 8, o, ov, kt) == A, kt
    assert sk(hk, p, n, 8, o, U16, 2) == A and sk(hk, p, n, 8, o, U16, -1) == A
    assert sk(h4, p, 0, 0, o, 0) == A and sk(h4, None, 0, 0, o) == A  # (a keys call on a pairs handle: the argument comes first)
    # 2. GS_ERR_MODE: before the value pointers and the sizes
    assert sk(h4, p, n, 8, o) == M and sk(h8, p, 0, 0, o) == M
    assert sp(hk, p, v, n, 8, o, ov) == M and sp(hk, p, None, 0, 0, o, None) == M
    # 3. GS_ERR_ARG: the value pointers, before the sizes; d_vals == NULL needs 4-byte values
    assert sp(h4, p, v, n, 8, o, None) == A and sp(h4, p, v, n, 8, o, ov + 8) == A and sp(h4, p, v + 4, n, 8, o, ov) == A
    assert sp(h8, p, None, n, 8, o, ov) == A and sp(h8, p, None, 0, 0, o, ov) == A and sp(h4, p, v, 0, 0, o, None) == A
    # 4. GS_ERR_SIZE: before the overlap test
    for h, call in ((hk, lambda n_, k, out_p=o: sk(hk, p, n_, k, out_p)), (h4, lambda n_, k, out_p=o: sp(h4, p, None, n_, k, out_p, ov))):
        assert call(0, 1) == S and call(n + 1, 8) == S and call(n, 0) == S and call(100, 101) == S and call(n, max_k + 1) == S
        assert call(n, 0, p) == S and call(n + 1, 8, p) == S  # (overlapping as well)
        assert call(n, max_k) == OK and call(1, 1) == OK
    # 5. GS_ERR_ARG: overlap, the extents counted in 2-byte elements: 1000 keys end at byte 2000, a multiple of 16
    assert sk(hk, p, 1000, 8, p + 2000) == OK and sk(hk, p, 1000, 8, p + 2000 - 16) == A
    assert sk(hk, p, 1001, 8, p + 2000) == A and sk(hk, p, 1001, 8, p + 2016) == OK  # 2002 bytes of input
    assert sk(hk, p + 16, 1000, 8, p) == OK and sk(hk, p + 16, 1000, 9, p) == A      # 16 and 18 bytes of output
    assert sk(hk, p, n, 8, p) == A
    assert sp(h8, p, v, 1000, 8, o, v + 8000) == OK and sp(h8, p, v, 1000, 8, o, v + 8000 - 16) == A
    assert sp(h8, p, v, 1000, 8, o, ov) == OK and sp(h4, p, None, 1000, 8, o, o) == A  # (an output on the other output)
    torch.cuda.synchronize()
    for h in (hk, h4, h8):
        assert h.status() == 0
    # a refused call leaves a filled output untouched and GS_TOPK16_ROUTE_NONE in the report, also behind a call that went through
    out.fill_(FILL16)
    outv.fill_(FILL)
    assert sk(hk, p, n, 8, o + 65536) == OK and (hk.last()["route"], hk.last()["hist"]) == (COUNT, HIST_GLOBAL)
    assert sp(h4, p, None, 1000, 8, o + 65536, ov + 65536) == OK and h4.last()["route"] == TILE
    torch.cuda.synchronize()
    for refused in (sk(hk, p, n, max_k + 1, o), sk(hk, p, n, 8, o, 2), sk(hk, p, n, 8, p), sp(h4, p, None, n, 0, o, ov), sp(h4, p, v + 4, n, 8, o, ov),
                    sk(h4, p, n, 8, o)):
        assert refused != OK
    assert hk.last()["route"] == NONE and h4.last()["route"] == NONE
    assert bool((out[:32768] == FILL16).all()) and bool((outv[:8192] == FILL).all()), "a refused call writes nothing"
    # the COUNT route's histogram: three values and no other
    assert lib.gs_topk16_set_count_histogram(None, 0) == A and lib.gs_topk16_set_count_histogram(hk._h, 3) == A
    for which in (HIST_SLICES, HIST_GLOBAL, HIST_AUTO):
        assert lib.gs_topk16_set_count_histogram(hk._h, which) == OK
    # the 32-bit entry keeps refusing the 16-bit key types
    t32 = gpu.TopK(4096, 8)
    for kt in KEY_TYPES:
        assert lib.gs_topk_select_keys(t32._h, p, 4096, 8, o, kt, 0, None) == A
    t32.close()
    # the Python layer: 2-byte tensors only, 16-bit key types only
    with pytest.raises(ValueError):
        hk.select(torch.zeros(4096, dtype=torch.int32, device="cuda"), 8, torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        gpu.TopK16(4096, 8, key_type=gpu.KEY_FLOAT32)
    with pytest.raises(ValueError):
        hk.select(keys, 8, out, None, outv)  # out_values on a keys-only handle
    for h in (hk, h4, h8):
        h.close()


# ---- functional.topk16 -------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(_torch().int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("dtype_name,key_type", [("float16", F16), ("bfloat16", BF16), ("int16", I16)])
def test_functional_topk16(gpu, dtype_name, key_type):
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    # NaN-free and tie-free: a permutation of distinct representable values; one TILE-sized and one SELECT-sized vector
    for n, k in ((1000, 17), (40000, 300)):
        if key_type == I16:
            distinct = (np.arange(n) - n // 2).astype(np.int16).view(np.uint16)
        elif key_type == F16:  # finite, non-zero float16 patterns of both signs
            distinct = np.concatenate([0x0400 + np.arange(n // 2), 0x8400 + np.arange(n - n // 2)]).astype(np.uint16)
        else:                  # finite, non-zero bfloat16 patterns of both signs
            distinct = np.concatenate([0x0080 + np.arange(n // 2), 0x8080 + np.arange(n - n // 2)]).astype(np.uint16)
        x = torch.from_numpy(np.random.default_rng(5).permutation(distinct).view(np.int16)).cuda().view(dtype)
        for largest in (True, False):
            v, i = gpu.topk16(x, k, largest=largest)
            tv, ti = torch.topk(x, k, largest=largest)
            assert v.shape == (k,) and v.dtype == dtype and i.dtype == torch.int32
            np.testing.assert_array_equal(_bits(v), _bits(tv))
            np.testing.assert_array_equal(i.cpu().numpy(), ti.cpu().numpy().astype(np.int32))
    # with ties (and, for the floats, NaNs and both zeros): the library's order, as the reference states it
    t = _random16(50001, 9) & np.uint16(0xFC07)
    xt = torch.from_numpy(t.view(np.int16).copy()).cuda().view(dtype)
    for largest in (True, False):
        v, i = gpu.topk16(xt, 4500, largest=largest)
        rk, rv = gpu.topk_reference(t, 4500, None, key_type, largest)
        np.testing.assert_array_equal(_bits(v), rk)
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
    # carried int64 values
    vals = torch.arange(50001, dtype=torch.int64, device="cuda") * 3 + 1
    v, w = gpu.topk16(xt, 12, largest=False, values=vals)
    rk, rv = gpu.topk_reference(t, 12, np.arange(50001, dtype=np.uint64) * 3 + 1, key_type, False)
    np.testing.assert_array_equal(_bits(v), rk)
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint64), rv)
    # a 2-D input is the row-wise call of topk
    m = xt[:50000].view(50, 1000)
    for largest in (True, False):
        a, b = gpu.topk16(m, 9, largest=largest), gpu.topk(m, 9, largest=largest)
        assert a[0].shape == (50, 9) and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])
    # other dtypes name topk; topk keeps refusing the 1-D tensor and names both ways out
    with pytest.raises(TypeError, match="topk"):
        gpu.topk16(torch.zeros(100, dtype=torch.float32, device="cuda"), 5)
    with pytest.raises(TypeError, match=r"x\[None, :\]"):
        gpu.topk(xt, 5)
    with pytest.raises(ValueError):
        gpu.topk16(xt, 0)


def test_functional_topk16_on_uint16_storage(gpu):
    """int16 storage with unsigned=True, and a torch.uint16 tensor where this torch has the dtype: the same keys, the same result."""
    torch = _torch()
    t = _random16(45000, 11)
    x = torch.from_numpy(t.view(np.int16).copy()).cuda()
    rk, rv = gpu.topk_reference(t, 9, None, U16, True)
    views = [(x, True)] + ([(x.view(torch.uint16), False)] if hasattr(torch, "uint16") else [])
    for view, unsigned in views:
        v, i = gpu.topk16(view, 9, unsigned=unsigned)
        assert v.dtype == view.dtype
        np.testing.assert_array_equal(_bits(v), rk)
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
