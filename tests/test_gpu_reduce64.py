"""GPU tests of reduce by key on 64-bit keys (gs_reduce64_* in include/gpusort.h, gpusorting_amd/reduce64.py,
functional.reduce_by_key64).  Keys, counts, integer sums and every MIN / MAX are compared exactly against reduce_by_key64_reference
(tests/test_reduce64_cpu.py checks that one against numpy and by hand).  Float sums: the test values are drawn from {-1, -0.5, -0.0, 0,
0.5, 1}, so every partial sum in any order is a multiple of 0.5 below 2^23 in magnitude (n <= 513 * 2 * 4096 + 1 < 2^23) and exact in
float32 and float64: they are compared BITWISE as well.  General floats are compared against the float64 / integer sum within
|got - exact| <= (m - 1) * eps * sum|v| per run of length m, eps = 2^-24 for float32 and 2^-53 for float64: the bound of any summation
order.  On zero-extended 32-bit keys the float sums are BITWISE those of gs_reduce_by_key: the tree is the same one.  Sizes come from
gs_unique_plan and from the pairs sorter's single-workgroup edge for 8-byte keys (8192 with both value widths)."""
import numpy as np
import pytest

from guard_arena import FILLS, Arena
from test_reduce_cpu import F32_ASCENDING, f64_ascending
from test_unique64_cpu import draws64

pytestmark = pytest.mark.gpu

U32 = 0
U64, I64, F64 = 3, 4, 5
VI32, VU32, VF32, VI64, VU64, VF64 = range(6)
SUM, MIN, MAX = range(3)
NONE, SORTED, CONSECUTIVE = 0, 1, 2
NP = {VI32: np.int32, VU32: np.uint32, VF32: np.float32, VI64: np.int64, VU64: np.uint64, VF64: np.float64}
TILE = 4096
MAXN = 513 * 2 * TILE + 1  # the largest size of the file: 514 ranges of two tiles, the last one holds one element
FILL = 0x5A5A5A5A
FLOAT_POOL = np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 1.0])
HI = np.uint64(1) << np.uint64(32)
W_N = 2 * TILE + 1
W_BASE = np.uint64(0x0123456789ABCDEF)


def _torch():
    import torch
    return torch


def _vb(vt):
    return np.dtype(NP[vt]).itemsize


def _dev(a):
    """A host array of 4- or 8-byte elements as an int32 / int64 device tensor with the same bits."""
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()).cuda()


def _host(t, n=None):
    a = (t if n is None else t[:n]).cpu().numpy()
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _bits(a, vt):
    """A reference result as the unsigned patterns the device must deliver (a float64 sum is rounded to the value type: exact here)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64 and vt == VF32:
        a = a.astype(np.float32)
    assert a.dtype.itemsize == _vb(vt)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _handle(gpu, vb, kt=U64, descending=False):
    """One handle of capacity MAXN per (value width, key type, order) for the whole file: every test is a reuse of it as well."""
    key = (vb, kt, descending)
    if key not in _handles:
        _handles[key] = gpu.ReduceByKey64(MAXN, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, kt, vb)
    return _handles[key]


def _values(n, seed, vt):
    """Floats from FLOAT_POOL (sums exact in any order), integers full-range random (the modular sum is exact)."""
    rng = np.random.default_rng(seed)
    if vt in (VF32, VF64):
        return FLOAT_POOL[rng.integers(0, FLOAT_POOL.size, n)].astype(NP[vt])
    info = np.iinfo(NP[vt])
    return rng.integers(info.min, int(info.max) + 1, n, dtype=NP[vt])


def _positional(n, vt):
    """Position-dependent integers: a dropped, doubled or misplaced element changes a sum, and the extremes are all different."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    return x if _vb(vt) == 8 else (x >> np.uint64(32)).astype(np.uint32)


def _compare(gpu, h, keys, vals, entry, kt, descending, vt, op, counts=True):
    """Runs `entry` and compares every delivered output with the reference, bit for bit; returns u."""
    n = keys.size
    rk, rv, rc = gpu.reduce_by_key64_reference(keys, vals, kt, descending, vt, op, consecutive=entry == "consecutive")
    dk, dv = _dev(keys), _dev(vals)
    call = h.reduce_by_key if entry == "sorted" else h.reduce_by_key_consecutive
    ok, ov, oc, num = call(dk, dv, op, vt, counts=counts)
    h.check()
    u = int(num.item())
    assert u == rk.size, (entry, n, u, rk.size)
    rep = h.last()
    assert (rep["route"], rep["n"], rep["u"], rep["status"]) == (SORTED if entry == "sorted" else CONSECUTIVE, n, u, 0)
    assert (rep["ranges"], rep["per_range"], rep["tile"]) == gpu.unique_plan(n) and (rep["value_type"], rep["op"]) == (vt, op)
    assert ok.element_size() == 8
    np.testing.assert_array_equal(_host(ok, u), rk)
    np.testing.assert_array_equal(_host(ov, u), _bits(rv, vt))
    assert (oc is not None) == counts
    if oc is not None:
        np.testing.assert_array_equal(_host(oc, u), rc)
    np.testing.assert_array_equal(_host(dk), keys.view(np.uint64))  # the inputs are not written
    np.testing.assert_array_equal(_host(dv), _bits(vals, vt))
    return u


# ---- types and ops -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vt", range(6))
@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("kt", (U64, I64, F64))
def test_types_and_ops(gpu, kt, descending, vt):
    """3 key types x 2 orders x 6 value types, the three ops inside; both entries; out_counts and d_out_num given and NULL."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    n = 5000
    keys, vals = draws64(n, 100 + kt, 37), _values(n, 200 + vt, vt)
    h = _handle(gpu, _vb(vt), kt, descending)
    for op in (SUM, MIN, MAX):
        assert _compare(gpu, h, keys, vals, "sorted", kt, descending, vt, op) <= 37
        _compare(gpu, h, np.sort(keys), vals, "consecutive", kt, descending, vt, op, counts=op != MIN)
        rk, rv, rc = gpu.reduce_by_key64_reference(keys, vals, kt, descending, vt, op)  # neither out_counts nor d_out_num
        dk, dv = _dev(keys), _dev(vals)
        ok, ov = _torch().empty_like(dk), _torch().empty_like(dv)
        assert lib.gs_reduce64_by_key(h._h, dk.data_ptr(), dv.data_ptr(), n, ok.data_ptr(), ov.data_ptr(), None, None, kt, int(descending), vt, op,
                                      None) == _lib.GS_OK
        h.check()
        assert h.last()["u"] == rk.size
        np.testing.assert_array_equal(_host(ok, rk.size), rk)
        np.testing.assert_array_equal(_host(ov, rk.size), _bits(rv, vt))


@pytest.mark.parametrize("vt", range(6))
def test_ops_and_value_types_at_2_20(gpu, vt):
    """All three ops x the six value types above the sorter's single workgroup: 1000 keys, n = 2^20 + 1; integers depend on the position."""
    n = (1 << 20) + 1
    keys = draws64(n, 300, 1000)
    vals = _values(n, 301 + vt, vt) if vt in (VF32, VF64) else _positional(n, vt)
    for op in (SUM, MIN, MAX):
        assert _compare(gpu, _handle(gpu, _vb(vt)), keys, vals, "sorted", U64, False, vt, op) == 1000


# ---- the word split ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diff", (1, 1 << 32), ids=("low", "high"))
@pytest.mark.parametrize("at", (8, 512, TILE, 2 * TILE), ids=("thread", "wave", "tile", "range"))
def test_word_split_at_every_edge(gpu, at, diff):
    """A step in one word only at element `at`, whose left neighbour is held by another thread (8: through the shuffle), wave, tile or
    workgroup (512, 4096, 8192: lane 0 reads it from memory); a single key
    that differs there; and the key in front of the edge.  Position-dependent uint64 sums and float32 sums."""
    for vt, vals in ((VU64, _positional(W_N, VU64)), (VF32, _values(W_N, at, VF32))):
        h = _handle(gpu, _vb(vt))
        step = np.full(W_N, W_BASE, np.uint64)
        step[at:] += np.uint64(diff)
        assert _compare(gpu, h, step, vals, "consecutive", U64, False, vt, SUM) == 2
        one = np.full(W_N, W_BASE, np.uint64)
        one[at] += np.uint64(diff)
        assert _compare(gpu, h, one, vals, "consecutive", U64, False, vt, SUM) == (3 if at + 1 < W_N else 2)
        before = np.full(W_N, W_BASE, np.uint64)
        before[at - 1] += np.uint64(diff)
        assert _compare(gpu, h, before, vals, "consecutive", U64, False, vt, SUM) == 3


@pytest.mark.parametrize("kind", ("high_only", "low_only", "pairs_high", "pairs_low"))
def test_word_split_pools(gpu, kind):
    i = np.arange(24, dtype=np.uint64)
    a = i * (HI << np.uint64(4)) + np.uint64(0x89ABCDEE)
    pool = {"high_only": W_BASE + i * HI, "low_only": W_BASE + i, "pairs_high": np.concatenate([a, a + HI]),
            "pairs_low": np.concatenate([a, a + np.uint64(1)])}[kind]
    rng = np.random.default_rng(len(kind))
    laid = np.sort(pool[rng.integers(0, pool.size, W_N)])
    vals = _positional(W_N, VU64)
    assert _compare(gpu, _handle(gpu, 8), laid, vals, "consecutive", U64, False, VU64, SUM) == pool.size
    shuffled = laid.copy()
    rng.shuffle(shuffled)
    for descending in (False, True):
        assert _compare(gpu, _handle(gpu, 8, U64, descending), shuffled, vals, "sorted", U64, descending, VU64, SUM) == pool.size
        assert _compare(gpu, _handle(gpu, 4, U64, descending), shuffled, _values(W_N, 3, VF32), "sorted", U64, descending, VF32, SUM) == pool.size


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, (1 << 20) + 1, (1 << 22) + 5)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    """A wave, a tile, per_range -+ 1, the pairs sorter's single-workgroup edge for 8-byte keys (8192) -+ 1, 2^20 + 1 and the first plan of
    two-tile ranges: 7 distinct keys and all keys distinct; float32 SUM, int64 SUM, uint32 MIN."""
    few, all_distinct = draws64(n, n, 7), draws64(n, n + 1, 0)
    for vt, op in ((VF32, SUM), (VI64, SUM), (VU32, MIN)):
        vals = _values(n, n + vt, vt) if vt == VF32 else _positional(n, vt)
        h = _handle(gpu, _vb(vt))
        assert _compare(gpu, h, few, vals, "sorted", U64, False, vt, op) == np.unique(few).size
        assert _compare(gpu, h, all_distinct, vals, "sorted", U64, False, vt, op) == n


@pytest.mark.parametrize("word", ("low", "high"))
@pytest.mark.parametrize("n", ((1 << 22) + 1, MAXN - 2, MAXN))
def test_ranges_of_two_tiles(gpu, n, word):
    """Runs of three across every edge and runs of 2 * TILE + 1 (whole tiles and ranges without a head: the carry crosses them), the run's
    number in one word of the key; position-dependent int64 SUM and uint32 MIN."""
    assert gpu.unique_plan(n)[1] == 2 * TILE
    shift = np.uint64(32 if word == "high" else 0)
    const = W_BASE & np.uint64(0xFFFFFFFF) if word == "high" else W_BASE & ~(HI - np.uint64(1))
    for run in (3, 2 * TILE + 1):
        keys = ((np.arange(n, dtype=np.uint64) // np.uint64(run)) << shift) + const
        for vt, op in ((VI64, SUM), (VU32, MIN)):
            assert _compare(gpu, _handle(gpu, _vb(vt)), keys, _positional(n, vt), "consecutive", U64, False, vt, op) == -(-n // run)


def test_every_element_enters_its_run_exactly_once(gpu):
    """uint64 SUM of 1 << (i % 64) over runs of at most 64 neighbours: the sum of a run is the OR of 64 different bits at the most, so
    an element that is dropped, doubled or handed to the neighbouring run shows in the bits.  The counts are checked beside it."""
    n = 7 * TILE + 77
    rng = np.random.default_rng(64)
    heads = np.cumsum(rng.integers(1, 65, n))
    flag = np.zeros(n, np.uint64)
    flag[heads[heads < n]] = 1
    keys = np.cumsum(flag, dtype=np.uint64) * HI + W_BASE  # the run's number in the high word
    vals = np.uint64(1) << (np.arange(n, dtype=np.uint64) % np.uint64(64))
    h = _handle(gpu, 8)
    u = _compare(gpu, h, keys, vals, "consecutive", U64, False, VU64, SUM)
    ok, ov, oc, num = h.reduce_by_key_consecutive(_dev(keys), _dev(vals), SUM, VU64)
    got, cnt = _host(ov, u), _host(oc, u)
    assert int(cnt.sum()) == n and cnt.max() <= 64
    assert np.array_equal(np.array([bin(int(x)).count("1") for x in got]), cnt)
    shuffled = np.random.default_rng(65).permutation(n)
    _compare(gpu, h, keys[shuffled], vals[shuffled], "sorted", U64, False, VU64, SUM)


# ---- float sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("vt", (VF32, VF64))
def test_float_sums_on_zero_extended_keys_are_bitwise_those_of_the_32_bit_family(gpu, vt, descending):
    """General floats (inexact sums): the tree depends on n and on where the runs lie, not on the width of the keys."""
    n = (1 << 20) + 1
    rng = np.random.default_rng(90 + vt)
    k32 = rng.integers(0, 1 << 32, 3000).astype(np.uint32)[rng.integers(0, 3000, n)]
    vals = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(NP[vt])
    order = gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING
    h32 = gpu.ReduceByKey(n, order, gpu.KEY_UINT32, _vb(vt))
    dv = _dev(vals)
    ok, ov, oc, num = h32.reduce_by_key(_dev(k32), dv, SUM, vt)
    h32.check()
    u = int(num.item())
    h64 = _handle(gpu, _vb(vt), U64, descending)
    qk, qv, qc, qnum = h64.reduce_by_key(_dev(k32.astype(np.uint64)), dv, SUM, vt)
    h64.check()
    assert int(qnum.item()) == u
    np.testing.assert_array_equal(_host(qk, u), _host(ok, u).astype(np.uint64))
    np.testing.assert_array_equal(_host(qc, u), _host(oc, u))
    np.testing.assert_array_equal(_host(qv, u), _host(ov, u))  # bit for bit
    h32.close()


@pytest.mark.parametrize("vt", (VF32, VF64))
def test_general_floats_within_the_bound_of_any_order_and_reproducible(gpu, vt):
    """Random floats, n = 2^20 + 1, 1000 keys on both words: |got - exact| <= (m - 1) * eps * sum|v| per run of length m, eps = 2^-24
    (float32; exact = the float64 sum) or 2^-53 (float64; exact = the integer sum of the values scaled by 2^40: the values are
    multiples of 2^-40 below 2^12, so the integer sum is the exact one); the call twice and once more on a second handle: bitwise equal."""
    n = (1 << 20) + 1
    rng = np.random.default_rng(77)
    keys = draws64(n, 78, 1000)
    if vt == VF32:
        vals = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
        rk, exact, rc = gpu.reduce_by_key64_reference(keys, vals, U64, False, VF32, SUM)
        _, mass, _ = gpu.reduce_by_key64_reference(keys, np.abs(vals), U64, False, VF32, SUM)
        eps = 2.0 ** -24
    else:
        scaled = rng.integers(-(1 << 52), 1 << 52, n, dtype=np.int64)
        vals = scaled.astype(np.float64) * 2.0 ** -40  # exact: 53 bits
        rk, isum, rc = gpu.reduce_by_key64_reference(keys, scaled, U64, False, VI64, SUM)  # (runs of about 1050 values below 2^52: no wrap)
        _, imass, _ = gpu.reduce_by_key64_reference(keys, np.abs(scaled), U64, False, VI64, SUM)
        eps = 2.0 ** -53
    dk, dv = _dev(keys), _dev(vals)
    h = _handle(gpu, _vb(vt))
    second = gpu.ReduceByKey64(n, value_bytes=_vb(vt))
    outs = []
    for hh in (h, h, second):
        ok, ov, oc, num = hh.reduce_by_key(dk, dv, "sum", vt)
        hh.check()
        u = int(num.item())
        assert u == rk.size
        np.testing.assert_array_equal(_host(ok, u), rk)
        np.testing.assert_array_equal(_host(oc, u), rc)
        outs.append(_host(ov, u).copy())
    second.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    if vt == VF32:
        err = np.abs(outs[0].view(np.float32).astype(np.float64) - exact)
        bound = (rc.astype(np.float64) - 1) * eps * mass
        ok_ = err <= bound
    else:  # in integers of 2^-40: got is a multiple of 2^-40 as well (sums of such multiples, rounded to 53 bits above 2^12)
        got = [int(x * 2.0 ** 40) for x in outs[0].view(np.float64)]
        assert all(float(g) * 2.0 ** -40 == x for g, x in zip(got, outs[0].view(np.float64)))
        err = np.array([abs(g - int(s)) for g, s in zip(got, isum)], dtype=np.float64)
        bound = (rc.astype(np.float64) - 1) * eps * imass.astype(np.float64)
        ok_ = err <= bound
    print("general floats vt=%d: worst err / bound = %.3g" % (vt, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(ok_)


@pytest.mark.parametrize("vt", (VF32, VF64))
def test_a_run_of_one_returns_its_value_bit_for_bit(gpu, vt):
    """All keys distinct, values = any bit pattern, signalling and quiet NaNs with payloads among them: SUM, MIN and MAX each return the
    value itself."""
    n = 3 * TILE + 5
    rng = np.random.default_rng(5)
    u = np.uint32 if vt == VF32 else np.uint64
    vals = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
    special = (F32_ASCENDING if vt == VF32 else f64_ascending()).tolist()
    special += [0x7F800001, 0xFF80ABCD, 0x7FA00000] if vt == VF32 else [0x7FF0000000000001, 0xFFF000000000ABCD, 0x7FF4000000000000]
    vals[:len(special)] = special
    keys = draws64(n, 6, 0)
    order = np.argsort(keys, kind="stable")
    for op in (SUM, MIN, MAX):
        ok, ov, oc, num = _handle(gpu, _vb(vt)).reduce_by_key(_dev(keys), _dev(vals), op, vt)
        assert int(num.item()) == n
        np.testing.assert_array_equal(_host(ov), vals[order])
        ok, ov, oc, num = _handle(gpu, _vb(vt)).reduce_by_key_consecutive(_dev(keys), _dev(vals), op, vt)
        np.testing.assert_array_equal(_host(ov), vals)


# ---- guard arena ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,vt,op,fill", [("sorted", VI64, SUM, f) for f in FILLS] + [("consecutive", VF32, SUM, "hash"), ("consecutive", VU32, MAX, 0xFF),
                                                                                       ("sorted", VF32, MIN, 0x00)])
def test_outputs_on_a_guard_arena(gpu, entry, vt, op, fill):
    """n < max_keys, u < n, outputs at their capacity n: nothing at or behind u of out_keys (8-byte) / out_values / out_counts and nothing
    but the one word of d_out_num is written, the pointers are 16-byte aligned and no more, and the inputs are read only."""
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    n = 3 * TILE + 77
    keys, vals = draws64(n, 9, 50), _values(n, 10, vt)
    if entry == "consecutive":
        keys = np.sort(keys)[::-1].copy()
    rk, rv, rc = gpu.reduce_by_key64_reference(keys, vals, U64, True, vt, op, consecutive=entry == "consecutive")
    u = rk.size
    assert 1 < u < n
    vd = np.uint32 if _vb(vt) == 4 else np.uint64
    arena = Arena.for_views([(n, np.uint64), (n, vd), (n, np.uint64), (n, vd), (n, np.uint32), (4, np.uint32)], "cuda", fill)
    dk = arena.carve(n, np.uint64, 1, "keys")
    dv = arena.carve(n, vd, 3, "values")
    ok = arena.carve(n, np.uint64, 5, "out_keys")
    ov = arena.carve(n, vd, 7, "out_values")
    oc = arena.carve(n, np.uint32, 9, "out_counts")
    num = arena.carve(4, np.uint32, 11, "out_num")
    arena.write(dk, keys)
    arena.write(dv, _bits(vals, vt))
    for view in (ok, ov, oc):
        arena.live(view, u)
    arena.live(num, 1)
    h = _handle(gpu, _vb(vt), U64, True)
    if entry == "sorted":
        st = lib.gs_reduce64_by_key(h._h, dk.data_ptr(), dv.data_ptr(), n, ok.data_ptr(), ov.data_ptr(), oc.data_ptr(), num.data_ptr(), U64, 1, vt, op, None)
    else:
        st = lib.gs_reduce64_by_key_consecutive(h._h, dk.data_ptr(), dv.data_ptr(), n, ok.data_ptr(), ov.data_ptr(), oc.data_ptr(), num.data_ptr(), vt, op,
                                                None)
    assert st == _lib.GS_OK
    torch.cuda.synchronize()
    h.check()
    arena.verify()
    assert int(_host(num)[0]) == u and h.last()["u"] == u
    np.testing.assert_array_equal(_host(ok, u), rk)
    np.testing.assert_array_equal(_host(ov, u), _bits(rv, vt))
    np.testing.assert_array_equal(_host(oc, u), rc)


# ---- handle reuse --------------------------------------------------------------------------------------------------------------------
def test_handle_reuse_and_report(gpu):
    """A large call, a small one, the consecutive entry, other value types and ops on one handle: each call's report, and the check."""
    from gpusorting_amd import reduce64
    n = (1 << 20) + 1
    h = gpu.ReduceByKey64(n, value_bytes=8)
    rep = h.last()
    assert rep["route"] == NONE and rep["n"] == 0 and rep["u"] == 0 and h.status() == 0
    assert h.temp_bytes == reduce64.temp_bytes(n, 8) > 32 * n
    for keys, vt, op, entry in ((draws64(n, 70, 1000), VI64, SUM, "sorted"), (draws64(300, 71, 5), VF64, MAX, "sorted"),
                                (np.sort(draws64(70001, 73, 99)), VU64, MIN, "consecutive"), (draws64(n, 72, 0), VF64, SUM, "sorted"),
                                (draws64(2, 74, 0), VI64, MAX, "sorted")):
        _compare(gpu, h, keys, _values(keys.size, 75, vt), entry, U64, False, vt, op)
        assert h.last()["rank"] in (0, 1) and h.status() == 0
    with pytest.raises(gpu.GpuSortError):  # a 4-byte value type on the 8-byte handle
        h.reduce_by_key(_dev(draws64(64, 1, 3)), _dev(_values(64, 2, VI32)))
    assert h.last()["route"] == NONE
    h.close()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------
def test_captured_graph_replayed_on_new_data_with_another_u(gpu):
    """Both entries captured one after the other on one stream into one graph, replayed on new data."""
    from gpusorting_amd import _lib
    from gpusorting_amd.onesweep import _stream_ptr
    torch = _torch()
    lib = _lib.load()
    n = 100003
    hs, hc = gpu.ReduceByKey64(n, gpu.ORDER_DESCENDING, I64, 4), gpu.ReduceByKey64(n, value_bytes=8)
    dk, dv4, dv8 = _dev(draws64(n, 31, 500)), _dev(_values(n, 30, VF32)), _dev(_values(n, 30, VI64))
    ok, ok2, ov8 = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3))
    oc, oc2, ov4 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    num, num2 = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))

    def call():
        s = _stream_ptr()
        assert lib.gs_reduce64_by_key(hs._h, dk.data_ptr(), dv4.data_ptr(), n, ok.data_ptr(), ov4.data_ptr(), oc.data_ptr(), num.data_ptr(), I64, 1, VF32,
                                      SUM, s) == _lib.GS_OK
        assert lib.gs_reduce64_by_key_consecutive(hc._h, dk.data_ptr(), dv8.data_ptr(), n, ok2.data_ptr(), ov8.data_ptr(), oc2.data_ptr(), num2.data_ptr(),
                                                  VI64, SUM, s) == _lib.GS_OK

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    seen = set()
    for seed, distinct in ((32, 0), (33, 40), (34, 70000)):
        keys, v4, v8 = draws64(n, seed, distinct), _values(n, seed, VF32), _values(n, seed, VI64)
        dk.copy_(_dev(keys))
        dv4.copy_(_dev(v4))
        dv8.copy_(_dev(v8))
        for t in (ok, oc, ok2, oc2, ov4, ov8, num, num2):
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        hs.check()
        hc.check()
        rk, rv, rc = gpu.reduce_by_key64_reference(keys, v4, I64, True, VF32, SUM)
        u = int(num.item())
        assert u == rk.size == hs.last()["u"]
        seen.add(u)
        np.testing.assert_array_equal(_host(ok, u), rk)
        np.testing.assert_array_equal(_host(ov4, u), _bits(rv, VF32))
        np.testing.assert_array_equal(_host(oc, u), rc)
        assert u == n or bool((ok[u:] == -1).all() and (oc[u:] == -1).all() and (ov4[u:] == -1).all())
        rk, rv, rc = gpu.reduce_by_key64_reference(keys, v8, U64, False, VI64, SUM, consecutive=True)
        u2 = int(num2.item())
        assert u2 == rk.size == hc.last()["u"]
        np.testing.assert_array_equal(_host(ok2, u2), rk)
        np.testing.assert_array_equal(_host(ov8, u2), _bits(rv, VI64))
        np.testing.assert_array_equal(_host(oc2, u2), rc)
        assert u2 == n or bool((ok2[u2:] == -1).all() and (ov8[u2:] == -1).all())
    assert len(seen) == 3
    hs.close()
    hc.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    """The error table of the header, in its stated order."""
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    OK, A, S, M = _lib.GS_OK, _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    n = 10000
    bufs = [torch.full((4 * n + 64,), FILL, dtype=torch.int32, device="cuda") for _ in range(6)]  # (room for two 8-byte arrays)
    k, v, ok, ov, oc, num = (b.data_ptr() for b in bufs)
    h4, h8 = gpu.ReduceByKey64(n, value_bytes=4), gpu.ReduceByKey64(n, value_bytes=8)

    def srt(h, pk=k, pv=v, n_=n, pok=ok, pov=ov, poc=oc, pnum=num, kt=U64, order=0, vt=VI32, op=SUM):
        return lib.gs_reduce64_by_key(h._h if h else None, pk, pv, n_, pok, pov, poc, pnum, kt, order, vt, op, None)

    def con(h, pk=k, pv=v, n_=n, pok=ok, pov=ov, poc=oc, pnum=num, vt=VI32, op=SUM):
        return lib.gs_reduce64_by_key_consecutive(h._h if h else None, pk, pv, n_, pok, pov, poc, pnum, vt, op, None)

    # 1. GS_ERR_ARG: the null handle first of all
    assert srt(None, None, None, 0, None, None, kt=99, order=7, vt=99, op=99) == A and con(None, None, None, 0, None, None, vt=99, op=99) == A
    # 2. GS_ERR_ARG: the four required pointers, then key type and order, then value type and op — before the width and the sizes
    for call in (srt, con):
        for name, p in (("pk", k), ("pv", v), ("pok", ok), ("pov", ov)):
            assert call(h4, **{name: None}) == A and call(h4, **{name: p + 4}) == A and call(h4, **{name: p + 8}) == A, name
            assert call(h4, n_=0, vt=VI64, **{name: None}) == A  # (before the width and the size)
        for vt in (6, 7, -1, 99):
            assert call(h4, vt=vt) == A and call(h8, vt=vt, n_=0) == A
        for op in (3, -1, 99):
            assert call(h4, op=op) == A and call(h8, op=op, vt=VI64, n_=0) == A
    for kt in (0, 1, 2, 6, 7, 8, 9, 10, -1):  # the 32-bit and the 16-bit key types
        assert srt(h4, kt=kt) == A and srt(h8, kt=kt) == A and srt(h4, kt=kt, vt=VI64) == A, kt
    assert srt(h4, order=2) == A and srt(h8, order=-1, vt=VI64) == A and srt(h4, order=2, vt=VF64, n_=0) == A
    # 3. GS_ERR_MODE: a value type whose width is not the handle's, before the remaining pointers and the sizes
    for call in (srt, con):
        for vt in (VI64, VU64, VF64):
            assert call(h4, vt=vt) == M and call(h4, vt=vt, n_=0) == M and call(h4, vt=vt, poc=oc + 4) == M and call(h4, vt=vt, pok=k) == M
        for vt in (VI32, VU32, VF32):
            assert call(h8, vt=vt) == M and call(h8, vt=vt, n_=n + 1) == M and call(h8, vt=vt, pnum=num + 2) == M
    # 4. GS_ERR_ARG: the optional pointers, before the sizes
    for call in (srt, con):
        assert call(h4, poc=oc + 4, n_=0) == A and call(h4, poc=oc + 8) == A and call(h4, pnum=num + 2, n_=n + 1) == A and call(h4, pnum=num + 1) == A
    # 5. GS_ERR_SIZE: before the overlap test
    for call, h, vt in ((srt, h4, VF32), (con, h4, VU32), (srt, h8, VF64), (con, h8, VI64)):
        assert call(h, n_=0, vt=vt) == S and call(h, n_=n + 1, vt=vt) == S and call(h, n_=0, pok=k, vt=vt) == S and call(h, n_=n + 1, pov=v, vt=vt) == S
    # 6. GS_ERR_ARG: each overlapping pair; 8 n bytes for the keys and out_keys, n values, 4 n for the counts, one word at d_out_num
    m = 1000  # 4000 / 8000 bytes: multiples of 16
    for call, h, vt, vb in ((srt, h4, VI32, 4), (con, h4, VF32, 4), (srt, h8, VI64, 8), (con, h8, VF64, 8)):
        size = dict(pk=8 * m, pv=vb * m, pok=8 * m, pov=vb * m, poc=4 * m)
        names = tuple(size)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                base = dict(pk=k, pv=v, pok=ok, pov=ov, poc=oc)
                base[b] = base[a] + size[a] - 16
                assert call(h, n_=m, vt=vt, **base) == A, (a, b)
                base[b] = base[a] + size[a]
                assert call(h, n_=m, vt=vt, **base) == OK, (a, b)
            at = dict(pk=k, pv=v, pok=ok, pov=ov, poc=oc)[a]
            assert call(h, n_=m, vt=vt, pnum=at + size[a] - 4) == A and call(h, n_=m, vt=vt, pnum=at) == A, a
            assert call(h, n_=m, vt=vt, pnum=at + size[a]) == OK, a
    assert srt(h4, n_=m, pv=k + 4 * m) == A and srt(h4, n_=m, pov=ok + 4 * m) == A  # (what a check on 4 n bytes of keys would let through)
    # what may be NULL
    assert srt(h4, poc=None, pnum=None) == OK and con(h8, poc=None, pnum=None, vt=VF64) == OK
    assert srt(h4, n_=1) == OK and con(h4, n_=1) == OK and srt(h8, n_=1, vt=VU64, op=MAX) == OK
    torch.cuda.synchronize()
    assert h4.status() == 0 and h8.status() == 0
    # a refused call leaves the outputs untouched and route NONE, also behind a call that went through
    for b in bufs[2:]:
        b.fill_(FILL)
    half = 8 * (n + 32)
    assert srt(h4, n_=m, pok=ok + half, pov=ov + half, poc=oc + half) == OK and h4.last()["route"] == SORTED
    assert con(h8, n_=m, pok=ok + half, pov=ov + half, poc=oc + half, vt=VI64) == OK and h8.last()["route"] == CONSECUTIVE
    torch.cuda.synchronize()
    for refused in (srt(h4, n_=n + 1), srt(h4, kt=0), srt(h4, pok=k), srt(h4, vt=VI64), srt(h4, op=5), con(h4, pov=None), con(h4, poc=oc + 4)):
        assert refused != OK
    for refused in (con(h8, n_=0, vt=VI64), ):
        assert refused != OK
    assert h4.last()["route"] == NONE and h8.last()["route"] == NONE
    for b in bufs[2:5]:
        assert bool((b[:2 * n] == FILL).all()), "a refused call writes nothing"
    # the Python layer
    with pytest.raises(ValueError):
        gpu.ReduceByKey64(4096, key_type=gpu.KEY_UINT32)
    with pytest.raises(gpu.GpuSortError):
        gpu.ReduceByKey64(4096, value_bytes=2)
    with pytest.raises(ValueError):
        h4.reduce_by_key(torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        h4.reduce_by_key(torch.zeros(64, dtype=torch.int64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda"), "prod")
    h4.close()
    h8.close()


# ---- functional ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", ("int32", "int64"))
def test_functional_against_torch_unique_and_scatter(gpu, vdtype):
    """Integer data on int64 keys: torch.unique + index_add_ / scatter_reduce is the same statement."""
    torch = _torch()
    n = 3 * TILE + 11
    host = draws64(n, 81, 300)
    keys = _dev(host)
    vt = VI32 if vdtype == "int32" else VI64
    vals = _dev(_values(n, 82, vt))
    uk, inverse, cnt = torch.unique(keys, sorted=True, return_inverse=True, return_counts=True)
    for op, red in (("sum", None), ("min", "amin"), ("max", "amax")):
        want = torch.zeros(uk.numel(), dtype=vals.dtype, device="cuda")
        if red is None:
            want.index_add_(0, inverse, vals)
        else:
            want.scatter_reduce_(0, inverse, vals, red, include_self=False)
        gk, gv, gc = gpu.reduce_by_key64(keys, vals, op, return_counts=True)
        assert gk.dtype == keys.dtype and gv.dtype == vals.dtype and gc.dtype == torch.int32
        assert torch.equal(gk, uk) and torch.equal(gv, want) and torch.equal(gc.to(torch.int64), cnt)
        gk, gv = gpu.reduce_by_key64(keys, vals, op, descending=True)
        assert torch.equal(gk, uk.flip(0)) and torch.equal(gv, want.flip(0))
        sk, perm = torch.sort(keys, stable=True)  # consecutive on the sorted keys: the same groups
        ck, cv, cc = gpu.reduce_by_key_consecutive64(sk, vals[perm].contiguous(), op, return_counts=True)
        assert torch.equal(ck, uk) and torch.equal(cv, want) and torch.equal(cc.to(torch.int64), cnt)
    np.testing.assert_array_equal(_host(keys), host)  # not written


def test_functional_unsigned_floats_and_empty(gpu):
    torch = _torch()
    host = draws64(5000, 91, 64)  # patterns on both sides of the sign bit
    assert (host >> np.uint64(63)).any() and not (host >> np.uint64(63)).all()
    keys = _dev(host)
    v = _values(5000, 92, VF32)
    vals = torch.from_numpy(v).cuda()
    for descending in (False, True):
        rk, rv, rc = gpu.reduce_by_key64_reference(host, v, U64, descending, VF32, SUM)
        gk, gv, gc = gpu.reduce_by_key64(keys, vals, descending=descending, return_counts=True, unsigned=True)
        assert gv.dtype == torch.float32
        np.testing.assert_array_equal(_host(gk), rk)
        np.testing.assert_array_equal(_host(gv), _bits(rv, VF32))
        np.testing.assert_array_equal(_host(gc), rc)
    assert not np.array_equal(_host(gpu.reduce_by_key64(keys, vals)[0]), _host(gpu.reduce_by_key64(keys, vals, unsigned=True)[0]))
    fk = keys.view(torch.float64)  # float64 keys, float64 values, max by the total order
    v64 = _values(5000, 93, VF64)
    rk, rv, rc = gpu.reduce_by_key64_reference(host, v64, F64, False, VF64, MAX)
    gk, gv = gpu.reduce_by_key64(fk, torch.from_numpy(v64).cuda(), "max")
    assert gk.dtype == torch.float64 and gv.dtype == torch.float64
    np.testing.assert_array_equal(_host(gk), rk)
    np.testing.assert_array_equal(_host(gv), _bits(rv, VF64))
    for kd, vd in ((torch.int64, torch.float32), (torch.float64, torch.int64)):
        ek, ev = torch.empty(0, dtype=kd, device="cuda"), torch.empty(0, dtype=vd, device="cuda")
        for f in (gpu.reduce_by_key64, gpu.reduce_by_key_consecutive64):
            got = f(ek, ev, return_counts=True)
            assert len(got) == 3 and got[0].dtype == kd and got[1].dtype == vd and got[2].dtype == torch.int32 and all(g.numel() == 0 for g in got)
            assert len(f(ek, ev)) == 2
    with pytest.raises(TypeError, match="reduce_by_key64"):
        gpu.reduce_by_key64(torch.zeros(4, dtype=torch.int32, device="cuda"), vals[:4])
