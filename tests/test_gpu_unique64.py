"""GPU tests of unique / run-length encode on 64-bit keys (gs_unique64_* in include/gpusort.h, gpusorting_amd/unique64.py,
functional.unique64).  Every comparison is exact against unique64_reference (tests/test_unique64_cpu.py checks that one against numpy
and by hand).  Sizes come from gs_unique_plan (tile 4096, one range per tile up to 2^22 elements, two tiles per range behind) and from
the embedded sorter's single-workgroup edge for 8-byte keys (8192 with every value width), not from a workload.  What a stage on 8-byte
keys can get wrong and a 4-byte one cannot is the split of a key into two words: the word-split tests lay keys that differ in one word
only across every kind of edge."""
import numpy as np
import pytest

from guard_arena import FILLS, Arena
from test_unique64_cpu import F64_ASCENDING, draws64

pytestmark = pytest.mark.gpu

U64, I64, F64 = 3, 4, 5
NONE, KEYS, POSITIONS, CONSECUTIVE = 0, 1, 2, 3
TILE = 4096
MAXN = 513 * 2 * TILE + 1  # the largest size of the file: 514 ranges of two tiles, the last one holds one element
FILL = 0x5A5A5A5A
HI = np.uint64(1) << np.uint64(32)


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()


def _host(t, n=None):
    t = t if n is None else t[:n]
    return t.cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _handle(gpu, positions, kt=U64, descending=False):
    """One handle of capacity MAXN per (positions, key type, order) for the whole file: every test is a reuse of it as well."""
    key = (positions, kt, descending)
    if key not in _handles:
        _handles[key] = gpu.Unique64(MAXN, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, kt, positions=positions)
    return _handles[key]


def _compare(gpu, h, keys, entry, kt=U64, descending=False, counts=True, first=True, inverse=True):
    """Runs `entry` on the uint64 patterns `keys` and compares every delivered output with the reference; returns u."""
    n = keys.size
    rk, rc, rf, ri = gpu.unique64_reference(keys, kt, descending, consecutive=entry == "consecutive")
    d = _dev(keys)
    if entry == "keys":
        ok, oc, num = h.unique(d, counts=counts)
        of = oi = None
    elif entry == "positions":
        ok, oc, of, oi, num = h.unique_positions(d, counts=counts, first=first, inverse=inverse)
    else:
        ok, oc, oi, num = h.unique_consecutive(d, counts=counts, inverse=inverse)
        of = None
    h.check()
    u = int(num.item())
    assert u == rk.size, (entry, n, u, rk.size)
    rep = h.last()
    assert (rep["route"], rep["n"], rep["u"], rep["status"]) == ({"keys": KEYS, "positions": POSITIONS, "consecutive": CONSECUTIVE}[entry], n, u, 0)
    assert (rep["ranges"], rep["per_range"], rep["tile"]) == gpu.unique_plan(n)
    assert ok.element_size() == 8
    np.testing.assert_array_equal(_host(ok, u), rk)
    assert (oc is not None) == counts
    if oc is not None:
        np.testing.assert_array_equal(_host(oc, u), rc)
    if of is not None:
        np.testing.assert_array_equal(_host(of, u), rf)
    if oi is not None:
        np.testing.assert_array_equal(_host(oi), ri)
    np.testing.assert_array_equal(_host(d), keys)  # the input is not written
    return u


# ---- types and modes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U64, I64, F64))
@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("entry", ("keys", "positions", "only_inverse", "only_first"))
def test_types_and_modes(gpu, kt, descending, entry):
    keys = draws64(5000, 100 + kt, 37)  # 37 patterns spread over both words, on both sides of the sign bit
    if entry == "keys":
        for positions in (False, True):  # gs_unique64_keys works on either handle
            assert _compare(gpu, _handle(gpu, positions, kt, descending), keys, "keys", kt, descending) <= 37
    else:
        want = {"positions": (True, True, True), "only_inverse": (False, False, True), "only_first": (False, True, False)}[entry]
        _compare(gpu, _handle(gpu, True, kt, descending), keys, "positions", kt, descending, *want)


# ---- the word split ------------------------------------------------------------------------------------------------------------------
W_N = 2 * TILE + 1  # three ranges of one tile: the range edges are the tile edges 4096 and 8192
W_BASE = np.uint64(0x0123456789ABCDEF)


def _pool(kind):
    """Patterns that differ from one another only where `kind` says; as sorted neighbours a stage that compares one word merges them."""
    i = np.arange(24, dtype=np.uint64)
    if kind == "high_only":
        return W_BASE + i * HI
    if kind == "low_only":
        return W_BASE + i
    if kind == "pairs_high":  # (a, a + 2^32): neighbours in the sorted order wherever no other a lies between
        a = i * (HI << np.uint64(4)) + np.uint64(0x89ABCDEF)
        return np.concatenate([a, a + HI])
    a = i * (HI << np.uint64(4)) + np.uint64(0x89ABCDEE)  # pairs_low: (a, a + 1)
    return np.concatenate([a, a + np.uint64(1)])


@pytest.mark.parametrize("diff", (1, 1 << 32), ids=("low", "high"))
@pytest.mark.parametrize("at", (8, 512, TILE, 2 * TILE), ids=("thread", "wave", "tile", "range"))
def test_word_split_at_every_edge(gpu, at, diff):
    """The left neighbour of element `at` is the last key of another thread: at 8 it comes from the lane below through the shuffle (both
    words); at 512, 4096 and 8192 lane 0 of a wave reads it from memory, and it belongs to another wave, tile or workgroup (with three
    ranges of one tile every tile edge is a range edge; a tile edge inside a range is test_ranges_of_two_tiles').  A step there, a single
    key that differs, and the key in front of the edge, in one word only."""
    h = _handle(gpu, False)
    step = np.full(W_N, W_BASE, np.uint64)
    step[at:] += np.uint64(diff)
    assert _compare(gpu, h, step, "consecutive") == 2
    one = np.full(W_N, W_BASE, np.uint64)
    one[at] += np.uint64(diff)
    assert _compare(gpu, h, one, "consecutive") == (3 if at + 1 < W_N else 2)
    before = np.full(W_N, W_BASE, np.uint64)  # the key in front of the edge: the value a lane hands upwards
    before[at - 1] += np.uint64(diff)
    assert _compare(gpu, _handle(gpu, True), before, "consecutive") == 3


@pytest.mark.parametrize("kind", ("high_only", "low_only", "pairs_high", "pairs_low"))
def test_word_split_pools(gpu, kind):
    pool = _pool(kind)
    rng = np.random.default_rng(len(kind))
    laid = np.sort(pool[rng.integers(0, pool.size, W_N)])
    assert _compare(gpu, _handle(gpu, False), laid, "consecutive") == pool.size
    shuffled = laid.copy()
    rng.shuffle(shuffled)
    for descending in (False, True):
        assert _compare(gpu, _handle(gpu, False, U64, descending), shuffled, "keys", U64, descending) == pool.size
        assert _compare(gpu, _handle(gpu, True, U64, descending), shuffled, "positions", U64, descending) == pool.size


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
# a wave, a tile, per_range -+ 1 of plans with two and three ranges, the sorter's single-workgroup edge for 8-byte keys (8192) -+ 1,
# 2^20 + 1 and 2^22 + 5 (the first plan whose ranges are two tiles)
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, (1 << 20) + 1, (1 << 22) + 5)


def test_the_plans_the_sizes_rely_on(gpu):
    assert gpu.unique_plan(TILE) == (1, TILE, TILE) and gpu.unique_plan(TILE + 1) == (2, TILE, TILE)
    assert gpu.unique_plan(2 * TILE - 1) == (2, TILE, TILE) and gpu.unique_plan(W_N) == (3, TILE, TILE)
    assert gpu.unique_plan(1 << 22) == (1024, TILE, TILE) and gpu.unique_plan((1 << 22) + 5) == (513, 2 * TILE, TILE)
    assert gpu.unique_plan(MAXN - 2) == (513, 2 * TILE, TILE) and gpu.unique_plan(MAXN) == (514, 2 * TILE, TILE)


@pytest.mark.parametrize("entry,n", [(e, n) for e in ("keys", "positions") for n in SIZES])
def test_sizes(gpu, entry, n):
    h = _handle(gpu, entry == "positions")
    few = draws64(n, n, 7)
    assert _compare(gpu, h, few, entry) == np.unique(few).size <= 7
    assert _compare(gpu, h, draws64(n, n + 1, 0), entry) == n


@pytest.mark.parametrize("word", ("low", "high"))
@pytest.mark.parametrize("n", ((1 << 22) + 1, MAXN - 2, MAXN))
def test_ranges_of_two_tiles(gpu, n, word):
    """per_range -+ 1 and a last range of one element where a range is two tiles, through the run-length stage's own entry: runs of
    three across every edge, and runs of 2 * TILE + 1 that leave whole tiles and ranges without a head; the run's number in one word."""
    h = _handle(gpu, False)
    shift = np.uint64(32 if word == "high" else 0)
    for run in (3, 2 * TILE + 1):
        keys = ((np.arange(n, dtype=np.uint64) // np.uint64(run)) << shift) + (W_BASE & np.uint64(0xFFFFFFFF) if word == "high" else W_BASE & ~(HI - np.uint64(1)))
        assert _compare(gpu, h, keys, "consecutive") == -(-n // run)


# ---- agreement with the 32-bit family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", (False, True))
def test_zero_extended_keys_agree_with_the_32_bit_family(gpu, descending):
    n = (1 << 20) + 1
    rng = np.random.default_rng(64)
    k32 = rng.integers(0, 1 << 32, 50000).astype(np.uint32)[rng.integers(0, 50000, n)]
    order = gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING
    h32 = gpu.Unique(n, order, gpu.KEY_UINT32, positions=True)
    ok, oc, of, oi, num = h32.unique_positions(_dev(k32))
    h32.check()
    u = int(num.item())
    h64 = _handle(gpu, True, U64, descending)
    qk, qc, qf, qi, qnum = h64.unique_positions(_dev(k32.astype(np.uint64)))
    h64.check()
    assert int(qnum.item()) == u
    np.testing.assert_array_equal(_host(qk, u), _host(ok, u).astype(np.uint64))
    np.testing.assert_array_equal(_host(qc, u), _host(oc, u))
    np.testing.assert_array_equal(_host(qf, u), _host(of, u))
    np.testing.assert_array_equal(_host(qi), _host(oi))
    h32.close()


# ---- guard arena ---------------------------------------------------------------------------------------------------------------------
def _raw(lib, h, entry, stream, n, pk, pok, poc, pof, poi, pnum, kt=U64, order=0):
    if entry == "keys":
        return lib.gs_unique64_keys(h._h if h else None, pk, n, pok, poc, pnum, kt, order, stream)
    if entry == "positions":
        return lib.gs_unique64_positions(h._h if h else None, pk, n, pok, poc, pof, poi, pnum, kt, order, stream)
    return lib.gs_unique64_consecutive(h._h if h else None, pk, n, pok, poc, poi, pnum, stream)


@pytest.mark.parametrize("entry,fill", [("positions", f) for f in FILLS] + [("keys", "hash"), ("consecutive", "hash"), ("consecutive", 0xFF)])
def test_outputs_on_a_guard_arena(gpu, entry, fill):
    """n < max_keys, u < n: nothing outside [0, u) of out_keys (8-byte) / out_counts / out_first, [0, n) of out_inverse and the one word
    of d_out_num is written, the pointers are 16-byte aligned and no more, and the input is read only."""
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    n, cap = 3 * TILE + 77, 3 * TILE + 77 + 300
    keys = draws64(n, 9, 50)
    if entry == "consecutive":
        keys = np.sort(keys)[::-1].copy()
    rk, rc, rf, ri = gpu.unique64_reference(keys, U64, True, consecutive=entry == "consecutive")
    u = rk.size
    assert 1 < u < n
    arena = Arena.for_views([(cap, np.uint64)] * 2 + [(cap, np.uint32)] * 3 + [(4, np.uint32)], "cuda", fill)
    dk, ok = arena.carve(cap, np.uint64, 1, "keys"), arena.carve(cap, np.uint64, 3, "out_keys")
    oc, of, oi = (arena.carve(cap, np.uint32, skew, name) for skew, name in ((5, "out_counts"), (7, "out_first"), (9, "out_inverse")))
    num = arena.carve(4, np.uint32, 11, "out_num")
    arena.write(dk, keys)
    arena.live(ok, u)
    arena.live(num, 1)
    arena.live(oc, u)
    if entry == "positions":
        arena.live(of, u)
    if entry != "keys":
        arena.live(oi, n)
    h = _handle(gpu, True, U64, True)
    st = _raw(lib, h, entry, None, n, dk.data_ptr(), ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), U64, 1)
    assert st == _lib.GS_OK
    torch.cuda.synchronize()
    h.check()
    arena.verify()
    assert int(_host(num)[0]) == u and h.last()["u"] == u
    np.testing.assert_array_equal(_host(ok, u), rk)
    np.testing.assert_array_equal(_host(oc, u), rc)
    if entry == "positions":
        np.testing.assert_array_equal(_host(of, u), rf)
    if entry != "keys":
        np.testing.assert_array_equal(_host(oi, n), ri)


# ---- handle reuse --------------------------------------------------------------------------------------------------------------------
def test_handle_reuse_and_report(gpu):
    """A large call, a small one, then the consecutive entry on one handle: each call's report, and the check."""
    import importlib
    unique64 = importlib.import_module("gpusorting_amd.unique64")  # (the package attribute of that name is the function)
    n = (1 << 20) + 1
    h = gpu.Unique64(n, positions=True)
    assert h.last()["route"] == NONE and h.status() == 0
    assert h.temp_bytes == unique64.temp_bytes(n, gpu.MODE_PAIRS, 4) > 24 * n  # two 8-byte key buffers, two of positions
    for keys, entry in ((draws64(n, 70, 1000), "positions"), (draws64(300, 71, 5), "positions"), (draws64(n, 72, 0), "keys"),
                        (np.sort(draws64(70001, 73, 99)), "consecutive"), (draws64(2, 74, 0), "keys")):
        _compare(gpu, h, keys, entry)  # (route, n, u and the plan are compared there)
        assert h.last()["rank"] in (0, 1) and h.status() == 0
    h.close()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("keys", "positions"))
def test_captured_graph_replayed_on_new_data_with_another_u(gpu, entry):
    from gpusorting_amd import _lib
    from gpusorting_amd.onesweep import _stream_ptr
    torch = _torch()
    lib = _lib.load()
    n = 100003
    h = gpu.Unique64(n, gpu.ORDER_DESCENDING, I64, positions=entry == "positions")
    dk = _dev(draws64(n, 31, 500))
    ok = torch.empty(n, dtype=torch.int64, device="cuda")
    oc, of, oi = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    num = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        st = _raw(lib, h, entry, _stream_ptr(), n, dk.data_ptr(), ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), I64, 1)
        assert st == _lib.GS_OK

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
        keys = draws64(n, seed, distinct)
        dk.copy_(_dev(keys))
        for t in (ok, oc, of, oi, num):
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rc, rf, ri = gpu.unique64_reference(keys, I64, True)
        u = int(num.item())
        assert u == rk.size == h.last()["u"]
        seen.add(u)
        np.testing.assert_array_equal(_host(ok, u), rk)
        np.testing.assert_array_equal(_host(oc, u), rc)
        assert u == n or bool((ok[u:] == -1).all() and (oc[u:] == -1).all())
        if entry == "positions":
            np.testing.assert_array_equal(_host(of, u), rf)
            np.testing.assert_array_equal(_host(oi), ri)
    assert len(seen) == 3
    h.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    OK, A, S, M = _lib.GS_OK, _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    n = 10000
    wide = [torch.full((n + 64,), FILL, dtype=torch.int64, device="cuda") for _ in range(2)]
    narrow = [torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda") for _ in range(4)]
    k, ok = (b.data_ptr() for b in wide)
    oc, of, oi, num = (b.data_ptr() for b in narrow)
    hk, hp = gpu.Unique64(n), gpu.Unique64(n, positions=True)

    def keys(h, pk=k, n_=n, pok=ok, poc=oc, pnum=num, kt=U64, order=0):
        return lib.gs_unique64_keys(h._h if h else None, pk, n_, pok, poc, pnum, kt, order, None)

    def pos(h, pk=k, n_=n, pok=ok, poc=oc, pof=of, poi=oi, pnum=num, kt=U64, order=0):
        return lib.gs_unique64_positions(h._h if h else None, pk, n_, pok, poc, pof, poi, pnum, kt, order, None)

    def con(h, pk=k, n_=n, pok=ok, poc=oc, poi=oi, pnum=num):
        return lib.gs_unique64_consecutive(h._h if h else None, pk, n_, pok, poc, poi, pnum, None)

    # 1. GS_ERR_ARG: the null handle first of all; d_keys, d_out_keys, key type, order — before the mode and the sizes
    assert keys(None, None, 0, None, kt=99, order=7) == A and pos(None, None, 0, None, kt=99, order=7) == A and con(None, None, 0, None) == A
    for call in (keys, pos, con):
        h = hp
        assert call(h, None) == A and call(h, pok=None) == A and call(h, k + 8) == A and call(h, pok=ok + 8) == A
        assert call(h, None, 0) == A  # (before the size)
    for kt in (0, 1, 2, 6, 7, 8, 9, 10, -1):  # the 32-bit and the 16-bit key types
        assert keys(hk, kt=kt) == A and keys(hp, kt=kt) == A and pos(hp, kt=kt) == A and pos(hk, kt=kt) == A, kt
    assert keys(hk, order=2) == A and pos(hp, order=-1) == A and pos(hk, order=2) == A
    # 2. GS_ERR_MODE: gs_unique64_positions on a keys-only handle, before the remaining pointers and the sizes
    assert pos(hk) == M and pos(hk, n_=0) == M and pos(hk, poc=oc + 4) == M and pos(hk, pok=k) == M
    assert pos(hk, poc=None, pof=None, poi=None, pnum=None) == M
    # 3. GS_ERR_ARG: the remaining pointers, before the sizes
    assert keys(hk, poc=oc + 4, n_=0) == A and keys(hk, pnum=num + 2) == A and pos(hp, pof=of + 8, n_=0) == A and pos(hp, poi=oi + 4) == A
    assert con(hk, poi=oi + 12, n_=0) == A and con(hp, poc=oc + 2) == A
    # 4. GS_ERR_SIZE: before the overlap test
    for call, h in ((keys, hk), (keys, hp), (pos, hp), (con, hk), (con, hp)):
        assert call(h, n_=0) == S and call(h, n_=n + 1) == S and call(h, n_=0, pok=k) == S and call(h, n_=n + 1, pok=k) == S
    # 5. GS_ERR_ARG: each overlapping pair; 8 n bytes for the keys and out_keys, 4 n for the rest, one word at d_out_num; touching is fine
    m = 1000
    assert keys(hk, n_=m, pok=k + 8 * m) == OK and keys(hk, n_=m, pok=k + 8 * m - 16) == A and keys(hk, n_=m, pok=k) == A
    assert keys(hk, n_=m, pok=k + 4 * m) == A  # (what a check on 4 n bytes would let through)
    assert keys(hk, n_=m, poc=k) == A and keys(hk, n_=m, poc=ok + 8 * m - 16) == A and keys(hk, n_=m, poc=ok + 8 * m) == OK
    assert keys(hk, n_=m, poc=k + 8 * m - 4 * m) == A and keys(hk, n_=m, pok=oc + 4 * m) == OK and keys(hk, n_=m, pok=oc + 4 * m - 16) == A
    assert keys(hk, n_=m, pnum=k + 8 * m - 4) == A and keys(hk, n_=m, pnum=ok) == A and keys(hk, n_=m, pnum=oc + 4 * m - 4) == A
    assert keys(hk, n_=m, pnum=k + 8 * m) == OK
    names = ("pk", "pok", "poc", "pof", "poi")
    width = dict(pk=8, pok=8, poc=4, pof=4, poi=4)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            base = dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)
            base[b] = base[a] + width[a] * m - 16
            assert pos(hp, n_=m, **base) == A, (a, b)
            base[b] = base[a] + width[a] * m
            assert pos(hp, n_=m, **base) == OK, (a, b)
        assert pos(hp, n_=m, pnum=dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)[a] + width[a] * m - 4) == A, a
    assert con(hk, n_=m, poi=k) == A and con(hk, n_=m, poi=ok + 16) == A and con(hk, n_=m, poc=oi) == A and con(hk, n_=m, poi=k + 8 * m) == OK
    # what may be NULL
    assert keys(hk, poc=None, pnum=None) == OK and pos(hp, poc=None, pof=None, poi=None, pnum=None) == OK and con(hp, poc=None, poi=None, pnum=None) == OK
    assert keys(hk, n_=1) == OK and pos(hp, n_=1) == OK and con(hk, n_=1) == OK
    torch.cuda.synchronize()
    assert hk.status() == 0 and hp.status() == 0
    # a refused call leaves the outputs untouched and route NONE, also behind a call that went through
    for b in wide[1:] + narrow:
        b.fill_(FILL)
    half8, half4 = 8 * (n // 2 + 32), 4 * (n // 2 + 32)
    assert keys(hk, n_=m, pok=ok + half8, poc=oc + half4) == OK and hk.last()["route"] == KEYS
    assert pos(hp, n_=m, pok=ok + half8, poc=oc + half4, pof=of + half4, poi=oi + half4) == OK and hp.last()["route"] == POSITIONS
    torch.cuda.synchronize()
    for refused in (keys(hk, n_=n + 1), keys(hk, kt=0), keys(hk, pok=k), pos(hk), pos(hp, poi=oi + 4), pos(hp, n_=0), con(hp, pok=None)):
        assert refused != OK
    assert hk.last()["route"] == NONE and hp.last()["route"] == NONE
    for b in wide[1:] + narrow[:3]:
        assert bool((b[:n // 2] == FILL).all()), "a refused call writes nothing"
    # the Python layer
    with pytest.raises(ValueError):
        gpu.Unique64(4096, key_type=gpu.KEY_UINT32)
    with pytest.raises(ValueError):
        hk.unique(torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(gpu.GpuSortError):
        hk.unique_positions(torch.zeros(64, dtype=torch.int64, device="cuda"))
    hk.close()
    hp.close()


# ---- functional ----------------------------------------------------------------------------------------------------------------------
FLAGS = [(i, c, x) for i in (False, True) for c in (False, True) for x in (False, True)]


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


@pytest.mark.parametrize("dtype_name", ("int64", "float64"))
def test_functional_unique64(gpu, dtype_name):
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    n = 3 * TILE + 11
    rng = np.random.default_rng(82)
    if dtype_name == "int64":
        host = draws64(n, 81, 300)
        kt = I64
    else:  # the fourteen special patterns, each many times, in a shuffled order
        host = F64_ASCENDING[rng.integers(0, F64_ASCENDING.size, n)]
        kt = F64
    t = _dev(host).view(dtype)
    for descending in (False, True):
        rk, rc, rf, ri = gpu.unique64_reference(host, kt, descending)
        if dtype_name == "float64":
            assert rk.tolist() == (F64_ASCENDING[::-1] if descending else F64_ASCENDING).tolist()  # -0.0 in front of +0.0, NaNs by their bits
        for inv, cnt, idx in FLAGS:
            got = _tuple(gpu.unique64(t, return_inverse=inv, return_counts=cnt, return_index=idx, descending=descending))
            assert len(got) == 1 + inv + cnt + idx and got[0].dtype == dtype and all(g.dtype == torch.int32 for g in got[1:])
            expect = [rk] + ([ri] if inv else []) + ([rc] if cnt else []) + ([rf] if idx else [])
            for g, e in zip(got, expect):
                assert g.shape == e.shape
                np.testing.assert_array_equal(_host(g), e)
            if dtype_name == "int64" and not descending and not idx:  # torch.unique on integers is the same statement
                want = _tuple(torch.unique(t, sorted=True, return_inverse=inv, return_counts=cnt))
                for g, w in zip(got, want):
                    assert torch.equal(g.to(torch.int64), w.to(torch.int64))
    # consecutive
    runs = np.sort(host) if dtype_name == "int64" else host
    tr = _dev(runs).view(dtype)
    rk, rc, rf, ri = gpu.unique64_reference(runs, consecutive=True)
    for inv, cnt in ((False, False), (True, False), (False, True), (True, True)):
        got = _tuple(gpu.unique_consecutive64(tr, return_inverse=inv, return_counts=cnt))
        expect = [rk] + ([ri] if inv else []) + ([rc] if cnt else [])
        assert len(got) == len(expect) and got[0].dtype == dtype
        for g, e in zip(got, expect):
            np.testing.assert_array_equal(_host(g), e)
        if dtype_name == "int64":
            want = _tuple(torch.unique_consecutive(tr, return_inverse=inv, return_counts=cnt))
            for g, w in zip(got, want):
                assert torch.equal(g.to(torch.int64), w.to(torch.int64))
    np.testing.assert_array_equal(_host(t.view(torch.int64)), host)  # not written


def test_functional_unique64_unsigned_and_empty(gpu):
    torch = _torch()
    host = draws64(5000, 91, 64)  # patterns on both sides of the sign bit
    assert (host >> np.uint64(63)).any() and not (host >> np.uint64(63)).all()
    t = _dev(host)
    for descending in (False, True):
        rk, rc, rf, ri = gpu.unique64_reference(host, U64, descending)
        ok, oi, oc, of = gpu.unique64(t, True, True, True, descending=descending, unsigned=True)
        for g, e in ((ok, rk), (oi, ri), (oc, rc), (of, rf)):
            np.testing.assert_array_equal(_host(g), e)
    assert not np.array_equal(_host(gpu.unique64(t)), _host(gpu.unique64(t, unsigned=True)))
    if hasattr(torch, "uint64"):
        np.testing.assert_array_equal(_host(gpu.unique64(t.view(torch.uint64)).view(torch.int64)), gpu.unique64_reference(host, U64)[0])
    for dtype in (torch.int64, torch.float64):
        e = torch.empty(0, dtype=dtype, device="cuda")
        got = gpu.unique64(e, True, True, True)
        assert len(got) == 4 and got[0].dtype == dtype and all(g.numel() == 0 for g in got) and all(g.dtype == torch.int32 for g in got[1:])
        got = gpu.unique_consecutive64(e, True, True)
        assert len(got) == 3 and all(g.numel() == 0 for g in got)
        assert gpu.unique64(e).numel() == 0 and gpu.unique_consecutive64(e).numel() == 0
    with pytest.raises(TypeError, match="unique64"):
        gpu.unique64(torch.zeros(4, dtype=torch.int32, device="cuda"))
