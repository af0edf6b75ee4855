"""GPU tests of unique / run-length encode (gs_unique_* in include/gpusort.h, gpusorting_amd/unique.py, functional.unique).  Every
comparison is exact against unique_reference (tests/test_unique_cpu.py checks that one against numpy and by hand).  Sizes come from
gs_unique_plan (tile 4096, one range per tile up to 2^22 elements, two tiles per range behind) and from the embedded sorter's route
edges, not from a workload."""
import numpy as np
import pytest

from guard_arena import FILLS, Arena
from test_unique_cpu import F32_ASCENDING, float_special_case

pytestmark = pytest.mark.gpu

U32, I32, F32 = 0, 1, 2
NONE, KEYS, POSITIONS, CONSECUTIVE = 0, 1, 2, 3
TILE = 4096
MAXN = 513 * 2 * TILE + 1  # the largest size of the file: 514 ranges of two tiles, the last one holds one element
FILL = 0x5A5A5A5A


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _host(t, n=None):
    return (t if n is None else t[:n]).cpu().numpy().view(np.uint32)


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _handle(gpu, positions, kt=U32, descending=False):
    """One handle of capacity MAXN per (positions, key type, order) for the whole file: every test is a reuse of it as well."""
    key = (positions, kt, descending)
    if key not in _handles:
        _handles[key] = gpu.Unique(MAXN, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, kt, positions=positions)
    return _handles[key]


def _compare(gpu, h, keys, entry, kt=U32, descending=False, counts=True, first=True, inverse=True):
    """Runs `entry` on the uint32 patterns `keys` and compares every delivered output with the reference; returns u."""
    n = keys.size
    rk, rc, rf, ri = gpu.unique_reference(keys, kt, descending, consecutive=entry == "consecutive")
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


def _draws(n, seed, distinct, kt=U32):
    """n draws from `distinct` random 32-bit patterns (floats: no care taken, any pattern is a key); distinct == 0: all different."""
    rng = np.random.default_rng(seed)
    if distinct == 0:
        return (rng.permutation(n).astype(np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)  # (an odd multiplier: a bijection)
    pool = rng.integers(0, 1 << 32, distinct).astype(np.uint32)
    return pool[rng.integers(0, distinct, n)]


# ---- types and modes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U32, I32, F32))
@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("entry", ("keys", "positions", "only_inverse", "only_first"))
def test_types_and_modes(gpu, kt, descending, entry):
    keys = _draws(5000, 100 + kt, 37, kt)
    if entry == "keys":
        for positions in (False, True):  # gs_unique_keys works on either handle
            assert _compare(gpu, _handle(gpu, positions, kt, descending), keys, "keys", kt, descending) <= 37
    else:
        want = {"positions": (True, True, True), "only_inverse": (False, False, True), "only_first": (False, True, False)}[entry]
        _compare(gpu, _handle(gpu, True, kt, descending), keys, "positions", kt, descending, *want)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def _sizes(entry):
    """The run-length stage's edges (a wave, a tile, per_range -+ 1 of plans with two and three ranges), the sorter's single-tile edge
    for the entry, 2^20 + 1 and one size above the sorter's mid route."""
    edge = (32768, 32769, (1 << 20) + 1, (1 << 21) + 3) if entry == "keys" else (16384, 16385, (1 << 20) + 1, (1 << 22) + 5)
    return (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1) + edge


def test_the_plans_the_sizes_rely_on(gpu):
    assert gpu.unique_plan(TILE) == (1, TILE, TILE) and gpu.unique_plan(TILE + 1) == (2, TILE, TILE)
    assert gpu.unique_plan(2 * TILE - 1) == (2, TILE, TILE) and gpu.unique_plan(2 * TILE + 1) == (3, TILE, TILE)
    assert gpu.unique_plan(1 << 22) == (1024, TILE, TILE) and gpu.unique_plan((1 << 22) + 5) == (513, 2 * TILE, TILE)
    assert gpu.unique_plan(MAXN - 2) == (513, 2 * TILE, TILE) and gpu.unique_plan(MAXN) == (514, 2 * TILE, TILE)


@pytest.mark.parametrize("n", ((1 << 22) + 1, MAXN - 2, MAXN))
def test_ranges_of_two_tiles(gpu, n):
    """per_range -+ 1 and a last range of one element where a range is two tiles, through the run-length stage's own entry (its
    reference needs no sort): runs of three across every edge, and runs of 2 * TILE + 1 that leave whole tiles and ranges without a head."""
    h = _handle(gpu, False)
    assert _compare(gpu, h, np.arange(n, dtype=np.uint32) // 3, "consecutive") == -(-n // 3)
    assert _compare(gpu, h, np.arange(n, dtype=np.uint32) // (2 * TILE + 1), "consecutive") == -(-n // (2 * TILE + 1))


@pytest.mark.parametrize("entry,n", [(e, n) for e in ("keys", "positions") for n in _sizes(e)])
def test_sizes(gpu, entry, n):
    h = _handle(gpu, entry == "positions")
    few = _draws(n, n, 7)
    assert _compare(gpu, h, few, entry) == min(7, np.unique(few).size)
    assert _compare(gpu, h, _draws(n, n + 1, 0), entry) == n


def test_two_values_among_2_27_keys(gpu):
    """The size at which it shows: the keys-only sorter's position-chain plan left a few keys of such an input out of order in one
    run of four (every one a run of its own: u = 3 .. 5 instead of 2), so the handle's sorter does not take it.  Eight calls; the
    expectation is written by hand from the draws (two values, how often each was drawn)."""
    torch = _torch()
    n = 1 << 27
    gen = torch.Generator(device="cuda")
    gen.manual_seed(27)
    which = torch.randint(0, 2, (n,), device="cuda", generator=gen, dtype=torch.int8)
    ones = int(which.sum(dtype=torch.int64).item())
    lo, hi = 0x277B4B58, 0x3E121E97
    keys = torch.where(which != 0, hi, lo).to(torch.int32)
    del which
    h = gpu.Unique(n)
    for _ in range(8):
        ok, oc, num = h.unique(keys)
        assert int(num.item()) == 2
        assert _host(ok, 2).tolist() == [lo, hi] and _host(oc, 2).tolist() == [n - ones, ones]
    h.check()
    h.close()


# ---- structure -----------------------------------------------------------------------------------------------------------------------
S_N = 5 * TILE + 100  # six ranges of one tile each
S_NAMES = ("all_equal", "all_distinct", "straddle", "two_ranges_exact", "two_ranges_headless", "tile_edges", "alternating", "last_differs",
           "first_differs", "float_specials")


def _laid(name):
    """Sorted (ascending, unsigned) input laid by hand, except `alternating`; float_specials: ascending by the float order."""
    n, per = S_N, TILE
    s = np.arange(n, dtype=np.uint32) * 2 + 1
    if name == "all_equal":
        s[:] = 7
    elif name == "straddle":  # one run: the last element of range 1 and the first of range 2
        s[2 * per] = s[2 * per - 1]
    elif name == "two_ranges_exact":  # [per, 3 per): its head is the first element of range 1, range 2 holds none
        s[per:3 * per] = s[per]
    elif name == "two_ranges_headless":  # it starts on the last element of range 0: ranges 1 and 2 hold no head
        s[per - 1:3 * per] = s[per - 1]
    elif name == "tile_edges":
        s = (np.arange(n, dtype=np.uint32) // TILE) * 5
    elif name == "alternating":
        s = np.where(np.arange(n) % 2 == 0, 11, 4).astype(np.uint32)
    elif name == "last_differs":
        s[:] = 3
        s[-1] = 4
    elif name == "first_differs":
        s[:] = 3
        s[0] = 2
    elif name == "float_specials":
        copies = np.full(F32_ASCENDING.size, n // F32_ASCENDING.size)
        copies[7] += n - copies.sum()
        s = np.repeat(F32_ASCENDING, copies)
    assert s.size == n
    return s


@pytest.mark.parametrize("name", S_NAMES)
def test_structure_consecutive(gpu, name):
    s = _laid(name)
    u = _compare(gpu, _handle(gpu, False), s, "consecutive")
    expect = {"all_equal": 1, "all_distinct": S_N, "straddle": S_N - 1, "two_ranges_exact": S_N - 2 * TILE + 1,
              "two_ranges_headless": S_N - 2 * TILE, "tile_edges": 6, "alternating": S_N, "last_differs": 2, "first_differs": 2,
              "float_specials": F32_ASCENDING.size}[name]
    assert u == expect
    _compare(gpu, _handle(gpu, True), s, "consecutive", counts=False)  # either handle; only the inverse


@pytest.mark.parametrize("name", S_NAMES)
@pytest.mark.parametrize("descending", (False, True))
def test_structure_positions_on_a_shuffled_copy(gpu, name, descending):
    s = _laid(name)
    np.random.default_rng(17).shuffle(s)
    kt = F32 if name == "float_specials" else U32
    _compare(gpu, _handle(gpu, True, kt, descending), s, "positions", kt, descending)


# ---- descending first ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", (False, True))
def test_first_is_the_lowest_position_in_both_orders(gpu, descending):
    """Known positions, no reference: value v lies at v + 40 * j, j = 0 .. ; a second array with long runs across tiles."""
    small = np.tile(np.arange(40, dtype=np.uint32), 300)
    large = _draws(3 * TILE + 5, 5, 3)
    for keys in (small, large):
        ok, oc, of, oi, num = _handle(gpu, True, U32, descending).unique_positions(_dev(keys))
        u = int(num.item())
        got_keys, got_first = _host(ok, u), _host(of, u)
        for k, f in zip(got_keys.tolist(), got_first.tolist()):
            assert f == int(np.flatnonzero(keys == k)[0]), (k, f)
    ok, oc, of, oi, num = _handle(gpu, True, U32, descending).unique_positions(_dev(small))
    assert _host(of, 40).tolist() == (list(range(39, -1, -1)) if descending else list(range(40)))


# ---- guard arena ---------------------------------------------------------------------------------------------------------------------
def _raw(lib, h, entry, stream, n, pk, pok, poc, pof, poi, pnum, kt=U32, order=0):
    if entry == "keys":
        return lib.gs_unique_keys(h._h if h else None, pk, n, pok, poc, pnum, kt, order, stream)
    if entry == "positions":
        return lib.gs_unique_positions(h._h if h else None, pk, n, pok, poc, pof, poi, pnum, kt, order, stream)
    return lib.gs_unique_consecutive(h._h if h else None, pk, n, pok, poc, poi, pnum, stream)


@pytest.mark.parametrize("entry,fill", [("positions", f) for f in FILLS] + [("keys", "hash"), ("consecutive", "hash"), ("consecutive", 0xFF)])
def test_outputs_on_a_guard_arena(gpu, entry, fill):
    """n < max_keys, u < n: nothing outside [0, u) of out_keys / out_counts / out_first, [0, n) of out_inverse and the one word of
    d_out_num is written, the pointers are 16-byte aligned and no more, and the input is read only."""
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    n, cap = 3 * TILE + 77, 3 * TILE + 77 + 300
    keys = _draws(n, 9, 50)
    if entry == "consecutive":
        keys = np.sort(keys)[::-1].copy()
    rk, rc, rf, ri = gpu.unique_reference(keys, U32, True, consecutive=entry == "consecutive")
    u = rk.size
    assert 1 < u < n
    arena = Arena.for_views([(cap, np.uint32)] * 5 + [(4, np.uint32)], "cuda", fill)
    dk, ok, oc, of, oi = (arena.carve(cap, np.uint32, skew, name) for skew, name in ((1, "keys"), (3, "out_keys"), (5, "out_counts"), (7, "out_first"),
                                                                                     (9, "out_inverse")))
    num = arena.carve(4, np.uint32, 11, "out_num")
    arena.write(dk, keys)
    arena.live(ok, u)
    arena.live(num, 1)
    arena.live(oc, u)
    if entry == "positions":
        arena.live(of, u)
    if entry != "keys":
        arena.live(oi, n)
    h = _handle(gpu, True, U32, True)
    st = _raw(lib, h, entry, None, n, dk.data_ptr(), ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), U32, 1)
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
        np.testing.assert_array_equal(_host(oi, n), ri)  # all n entries: the ranks are below u, the 0xFF and hash fills are not


# ---- handle reuse --------------------------------------------------------------------------------------------------------------------
def test_handle_reuse_and_report(gpu):
    """A large call, a small one, then the consecutive entry on one handle: each call's report, and the check."""
    h = gpu.Unique((1 << 20) + 1, positions=True)
    assert h.last()["route"] == NONE and h.status() == 0 and h.temp_bytes > 16 << 20
    for keys, entry in ((_draws((1 << 20) + 1, 70, 1000), "positions"), (_draws(300, 71, 5), "positions"), (_draws((1 << 20) + 1, 72, 0), "keys"),
                        (np.sort(_draws(70001, 73, 99)), "consecutive"), (_draws(2, 74, 0), "keys")):
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
    h = gpu.Unique(n, gpu.ORDER_DESCENDING, I32, positions=entry == "positions")
    dk = _dev(_draws(n, 31, 500))
    ok, oc, of, oi = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4))
    num = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        st = _raw(lib, h, entry, _stream_ptr(), n, dk.data_ptr(), ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), I32, 1)
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
        keys = _draws(n, seed, distinct)
        dk.copy_(_dev(keys))
        for t in (ok, oc, of, oi, num):
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rc, rf, ri = gpu.unique_reference(keys, I32, True)
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
    bufs = [torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda") for _ in range(6)]
    k, ok, oc, of, oi, num = (b.data_ptr() for b in bufs)
    hk, hp = gpu.Unique(n), gpu.Unique(n, positions=True)

    def keys(h, pk=k, n_=n, pok=ok, poc=oc, pnum=num, kt=U32, order=0):
        return lib.gs_unique_keys(h._h if h else None, pk, n_, pok, poc, pnum, kt, order, None)

    def pos(h, pk=k, n_=n, pok=ok, poc=oc, pof=of, poi=oi, pnum=num, kt=U32, order=0):
        return lib.gs_unique_positions(h._h if h else None, pk, n_, pok, poc, pof, poi, pnum, kt, order, None)

    def con(h, pk=k, n_=n, pok=ok, poc=oc, poi=oi, pnum=num):
        return lib.gs_unique_consecutive(h._h if h else None, pk, n_, pok, poc, poi, pnum, None)

    # 1. GS_ERR_ARG: the null handle first of all; d_keys, d_out_keys, key type, order — before the mode and the sizes
    assert keys(None, None, 0, None, kt=99, order=7) == A and pos(None, None, 0, None, kt=99, order=7) == A and con(None, None, 0, None) == A
    for call in (keys, pos, con):
        h = hp
        assert call(h, None) == A and call(h, pok=None) == A and call(h, k + 4) == A and call(h, pok=ok + 8) == A
        assert call(h, None, 0) == A  # (before the size)
    for kt in (3, 4, 5, 6, 7, 8, 9, 10, -1):  # the 64-bit and the 16-bit key types
        assert keys(hk, kt=kt) == A and keys(hp, kt=kt) == A and pos(hp, kt=kt) == A and pos(hk, kt=kt) == A, kt
    assert keys(hk, order=2) == A and pos(hp, order=-1) == A and pos(hk, order=2) == A
    # 2. GS_ERR_MODE: gs_unique_positions on a keys-only handle, before the remaining pointers and the sizes
    assert pos(hk) == M and pos(hk, n_=0) == M and pos(hk, poc=oc + 4) == M and pos(hk, pok=k) == M
    assert pos(hk, poc=None, pof=None, poi=None, pnum=None) == M  # (asking for nothing more than gs_unique_keys gives does not help)
    # 3. GS_ERR_ARG: the remaining pointers, before the sizes
    assert keys(hk, poc=oc + 4, n_=0) == A and keys(hk, pnum=num + 2) == A and pos(hp, pof=of + 8, n_=0) == A and pos(hp, poi=oi + 4) == A
    assert con(hk, poi=oi + 12, n_=0) == A and con(hp, poc=oc + 2) == A
    # 4. GS_ERR_SIZE: before the overlap test
    for call, h in ((keys, hk), (keys, hp), (pos, hp), (con, hk), (con, hp)):
        assert call(h, n_=0) == S and call(h, n_=n + 1) == S and call(h, n_=0, pok=k) == S and call(h, n_=n + 1, pok=k) == S
    # 5. GS_ERR_ARG: each overlapping pair; n elements each, one word at d_out_num; buffers that touch are fine
    m = 1000  # 4000 bytes: a multiple of 16
    assert keys(hk, n_=m, pok=k + 4 * m) == OK and keys(hk, n_=m, pok=k + 4 * m - 16) == A and keys(hk, n_=m, pok=k) == A
    assert keys(hk, n_=m, poc=k) == A and keys(hk, n_=m, poc=ok + 4 * m - 16) == A and keys(hk, n_=m, poc=ok + 4 * m) == OK
    assert keys(hk, n_=m, pnum=k + 4 * m - 4) == A and keys(hk, n_=m, pnum=ok) == A and keys(hk, n_=m, pnum=oc + 4 * m - 4) == A
    assert keys(hk, n_=m, pnum=k + 4 * m) == OK
    names = ("pk", "pok", "poc", "pof", "poi")
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            base = dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)
            base[b] = base[a] + 4 * m - 16
            assert pos(hp, n_=m, **base) == A, (a, b)
            base[b] = base[a] + 4 * m
            assert pos(hp, n_=m, **base) == OK, (a, b)
        assert pos(hp, n_=m, pnum=dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)[a] + 4 * m - 4) == A, a
    assert con(hk, n_=m, poi=k) == A and con(hk, n_=m, poi=ok + 16) == A and con(hk, n_=m, poc=oi) == A and con(hk, n_=m, poi=k + 4 * m) == OK
    # what may be NULL
    assert keys(hk, poc=None, pnum=None) == OK and pos(hp, poc=None, pof=None, poi=None, pnum=None) == OK and con(hp, poc=None, poi=None, pnum=None) == OK
    assert keys(hk, n_=1) == OK and pos(hp, n_=1) == OK and con(hk, n_=1) == OK
    torch.cuda.synchronize()
    assert hk.status() == 0 and hp.status() == 0
    # a refused call leaves the outputs untouched and route NONE, also behind a call that went through
    for b in bufs[1:]:
        b.fill_(FILL)
    half = 4 * (n // 2 + 32)
    assert keys(hk, n_=m, pok=ok + half, poc=oc + half) == OK and hk.last()["route"] == KEYS
    assert pos(hp, n_=m, pok=ok + half, poc=oc + half, pof=of + half, poi=oi + half) == OK and hp.last()["route"] == POSITIONS
    torch.cuda.synchronize()
    for refused in (keys(hk, n_=n + 1), keys(hk, kt=3), keys(hk, pok=k), pos(hk), pos(hp, poi=oi + 4), pos(hp, n_=0), con(hp, pok=None)):
        assert refused != OK
    assert hk.last()["route"] == NONE and hp.last()["route"] == NONE
    for b in bufs[1:5]:
        assert bool((b[:n // 2] == FILL).all()), "a refused call writes nothing"
    # the Python layer
    with pytest.raises(ValueError):
        gpu.Unique(4096, key_type=gpu.KEY_UINT64)
    with pytest.raises(ValueError):
        hk.unique(torch.zeros(64, dtype=torch.int16, device="cuda"))
    with pytest.raises(gpu.GpuSortError):
        hk.unique_positions(torch.zeros(64, dtype=torch.int32, device="cuda"))
    hk.close()
    hp.close()


# ---- functional ----------------------------------------------------------------------------------------------------------------------
FLAGS = [(i, c, x) for i in (False, True) for c in (False, True) for x in (False, True)]


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


@pytest.mark.parametrize("dtype_name", ("int32", "float32"))
def test_functional_unique(gpu, dtype_name):
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    n = 3 * TILE + 11
    if dtype_name == "int32":
        host = _draws(n, 81, 300)
        kt = I32
    else:
        host = float_special_case(np.random.default_rng(82), copies=(300,) * 13 + (n - 3900,))[0]
        kt = F32
    t = _dev(host).view(dtype)
    for descending in (False, True):
        rk, rc, rf, ri = gpu.unique_reference(host, kt, descending)
        for inv, cnt, idx in FLAGS:
            got = _tuple(gpu.unique(t, return_inverse=inv, return_counts=cnt, return_index=idx, descending=descending))
            assert len(got) == 1 + inv + cnt + idx and got[0].dtype == dtype and all(g.dtype == torch.int32 for g in got[1:])
            expect = [rk] + ([ri] if inv else []) + ([rc] if cnt else []) + ([rf] if idx else [])
            for g, e in zip(got, expect):
                assert g.shape == e.shape
                np.testing.assert_array_equal(_host(g), e)
            if dtype_name == "int32" and not descending and not idx:  # torch.unique on integers is the same statement
                want = _tuple(torch.unique(t, sorted=True, return_inverse=inv, return_counts=cnt))
                for g, w in zip(got, want):
                    assert torch.equal(g.to(torch.int64), w.to(torch.int64))
    # consecutive
    runs = np.sort(host) if dtype_name == "int32" else host
    tr = _dev(runs).view(dtype)
    rk, rc, rf, ri = gpu.unique_reference(runs, consecutive=True)
    for inv, cnt in ((False, False), (True, False), (False, True), (True, True)):
        got = _tuple(gpu.unique_consecutive(tr, return_inverse=inv, return_counts=cnt))
        expect = [rk] + ([ri] if inv else []) + ([rc] if cnt else [])
        assert len(got) == len(expect) and got[0].dtype == dtype
        for g, e in zip(got, expect):
            np.testing.assert_array_equal(_host(g), e)
        if dtype_name == "int32":
            want = _tuple(torch.unique_consecutive(tr, return_inverse=inv, return_counts=cnt))
            for g, w in zip(got, want):
                assert torch.equal(g.to(torch.int64), w.to(torch.int64))
    np.testing.assert_array_equal(_host(t.view(torch.int32)), host)  # not written


def test_functional_unique_unsigned_and_empty(gpu):
    torch = _torch()
    host = _draws(5000, 91, 64)  # patterns on both sides of the sign bit
    assert (host >> 31).any() and not (host >> 31).all()
    t = _dev(host)
    for descending in (False, True):
        rk, rc, rf, ri = gpu.unique_reference(host, U32, descending)
        ok, oi, oc, of = gpu.unique(t, True, True, True, descending=descending, unsigned=True)
        for g, e in ((ok, rk), (oi, ri), (oc, rc), (of, rf)):
            np.testing.assert_array_equal(_host(g), e)
    assert not np.array_equal(_host(gpu.unique(t)), _host(gpu.unique(t, unsigned=True)))
    if hasattr(torch, "uint32"):
        np.testing.assert_array_equal(_host(gpu.unique(t.view(torch.uint32)).view(torch.int32)), gpu.unique_reference(host, U32)[0])
    for dtype in (torch.int32, torch.float32):
        e = torch.empty(0, dtype=dtype, device="cuda")
        got = gpu.unique(e, True, True, True)
        assert len(got) == 4 and got[0].dtype == dtype and all(g.numel() == 0 for g in got) and all(g.dtype == torch.int32 for g in got[1:])
        got = gpu.unique_consecutive(e, True, True)
        assert len(got) == 3 and all(g.numel() == 0 for g in got)
        assert gpu.unique(e).numel() == 0 and gpu.unique_consecutive(e).numel() == 0
