"""GPU tests of unique / run-length encode on 16-bit keys (gs_unique16_* in include/gpusort.h, gpusorting_amd/unique16.py,
functional.unique16).  Every comparison is exact against unique16_reference (tests/test_unique16_cpu.py checks that one against numpy
and by hand).  Sizes come from the kernels: a 16-byte load holds 8 keys, the histogram's tile is 8192 with four loads in flight,
gs_sort16_plan goes from 128 ranges of one tile to 65 of two at 2^20 + 1, the first-position kernel's ranges are at least four tiles
and the LDS inverse's at least eight, gs_unique_plan's tile is 4096 — not from a workload."""
import numpy as np
import pytest

from guard_arena import FILLS, Arena
from test_unique16_cpu import SPECIALS, special_case

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
KTS = (U16, I16, F16, BF16)
NONE, HISTOGRAM, CONSECUTIVE = 0, 1, 2
FIRST, INV_LDS, INV_GATHER = 1, 2, 4
AUTO, LDS, GATHER = 0, 1, 2
TILE, CTILE, BINS = 8192, 4096, 65536
MAXN = 65 * 2 * TILE + 1  # 66 histogram ranges of two tiles, the last one holds one element
LDS_MIN = 1 << 22  # GS_UNIQUE16_INVERSE_LDS_MIN (test_the_lds_inverse_... holds it against the binding)
FILL = 0x5A5A5A5A
FILL16 = 0x5A5A


def _torch():
    import torch
    return torch


def _dev(a):
    """2-byte patterns as an int16 device tensor (the handle's key type says what they are)."""
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).cuda()


def _host16(t, n=None):
    return (t if n is None else t[:n]).cpu().numpy().view(np.uint16)


def _host(t, n=None):
    return (t if n is None else t[:n]).cpu().numpy().view(np.uint32)


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _handle(gpu, kt=U16, descending=False):
    """One handle of capacity MAXN per (key type, order) for the whole file: every test is a reuse of it as well."""
    key = (kt, descending)
    if key not in _handles:
        _handles[key] = gpu.Unique16(MAXN, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, kt)
    return _handles[key]


def _first_ranges(n):
    return -(-n // (max(4, -(-(-(-n // 256)) // TILE)) * TILE))


def _lds_ranges(n):
    return -(-n // (max(8, -(-(-(-n // 256)) // TILE)) * TILE))


def _compare(gpu, h, keys, entry="unique", kt=U16, descending=False, counts=True, first=True, inverse=True, form=AUTO):
    """Runs `entry` on the uint16 patterns `keys` and compares every delivered output and the report with the reference; returns u."""
    n = keys.size
    rk, rc, rf, ri = gpu.unique16_reference(keys, kt, descending, consecutive=entry == "consecutive")
    d = _dev(keys)
    if entry == "unique":
        h.set_inverse_form(form)
        ok, oc, of, oi, num = h.unique(d, counts=counts, first=first, inverse=inverse)
        h.set_inverse_form(AUTO)
        assert ok.numel() == min(n, BINS) and (oi is None or oi.numel() == n)
    else:
        ok, oc, oi, num = h.unique_consecutive(d, counts=counts, inverse=inverse)
        of = None
    h.check()
    u = int(num.item())
    assert u == rk.size, (entry, n, u, rk.size)
    rep = h.last()
    assert (rep["route"], rep["n"], rep["u"], rep["status"]) == (HISTOGRAM if entry == "unique" else CONSECUTIVE, n, u, 0)
    if entry == "unique":
        lds = form == LDS or (form == AUTO and n >= LDS_MIN)
        assert rep["ran"] == (FIRST if first else 0) | ((INV_LDS if lds else INV_GATHER) if inverse else 0)
        plan = gpu.sort16_plan(n)
        assert (rep["ranges"], rep["per_range"], rep["tile"]) == (plan["ranges"], plan["per_range"], plan["tile"])
        assert rep["first_ranges"] == (_first_ranges(n) if first else 0)
        assert rep["inverse_ranges"] == ((_lds_ranges(n) if lds else -(-n // TILE)) if inverse else 0)
    else:
        assert rep["ran"] == 0 and (rep["ranges"], rep["per_range"], rep["tile"]) == gpu.unique_plan(n)
    np.testing.assert_array_equal(_host16(ok, u), rk)
    assert (oc is not None) == counts and (oi is not None) == inverse and (of is not None) == (first and entry == "unique")
    if oc is not None:
        np.testing.assert_array_equal(_host(oc, u), rc)
    if of is not None:
        np.testing.assert_array_equal(_host(of, u), rf)
    if oi is not None:
        np.testing.assert_array_equal(_host(oi), ri)
    np.testing.assert_array_equal(_host16(d), keys)  # the input is not written
    return u


def _draws(n, seed, distinct):
    """n draws from `distinct` random 16-bit patterns (floats: no care taken, any pattern is a key)."""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(BINS)[:distinct].astype(np.uint16)
    return pool[rng.integers(0, distinct, n)]


# ---- types and orders ----------------------------------------------------------------------------------------------------------------
WANT = [(c, f, i) for c in (False, True) for f in (False, True) for i in (False, True)]


@pytest.mark.parametrize("kt", KTS)
@pytest.mark.parametrize("descending", (False, True))
def test_types_orders_and_every_combination_of_optional_outputs(gpu, kt, descending):
    keys = _draws(5000, 100 + kt, 37)
    h = _handle(gpu, kt, descending)
    for counts, first, inverse in WANT:
        assert _compare(gpu, h, keys, "unique", kt, descending, counts, first, inverse) <= 37
    _compare(gpu, h, keys, "unique", kt, descending, form=LDS)
    for counts, inverse in ((False, False), (True, False), (False, True), (True, True)):
        _compare(gpu, h, np.sort(keys), "consecutive", counts=counts, inverse=inverse)


@pytest.mark.parametrize("kt", (F16, BF16))
@pytest.mark.parametrize("descending", (False, True))
def test_float_specials_are_keys_of_their_own(gpu, kt, descending):
    values, copies = special_case(kt, np.random.default_rng(6), copies=(300, 1, 2, 500, 1, 400, 200, 600, 1, 2, 3, 1, 2, 4))
    assert _compare(gpu, _handle(gpu, kt, descending), values, "unique", kt, descending) == SPECIALS[kt].size


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 7, 8, 9, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1, 1 << 20, (1 << 20) + 1, MAXN)
CSIZES = (1, 2, 7, 8, 9, 63, 64, 65, CTILE - 1, CTILE, CTILE + 1, (1 << 22) + 1, 513 * 2 * CTILE + 1)


def test_the_plans_the_sizes_rely_on(gpu):
    p = gpu.sort16_plan
    assert (p(TILE)["ranges"], p(TILE)["per_range"], p(TILE)["tile"]) == (1, TILE, TILE) and p(TILE + 1)["ranges"] == 2
    assert (p(1 << 20)["ranges"], p(1 << 20)["per_range"]) == (128, TILE) and (p((1 << 20) + 1)["ranges"], p((1 << 20) + 1)["per_range"]) == (65, 2 * TILE)
    assert (p(MAXN)["ranges"], p(MAXN)["per_range"]) == (66, 2 * TILE) and MAXN - 65 * 2 * TILE == 1
    # the first-position kernel: ranges of four tiles up to 2^23 elements; the LDS inverse: of eight tiles up to 2^24
    assert [_first_ranges(n) for n in (1, 4 * TILE, 4 * TILE + 1, MAXN, 1 << 23, (1 << 23) + 1)] == [1, 1, 2, 33, 256, 205]
    assert [_lds_ranges(n) for n in (1, 8 * TILE, 8 * TILE + 1, MAXN, (1 << 21) + 1)] == [1, 1, 2, 17, 33]
    assert gpu.unique_plan(CTILE) == (1, CTILE, CTILE) and gpu.unique_plan(CTILE + 1) == (2, CTILE, CTILE)
    assert gpu.unique_plan((1 << 22) + 1) == (513, 2 * CTILE, CTILE) and gpu.unique_plan(513 * 2 * CTILE + 1) == (514, 2 * CTILE, CTILE)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    h = _handle(gpu)
    few = _draws(n, n, 7)
    assert _compare(gpu, h, few) == np.unique(few).size
    many = _draws(n, n + 1, 60000)
    _compare(gpu, h, many, form=LDS if n % 2 else GATHER)
    _compare(gpu, h, many, form=GATHER if n % 2 else LDS, counts=False, first=False)


def test_the_lds_inverse_with_ranges_longer_than_its_unroll_and_the_auto_rule(gpu):
    """(1 << 21) + 1 elements: 33 ranges of eight tiles, so the four-loads-in-flight loop of the LDS inverse runs twice and a last range
    holds one element; 2^22 is where AUTO goes over to the LDS table."""
    from gpusorting_amd import _lib
    assert _lib.GS_UNIQUE16_INVERSE_LDS_MIN == 1 << 22
    h = gpu.Unique16(1 << 22, gpu.ORDER_DESCENDING, gpu.KEY_BFLOAT16)
    _compare(gpu, h, _draws((1 << 21) + 1, 5, 40000), "unique", BF16, True, form=LDS)
    _compare(gpu, h, _draws((1 << 22) - 1, 6, 3), "unique", BF16, True, counts=False, first=False)  # AUTO: the gather
    _compare(gpu, h, _draws(1 << 22, 7, 50000), "unique", BF16, True, counts=False, first=False)    # AUTO: the LDS table
    h.close()


@pytest.mark.parametrize("n", CSIZES)
def test_sizes_consecutive(gpu, n):
    """Runs of three across every wave, tile and range edge, runs longer than two tiles, and all heads."""
    h = gpu.Unique16(n) if n > MAXN else _handle(gpu)
    i = np.arange(n, dtype=np.uint32)
    assert _compare(gpu, h, (i // 3).astype(np.uint16), "consecutive") == -(-n // 3)
    assert _compare(gpu, h, (i // (2 * CTILE + 1)).astype(np.uint16), "consecutive") == -(-n // (2 * CTILE + 1))
    assert _compare(gpu, h, i.astype(np.uint16), "consecutive") == n  # (a wrap at 65 536 is a head too)
    if n > MAXN:
        h.close()


# ---- u edges -------------------------------------------------------------------------------------------------------------------------
def test_one_and_two_distinct_keys(gpu):
    h = _handle(gpu)
    n = 5 * TILE + 100
    assert _compare(gpu, h, np.full(n, 0x1234, np.uint16)) == 1          # the histogram's one-add-per-wave shortcut; first = 0
    assert _compare(gpu, h, np.full(n, 0x1234, np.uint16), "consecutive") == 1
    alt = np.where(np.arange(n) % 2 == 0, 11, 4).astype(np.uint16)
    assert _compare(gpu, h, alt) == 2
    assert _compare(gpu, h, alt, "consecutive") == n


@pytest.mark.parametrize("kt", KTS)
@pytest.mark.parametrize("descending", (False, True))
def test_every_pattern_is_a_key(gpu, kt, descending):
    """u = 65 536: rank 65 535 fits the rank table's 16 bits, u does not.  NaN and -0.0 patterns are keys like the others."""
    rng = np.random.default_rng(900 + kt)
    perm = rng.permutation(BINS).astype(np.uint16)
    h = _handle(gpu, kt, descending)
    assert _compare(gpu, h, perm, "unique", kt, descending, form=LDS) == BINS
    more = np.concatenate([perm, perm[rng.integers(0, BINS, 1000)]])
    assert _compare(gpu, h, more, "unique", kt, descending) == BINS


@pytest.mark.parametrize("distinct", (36, 37))
def test_nothing_at_or_behind_u_is_written(gpu, distinct):
    """u even and odd on prefilled outputs: out_keys is written with 2-byte stores, so the neighbour of out_keys[u - 1] survives."""
    torch = _torch()
    from gpusorting_amd import _lib
    lib = _lib.load()
    n = 3 * TILE + 5
    keys = np.arange(n, dtype=np.uint32) * 7 % distinct
    keys = (keys * 1000 + 3).astype(np.uint16)
    for entry in ("unique", "consecutive"):
        src = keys if entry == "unique" else np.sort(keys)
        rk, rc, rf, ri = gpu.unique16_reference(src, U16, True, consecutive=entry == "consecutive")
        u = rk.size
        assert u == distinct
        d = _dev(src)
        ok = torch.full((n,), FILL16, dtype=torch.int16, device="cuda")
        oc, of, oi = (torch.full((n,), FILL, dtype=torch.int32, device="cuda") for _ in range(3))
        num = torch.zeros(1, dtype=torch.int32, device="cuda")
        h = _handle(gpu, U16, True)
        if entry == "unique":
            st = lib.gs_unique16_unique(h._h, d.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), U16, 1, None)
        else:
            st = lib.gs_unique16_consecutive(h._h, d.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), oi.data_ptr(), num.data_ptr(), None)
        assert st == _lib.GS_OK
        h.check()
        assert int(num.item()) == u
        np.testing.assert_array_equal(_host16(ok, u), rk)
        np.testing.assert_array_equal(_host(oc, u), rc)
        np.testing.assert_array_equal(_host(oi), ri)
        assert bool((ok[u:] == FILL16).all()) and bool((oc[u:] == FILL).all())
        if entry == "unique":
            np.testing.assert_array_equal(_host(of, u), rf)
            assert bool((of[u:] == FILL).all())


# ---- first positions -----------------------------------------------------------------------------------------------------------------
FIRST_CASES = ("early_range", "last_range_only", "rising_period_512", "falling_period_512", "falling_period_37", "all_equal", "second_tile")


def _first_case(name):
    """Laid by hand; the cases a wrongly ordered filter passes by luck on random data.  Twelve tiles and nine elements: three ranges
    of four tiles and a last one of nine elements."""
    n = 12 * TILE + 9
    i = np.arange(n, dtype=np.uint32)
    if name == "early_range":  # key 7 once in range 0, then nearly all of ranges 1 and 2
        s = (i % 5 + 100).astype(np.uint16)
        s[4 * TILE + 50:] = 7
        s[3] = 7
        s[-5:] = 9
    elif name == "last_range_only":
        s = (i % 300).astype(np.uint16)
        s[8 * TILE + 4000:8 * TILE + 4003] = 40000
        s[-1] = 50000
    elif name == "rising_period_512":  # every bin once per wave of a tile, at the same lane and slot
        s = (i % 512).astype(np.uint16)
    elif name == "falling_period_512":  # ... and the bins of a thread fall: the filters see the tile's bins in the other order
        s = (511 - i % 512).astype(np.uint16)
    elif name == "falling_period_37":
        s = ((36 - i % 37) * 1771).astype(np.uint16)
    elif name == "all_equal":
        s = np.full(n, 0xBEEF, np.uint16)
    else:  # second_tile: tile 0 holds other keys; in tile 1 every bin lies in all sixteen waves, high 4 bin bits apart on equal low 12
        s = (i % 64 + 1000).astype(np.uint16)
        t = i[TILE:2 * TILE] - TILE
        s[TILE:2 * TILE] = (((t % 16) << 12) | ((TILE - 1 - t) % 512 // 16)).astype(np.uint16)
    return s


@pytest.mark.parametrize("name", FIRST_CASES)
@pytest.mark.parametrize("descending", (False, True))
def test_first_is_the_lowest_position(gpu, name, descending):
    keys = _first_case(name)
    h = _handle(gpu, I16, descending)
    _compare(gpu, h, keys, "unique", I16, descending)
    ok, oc, of, oi, num = h.unique(_dev(keys), counts=False, inverse=False)  # no reference: the definition itself
    u = int(num.item())
    for k, f in zip(_host16(ok, u).tolist()[:50], _host(of, u).tolist()[:50]):
        assert f == int(np.flatnonzero(keys == k)[0]), (k, f)
    if name == "all_equal":
        assert _host(of, 1).tolist() == [0]


# ---- guard arena ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,fill", [("unique", f) for f in FILLS] + [("consecutive", "hash"), ("consecutive", 0xFF)])
def test_outputs_on_a_guard_arena(gpu, entry, fill):
    """n < max_keys, u < the outputs' room: nothing outside [0, u) of out_keys / out_counts / out_first, [0, n) of out_inverse and the
    one word of d_out_num is written, the pointers are 16-byte aligned and no more, and the input is read only."""
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    n, cap = 3 * TILE + 77, 3 * TILE + 77 + 300
    keys = _draws(n, 9, 51)
    if entry == "consecutive":
        keys = np.sort(keys)[::-1].copy()
    rk, rc, rf, ri = gpu.unique16_reference(keys, F16, True, consecutive=entry == "consecutive")
    u = rk.size
    assert 1 < u < n and u % 2 == 1
    arena = Arena.for_views([(2 * cap, np.uint8)] * 2 + [(cap, np.uint32)] * 3 + [(4, np.uint32)], "cuda", fill)
    dk, ok = arena.carve(2 * cap, np.uint8, 1, "keys"), arena.carve(2 * cap, np.uint8, 3, "out_keys")
    oc, of, oi = (arena.carve(cap, np.uint32, skew, name) for skew, name in ((5, "out_counts"), (7, "out_first"), (9, "out_inverse")))
    num = arena.carve(4, np.uint32, 11, "out_num")
    arena.write(dk, keys.view(np.uint8))
    arena.live(ok, 2 * u)
    arena.live(num, 1)
    arena.live(oc, u)
    arena.live(oi, n)
    h = _handle(gpu, F16, True)
    if entry == "unique":
        arena.live(of, u)
        st = lib.gs_unique16_unique(h._h, dk.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), F16, 1, None)
    else:
        st = lib.gs_unique16_consecutive(h._h, dk.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), oi.data_ptr(), num.data_ptr(), None)
    assert st == _lib.GS_OK
    torch.cuda.synchronize()
    h.check()
    arena.verify()
    assert int(_host(num)[0]) == u and h.last()["u"] == u
    np.testing.assert_array_equal(ok[:2 * u].cpu().numpy().view(np.uint16), rk)
    np.testing.assert_array_equal(_host(oc, u), rc)
    if entry == "unique":
        np.testing.assert_array_equal(_host(of, u), rf)
    np.testing.assert_array_equal(_host(oi, n), ri)


# ---- handle reuse --------------------------------------------------------------------------------------------------------------------
def test_handle_reuse_and_report(gpu):
    """A large call, a small one, another type and order, then the consecutive entry on one handle: each call's report, and the check."""
    h = gpu.Unique16((1 << 20) + 1)
    assert h.last()["route"] == NONE and h.status() == 0 and h.temp_bytes == 672000
    for keys, entry, kt, desc in ((_draws((1 << 20) + 1, 70, 1000), "unique", U16, False), (_draws(300, 71, 5), "unique", U16, False),
                                  (_draws(70001, 72, 60000), "unique", BF16, True), (np.sort(_draws(70001, 73, 99)), "consecutive", U16, False),
                                  (_draws(2, 74, 2), "unique", I16, True)):
        h.key_type, h.order = kt, int(desc)
        _compare(gpu, h, keys, entry, kt, desc)  # (route, n, u, the ran-kernel mask and the plans are compared there)
        assert h.status() == 0
    h.close()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("unique", "consecutive"))
def test_captured_graph_replayed_on_new_data_with_another_u(gpu, entry):
    from gpusorting_amd import _lib
    from gpusorting_amd.onesweep import _stream_ptr
    torch = _torch()
    lib = _lib.load()
    n = 100003
    h = gpu.Unique16(n, gpu.ORDER_DESCENDING, gpu.KEY_INT16)
    dk = _dev(_draws(n, 31, 500))
    ok = torch.empty(n, dtype=torch.int16, device="cuda")
    oc, of, oi = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    num = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        if entry == "unique":
            st = lib.gs_unique16_unique(h._h, dk.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), of.data_ptr(), oi.data_ptr(), num.data_ptr(), I16, 1, _stream_ptr())
        else:
            st = lib.gs_unique16_consecutive(h._h, dk.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), oi.data_ptr(), num.data_ptr(), _stream_ptr())
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
    seen, firsts = set(), []
    for seed, distinct in ((32, 65536), (33, 40), (34, 7000)):
        keys = _draws(n, seed, distinct)
        if entry == "consecutive":
            keys = np.sort(keys)
        dk.copy_(_dev(keys))
        ok.fill_(FILL16)
        for t in (oc, of, oi, num):
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rc, rf, ri = gpu.unique16_reference(keys, I16, True, consecutive=entry == "consecutive")
        u = int(num.item())
        assert u == rk.size == h.last()["u"]
        seen.add(u)
        np.testing.assert_array_equal(_host16(ok, u), rk)
        np.testing.assert_array_equal(_host(oc, u), rc)
        np.testing.assert_array_equal(_host(oi), ri)
        assert bool((ok[u:] == FILL16).all() and (oc[u:] == -1).all())
        if entry == "unique":
            np.testing.assert_array_equal(_host(of, u), rf)
            firsts.append(rf[:8].tolist())
    assert len(seen) == 3 and (entry != "unique" or firsts[0] != firsts[1] != firsts[2])
    h.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    OK, A, S = _lib.GS_OK, _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE
    n = 10000
    bufs = [torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda") for _ in range(6)]
    k, ok, oc, of, oi, num = (b.data_ptr() for b in bufs)
    h = gpu.Unique16(n)

    def uni(h_, pk=k, n_=n, pok=ok, poc=oc, pof=of, poi=oi, pnum=num, kt=U16, order=0):
        return lib.gs_unique16_unique(h_._h if h_ else None, pk, n_, pok, poc, pof, poi, pnum, kt, order, None)

    def con(h_, pk=k, n_=n, pok=ok, poc=oc, poi=oi, pnum=num):
        return lib.gs_unique16_consecutive(h_._h if h_ else None, pk, n_, pok, poc, poi, pnum, None)

    # 1. GS_ERR_ARG: the null handle first of all
    assert uni(None, None, 0, None, kt=99, order=7) == A and con(None, None, 0, None) == A
    # 2. d_keys, d_out_keys, key type, order — before the remaining pointers and the sizes
    for call in (uni, con):
        assert call(h, None) == A and call(h, pok=None) == A and call(h, k + 4) == A and call(h, pok=ok + 8) == A
        assert call(h, None, 0) == A  # (before the size)
    for kt in (0, 1, 2, 3, 4, 5, 10, -1):  # the 32-bit and the 64-bit key types
        assert uni(h, kt=kt) == A and uni(h, kt=kt, n_=0) == A, kt
    assert uni(h, order=2) == A and uni(h, order=-1, n_=0) == A
    # 3. GS_ERR_ARG: the remaining pointers, before the sizes
    assert uni(h, poc=oc + 4, n_=0) == A and uni(h, pnum=num + 2) == A and uni(h, pof=of + 8, n_=0) == A and uni(h, poi=oi + 4) == A
    assert con(h, poi=oi + 12, n_=0) == A and con(h, poc=oc + 2) == A and con(h, pnum=num + 1, n_=n + 1) == A
    # 4. GS_ERR_SIZE: before the overlap test
    for call in (uni, con):
        assert call(h, n_=0) == S and call(h, n_=n + 1) == S and call(h, n_=0, pok=k) == S and call(h, n_=n + 1, pok=k) == S
    # 5. GS_ERR_ARG: each overlapping pair, outputs at their capacities (m < 65 536: m elements each); buffers that touch are fine
    m = 1000  # 2000 bytes of keys: a multiple of 16
    width = dict(pk=2, pok=2, poc=4, pof=4, poi=4)
    names = ("pk", "pok", "poc", "pof", "poi")
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            base = dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)
            base[b] = base[a] + width[a] * m - 16
            assert uni(h, n_=m, **base) == A, (a, b)
            base[b] = base[a] + width[a] * m
            assert uni(h, n_=m, **base) == OK, (a, b)
        assert uni(h, n_=m, pnum=dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)[a] + width[a] * m - 4) == A, a
        assert uni(h, n_=m, pnum=dict(pk=k, pok=ok, poc=oc, pof=of, poi=oi)[a] + width[a] * m) == OK, a
    assert con(h, n_=m, poi=k) == A and con(h, n_=m, poi=ok + 16) == A and con(h, n_=m, poc=oi) == A and con(h, n_=m, poi=k + 2 * m) == OK
    # above 65 536 elements gs_unique16_unique's small outputs hold 65 536, the consecutive entry's n
    big = gpu.Unique16(1 << 17)
    bb = [torch.full((1 << 17,), FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    bk, bok, boc = (b.data_ptr() for b in bb)
    N = 1 << 17
    assert uni(big, bk, N, bok, bok + 2 * 65536, None, None, None) == OK and uni(big, bk, N, bok, bok + 2 * 65536 - 16, None, None, None) == A
    assert uni(big, bk, N, bok, boc, boc + 4 * 65536 - 16, None, None) == A and uni(big, bk, N, bok, boc, boc + 4 * 65536, None, None) == OK
    assert con(big, bk, N, bok, bok + 2 * 65536, None, None) == A and con(big, bk, N, bok, boc, None, None) == OK
    big.close()
    # what may be NULL: every output but d_out_keys, d_out_num as well
    assert uni(h, poc=None, pof=None, poi=None, pnum=None) == OK and con(h, poc=None, poi=None, pnum=None) == OK
    assert uni(h, pok=None, poc=None, pof=None, poi=None, pnum=None) == A
    assert uni(h, n_=1) == OK and con(h, n_=1) == OK
    torch.cuda.synchronize()
    assert h.status() == 0
    # a refused call leaves the outputs untouched and route NONE, also behind a call that went through
    for b in bufs[1:]:
        b.fill_(FILL)
    half = 4 * (n // 2 + 32)
    assert uni(h, n_=m, pok=ok + half, poc=oc + half, pof=of + half, poi=oi + half) == OK and h.last()["route"] == HISTOGRAM
    torch.cuda.synchronize()
    for refused in (uni(h, n_=n + 1), uni(h, kt=2), uni(h, pok=k), uni(h, poi=oi + 4), uni(h, n_=0), con(h, pok=None)):
        assert refused != OK
        assert h.last()["route"] == NONE
    for b in bufs[1:5]:
        assert bool((b[:n // 2] == FILL).all()), "a refused call writes nothing"
    assert lib.gs_unique16_set_inverse_form(h._h, 3) == A and lib.gs_unique16_set_inverse_form(h._h, 2) == OK
    rep = (_lib.C.c_uint32 * 16)()
    assert lib.gs_unique16_last(h._h, rep, _lib.GS_UNIQUE16_REPORT_WORDS - 1, None) == A and lib.gs_unique16_last(h._h, None, 16, None) == A
    # the Python layer
    with pytest.raises(ValueError):
        gpu.Unique16(4096, key_type=gpu.KEY_UINT32)
    with pytest.raises(ValueError):
        h.unique(torch.zeros(64, dtype=torch.int32, device="cuda"))
    h.close()


# ---- functional ----------------------------------------------------------------------------------------------------------------------
FLAGS = [(i, c, x) for i in (False, True) for c in (False, True) for x in (False, True)]


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


def _host_any(t):
    return t.cpu().view(_torch().int16).numpy().view(np.uint16) if t.element_size() == 2 else _host(t)


@pytest.mark.parametrize("dtype_name", ("float16", "bfloat16", "int16", "uint16"))
def test_functional_unique16(gpu, dtype_name):
    torch = _torch()
    unsigned = not hasattr(torch, dtype_name)  # a torch without uint16: int16 storage with unsigned=True
    dtype = torch.int16 if unsigned else getattr(torch, dtype_name)
    kt = {"float16": F16, "bfloat16": BF16, "int16": I16, "uint16": U16}[dtype_name]
    n = 3 * TILE + 11
    host = special_case(kt, np.random.default_rng(82), copies=(300,) * 13 + (n - 3900,))[0] if kt in SPECIALS else _draws(n, 81, 300)
    t = _dev(host).view(dtype)
    for descending in (False, True):
        rk, rc, rf, ri = gpu.unique16_reference(host, kt, descending)
        for inv, cnt, idx in FLAGS:
            got = _tuple(gpu.unique16(t, return_inverse=inv, return_counts=cnt, return_index=idx, descending=descending, unsigned=unsigned))
            assert len(got) == 1 + inv + cnt + idx and got[0].dtype == dtype and all(g.dtype == torch.int32 for g in got[1:])
            expect = [rk] + ([ri] if inv else []) + ([rc] if cnt else []) + ([rf] if idx else [])
            for g, e in zip(got, expect):
                assert g.shape == e.shape
                np.testing.assert_array_equal(_host_any(g), e)
            if dtype_name == "int16" and not descending and not idx:  # torch.unique on integers is the same statement
                want = _tuple(torch.unique(t, sorted=True, return_inverse=inv, return_counts=cnt))
                for g, w in zip(got, want):
                    assert torch.equal(g.to(torch.int64), w.to(torch.int64))
    runs = np.sort(host) if kt not in SPECIALS else host
    tr = _dev(runs).view(dtype)
    rk, rc, rf, ri = gpu.unique16_reference(runs, consecutive=True)
    for inv, cnt in ((False, False), (True, False), (False, True), (True, True)):
        got = _tuple(gpu.unique_consecutive16(tr, return_inverse=inv, return_counts=cnt))
        expect = [rk] + ([ri] if inv else []) + ([rc] if cnt else [])
        assert len(got) == len(expect) and got[0].dtype == dtype
        for g, e in zip(got, expect):
            np.testing.assert_array_equal(_host_any(g), e)
        if dtype_name == "int16":
            want = _tuple(torch.unique_consecutive(tr, return_inverse=inv, return_counts=cnt))
            for g, w in zip(got, want):
                assert torch.equal(g.to(torch.int64), w.to(torch.int64))
    np.testing.assert_array_equal(_host_any(t), host)  # not written


def test_functional_unique16_unsigned_and_empty(gpu):
    torch = _torch()
    host = _draws(5000, 91, 64)  # patterns on both sides of the sign bit
    assert (host >> 15).any() and not (host >> 15).all()
    t = _dev(host)
    for descending in (False, True):
        rk, rc, rf, ri = gpu.unique16_reference(host, U16, descending)
        ok, oi, oc, of = gpu.unique16(t, True, True, True, descending=descending, unsigned=True)
        for g, e in ((ok, rk), (oi, ri), (oc, rc), (of, rf)):
            np.testing.assert_array_equal(_host_any(g), e)
    assert not np.array_equal(_host_any(gpu.unique16(t)), _host_any(gpu.unique16(t, unsigned=True)))
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        e = torch.empty(0, dtype=dtype, device="cuda")
        got = gpu.unique16(e, True, True, True)
        assert len(got) == 4 and got[0].dtype == dtype and all(g.numel() == 0 for g in got) and all(g.dtype == torch.int32 for g in got[1:])
        got = gpu.unique_consecutive16(e, True, True)
        assert len(got) == 3 and all(g.numel() == 0 for g in got)
        assert gpu.unique16(e).numel() == 0 and gpu.unique_consecutive16(e).numel() == 0
    # the 32-bit entries keep refusing 16-bit tensors, and the other way round
    with pytest.raises(TypeError, match="unique"):
        gpu.unique(t)
    with pytest.raises(TypeError, match="unique"):
        gpu.unique16(t.to(torch.int32))
