"""GPU tests of the merge (gs_merge_* in include/gpusort.h, gpusorting_amd/_merge.py, merge_kernels.hpp).  Every result is compared
bit for bit with merge_reference (tests/test_merge_cpu.py checks that one against a brute-force statement).  Shapes come from
gs_merge_plan (T outputs per tile, VT per thread) and are the smallest at which each mechanism can go wrong: at most a few tiles.  The
report of every call is checked too: the form, the sizes, the tiles that ran (the plan's grid) and the one-sided tiles, counted from
the reference's positions."""
import ctypes as C

import numpy as np
import pytest

from guard_arena import Arena
from test_merge_cpu import F32, F64, I32, I64, KEY_TYPES, U32, U64, draws, specials, word_dtype

pytestmark = pytest.mark.gpu

NONE, KEYS, PAIRS, POSITIONS = 0, 1, 2, 3
FORMS = ("keys", "pairs4", "pairs8", "positions")
MAXN = 1 << 16
SENTINEL = -7


def _torch():
    import torch
    return torch


def _m():
    from gpusorting_amd import _merge
    return _merge


def _dev(a):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()


def _host(t, n=None):
    t = t if n is None else t[:n]
    return t.cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


def _plan(kt=U32, n=1):
    return _m().merge_plan(n, 0, 8 if kt >= U64 else 4)


def _sorted(bits, kt, descending):
    """`bits` in the order the library's sort leaves them."""
    return bits[np.argsort(_m()._words(bits, kt, descending), kind="stable")].copy()


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _handle(gpu, kt):
    """One handle of capacity MAXN per key width for the whole file: every test is a reuse of it as well."""
    wide = kt >= U64
    if wide not in _handles:
        _handles[wide] = _m().Merge(MAXN, U64 if wide else U32)
    return _handles[wide]


def _values(n, width, seed):
    """n distinct values of `width` bytes whose top bits are set: a value moved as half its width or as an index is seen."""
    dt = np.uint64 if width == 8 else np.uint32
    v = np.arange(n, dtype=dt) * dt(0x9E3779B1 if width == 4 else 0x9E3779B97F4A7C15) + dt(seed)
    return v


def _copy_tiles(src, na, T):
    """The tiles of T outputs that lie wholly in one input, from the reference's positions."""
    count = 0
    for t0 in range(0, src.size, T):
        side = src[t0:t0 + T] >= na
        count += int(side.all() or not side.any())
    return count


def _order(gpu, descending):
    return gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING


def _run(gpu, form, a, b, kt=U32, descending=False):
    """Runs `form` on the sorted bit patterns a / b, compares every output with the reference, checks the tail of the outputs, that
    no input was written, and the report; returns the report."""
    torch = _torch()
    h = _handle(gpu, kt)
    na, nb, n = a.size, b.size, a.size + b.size
    width = {"pairs4": 4, "pairs8": 8}.get(form)
    va, vb = (_values(na, width, 1), _values(nb, width, 2)) if width else (None, None)
    want = _m().merge_reference(a, b, kt, descending, va, vb)
    da, db = _dev(a), _dev(b)
    out = torch.full((n + 64,), SENTINEL, dtype=da.dtype, device="cuda")
    order = _order(gpu, descending)
    aux = None
    if form == "keys":
        h.merge(da, db, na, nb, out=out, key_type=kt, order=order)
    elif form == "positions":
        aux = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device="cuda")
        h.merge_positions(da, db, na, nb, out_keys=out, out_src=aux, key_type=kt, order=order)
        want_aux = want[1]
    else:
        dva, dvb = _dev(va), _dev(vb)
        aux = torch.full((n + 64,), SENTINEL, dtype=dva.dtype, device="cuda")
        h.merge_pairs(da, dva, db, dvb, na, nb, out_keys=out, out_values=aux, key_type=kt, order=order)
        want_aux = want[2]
    got = _host(out, n)
    bad = np.flatnonzero(got != want[0])
    assert bad.size == 0, (form, kt, descending, na, nb, bad[:5], got[bad[:5]], want[0][bad[:5]])
    assert bool((out[n:] == SENTINEL).all()), "written behind element na + nb of out_keys"
    if aux is not None:
        got = _host(aux, n)
        bad = np.flatnonzero(got != want_aux)
        assert bad.size == 0, (form, kt, descending, na, nb, bad[:5], got[bad[:5]], want_aux[bad[:5]])
        assert bool((aux[n:] == SENTINEL).all()), "written behind element na + nb of the second output"
    np.testing.assert_array_equal(_host(da), a)
    np.testing.assert_array_equal(_host(db), b)
    if width:
        np.testing.assert_array_equal(_host(dva), va)
        np.testing.assert_array_equal(_host(dvb), vb)
    rep = h.last()
    p = _m().merge_plan(na, nb, 8 if kt >= U64 else 4)
    assert (rep["form"], rep["na"], rep["nb"]) == ({"keys": KEYS, "positions": POSITIONS}.get(form, PAIRS), na, nb)
    assert rep["plan"] == p and rep["tiles"] == p["grid"]
    assert rep["copy_tiles"] == _copy_tiles(want[1], na, p["tile"]), (form, na, nb)
    return rep


# ---- sizes and splits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U32, U64))
def test_sizes_and_splits(gpu, kt):
    """na + nb around VT, T and a few tiles, crossed with the splits: a side empty, a side of one, balanced, every A before every B and
    the other way round, strictly interleaved, one side a 64th of the other.  The disjoint ranges are copies but for the tile the
    border falls in; the interleaved ones have no copy tile unless a tile holds one output."""
    p = _plan(kt)
    T, VT = p["tile"], p["vt"]
    dt = word_dtype(kt)
    rng = np.random.default_rng(3 + kt)
    h = _handle(gpu, kt)
    for n in (1, 2, VT - 1, VT, VT + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 5 * T + 3):
        pool = rng.integers(0, 1 << 62 if kt == U64 else 1 << 32, max(2, n // 3), dtype=dt)  # about three of every key
        for na in sorted({0, n, min(1, n), max(n - 1, 0), n // 2}):  # a side empty, a side of one, balanced
            a, b = _sorted(pool[rng.integers(0, pool.size, na)], kt, False), _sorted(pool[rng.integers(0, pool.size, n - na)], kt, False)
            _run(gpu, "keys", a, b, kt)
        na = n // 2
        lo, hi = np.arange(na, dtype=dt), np.arange(n - na, dtype=dt) + dt(na)
        for a, b in ((lo, hi), (hi, lo)):  # every A before every B; every B before every A
            rep = _run(gpu, "keys", a, b, kt)
            assert rep["copy_tiles"] >= rep["tiles"] - 1
        a, b = np.arange(n - na, dtype=dt) * dt(2), np.arange(na, dtype=dt) * dt(2) + dt(1)  # strictly interleaved
        rep = _run(gpu, "keys", a, b, kt)
        if n % T != 1:
            assert rep["copy_tiles"] == 0
        small = max(n // 65, 1 if n > 1 else 0)  # one side 1/64 of the other
        if small:
            big = np.sort(rng.integers(0, 1 << 31, n - small).astype(dt))
            few = np.sort(rng.integers(0, 1 << 31, small).astype(dt))
            _run(gpu, "keys", big, few, kt)
            _run(gpu, "keys", few, big, kt)
    assert h.last()["form"] == KEYS


# ---- ties at every border --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U32, F64))
def test_ties_across_tile_and_thread_borders(gpu, kt):
    """Both sides all equal; and a run of one key longer than T in both inputs, behind VT - 1 and VT + 1 smaller keys, so that the run
    crosses tile borders and starts and ends one off a thread border: through the positions and through values A's elements come
    first and both sides keep their order (the reference says so; the run is looked at once more by hand)."""
    p = _plan(kt)
    T, VT = p["tile"], p["vt"]
    dt = word_dtype(kt)
    x = specials(kt)[7] if kt == F64 else dt(77)  # (+0.0 as a double)
    for na, nb in ((T + 3, 2 * T - 1), (1, 3 * T), (VT + 1, VT - 1), (2 * T, 2 * T)):
        same_a, same_b = np.full(na, x, dtype=dt), np.full(nb, x, dtype=dt)
        for form in ("positions", "pairs4"):
            _run(gpu, form, same_a, same_b, kt)
    for descending in (False, True):
        below, above = (specials(kt)[3], specials(kt)[10]) if kt == F64 else (dt(5), dt(900))  # -1.0 < +0.0 < 1.0
        if descending:
            below, above = above, below
        a = np.concatenate([np.full(VT - 1, below, dtype=dt), np.full(T + VT + 1, x, dtype=dt), np.full(2 * VT + 1, above, dtype=dt)])
        b = np.concatenate([np.full(VT + 1, below, dtype=dt), np.full(T + 2 * VT - 1, x, dtype=dt), np.full(3, above, dtype=dt)])
        for form in ("positions", "pairs8", "pairs4"):
            _run(gpu, form, a, b, kt, descending)
        keys, src = (_host(t) for t in _m().argmerge(_dev(a).view(_torch().float64) if kt == F64 else _dev(a),
                                                     _dev(b).view(_torch().float64) if kt == F64 else _dev(b), descending=descending,
                                                     unsigned=kt == U32))
        run = src[keys == x].astype(np.int64)
        from_a, from_b = run[run < a.size], run[run >= a.size]
        assert from_a.size == T + VT + 1 and from_b.size == T + 2 * VT - 1
        np.testing.assert_array_equal(run, np.concatenate([from_a, from_b]))  # all of A's in front of all of B's
        assert (np.diff(from_a) == 1).all() and (np.diff(from_b) == 1).all()   # each side in its input order


# ---- types and orders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", (False, True), ids=("asc", "desc"))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_types_orders_and_forms(gpu, kt, descending):
    """All six key types, both orders, every form (4- and 8-byte values) at 2 T + 1 outputs: every special on both sides, many
    duplicates inside and across the sides."""
    T = _plan(kt)["tile"]
    na = T - 37
    a = _sorted(draws(kt, na, 40 + kt, distinct=300), kt, descending)
    b = _sorted(np.concatenate([draws(kt, 2 * T + 1 - na - 50, 50 + kt, distinct=300), a[::na // 50][:50]]), kt, descending)
    assert a.size + b.size == 2 * T + 1
    for form in FORMS:
        _run(gpu, form, a, b, kt, descending)


# ---- the stable pairs sort of the concatenation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U32, F64))
def test_merge_by_key_is_the_stable_pairs_sort_of_the_concatenation(gpu, kt):
    torch = _torch()
    T = _plan(kt)["tile"]
    na, nb = 2 * T - 5, T + 10
    a, b = _sorted(draws(kt, na, 60, distinct=500), kt, False), _sorted(draws(kt, nb, 61, distinct=500), kt, False)
    as_keys = (lambda t: t.view(torch.float64)) if kt == F64 else (lambda t: t)
    da, db = as_keys(_dev(a)), as_keys(_dev(b))
    pos = torch.arange(na + nb, dtype=torch.int32, device="cuda")
    keys, vals = _m().merge_by_key(da, pos[:na].clone(), db, pos[na:].clone(), unsigned=kt == U32)
    sk, sv = torch.cat([da, db]), pos.clone()
    sorter = gpu.OneSweep(na + nb, key_type=gpu.KEY_FLOAT64 if kt == F64 else gpu.KEY_UINT32, mode=gpu.MODE_PAIRS, value_bytes=4)
    sorter.sort(sk, sv)
    sorter.check()
    assert keys.dtype == da.dtype and vals.dtype == torch.int32
    np.testing.assert_array_equal(_host(keys.view(torch.int64) if kt == F64 else keys), _host(sk.view(torch.int64) if kt == F64 else sk))
    np.testing.assert_array_equal(_host(vals), _host(sv))
    sorter.close()


# ---- the buffer contract ---------------------------------------------------------------------------------------------------------------
def _arena_call(gpu, form, a, b, kt, fill, slack=100, descending=False):
    """`form` on views of one guard arena that are 16-byte and not 32-byte aligned, the outputs `slack` elements longer than na + nb;
    returns (arena, out_keys view, second output view or None, n)."""
    h = _handle(gpu, kt)
    kd = word_dtype(kt)
    na, nb, n = a.size, b.size, a.size + b.size
    width = {"pairs4": 4, "pairs8": 8, "positions": 4}.get(form)
    vd = np.uint64 if width == 8 else np.uint32
    specs = [(na, kd), (nb, kd), (n + slack, kd)] + ([(n + slack, vd)] if width else []) + ([(na, vd), (nb, vd)] if form.startswith("pairs") else [])
    arena = Arena.for_views(specs, "cuda", fill=fill)
    va_, vb_, vo = arena.carve(na, kd, 1, "a"), arena.carve(nb, kd, 3, "b"), arena.carve(n + slack, kd, 5, "out_keys")
    arena.write(va_, a)
    arena.write(vb_, b)
    arena.live(vo, n)
    order = _order(gpu, descending)
    aux = None
    if form == "keys":
        h.merge(va_, vb_, na, nb, out=vo, key_type=kt, order=order)
    elif form == "positions":
        aux = arena.carve(n + slack, vd, 7, "out_src")
        arena.live(aux, n)
        h.merge_positions(va_, vb_, na, nb, out_keys=vo, out_src=aux, key_type=kt, order=order)
    else:
        aux = arena.carve(n + slack, vd, 7, "out_values")
        arena.live(aux, n)
        xa, xb = arena.carve(na, vd, 9, "a_values"), arena.carve(nb, vd, 11, "b_values")
        arena.write(xa, _values(na, width, 1))
        arena.write(xb, _values(nb, width, 2))
        h.merge_pairs(va_, xa, vb_, xb, na, nb, out_keys=vo, out_values=aux, key_type=kt, order=order)
    _torch().cuda.synchronize()
    return arena, vo, aux, n


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
def test_buffer_contract_on_16_byte_aligned_views_with_guard_bands(gpu, fill):
    """Every form on 16-byte-only aligned views with guard bands, the outputs longer than na + nb: the result is the reference's, the
    tails and the bands are untouched, the inputs unchanged."""
    for kt in (I32, U64):
        T = _plan(kt)["tile"]
        na, nb = T + 13, T // 2 + 2
        a, b = _sorted(draws(kt, na, 70, distinct=200), kt, False), _sorted(draws(kt, nb, 71, distinct=200), kt, False)
        for form in FORMS:
            width = {"pairs4": 4, "pairs8": 8}.get(form)
            want = _m().merge_reference(a, b, kt, False, *((_values(na, width, 1), _values(nb, width, 2)) if width else ()))
            arena, vo, aux, n = _arena_call(gpu, form, a, b, kt, fill)
            arena.verify()
            np.testing.assert_array_equal(_host(vo, n), want[0])
            if aux is not None:
                np.testing.assert_array_equal(_host(aux, n), want[2] if width else want[1])


# ---- unsorted inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (I32, F64))
def test_unsorted_inputs_end_and_write_every_slot_once(gpu, kt):
    """Ordinary calls on inputs that are not sorted (random, and sorted the wrong way round): the output is unspecified, but the call
    returns, the guard bands and the tails are intact, every output slot was written (the outputs are pre-filled with 0xFF bytes, a
    pattern neither the keys nor the values nor a position hold) and every position is below na + nb."""
    T = _plan(kt)["tile"]
    dt = word_dtype(kt)
    rng = np.random.default_rng(80 + kt)
    na, nb = 2 * T + 5, T - 3
    n = na + nb
    unfilled = dt(~dt(0))
    random = (rng.integers(0, 1000, na).astype(dt), rng.integers(0, 1000, nb).astype(dt))
    backwards = (np.sort(random[0])[::-1].copy(), np.sort(random[1])[::-1].copy())
    one_sided = (np.sort(random[0]), random[1])
    for a, b in (random, backwards, one_sided):
        for form in FORMS:
            arena, vo, aux, n = _arena_call(gpu, form, a, b, kt, 0xFF)
            arena.verify()
            assert not (_host(vo, n) == unfilled).any(), (form, "an output key slot was not written")
            if form == "positions":
                src = _host(aux, n)
                assert (src < n).all(), (form, src.max())
            elif aux is not None:
                width = aux.element_size()
                got = _host(aux, n)
                assert not (got == got.dtype.type(~got.dtype.type(0))).any(), (form, "an output value slot was not written")
                known = np.concatenate([_values(na, width, 1), _values(nb, width, 2)])
                assert np.isin(got, known).all(), (form, "a value that no input holds")
    assert _handle(gpu, kt).last()["tiles"] == _m().merge_plan(na, nb, 8 if kt >= U64 else 4)["grid"]


# ---- argument errors behind the handle -------------------------------------------------------------------------------------------------
def test_argument_errors_in_the_order_of_the_header(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    cap = 4096
    h, h8 = _m().Merge(cap, U32), _m().Merge(cap, U64)
    buf = torch.zeros(8 * cap, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    a, b, out, aux, av, bv = (p + i * 8 * cap for i in range(6))
    ok_keys = lambda **kw: lib.gs_merge_keys(h._h, kw.get("a", a), kw.get("na", 100), kw.get("b", b), kw.get("nb", 50), kw.get("out", out),  # noqa: E731
                                             kw.get("kt", U32), kw.get("order", 0), None)
    ok_pairs = lambda **kw: lib.gs_merge_pairs(h._h, kw.get("a", a), kw.get("av", av), kw.get("na", 100), kw.get("b", b), kw.get("bv", bv),  # noqa: E731
                                               kw.get("nb", 50), kw.get("out", out), kw.get("aux", aux), kw.get("vb", 4), kw.get("kt", U32),
                                               kw.get("order", 0), None)
    ok_pos = lambda **kw: lib.gs_merge_positions(h._h, kw.get("a", a), kw.get("na", 100), kw.get("b", b), kw.get("nb", 50), kw.get("out", out),  # noqa: E731
                                                 kw.get("aux", aux), kw.get("kt", U32), kw.get("order", 0), None)

    def refused(status, want):
        assert status == want, (status, want)
        assert h.last()["form"] == NONE  # a refused call leaves no form behind

    assert ok_keys() == 0 and h.last()["form"] == KEYS
    # 2: pointers of non-empty sides and of outputs, key types, orders
    for kw in ({"a": None}, {"b": None}, {"out": None}, {"a": a + 8}, {"b": b + 4}, {"out": out + 8}):
        refused(ok_keys(**kw), A)
    for kw in ({"aux": None}, {"aux": aux + 8}, {"av": None}, {"bv": None}, {"av": av + 8}, {"bv": bv + 4}):
        refused(ok_pairs(**kw), A)
    for kw in ({"aux": None}, {"aux": aux + 4}):
        refused(ok_pos(**kw), A)
    for kt in (U64, I64, F64, 6, 7, 8, 9, 10, -1):  # a width that is not the handle's, the 16-bit ones included
        refused(ok_keys(kt=kt), A)
        refused(ok_pairs(kt=kt, vb=3), A)  # in front of the value width
    refused(lib.gs_merge_keys(h8._h, a, 100, b, 50, out, U32, 0, None), A)
    assert lib.gs_merge_keys(h8._h, a, 100, b, 50, out, I64, 1, None) == 0
    for order in (2, -1):
        refused(ok_keys(order=order), A)
        refused(ok_pos(order=order, na=0, nb=0), A)  # in front of the sizes
    # 3: the value width, in front of the sizes and of the overlap
    for vb in (0, 1, 2, 3, 16):
        refused(ok_pairs(vb=vb), M)
        refused(ok_pairs(vb=vb, na=0, nb=0), M)
        refused(ok_pairs(vb=vb, aux=out), M)
    # 4: the sizes, the sum in 64 bits, in front of the overlap
    for na, nb in ((0, 0), (cap, 1), (1, cap), (0xFFFFFFFF, 1), (0x80000000, 0x80000000), (0xFFFFFFFF, 0xFFFFFFFF)):
        refused(ok_keys(na=na, nb=nb), S)
        refused(ok_pairs(na=na, nb=nb, aux=out), S)
        refused(ok_pos(na=na, nb=nb), S)
    assert ok_keys(na=cap - 1, nb=1) == 0
    # 5: any two buffers overlapping
    for kw in ({"out": a}, {"out": a + 16}, {"b": a + 16 * 4}, {"out": b + 16}):
        refused(ok_keys(**kw), A)
    for kw in ({"aux": out}, {"aux": a}, {"av": a}, {"bv": out + 16}, {"av": bv}, {"aux": av + 32}):
        refused(ok_pairs(**kw), A)
    refused(ok_pos(aux=out + 64), A)
    # an empty side has no bytes: a null pointer, or any pointer, misaligned or inside another buffer
    for kw in ({"a": None, "na": 0}, {"b": None, "nb": 0}, {"a": out + 4, "na": 0}, {"b": a + 3, "nb": 0}):
        assert ok_keys(**kw) == 0, kw
        assert ok_pos(**kw) == 0, kw
    assert ok_pairs(a=None, av=None, na=0) == 0 and ok_pairs(b=None, bv=None, nb=0) == 0
    rep = h.last()
    assert (rep["form"], rep["na"], rep["nb"]) == (PAIRS, 100, 0)
    # the report's own arguments
    words = (C.c_uint32 * 16)()
    assert lib.gs_merge_last(h._h, None, 16, None) == A and lib.gs_merge_last(h._h, words, 15, None) == A
    torch.cuda.synchronize()
    h.close()
    h8.close()


def test_empty_side_as_a_null_pointer_gives_the_other_side(gpu):
    T = _plan(U32)["tile"]
    torch = _torch()
    a = _sorted(draws(F32, T + 9, 90), F32, True)
    da = _dev(a)
    h = _handle(gpu, F32)
    for form in ("keys", "positions", "pairs"):
        for left in (True, False):
            x, y = (da, None) if left else (None, da)
            if form == "keys":
                out, aux = h.merge(x, y, key_type=F32, order=gpu.ORDER_DESCENDING), None
            elif form == "positions":
                out, aux = h.merge_positions(x, y, key_type=F32, order=gpu.ORDER_DESCENDING)
            else:
                v = torch.arange(a.size, dtype=torch.int64, device="cuda")
                out, aux = h.merge_pairs(x, v if left else None, y, None if left else v, key_type=F32, order=gpu.ORDER_DESCENDING)
            np.testing.assert_array_equal(_host(out), a)
            if aux is not None:
                np.testing.assert_array_equal(aux.cpu().numpy(), np.arange(a.size))
            rep = h.last()
            assert rep["copy_tiles"] == rep["tiles"] == 2 and (rep["na"], rep["nb"]) == ((a.size, 0) if left else (0, a.size))


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("keys", "pairs8", "positions"))
def test_captured_graph_replayed_on_changed_contents(gpu, form):
    """One call captured on one stream and replayed on other contents of the same (na, nb), the second time with the sides' roles
    swapped (B holds the smaller keys): no host wait, the grid fixed by na + nb."""
    torch = _torch()
    kt, descending = I64, True
    T = _plan(kt)["tile"]
    na, nb = 2 * T + 77, T - 5
    h = _m().Merge(na + nb, kt, gpu.ORDER_DESCENDING)

    def inputs(seed, swapped=False):
        pool = draws(kt, na + nb, seed, distinct=3000)
        if swapped:  # every B in front of every A but for a few
            s = _sorted(pool, kt, descending)
            return _sorted(np.concatenate([s[nb + 3:], s[:3]]), kt, descending), s[3:nb + 3].copy()
        return _sorted(pool[:na], kt, descending), _sorted(pool[na:], kt, descending)

    a, b = inputs(100)
    va, vb = _values(na, 8, 1), _values(nb, 8, 2)
    da, db, dva, dvb = _dev(a), _dev(b), _dev(va), _dev(vb)
    out = torch.full((na + nb,), SENTINEL, dtype=torch.int64, device="cuda")
    aux = torch.full((na + nb,), SENTINEL, dtype=torch.int32 if form == "positions" else torch.int64, device="cuda")

    def call():
        if form == "keys":
            h.merge(da, db, out=out)
        elif form == "positions":
            h.merge_positions(da, db, out_keys=out, out_src=aux)
        else:
            h.merge_pairs(da, dva, db, dvb, out_keys=out, out_values=aux)

    def compare(a, b):
        want = _m().merge_reference(a, b, kt, descending, va, vb)
        np.testing.assert_array_equal(_host(out), want[0])
        if form != "keys":
            np.testing.assert_array_equal(_host(aux), want[1] if form == "positions" else want[2])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    compare(a, b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seed, swapped in ((200, False), (300, True)):
        a, b = inputs(seed, swapped)
        da.copy_(_dev(a))
        db.copy_(_dev(b))
        out.fill_(SENTINEL)
        aux.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        compare(a, b)
        rep = h.last()
        assert (rep["na"], rep["nb"], rep["tiles"]) == (na, nb, rep["plan"]["grid"]) and rep["plan"] == _m().merge_plan(na, nb, 8)
    h.close()


# ---- the tensor functions --------------------------------------------------------------------------------------------------------------
def test_tensor_functions_dtypes_unsigned_descending_and_the_cache(gpu):
    torch = _torch()
    m = _m()
    T = _plan(U32)["tile"]
    cases = [(torch.int32, I32, False), (torch.int32, U32, True), (torch.float32, F32, False), (torch.int64, I64, False),
             (torch.int64, U64, True), (torch.float64, F64, False)]
    for dt in ("uint32", "uint64"):
        if hasattr(torch, dt):
            cases.append((getattr(torch, dt), U32 if dt == "uint32" else U64, False))
    for dtype, kt, unsigned in cases:
        for descending in (False, True):
            a, b = _sorted(draws(kt, T + 5, 110 + kt, distinct=99), kt, descending), _sorted(draws(kt, 70, 120 + kt, distinct=99), kt, descending)
            da, db = _dev(a).view(dtype), _dev(b).view(dtype)
            want_keys, want_src = m.merge_reference(a, b, kt, descending)
            bits = lambda t: _host(t.view(torch.int64 if t.element_size() == 8 else torch.int32))  # noqa: E731
            got = m.merge(da, db, descending=descending, unsigned=unsigned)
            assert got.dtype == dtype and got.shape == (a.size + b.size,)
            np.testing.assert_array_equal(bits(got), want_keys)
            keys, src = m.argmerge(da, db, descending=descending, unsigned=unsigned)
            assert keys.dtype == dtype and src.dtype == torch.int32
            np.testing.assert_array_equal(bits(keys), want_keys)
            np.testing.assert_array_equal(_host(src), want_src)
            sdt = torch.int64 if da.element_size() == 8 else torch.int32
            assert torch.equal(torch.cat([da.view(sdt), db.view(sdt)])[src.long()], keys.view(sdt))  # any payload is gathered through src
            for vdtype in (torch.float32, torch.int64, torch.float64, torch.int32):
                va = torch.arange(a.size, device="cuda").to(vdtype)
                vb = (torch.arange(b.size, device="cuda") + 100000).to(vdtype)
                keys, vals = m.merge_by_key(da, va, db, vb, descending=descending, unsigned=unsigned)
                assert keys.dtype == dtype and vals.dtype == vdtype
                np.testing.assert_array_equal(bits(keys), want_keys)
                assert torch.equal(vals, torch.cat([va, vb])[src.long()])
    # empty sides, and both
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    x = torch.tensor([-0.0, 0.0, 1.0], device="cuda")
    assert m.merge(e, e).numel() == 0 and m.argmerge(e, e)[1].dtype == torch.int32 and m.merge_by_key(e, e, e, e)[1].numel() == 0
    assert torch.equal(m.merge(x, e).view(torch.int32), x.view(torch.int32)) and torch.equal(m.merge(e, x).view(torch.int32), x.view(torch.int32))
    assert m.argmerge(e, x)[1].tolist() == [0, 1, 2]
    # one handle per (device, stream, key width): reused by every call above, re-created when a call outgrows it
    key32 = (x.device.index, int(torch.cuda.current_stream(x.device).cuda_stream), False)
    h = m._merge_cache[key32]
    assert h.key_bytes == 4 and h.max_keys >= T + 75
    m.merge(x, x.clone())
    assert m._merge_cache[key32] is h and h.last()["form"] == KEYS
    with pytest.raises(m._lib.GpuSortError):
        m.merge(x, x)  # one buffer as both sides: no buffer of a call may overlap another
    big = torch.arange(h.max_keys, dtype=torch.int32, device="cuda")
    got = m.merge(big, x.view(torch.int32)[:1])
    assert m._merge_cache[key32] is not h and m._merge_cache[key32].max_keys > h.max_keys and got.numel() == big.numel() + 1
    with pytest.raises(TypeError):
        m.merge(big.to(torch.int16), big.to(torch.int16))
    with pytest.raises(ValueError):
        m.merge(big, big.cpu())
