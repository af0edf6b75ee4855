"""GPU tests of the sorted search (gs_search_* in include/gpusort.h, gpusorting_amd/search.py, functional.searchsorted).  Every result
is compared exactly, position by position, with searchsorted_reference (tests/test_search_cpu.py checks that one against a brute-force
count).  Shapes come from gs_search_plan (T queries per tile, a window of W keys, S keys per sample) and are the smallest at which
each mechanism can go wrong; routes are forced, so nothing depends on where the AUTO rule's boundary lies.  BINARY runs in both of
its forms: with the sample table ("table") and with every level in global memory ("plain")."""
import numpy as np
import pytest

from guard_arena import Arena
from test_search_cpu import F32, F64, I32, I64, KEY_TYPES, U32, U64, draws, sort_as_library, specials, word_dtype

pytestmark = pytest.mark.gpu

NONE, TILE, SORT, BINARY = 0, 1, 2, 3
FORMS = ("tile", "sort", "table", "plain")  # what a test runs: a route, BINARY in either form
MAXN, MAXM = 1 << 17, 1 << 15
SENTINEL = -7


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()


def _host(t, n=None):
    t = t if n is None else t[:n]
    return t.cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


def _plan(gpu, n, m, kt=U32):
    return gpu.search_plan(n, m, 8 if kt >= U64 else 4)


_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _handle(gpu, kt, engine=True):
    """One handle of capacity (MAXN, MAXM) per (key width, with the engine) for the whole file: every test is a reuse of it as well."""
    key = (kt >= U64, engine)
    if key not in _handles:
        _handles[key] = gpu.SortedSearch(MAXN, MAXM, U64 if kt >= U64 else U32, sort_queries=engine)
    return _handles[key]


def _force(h, form):
    from gpusorting_amd import search
    h.set_route({"tile": TILE, "sort": SORT}.get(form, BINARY))
    h.set_table({"table": search.TABLE_ON, "plain": search.TABLE_OFF}.get(form, search.TABLE_AUTO))


def _search(gpu, h, form, hay, queries, kt=U32, descending=False, right=False, want=None):
    """Runs `form` on the bit patterns hay / queries (for "tile" the queries must be in order), compares every position with the
    reference (or with `want`), checks the report and that neither input was written; returns the report."""
    n, m = hay.size, queries.size
    if want is None:
        want = gpu.searchsorted_reference(hay, queries, kt, descending, right)
    dh, dq = _dev(hay), _dev(queries)
    out = _torch().full((m + 64,), SENTINEL, dtype=_torch().int32, device="cuda")
    _force(h, form)
    st, _ = h.status(dh, dq, n, m, right=right, queries_sorted=form == "tile", out=out, key_type=kt,
                     order=gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING)
    assert st == 0, (form, st)
    got = _host(out, m)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (form, kt, descending, right, n, m, bad[:5], got[bad[:5]], want[bad[:5]])
    assert bool((out[m:] == SENTINEL).all()), "written behind element m of out"
    np.testing.assert_array_equal(_host(dh), hay)
    np.testing.assert_array_equal(_host(dq), queries)
    rep = h.last()
    assert (rep["route"], rep["n"], rep["m"]) == ({"tile": TILE, "sort": SORT}.get(form, BINARY), n, m)
    assert rep["plan"] == _plan(gpu, n, m, kt)
    if form in ("table", "plain"):
        assert rep["table"] == (form == "table")
    else:
        assert rep["lds_tiles"] + rep["global_tiles"] == rep["plan"]["tile_grid"]
    return rep


def _all_forms(gpu, hay, queries, kt=U32, descending=False, right=False, forms=FORMS):
    """Every form on one input: the queries as they lie for sort / table / plain, in the haystack's order for tile."""
    want = gpu.searchsorted_reference(hay, queries, kt, descending, right)
    reps = {}
    for form in forms:
        if form == "tile":
            qs = sort_as_library(queries, kt, descending)
            reps[form] = _search(gpu, _handle(gpu, kt), form, hay, qs, kt, descending, right)
        else:
            reps[form] = _search(gpu, _handle(gpu, kt, engine=form == "sort"), form, hay, queries, kt, descending, right, want)
    return reps


# ---- TILE: the window at its cap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("kt", (U32, U64))
def test_tile_windows_one_below_at_and_one_above_the_cap(gpu, kt, right):
    """Three tiles of T queries in one launch whose windows are exactly W - 1, W and W + 1 keys: the LDS form, its edge, and the search
    in global memory narrowed to the window, side by side.  The first window starts at an index that is no multiple of a 16-byte piece."""
    p = _plan(gpu, MAXN, MAXM, kt)
    T, W = p["tile"], p["window"]
    dt = word_dtype(kt)
    a = [5]
    for t in range(3):
        a.append(a[-1] + W - 1 + t)
    n = a[-1] + 7  # about 3 W
    hay = (np.arange(n, dtype=dt) * dt(2) + dt(10))  # distinct, even: odd queries miss
    rng = np.random.default_rng(7)
    tiles = []
    for t in range(3):
        inner = np.sort(rng.integers(int(hay[a[t]]), int(hay[a[t + 1] - 1]) + 1, T - 2).astype(dt))
        tiles.append(np.concatenate([[hay[a[t]]], inner, [hay[a[t + 1] - 1]]]).astype(dt))  # LEFT of the first: a[t]; RIGHT of the last: a[t + 1]
    queries = np.concatenate(tiles)
    rep = _search(gpu, _handle(gpu, kt), "tile", hay, queries, kt, False, right)
    assert (rep["lds_tiles"], rep["global_tiles"]) == (2, 1)
    rep = _search(gpu, _handle(gpu, kt), "sort", hay, np.random.default_rng(8).permutation(queries), kt, False, right)
    assert (rep["lds_tiles"], rep["global_tiles"]) == (2, 1)


# ---- TILE: small and empty cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (I32, F64))
def test_tile_small_sizes_and_empty_windows(gpu, kt):
    T = _plan(gpu, 1, 1, kt)["tile"]
    rng = np.random.default_rng(11)
    pool = draws(kt, 40, 12)
    h = _handle(gpu, kt)
    for n in (1, 2, 63, 64, 65):
        for m in (1, T - 1, T, T + 1, 2 * T + 3):
            for descending in (False, True):
                hay = sort_as_library(pool[rng.integers(0, pool.size, n)], kt, descending)
                queries = sort_as_library(pool[rng.integers(0, pool.size, m)], kt, descending)
                _search(gpu, h, "tile", hay, queries, kt, descending, right=bool((n + m) & 1))
    # a window of length 0: every query in front of the first key, or behind the last one
    mid = sort_as_library(draws(kt, 3000, 13), kt, False)
    hay, below, above = mid[1000:2000], mid[:1000], mid[2000:]
    for right in (False, True):
        for q, at in ((below, 0), (above, hay.size)):
            rep = _search(gpu, h, "tile", hay, q, kt, False, right)
            assert rep["lds_tiles"] == 1 and (gpu.searchsorted_reference(hay, q, kt, False, right) == at).all()
            _search(gpu, h, "tile", hay[::-1].copy(), q[::-1].copy(), kt, True, right)


# ---- duplicates across every boundary ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U32, I64))
def test_a_run_longer_than_the_window_and_the_sample_stride(gpu, kt):
    """One key repeated W + 100 times in a haystack large enough for S >= 2, queried with that key by more than a tile of equal queries:
    LEFT and RIGHT differ by the run's length, on every form; a window or sample off by one shows here."""
    p = _plan(gpu, MAXN, MAXM, kt)
    T, W = p["tile"], p["window"]
    dt = word_dtype(kt)
    run = W + 100
    lowkeys = sort_as_library(draws(kt, 10000, 21), kt, False)  # enough other keys for a haystack behind a full sample table
    key = lowkeys[4000]
    hay = np.concatenate([lowkeys[:4000][lowkeys[:4000] != key], np.full(run, key, dt), lowkeys[4001:][lowkeys[4001:] != key]])
    start = int(np.flatnonzero(hay == key)[0])
    assert _plan(gpu, hay.size, T + 5, kt)["stride"] >= 2 and run > W
    same = np.full(T + 5, key, dt)
    mixed = np.concatenate([same[:T], lowkeys[::3]])
    for descending in (False, True):
        hy = hay[::-1].copy() if descending else hay
        first = hy.size - start - run if descending else start
        for right in (False, True):
            want = np.full(T + 5, first + (run if right else 0), np.uint32)
            np.testing.assert_array_equal(gpu.searchsorted_reference(hy, same, kt, descending, right), want)
            reps = _all_forms(gpu, hy, same, kt, descending, right)
            assert reps["tile"]["global_tiles"] == 2 and reps["sort"]["global_tiles"] == 2  # one run wider than W: no tile fits LDS
            _all_forms(gpu, hy, mixed, kt, descending, right)


@pytest.mark.parametrize("kt", (F32, U64))
def test_haystack_all_equal(gpu, kt):
    sp = sort_as_library(specials(kt), kt, False)
    key = sp[5]
    for n in (1, 64, 5000, 20000):
        hay = np.full(n, key, word_dtype(kt))
        queries = np.concatenate([np.full(100, key, word_dtype(kt)), sp, sp[::-1]])
        for descending in (False, True):
            for right in (False, True):
                _all_forms(gpu, hay, queries, kt, descending, right)


# ---- BINARY: around every sample ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (U32, U64))
def test_binary_sizes_and_queries_around_the_samples(gpu, kt):
    """n one below, at and one above samples * S for S = 1, 2, 4 (the first size of each triple behind a full table doubles S); queries
    on hay[t S - 1], hay[t S], hay[t S + 1], the first and the last key, the values between keys and outside the haystack; runs of
    three equal keys lie across the samples.  The table form and the plain form on the same inputs."""
    dt = word_dtype(kt)
    cap = 65536 // dt().itemsize  # the table's capacity in samples: 64 KiB of words
    seen = set()
    for mult in (1, 2, 4):
        for n in (cap * mult - 1, cap * mult, cap * mult + 1):
            S = _plan(gpu, n, 1, kt)["stride"]
            assert S == (mult if n <= cap * mult else 2 * mult) and _plan(gpu, n, 1, kt)["samples"] == n // S
            seen.add(S)
            hay = (np.arange(n, dtype=dt) // dt(3)) * dt(2) + dt(2)
            t = np.unique(np.concatenate([np.arange(1, 6), np.arange(n // S - 4, n // S + 1), np.random.default_rng(n).integers(1, n // S, 40)]))
            idx = np.concatenate([t * S - 1, t * S, t * S + 1, [0, n - 1]])
            idx = idx[(idx >= 0) & (idx < n)]
            queries = np.concatenate([hay[idx], hay[idx] + dt(1), hay[idx] - dt(1), np.array([0, 1, int(hay[-1]) + 5], dtype=dt)])
            for right in (False, True):
                want = gpu.searchsorted_reference(hay, queries, kt, False, right)
                for form in ("table", "plain"):
                    _search(gpu, _handle(gpu, kt, engine=False), form, hay, queries, kt, False, right, want)
                hr = hay[::-1].copy()
                _search(gpu, _handle(gpu, kt, engine=False), "table", hr, queries, kt, True, right)
    assert seen == {1, 2, 4, 8}


# ---- SORT: results land at the original positions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", (F32, I64))
def test_sort_route_on_shuffled_queries_with_duplicates(gpu, kt):
    T = _plan(gpu, 1, 1, kt)["tile"]
    hay = sort_as_library(draws(kt, 30011, 41, distinct=4000), kt, False)
    for m in (1, T - 1, T, T + 1, 2 * T + 3):
        queries = draws(kt, m, 42 + m, distinct=max(1, m // 3))  # shuffled, with duplicates (_search checks the slots behind m)
        for descending in (False, True):
            _search(gpu, _handle(gpu, kt), "sort", hay[::-1].copy() if descending else hay, queries, kt, descending, right=bool(m & 1))


# ---- all types, orders and sides on every form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("descending", (False, True), ids=("asc", "desc"))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_types_orders_and_sides(gpu, kt, descending, right):
    hay = sort_as_library(draws(kt, 50021, 50 + kt, distinct=20000), kt, descending)
    queries = np.concatenate([draws(kt, 12000, 60 + kt), hay[np.random.default_rng(61).integers(0, hay.size, 8003)]])
    reps = _all_forms(gpu, hay, queries, kt, descending, right)
    assert reps["tile"]["lds_tiles"] + reps["tile"]["global_tiles"] == -(-queries.size // reps["tile"]["plan"]["tile"])


def test_a_haystack_sorted_descending_by_this_library_round_trips(gpu):
    """float32 keys with NaNs of both signs, infinities and signed zeros, sorted descending by gpusorting_amd.sort, searched by
    gpusorting_amd.searchsorted: hay[out - 1] and hay[out] bracket every query in the flipped order."""
    from gpusorting_amd.search import _words
    torch = _torch()
    keys = draws(F32, 40009, 71, distinct=9000)
    queries = np.concatenate([draws(F32, 9000, 72), keys[::5]])
    dh = gpu.sort(_dev(keys).view(torch.float32), descending=True)
    hay = _host(dh.view(torch.int32))
    np.testing.assert_array_equal(hay, sort_as_library(keys, F32, True))
    wh = _words(hay, F32, True).astype(np.uint64)
    for right in (False, True):
        for qs in (False, True):
            q = sort_as_library(queries, F32, True) if qs else queries
            wq = _words(q, F32, True).astype(np.uint64)
            out = gpu.searchsorted(dh, _dev(q).view(torch.float32), right=right, descending=True, queries_sorted=qs)
            assert out.dtype == torch.int32 and out.shape == (q.size,)
            o = out.cpu().numpy().astype(np.int64)
            np.testing.assert_array_equal(o, gpu.searchsorted_reference(hay, q, F32, True, right))
            lo_ok = (o == 0) | ((wh[np.maximum(o - 1, 0)] <= wq) if right else (wh[np.maximum(o - 1, 0)] < wq))
            hi_ok = (o == hay.size) | ((wh[np.minimum(o, hay.size - 1)] > wq) if right else (wh[np.minimum(o, hay.size - 1)] >= wq))
            assert lo_ok.all() and hi_ok.all()
    # the functional corner cases: empty haystack, empty queries, a shape, bucketize
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    assert gpu.searchsorted(e, dh[:5].clone()).tolist() == [0] * 5 and gpu.searchsorted(dh, e).shape == (0,)
    assert gpu.searchsorted(dh, dh[:6].clone().reshape(2, 3), descending=True).shape == (2, 3)
    b = torch.tensor([1, 3, 5, 7], dtype=torch.int32, device="cuda")
    v = torch.tensor([[0, 1, 2], [7, 8, 3]], dtype=torch.int32, device="cuda")
    for right in (False, True):
        assert torch.equal(gpu.bucketize(v, b, right=right), torch.bucketize(v, b, right=right).to(torch.int32))


@pytest.mark.parametrize("dtype", ("int32", "int64"))
def test_agreement_with_torch_searchsorted_on_integers(gpu, dtype):
    torch = _torch()
    dt = getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(5)
    lim = 3000 if dtype == "int32" else 1 << 40
    hay = torch.sort(torch.randint(-lim, lim, (60001,), generator=g, device="cuda", dtype=dt)).values
    q = torch.randint(-lim - 5, lim + 5, (20003,), generator=g, device="cuda", dtype=dt)
    qs = torch.sort(q).values
    for right in (False, True):
        assert torch.equal(gpu.searchsorted(hay, q, right=right), torch.searchsorted(hay, q, right=right).to(torch.int32))
        assert torch.equal(gpu.searchsorted(hay, qs, right=right, queries_sorted=True), torch.searchsorted(hay, qs, right=right).to(torch.int32))
        kt = I32 if dtype == "int32" else I64
        for form in FORMS:
            h = _handle(gpu, kt, engine=form != "table")
            _force(h, form)
            st, out = h.status(hay, qs if form == "tile" else q, right=right, queries_sorted=form == "tile", key_type=kt)
            assert st == 0 and torch.equal(out, torch.searchsorted(hay, qs if form == "tile" else q, right=right).to(torch.int32)), form


# ---- the memory contract ------------------------------------------------------------------------------------------------------------
def _arena_call(gpu, kt, form, fill, hay, queries, count_h, count_q, descending=False, right=False, queries_sorted=None):
    """One call on 16-byte-only aligned views with guard bands, n and m below the views' counts; returns (status, positions)."""
    dt = word_dtype(kt)
    n, m = hay.size, queries.size
    arena = Arena.for_views([(count_h, dt), (count_q, dt), (count_q, np.uint32)], "cuda", fill=fill)
    vh, vq, vo = arena.carve(count_h, dt, skew=1, name="hay"), arena.carve(count_q, dt, skew=3, name="queries"), arena.carve(count_q, np.uint32, skew=5, name="out")
    arena.write(vh, hay)
    arena.write(vq, queries)
    arena.live(vo, m)
    h = _handle(gpu, kt, engine=form in ("tile", "sort"))
    _force(h, form)
    st, _ = h.status(vh, vq, n, m, right=right, queries_sorted=(form == "tile") if queries_sorted is None else queries_sorted, out=vo, key_type=kt,
                     order=gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING)
    _torch().cuda.synchronize()
    got = arena.read(vo, np.uint32, m)
    arena.verify()
    return st, got


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kt", (F32, U64))
def test_guard_bands_and_16_byte_alignment(gpu, kt, form, fill):
    """n and m below the views' counts and no multiple of anything: what lies behind them is the fill (as a key the smallest, the largest,
    or noise) and must neither be read into a result nor written."""
    p = _plan(gpu, MAXN, MAXM, kt)
    n, m = 2 * p["window"] + 1237, 2 * p["tile"] + 77
    descending = fill == 0xFF
    hay = sort_as_library(draws(kt, n, 81, distinct=n // 2), kt, descending)
    queries = draws(kt, m, 82)
    if form == "tile":
        queries = sort_as_library(queries, kt, descending)
    st, got = _arena_call(gpu, kt, form, fill, hay, queries, n + 4099, m + 1031, descending, right=fill == "hash")
    assert st == 0
    np.testing.assert_array_equal(got, gpu.searchsorted_reference(hay, queries, kt, descending, fill == "hash"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kt", (I32, F64))
def test_unsorted_input_stays_inside_the_buffers(gpu, kt, form):
    """The haystack's order is not checked: on an unsorted haystack, and on queries falsely declared sorted, the positions are
    unspecified.  The call still returns GS_OK, every position is <= n and the bands are intact."""
    p = _plan(gpu, MAXN, MAXM, kt)
    n, m = 2 * p["window"] + 1237, 2 * p["tile"] + 77
    hay, queries = draws(kt, n, 91), draws(kt, m, 92)
    for right in (False, True):
        st, got = _arena_call(gpu, kt, form, "hash", hay, queries, n + 4099, m + 1031, right=right)  # (tile: queries declared sorted, falsely)
        assert st == 0 and int(got.max()) <= n
    st, got = _arena_call(gpu, kt, form, 0xFF, sort_as_library(hay, kt, False), queries, n + 4099, m + 1031, queries_sorted=True)
    assert st == 0 and int(got.max()) <= n  # a sorted haystack, queries falsely declared sorted, on every route


# ---- refusals that need a handle, the report ----------------------------------------------------------------------------------------
def test_argument_errors_and_the_report(gpu):
    import ctypes as C
    from gpusorting_amd import _lib, search
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    torch = _torch()
    n, m = 5000, 3000
    h = gpu.SortedSearch(n, m, U32, sort_queries=False)
    assert h.last()["route"] == NONE and h.last()["engine"] == 0
    assert h.temp_bytes == search.temp_bytes(n, m, 4, False) == 256 + 65536
    hay = torch.arange(n, dtype=torch.int32, device="cuda")
    q = torch.arange(m, dtype=torch.int32, device="cuda")
    out = torch.full((m,), SENTINEL, dtype=torch.int32, device="cuda")
    raw = lambda *a: lib.gs_search_sorted(h._h, *a, None)  # noqa: E731
    ok = (hay.data_ptr(), n, q.data_ptr(), m, out.data_ptr(), U32, 0, 0, 0)
    for i in (0, 2, 4):  # a null and a misaligned pointer in each place
        for bad in (None, ok[i] + 4):
            assert raw(*(ok[:i] + (bad,) + ok[i + 1:])) == A
    for kt in (U64, I64, F64, 6, 7, 8, 9, 10, -1):  # the other width, the 16-bit key types, no key type
        assert raw(*(ok[:5] + (kt,) + ok[6:])) == A, kt
    assert raw(*(ok[:6] + (2,) + ok[7:])) == A and raw(*(ok[:7] + (2,) + ok[8:])) == A  # order, side
    h.set_route("sort")
    assert raw(*ok) == M and raw(*(ok[:1] + (0,) + ok[2:])) == M  # needs the engine: answered in front of the sizes
    h.set_route("auto")
    for nn, mm in ((0, m), (n, 0), (n + 1, m), (n, m + 1)):
        assert raw(ok[0], nn, ok[2], mm, *ok[4:]) == S
    assert raw(ok[0], n, ok[0], m, *ok[4:]) == A and raw(ok[0], n, ok[2], m, ok[2] + 16, *ok[5:]) == A  # overlap
    assert h.last()["route"] == NONE and bool((out == SENTINEL).all())  # a refused call launches nothing
    assert raw(*ok) == 0 and h.last()["route"] == BINARY and h.last()["table"] == gpu.search_plan(n, m)["table"]  # AUTO without the engine: BINARY
    assert out.tolist() == list(range(m))
    assert lib.gs_search_set_route(h._h, 4) == A and lib.gs_search_set_table(h._h, 3) == A
    rep = (C.c_uint32 * _lib.GS_SEARCH_REPORT_WORDS)()
    assert lib.gs_search_last(h._h, rep, _lib.GS_SEARCH_REPORT_WORDS - 1, None) == A and lib.gs_search_last(h._h, None, 64, None) == A
    h.close()
    h8 = gpu.SortedSearch(n, m, I64, sort_queries=True)
    assert h8.last()["engine"] == 1 and h8.temp_bytes == search.temp_bytes(n, m, 8, True)
    assert lib.gs_search_sorted(h8._h, *ok, None) == A  # a 32-bit key type on the 8-byte handle
    h8.close()


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_captured_graph_replayed_on_changed_contents(gpu, form):
    """One call per route captured and replayed twice on other contents of the same sizes: no host wait, every grid fixed by (n, m)."""
    torch = _torch()
    kt, descending, right = F32, True, True
    n, m = 40009, 9001
    h = gpu.SortedSearch(n, m, kt, gpu.ORDER_DESCENDING, sort_queries=form in ("tile", "sort"))
    _force(h, form)

    def inputs(seed):
        hay = sort_as_library(draws(kt, n, seed, distinct=7000), kt, descending)
        q = draws(kt, m, seed + 1, distinct=5000)
        return hay, sort_as_library(q, kt, descending) if form == "tile" else q

    hay, q = inputs(100)
    dh, dq = _dev(hay), _dev(q)
    out = torch.full((m,), SENTINEL, dtype=torch.int32, device="cuda")

    def call():
        h.search(dh, dq, right=right, queries_sorted=form == "tile", out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(out), gpu.searchsorted_reference(hay, q, kt, descending, right))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seed in (200, 300):
        hay, q = inputs(seed)
        dh.copy_(_dev(hay))
        dq.copy_(_dev(q))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(out), gpu.searchsorted_reference(hay, q, kt, descending, right))
        rep = h.last()
        assert (rep["route"], rep["n"], rep["m"]) == ({"tile": TILE, "sort": SORT}.get(form, BINARY), n, m)
        assert rep["plan"] == gpu.search_plan(n, m, 4) and rep["table"] == (form == "table")
    h.close()


# ---- the functional layer's AUTO ----------------------------------------------------------------------------------------------------
def test_functional_auto_takes_the_route_of_the_plan(gpu):
    """gpusorting_amd.searchsorted on shuffled queries asks gs_search_plan: at the rule's constants (whatever they are) it makes a
    handle WITH the query sorter and the call takes SORT; one query fewer and it makes one without and takes BINARY; queries declared
    sorted take TILE.  Integers, ascending: the positions are torch.searchsorted's."""
    from gpusorting_amd import _lib, functional
    torch = _torch()
    n, m = _lib.GS_SEARCH_SORT_MIN_KEYS, _lib.GS_SEARCH_SORT_MIN_QUERIES
    g = torch.Generator(device="cuda").manual_seed(9)
    hay = torch.sort(torch.randint(-(1 << 30), 1 << 30, (n,), generator=g, device="cuda", dtype=torch.int32)).values
    q = torch.randint(-(1 << 30), 1 << 30, (m,), generator=g, device="cuda", dtype=torch.int32)

    def last(sort_queries):
        key = (hay.device.index, int(torch.cuda.current_stream(hay.device).cuda_stream), I32, gpu.ORDER_ASCENDING, sort_queries)
        h = functional._search_cache[key]
        assert h.sort_queries == sort_queries
        return h.last()

    assert gpu.search_plan(n, m)["route_unsorted"] == SORT and gpu.search_plan(n, m - 1)["route_unsorted"] == BINARY
    want = torch.searchsorted(hay, q, right=True).to(torch.int32)
    assert torch.equal(gpu.searchsorted(hay, q, right=True), want)
    rep = last(True)
    assert (rep["route"], rep["n"], rep["m"], rep["engine"]) == (SORT, n, m, 1)
    assert torch.equal(gpu.searchsorted(hay, q[:m - 1].clone(), right=True), want[:m - 1])
    rep = last(False)
    assert (rep["route"], rep["m"], rep["engine"]) == (BINARY, m - 1, 0) and rep["table"] == gpu.search_plan(n, m - 1)["table"]
    qs = torch.sort(q).values
    assert torch.equal(gpu.searchsorted(hay, qs, queries_sorted=True), torch.searchsorted(hay, qs).to(torch.int32))
    assert last(False)["route"] == TILE
