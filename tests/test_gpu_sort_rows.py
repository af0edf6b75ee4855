"""GPU tests of the row-wise sort (gs_sort_rows_* in include/gpusort.h; sortrows_kernels.hpp): every row of a [rows, row_len] matrix of
32-bit keys sorted on its own, keys only and with 4- and 8-byte values, on the LDS route (the segmented sort's kernels on uniform
offsets) and on the pass route (four passes of count, scan, scatter over all rows at once).  Everything is compared bit for bit with
sort_rows_reference, the numpy statement of the semantics (tests/test_sort_rows_cpu.py checks that one on the CPU).  Shapes come from
gs_sort_rows_plan and gs_segsort_max_lds_segment.  The last test asserts that the cases of this file reached every kernel form the build
compiles (gs_sort_rows_last's form mask).

With a tile of 4096 elements the shortest pass-route row is two tiles + 1 (8-byte values: the LDS limit is 8192), so the case "one
tile + 1" of a row is run as "whole tiles + 1": the LDS limit + 1, whose last tile holds one element.  A plan of ONE part with several
tiles needs rows x (tiles / 2) >= 1024 or a row of fewer than four tiles; below 2^19 elements only 8-byte values reach it (a row of
8193 .. 16383 elements), in both rank modes; keys only and 4-byte values walk several tiles per part in plans of several parts."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32, I32, F32 = 0, 1, 2
KEY_TYPES = (U32, I32, F32)
KEYS, PAIRS = 0, 1
ENTRIES = ("keys", "pairs4", "pairs8")
ROUTE_LDS, ROUTE_PASSES = 1, 2
TILE = 4096
_FORMS_SEEN = [0]   # union of gs_sort_rows_last's form masks over the file's cases


def _torch():
    import torch
    return torch


def _mode(entry):
    return (KEYS, 0) if entry == "keys" else (PAIRS, 8 if entry == "pairs8" else 4)


def _lds(entry):
    from gpusorting_amd import _lib
    return int(_lib.load().gs_segsort_max_lds_segment(*_mode(entry)))


def _plan(entry, rows, row_len):
    from gpusorting_amd.rowsort import sort_rows_plan
    return sort_rows_plan(rows, row_len, *_mode(entry))


def _values(rows, row_len, vb):
    """value = position within the row (8 bytes: the row number and a high bit on top): equal keys must come out in rising position."""
    pos = np.tile(np.arange(row_len, dtype=np.uint32), (rows, 1))
    if vb == 4:
        return pos
    return pos.astype(np.uint64) | (np.arange(rows, dtype=np.uint64)[:, None] << np.uint64(40)) | np.uint64(1 << 63)


def _handle(gpu, entry, max_keys, kt=U32, desc=False, rank=None):
    mode, vb = _mode(entry)
    h = gpu.RowSort(max_keys, order=1 if desc else 0, key_type=kt, mode=mode, value_bytes=vb)
    if rank is not None:
        h.set_rank_mode(rank)
        assert h.rank_mode == rank
    return h


def _note(h, entry, rows, row_len):
    """gs_sort_rows_check is GS_OK, gs_sort_rows_last agrees with gs_sort_rows_plan; the form mask joins the file's union."""
    h.check()
    last, p = h.last(), _plan(entry, rows, row_len)
    assert last["status"] == 0 and (last["rows"], last["row_len"]) == (rows, row_len)
    assert (last["route"], last["parts"], last["per_part"]) == (p["route"], p["parts"], p["per_part"])
    assert last["route"] == (ROUTE_LDS if row_len <= _lds(entry) else ROUTE_PASSES)
    scatter = sum(32 << b for b in range(6))
    if last["route"] == ROUTE_PASSES:   # clear, count, scan and exactly the scatter form of the value width and the rank mode
        v = ENTRIES.index(entry)
        assert last["forms"] == 1 | 8 | 16 | (32 << (2 * v + last["rank_mode"])), last
    else:
        assert last["forms"] == 1 | 2 | 4 and not last["forms"] & scatter, last
    _FORMS_SEEN[0] |= last["forms"]
    return last


def _run(gpu, h, entry, bits, kt, desc):
    """One call on fresh device copies of the [rows, row_len] uint32 array `bits`, compared with the reference."""
    torch = _torch()
    from gpusorting_amd.rowsort import sort_rows_reference
    rows, row_len = bits.shape
    dk = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32).copy()).cuda()
    vb = _mode(entry)[1]
    if vb == 0:
        h.sort(dk)
        rk, _ = sort_rows_reference(bits, None, kt, desc)
        rv = dv = None
    else:
        vals = _values(rows, row_len, vb)
        dv = torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()).cuda()
        h.sort(dk, dv)
        rk, rv = sort_rows_reference(bits, vals, kt, desc)
    last = _note(h, entry, rows, row_len)
    where = f"{entry} rows={rows} row_len={row_len} kt={kt} desc={desc} rank={last['rank_mode']} parts={last['parts']}"
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), rk, err_msg=where)
    if rv is not None:
        np.testing.assert_array_equal(dv.cpu().numpy().view(rv.dtype), rv, err_msg=where)
    return last


def _random_bits(rows, row_len, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (rows, row_len), dtype=np.uint64).astype(np.uint32)


_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0x00000001,
                      0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000], dtype=np.uint32)   # ±0 ±inf NaNs subnormals ...


def _float_bits(rows, row_len, seed):
    """Uniform bit patterns with ±0, ±inf, quiet and signalling NaNs of both signs and subnormals strewn in, each many times."""
    rng = np.random.default_rng(seed)
    bits = _random_bits(rows, row_len, seed)
    hit = rng.random((rows, row_len)) < 0.25
    bits[hit] = _SPECIALS[rng.integers(0, _SPECIALS.size, int(hit.sum()))]
    return bits


@pytest.mark.parametrize("rows", (1, 2, 5))
@pytest.mark.parametrize("entry", ENTRIES)
def test_route_boundary(gpu, entry, rows):
    """row_len = the LDS limit and the LDS limit + 1: the route switches exactly there, and both sides sort."""
    lds = _lds(entry)
    for i, (row_len, route) in enumerate(((lds, ROUTE_LDS), (lds + 1, ROUTE_PASSES))):
        desc = bool((i + rows) & 1)
        h = _handle(gpu, entry, rows * (lds + 1), U32, desc)
        last = _run(gpu, h, entry, _random_bits(rows, row_len, 10 * rows + i), U32, desc)
        assert last["route"] == route
        h.close()


def _pass_shapes(entry):
    """(rows, row_len, what) on the pass route — see the module's note on the tile and the LDS limit."""
    lds = _lds(entry)
    uneven = lds + 3 * TILE + 77
    shapes = [(1, lds + 1, "tiles+1"), (1, lds + 2 * TILE, "k tiles"), (1, lds + 2 * TILE - 1, "k tiles - 1"), (3, uneven, "uneven last part"),
              (3, lds + TILE + 1, "odd rows"), (2, lds + 5, "short tail")]
    p = _plan(entry, 3, uneven)
    assert p["parts"] > 1 and p["per_part"] >= 2 * TILE and 0 < uneven - (p["parts"] - 1) * p["per_part"] < p["per_part"] and uneven % TILE, p
    assert all(r * n < (1 << 19) and _plan(entry, r, n)["route"] == ROUTE_PASSES for r, n, _ in shapes)
    if entry == "pairs8":
        assert _plan(entry, 1, lds + 1)["parts"] == 1 and _plan(entry, 1, lds + 1)["per_part"] == 3 * TILE   # one part, several tiles
    return shapes


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ENTRIES)
def test_pass_route_shapes(gpu, entry, rank):
    shapes = _pass_shapes(entry)
    for desc in (False, True):
        h = _handle(gpu, entry, max(r * n for r, n, _ in shapes), U32, desc, rank)
        for i, (rows, row_len, _) in enumerate(shapes):
            last = _run(gpu, h, entry, _random_bits(rows, row_len, 100 + 7 * i + rank), U32, desc)
            assert last["route"] == ROUTE_PASSES and last["rank_mode"] == rank
        h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("desc", (False, True))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_orders_and_rank_modes(gpu, kt, desc, rank):
    """The three key types on bit patterns that hold ±0, ±inf, NaNs and subnormals (as uint32 and int32 they are just extremes)."""
    for entry in ENTRIES:
        rows, row_len = 3, _lds(entry) + TILE + 5
        h = _handle(gpu, entry, rows * row_len, kt, desc, rank)
        _run(gpu, h, entry, _float_bits(rows, row_len, 31 * kt + rank), kt, desc)
        _run(gpu, h, entry, _float_bits(65, 300, 32 * kt + rank), kt, desc)     # and the LDS route's wave class
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_distributions(gpu, entry):
    torch = _torch()
    from gpusorting_amd.rowsort import sort_rows_reference
    rows, row_len = 2, _lds(entry) + 2 * TILE + 9
    vb = _mode(entry)[1]
    for kt, desc in ((F32, False), (I32, True)):
        h = _handle(gpu, entry, rows * row_len, kt, desc)
        rnd = _random_bits(rows, row_len, 5)
        equal = np.full((rows, row_len), 0x3F800000, dtype=np.uint32)
        _run(gpu, h, entry, rnd, kt, desc)
        _run(gpu, h, entry, equal, kt, desc)
        if vb == 4:   # all equal: the values stay where they are, descending turns the row round
            dk = torch.from_numpy(equal.view(np.int32).copy()).cuda()
            dv = torch.from_numpy(_values(rows, row_len, 4).view(np.int32).copy()).cuda()
            h.sort(dk, dv)
            want = np.tile(np.arange(row_len, dtype=np.int32), (rows, 1))
            np.testing.assert_array_equal(dv.cpu().numpy(), want[:, ::-1] if desc else want)
        mixed = rnd.copy()
        mixed[0, :] = 0xBF800000                               # one row all equal beside a uniform one
        _run(gpu, h, entry, mixed, kt, desc)
        _run(gpu, h, entry, np.where(rnd & 4, np.uint32(0x80000001), np.uint32(0x7FFFFFFF)).astype(np.uint32), kt, desc)   # two values
        _run(gpu, h, entry, (rnd & np.uint32(0x03030303)) | np.uint32(0xFC000000), kt, desc)    # four values per digit: every base moves far
        srt = sort_rows_reference(rnd, None, kt, desc)[0]
        _run(gpu, h, entry, srt, kt, desc)                     # already sorted
        _run(gpu, h, entry, np.ascontiguousarray(srt[:, ::-1]), kt, desc)   # reverse sorted
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_lds_route(gpu, entry):
    """The classes of the segmented sort on uniform offsets: a single element, packed (2, 32), wave (33, 256), workgroup (257, 1024,
    8192); 65 rows fill a packed wave and start a second one."""
    for i, row_len in enumerate((1, 2, 32, 33, 256, 257, 1024, 8192)):
        desc, kt = bool(i & 1), KEY_TYPES[i % 3]
        h = _handle(gpu, entry, 65 * row_len, kt, desc, rank=(i >> 1) & 1)
        last = _run(gpu, h, entry, _float_bits(65, row_len, 200 + i), kt, desc)
        assert last["route"] == ROUTE_LDS
        h.close()


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_memory_contract(gpu, entry, fill):
    """16-byte-only aligned views with guard bands, rows * row_len smaller than the allocation and odd rows: nothing at or behind
    element rows * row_len of the keys, the values and both alt buffers changes, the LDS route leaves the alt buffers alone altogether,
    and what the scratch holds on entry does not influence the result."""
    from guard_arena import Arena
    from gpusorting_amd import _lib
    from gpusorting_amd.rowsort import sort_rows_reference
    lib = _lib.load()
    mode, vb = _mode(entry)
    vdt = np.uint64 if vb == 8 else np.uint32
    for rows, row_len in ((3, _lds(entry) + TILE + 3), (5, 257), (1, 7)):
        n = rows * row_len
        count = n + 21
        passes = row_len > _lds(entry)
        arena = Arena.for_views([(count, np.uint32)] * 2 + ([(count, vdt)] * 2 if mode == PAIRS else []), "cuda", fill)
        dk = arena.carve(count, np.uint32, 1, "keys")
        ak = arena.carve(count, np.uint32, 3, "alt_keys")
        bits = _random_bits(1, count, n)[0]
        arena.write(dk, bits)
        arena.live(dk, n)
        arena.live(ak, n if passes else 0)
        desc = rows == 5
        h = _handle(gpu, entry, count, I32, desc)
        if mode == PAIRS:
            dv = arena.carve(count, vdt, 5, "values")
            av = arena.carve(count, vdt, 7, "alt_values")
            vals = np.zeros(count, dtype=vdt)
            vals[:n] = _values(rows, row_len, vb).reshape(-1)
            arena.write(dv, vals)
            arena.live(dv, n)
            arena.live(av, n if passes else 0)
            st = lib.gs_sort_rows_pairs(h._h, dk.data_ptr(), dv.data_ptr(), ak.data_ptr(), av.data_ptr(), rows, row_len, I32, h.order, None)
        else:
            st = lib.gs_sort_rows_keys(h._h, dk.data_ptr(), ak.data_ptr(), rows, row_len, I32, h.order, None)
        assert st == 0
        _note(h, entry, rows, row_len)
        arena.verify()
        rk, rv = sort_rows_reference(bits[:n].reshape(rows, row_len), None if mode == KEYS else vals[:n].reshape(rows, row_len), I32, desc)
        np.testing.assert_array_equal(arena.read(dk, np.uint32, n).reshape(rows, row_len), rk, err_msg=f"{entry} {rows}x{row_len}")
        if mode == PAIRS:
            np.testing.assert_array_equal(arena.read(dv, vdt, n).reshape(rows, row_len), rv, err_msg=f"{entry} {rows}x{row_len}")
        h.close()


def test_error_returns(gpu):
    """GS_ERR_ARG / GS_ERR_MODE / GS_ERR_SIZE as the header lists them; a refused call writes nothing."""
    torch = _torch()
    from gpusorting_amd import _lib
    lib = _lib.load()
    rows, long = 2, _lds("pairs4") + 1          # a pass-route shape for 4-byte values; short rows of 100 take the LDS route
    n = rows * long
    assert (4 * n - 24) % 16 == 0               # (the overlapping pointers below are aligned: refused for the overlap alone)
    k = torch.full((n + 64,), 0x1234, dtype=torch.int32, device="cuda")
    v = torch.full((n + 64,), 77, dtype=torch.int32, device="cuda")
    ak = torch.full((n + 64,), 0x4321, dtype=torch.int32, device="cuda")
    av = torch.full((n + 64,), 88, dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (k, v, ak, av)]
    hk, hp = _handle(gpu, "keys", 2 * (_lds("keys") + 1)), _handle(gpu, "pairs4", n)
    kp, vp, akp, avp = (t.data_ptr() for t in (k, v, ak, av))
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    # keys entry
    assert lib.gs_sort_rows_keys(None, kp, akp, 4, 100, U32, 0, None) == A
    assert lib.gs_sort_rows_keys(hk._h, None, akp, 4, 100, U32, 0, None) == A
    assert lib.gs_sort_rows_keys(hk._h, kp + 4, akp, 4, 100, U32, 0, None) == A       # element-aligned only
    for kt in (3, 4, 5, 6, 7, 8, 9, 10, -1):                                           # the 64-bit and the 16-bit key types
        assert lib.gs_sort_rows_keys(hk._h, kp, akp, 4, 100, kt, 0, None) == A
    assert lib.gs_sort_rows_keys(hk._h, kp, akp, 4, 100, U32, 2, None) == A
    assert lib.gs_sort_rows_keys(hk._h, kp, akp, 0, 100, U32, 0, None) == S            # zero rows
    assert lib.gs_sort_rows_keys(hk._h, kp, akp, 4, 0, U32, 0, None) == S
    assert lib.gs_sort_rows_keys(hk._h, kp, akp, 3, _lds("keys") + 1, U32, 0, None) == S   # rows * row_len > max_keys
    assert lib.gs_sort_rows_keys(hk._h, kp, akp, 1 << 16, 1 << 16, U32, 0, None) == S  # the product wraps to 0 in 32 bits
    assert lib.gs_sort_rows_keys(hp._h, kp, akp, 4, 100, U32, 0, None) == M            # keys call on a pairs handle
    assert lib.gs_sort_rows_keys(hk._h, kp, None, 1, _lds("keys") + 1, U32, 0, None) == A   # NULL alt on the pass route
    assert lib.gs_sort_rows_keys(hk._h, kp, akp + 4, 1, _lds("keys") + 1, U32, 0, None) == A
    # pairs entry
    call = lib.gs_sort_rows_pairs
    assert call(None, kp, vp, akp, avp, rows, long, U32, 0, None) == A
    assert call(hp._h, None, vp, akp, avp, rows, long, U32, 0, None) == A
    assert call(hp._h, kp, None, akp, avp, rows, long, U32, 0, None) == A
    assert call(hp._h, kp, vp + 4, akp, avp, rows, long, U32, 0, None) == A
    assert call(hp._h, kp, vp, None, avp, rows, long, U32, 0, None) == A              # NULL alt on the pass route
    assert call(hp._h, kp, vp, akp, None, rows, long, U32, 0, None) == A
    assert call(hp._h, kp, vp, akp + 8, avp, rows, long, U32, 0, None) == A
    assert call(hp._h, kp, vp, akp, avp, rows, long, 8, 0, None) == A
    assert call(hp._h, kp, vp, akp, avp, 0, long, U32, 0, None) == S
    assert call(hp._h, kp, vp, akp, avp, rows + 1, long, U32, 0, None) == S
    assert call(hk._h, kp, vp, akp, avp, 4, 100, U32, 0, None) == M                   # pairs on a keys-only handle
    assert call(hp._h, kp, vp, kp + 4 * n - 24, avp, rows, long, U32, 0, None) == A   # any two buffers overlapping
    assert call(hp._h, kp, vp, akp, vp + 4 * n - 24, rows, long, U32, 0, None) == A
    assert lib.gs_sort_rows_set_rank_mode(hp._h, 2) == A
    r = (C.c_uint32 * 8)()
    assert lib.gs_sort_rows_last(hp._h, r, 7, None) == A and lib.gs_sort_rows_last(hp._h, None, 8, None) == A
    torch.cuda.synchronize()
    for t, b in zip((k, v, ak, av), before):
        assert torch.equal(t, b), "a refused call wrote to a buffer"
    # the same arguments, in order, are taken; on the LDS route the alt pointers may be NULL
    assert call(hp._h, kp, vp, akp, avp, rows, long, U32, 0, None) == 0
    hp.check()
    assert call(hp._h, kp, vp, None, None, 4, 100, U32, 0, None) == 0 and lib.gs_sort_rows_keys(hk._h, kp, None, 4, 100, U32, 0, None) == 0
    hp.check()
    hk.check()
    for h in (hk, hp):
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_call_twice_on_one_handle(gpu, entry):
    """Different shapes on one handle, pass route, LDS route and pass route again: the state is reset by every call."""
    lds = _lds(entry)
    h = _handle(gpu, entry, 3 * (lds + 3 * TILE), F32, True)
    for i, (rows, row_len) in enumerate(((3, lds + 2 * TILE + 9), (7, 300), (1, lds + 1), (65, 20), (2, lds + 3 * TILE))):
        _run(gpu, h, entry, _float_bits(rows, row_len, 50 + i), F32, True)
        assert h.status() == 0
    h.close()


def test_graph_capture(gpu):
    """One pass-route call (4-byte values) captured into a graph on one linear stream, replayed on fresh data."""
    torch = _torch()
    from gpusorting_amd.rowsort import sort_rows_reference
    rows, row_len = 3, _lds("pairs4") + 2 * TILE + 77
    h = _handle(gpu, "pairs4", rows * row_len, F32, True)
    dk = torch.empty((rows, row_len), dtype=torch.int32, device="cuda")
    dv = torch.empty((rows, row_len), dtype=torch.int32, device="cuda")
    vals = _values(rows, row_len, 4)

    def load(seed):
        bits = _float_bits(rows, row_len, seed)
        dk.copy_(torch.from_numpy(bits.view(np.int32).copy()))
        dv.copy_(torch.from_numpy(vals.view(np.int32).copy()))
        return bits

    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.sort(dk, dv)            # warm-up outside the capture (the alt buffers are allocated here)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.sort(dk, dv)
    for seed in (11, 12):
        bits = load(seed)
        graph.replay()
        torch.cuda.synchronize()
        _note(h, "pairs4", rows, row_len)
        rk, rv = sort_rows_reference(bits, vals, F32, True)
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), rv)
    h.close()


def test_tensor_convenience_layer(gpu):
    """gpusorting_amd.sort / sort_ / argsort on 2-D tensors: integer keys against torch.sort(dim=-1, stable=True), floats against the
    library's reference (NaN order); 1-D calls give what they gave before."""
    torch = _torch()
    from gpusorting_amd.rowsort import sort_rows_reference
    from gpusorting_amd.segsort import sortable_bits
    for rows, row_len in ((1, 1), (5, 300), (3, _lds("pairs4") + TILE + 1), (2, _lds("keys") + 5), (70, 33)):  # the cached handle grows and is reused
        bits = _random_bits(rows, row_len, rows + row_len) >> np.uint32(12)      # ties
        bits[:, ::3] |= np.uint32(0x80000000)
        t = torch.from_numpy(bits.view(np.int32).copy()).cuda()
        for desc in (False, True):
            out = gpu.sort(t, descending=desc)
            assert out.dtype == torch.int32 and out.shape == t.shape
            want, widx = torch.sort(t, dim=-1, descending=desc, stable=True)
            assert torch.equal(out, want), (rows, row_len, desc)
            perm = gpu.argsort(t, descending=desc)
            assert perm.dtype == torch.int32 and perm.shape == t.shape
            assert torch.equal(torch.gather(t, 1, perm.long()), want)
            if not desc:    # ascending, ties in rising position: torch's stable order (descending is the library's exact reverse)
                assert torch.equal(perm.long(), widx)
            np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), sort_rows_reference(bits, None, I32, desc)[1])
            assert torch.equal(t.cpu(), torch.from_numpy(bits.view(np.int32)))   # the input is not written
        # unsigned=True on int32 storage, 8-byte values, in place
        k2, v2 = gpu.sort(t, torch.arange(rows * row_len, dtype=torch.int64, device="cuda").reshape(rows, row_len), unsigned=True)
        rk, rv = sort_rows_reference(bits, np.arange(rows * row_len, dtype=np.int64).reshape(rows, row_len), U32, False)
        np.testing.assert_array_equal(k2.cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(v2.cpu().numpy(), rv)
        # float32 rows with NaNs of both signs and ±0
        fb = _float_bits(rows, row_len, 3 * rows)
        f = torch.from_numpy(fb.view(np.float32).copy()).cuda()
        v4 = torch.arange(row_len, dtype=torch.int32, device="cuda").repeat(rows, 1)
        gpu.sort_(f, v4, descending=True)
        rk, rp = sort_rows_reference(fb, None, F32, True)
        np.testing.assert_array_equal(f.view(torch.int32).cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(v4.cpu().numpy().view(np.uint32), rp)
    # 1-D calls are what they were: the 1-D engine's result
    bits = _random_bits(1, 70001, 9)[0]
    t = torch.from_numpy(bits.view(np.int32).copy()).cuda()
    order = np.argsort(sortable_bits(bits, I32), kind="stable")
    np.testing.assert_array_equal(gpu.sort(t).cpu().numpy().view(np.uint32), bits[order])
    np.testing.assert_array_equal(gpu.argsort(t).cpu().numpy(), order.astype(np.int32))
    # what a 2-D call refuses
    for dtype in (torch.float16, torch.bfloat16, torch.int16):
        with pytest.raises(TypeError, match="int32, uint32, float32"):
            gpu.sort(torch.zeros((4, 4), dtype=dtype, device="cuda"))
        with pytest.raises(TypeError, match="int32, uint32, float32"):
            gpu.argsort(torch.zeros((4, 4), dtype=dtype, device="cuda"))
    with pytest.raises(TypeError):
        gpu.sort(torch.zeros((4, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        gpu.sort_(torch.zeros((4, 8), dtype=torch.int32, device="cuda")[:, :4])                     # strided rows
    with pytest.raises(ValueError):
        gpu.sort(torch.zeros((4, 4), dtype=torch.int32, device="cuda"), torch.zeros((4, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        gpu.sort(torch.zeros((2, 2, 2), dtype=torch.int32, device="cuda"))


def test_zz_every_compiled_kernel_form_was_reached(gpu):
    """The forms this build compiles: clear, offsets, the LDS route; count, scan; the scatter for keys only, 4- and 8-byte values, each in
    both rank modes.  gs_sort_rows_last reports the forms a call launched; their union over this file's cases must be all of them (run
    the whole file: this test stands last)."""
    from gpusorting_amd.rowsort import SORT_ROWS_FORMS
    from gpusorting_amd import _lib
    assert len(SORT_ROWS_FORMS) == 11 and sum(SORT_ROWS_FORMS.values()) == _lib.GS_SORT_ROWS_F_ALL
    missing = [name for name, bit in SORT_ROWS_FORMS.items() if not _FORMS_SEEN[0] & bit]
    assert not missing, f"kernel forms no case of this file reached: {missing}"
