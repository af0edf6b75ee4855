"""The row-wise top-k (gs_topk_select_rows_*, gpusorting_amd/csrc/topk_rows_kernels.hpp) on the GPU: every case compares keys AND
values bit for bit with gpusorting_amd.topk_rows_reference (topk_reference per row, tests/test_topk_rows_cpu.py), calls check() and
asks rows_last() for the route.  Keys come from init_random with seeds, or are built against the structure of the stream select.
No counterpart in the reference project."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
LDS_ROW = {0: 32768, 4: 16384, 8: 8192}  # seg_max_lds: rows up to here are sorted in LDS
WAVE, TILE, STREAM, LOOP = 1, 2, 3, 4
MODES = ("keys", "pos", "v4", "v8")
FILL = 0x5EEDBEEF


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()


def _vb(mode):
    return {"keys": 0, "v4": 4, "v8": 8, "pos": 4}[mode]


def _max_k(gpu, mode):
    from gpusorting_amd.topk import rows_max_k
    vb = _vb(mode)
    return rows_max_k(gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _random(gpu, n, seed, preset=None):
    torch = _torch()
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.init_random(dk, seed, gpu.ENTROPY_PRESET_1 if preset is None else preset)
    torch.cuda.synchronize()
    return dk.cpu().numpy().view(np.uint32).copy()


def _values(n, mode):
    """Values that differ from the position, so that a position written for a value shows."""
    if mode == "v4":
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    if mode == "v8":
        return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x1F)
    return None


def _handle(gpu, max_keys, max_k, mode, key_type=0, descending=False):
    vb = _vb(mode)
    return gpu.TopK(max_keys, max_k, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type,
                    gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _extent(rows, row_len, stride):
    return (rows - 1) * stride + row_len


def _view2d(flat, rows, row_len, stride):
    return np.lib.stride_tricks.as_strided(flat, (rows, row_len), (stride * flat.itemsize, flat.itemsize), writeable=False)


def _route(gpu, row_len, k, mode):
    return WAVE if row_len <= 256 else TILE if row_len <= LDS_ROW[_vb(mode)] else STREAM if k <= _max_k(gpu, mode) else LOOP


class _Case:
    """One matrix on the device and its full per-row reference (k = row_len), computed once: the reference for a smaller k is its
    head, by the definition of topk_reference."""

    def __init__(self, gpu, flat, rows, row_len, stride, mode, key_type=0, descending=False):
        self.gpu, self.flat, self.rows, self.row_len, self.stride, self.mode = gpu, flat, rows, row_len, stride, mode
        self.key_type, self.descending = key_type, descending
        self.vals = _values(flat.size, mode)
        self.dk = _dev(flat)
        self.dv = _dev(self.vals) if self.vals is not None else None
        self.rk, self.rv = gpu.topk_rows_reference(_view2d(flat, rows, row_len, stride), row_len,
                                                   None if self.vals is None else _view2d(self.vals, rows, row_len, stride), key_type, descending)

    def run(self, h, k, route=None, pad=7):
        torch, gpu, vb = _torch(), self.gpu, _vb(self.mode)
        m = self.rows * k
        ok = torch.full((m + pad,), FILL, dtype=torch.int32, device="cuda")
        ov = torch.full((m + pad,), FILL, dtype=torch.int32 if vb == 4 else torch.int64, device="cuda") if vb else None
        h.select_rows(self.dk, self.rows, self.row_len, self.stride, k, ok, self.dv, ov)
        assert h.status() == 0
        rep = h.rows_last()
        assert (rep["rows"], rep["row_len"], rep["k"], rep["status"]) == (self.rows, self.row_len, k, 0)
        assert rep["route"] == (route or _route(gpu, self.row_len, k, self.mode)), rep
        hk = ok.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(hk[:m].reshape(self.rows, k), self.rk[:, :k].view(np.uint32))
        assert np.all(hk[m:] == FILL), "nothing behind element rows * k of the output keys is written"
        if vb:
            hv = ov.cpu().numpy().view(VALUE_DTYPE[vb])
            np.testing.assert_array_equal(hv[:m].reshape(self.rows, k), self.rv[:, :k].astype(VALUE_DTYPE[vb]))
            assert np.all(hv[m:] == FILL), "nothing behind element rows * k of the output values is written"
        return rep

    def inputs_unchanged(self):
        np.testing.assert_array_equal(self.dk.cpu().numpy().view(np.uint32), self.flat)
        if self.dv is not None:
            np.testing.assert_array_equal(self.dv.cpu().numpy().view(self.vals.dtype), self.vals)


def _row_lens(vb):
    L = LDS_ROW[vb]
    return (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, L - 1, L, L + 1, L + 4097)


# ---- route borders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("len_index", range(14))
def test_route_borders(gpu, mode, len_index):
    """Every row length around a route border, rows 1 / 3 / 67, strides row_len, row_len + 1 (odd, 4-byte-only row starts for one of
    them) and row_len + 13, k = 1, 2, min(64, row_len), min(gs_topk_rows_max_k, row_len)."""
    row_len = _row_lens(_vb(mode))[len_index]
    ks = sorted({1, min(2, row_len), min(64, row_len), min(_max_k(gpu, mode), row_len)})
    shapes = [(1, 0), (3, 1), (67, 1), (3, 13), (3, 0)] + ([(67, 0)] if row_len <= 1025 else [])
    h = _handle(gpu, _extent(67, row_len, row_len + 13), row_len, mode)
    for i, (rows, extra) in enumerate(shapes):
        stride = row_len + extra
        case = _Case(gpu, _random(gpu, _extent(rows, row_len, stride), 100 + len_index * 8 + i), rows, row_len, stride, mode)
        for k in ks:
            case.run(h, k)
        case.inputs_unchanged()
    h.close()


@pytest.mark.parametrize("key_type", [0, 1, 2])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("long_row", [False, True])
def test_types_and_orders(gpu, key_type, descending, long_row):
    mode = "pos"
    row_len, rows = (LDS_ROW[4] + 1 if long_row else 257), 5
    stride = row_len + 1
    flat = _random(gpu, _extent(rows, row_len, stride), 40 + key_type, gpu.ENTROPY_PRESET_1 if long_row else gpu.ENTROPY_PRESET_3)
    flat[::7] = flat[3]  # ties
    h = _handle(gpu, flat.size, row_len, mode, key_type, descending)
    case = _Case(gpu, flat, rows, row_len, stride, mode, key_type, descending)
    for k in (1, 50, 257):
        case.run(h, k)
    h.close()


# ---- structure of the stream select ----------------------------------------------------------------------------------------------
def _stream_case(gpu, keys2d, mode, descending, ks, key_type=0, stride_extra=1, reads=None):
    rows, row_len = keys2d.shape
    stride = row_len + stride_extra
    flat = np.full(_extent(rows, row_len, stride), 0xA5A5A5A5, dtype=np.uint32)
    for r in range(rows):
        flat[r * stride:r * stride + row_len] = keys2d[r].view(np.uint32)
    h = _handle(gpu, flat.size, max(ks), mode, key_type, descending)
    case = _Case(gpu, flat, rows, row_len, stride, mode, key_type, descending)
    for k in ks:
        rep = case.run(h, k, STREAM)
        if reads is not None:
            assert rep["reads"] == reads, rep
    case.inputs_unchanged()
    h.close()


@pytest.mark.parametrize("descending", [False, True])
def test_stream_every_key_equal(gpu, descending):
    L = LDS_ROW[4]
    _stream_case(gpu, np.full((2, L + 1), 0x12345678, dtype=np.uint32), "pos", descending, (1, 64, 4096), reads=4)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shared_bits,reads", [(16, 3), (24, 4)])
def test_stream_keys_share_their_top_bits(gpu, descending, shared_bits, reads):
    """All keys share their top 16 bits: the second level is needed (three reads); their top 24: the third, exact level (four reads;
    256 values over 2 L elements: every value is a run of ties that the LDS sort puts in position order)."""
    L = LDS_ROW[4]
    low = _random(gpu, 3 * 2 * L, 77).reshape(3, 2 * L) & np.uint32((1 << (32 - shared_bits)) - 1)
    _stream_case(gpu, low | np.uint32(0xABCDEF00 & ~((1 << (32 - shared_bits)) - 1)), "pos", descending, (1, 64, 1000), reads=reads)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("copies", ["few", "many"])
def test_stream_threshold_repeated_across_chunk_borders(gpu, descending, copies):
    """The threshold value T sits on both sides of every border of a 4096-element load chunk (and, with an odd stride, of the peeled
    chunks), k takes only a part of its copies: position-rank ties.  "few": all copies are staged and the LDS sort decides;
    "many": more copies than the staging holds, the gather takes the wanted share by rank."""
    L = LDS_ROW[4]
    rows, row_len = 3, 3 * L
    T = np.uint32(0x40000000)
    keys = (_random(gpu, rows * row_len, 55).reshape(rows, row_len) >> np.uint32(2)) | np.uint32(0x80000000)  # behind T (ascending)
    pos = np.arange(row_len)
    at_border = (pos % 4096 < 5) | (pos % 4096 >= 4091)
    keys[:, at_border if copies == "few" else (at_border | (pos % 3 == 0))] = T
    keys[:, 100::5000] = np.uint32(7)  # in front of T
    if descending:
        keys = ~keys
    count = int(np.count_nonzero(keys[0] == (~T if descending else T)))
    front = int(np.count_nonzero(keys[0] == (~np.uint32(7) if descending else np.uint32(7))))
    assert (count < 4096 - front) == (copies == "few")
    for mode in ("pos", "keys"):
        _stream_case(gpu, keys, mode, descending, (front + 1, front + min(count, 4000) // 2), stride_extra=1 if mode == "pos" else 2)


@pytest.mark.parametrize("descending", [False, True])
def test_stream_sorted_and_reverse_sorted_rows(gpu, descending):
    L = LDS_ROW[0]
    base = np.sort(_random(gpu, 2 * L + 3, 91))
    _stream_case(gpu, np.stack([base, base[::-1], np.sort(base >> np.uint32(12))]), "keys", descending, (1, 777))
    _stream_case(gpu, np.stack([base[:L // 2 + 1], base[::-1][:L // 2 + 1]]), "v4", descending, (33,))


def test_stream_all_equal_row_beside_random_rows(gpu):
    L = LDS_ROW[8]
    keys = _random(gpu, 5 * (L + 9), 13).reshape(5, L + 9)
    keys[1] = 0xFFFFFFFF
    keys[3] = 0
    for descending in (False, True):
        _stream_case(gpu, keys, "v8", descending, (1, 100, 1024), stride_extra=3)


@pytest.mark.parametrize("descending", [False, True])
def test_stream_float_rows_of_zeros_infinities_and_nans(gpu, descending):
    L = LDS_ROW[4]
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x3F800000, 0xBF800000], dtype=np.uint32)
    pick = _random(gpu, 3 * (L + 5), 17).reshape(3, L + 5)
    keys = special[pick % np.uint32(special.size)]
    keys[2, ::2] = pick[2, ::2]  # one row half random bit patterns
    _stream_case(gpu, keys, "pos", descending, (1, 9, 2048), key_type=2)


# ---- the loop route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["keys", "pos"])
def test_loop_route_above_the_stream_limit(gpu, mode):
    L = LDS_ROW[_vb(mode)]
    rows, row_len, k = 3, 2 * L, _max_k(gpu, mode) + 1
    for stride in (row_len, row_len + 1):  # aligned rows; rows and output rows off the 16-byte boundary
        flat = _random(gpu, _extent(rows, row_len, stride), 61)
        h = _handle(gpu, flat.size, k, mode, 2, True)
        case = _Case(gpu, flat, rows, row_len, stride, mode, 2, True)
        case.run(h, k, LOOP)
        case.inputs_unchanged()
        h.close()


@pytest.mark.parametrize("rows,route", [(2, LOOP), (3, STREAM)])
def test_few_very_long_rows_take_the_loop(gpu, rows, route):
    """The measured border of DESIGN.md 3.10: rows * (row_len + 7 * 2^19) <= 19 * row_len from row_len = 2^19 on is LOOP although k fits."""
    row_len, stride, k = 1 << 19, (1 << 19) + 1, 5
    flat = _random(gpu, _extent(rows, row_len, stride), 67)
    h = _handle(gpu, flat.size, k, "pos")
    case = _Case(gpu, flat, rows, row_len, stride, "pos")
    case.run(h, k, route)
    case.inputs_unchanged()
    h.close()


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,row_len,k", [(WAVE, 200, 9), (TILE, 3001, 65), (STREAM, 16384 + 4099, 130), (LOOP, 2 * 16384, 4097)])
@pytest.mark.parametrize("mode", ["pos", "v4"])
def test_memory_contract_on_a_guard_arena(gpu, route, row_len, k, mode):
    """Bases with 16 bytes of alignment and no more, guard bands around the inputs and the [rows, k] output; the gaps between the rows
    hold a key that would win every selection (0, ascending) and must never come out."""
    from guard_arena import Arena
    rows, stride = 3, row_len + 3
    n = _extent(rows, row_len, stride)
    if route == LOOP:
        assert k == _max_k(gpu, mode) + 1
    flat = np.zeros(n, dtype=np.uint32)
    body = _random(gpu, rows * row_len, 23) | np.uint32(1)
    for r in range(rows):
        flat[r * stride:r * stride + row_len] = body[r * row_len:(r + 1) * row_len]
    vals = _values(n, mode)
    spare = 11
    specs = [(n, np.uint32), (rows * k + spare, np.uint32), (rows * k + spare, np.uint32)] + ([(n, np.uint32)] if vals is not None else [])
    arena = Arena.for_views(specs, "cuda", fill="hash")
    dk = arena.carve(n, np.uint32, 1, "keys")
    ok = arena.carve(rows * k + spare, np.uint32, 3, "out_keys")
    ov = arena.carve(rows * k + spare, np.uint32, 5, "out_values")
    dv = None
    if vals is not None:
        dv = arena.carve(n, np.uint32, 7, "values")
        arena.write(dv, vals)
    arena.write(dk, flat)
    arena.live(ok, rows * k)
    arena.live(ov, rows * k)
    h = _handle(gpu, n, k, mode)
    h.select_rows(dk, rows, row_len, stride, k, ok, dv, ov)
    assert h.status() == 0
    assert h.rows_last()["route"] == route
    h.close()
    arena.verify()
    rk, rv = gpu.topk_rows_reference(_view2d(flat, rows, row_len, stride), k, None if vals is None else _view2d(vals, rows, row_len, stride))
    hk = arena.read(ok, np.uint32, rows * k)
    assert not np.any(hk == 0), "a key of a gap between two rows was selected"
    np.testing.assert_array_equal(hk.reshape(rows, k), rk)
    np.testing.assert_array_equal(arena.read(ov, np.uint32, rows * k).reshape(rows, k), rv)


# ---- further cases -----------------------------------------------------------------------------------------------------------------
def test_handle_reuse_across_shapes_and_routes(gpu):
    L = LDS_ROW[4]
    h = _handle(gpu, 4 * (2 * L + 8), 5000, "pos", 1, True)
    for i, (rows, row_len, extra, k) in enumerate([(4, 2 * L, 1, 300), (40, 100, 0, 100), (3, L, 2, 5000), (2, 2 * L, 8, 4100), (7, 300, 1, 1),
                                                   (4, L + 1, 0, 64), (64, 64, 0, 8)]):
        stride = row_len + extra
        case = _Case(gpu, _random(gpu, _extent(rows, row_len, stride), 200 + i), rows, row_len, stride, "pos", 1, True)
        case.run(h, k)
    # the 1-D call on the same handle is what it was
    keys = _random(gpu, 3 * L, 9)
    torch = _torch()
    ok = torch.empty(10, dtype=torch.int32, device="cuda")
    ov = torch.empty(10, dtype=torch.int32, device="cuda")
    h.select(_dev(keys), 10, ok, None, ov)
    h.check()
    rk, rv = gpu.topk_reference(keys, 10, None, 1, True)
    np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint32), rk.view(np.uint32))
    np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), rv)
    assert h.last()["route"] == 1
    h.close()


@pytest.mark.parametrize("row_len,k", [(64, 8), (5000, 40), (16384 + 77, 100)])
def test_captured_graph_replayed_on_new_data(gpu, row_len, k):
    torch = _torch()
    rows, stride = 9, row_len + 1
    n = _extent(rows, row_len, stride)
    h = _handle(gpu, n, k, "pos", 2, True)
    dk = _dev(_random(gpu, n, 31))
    ok = torch.empty(rows * k, dtype=torch.int32, device="cuda")
    ov = torch.empty(rows * k, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        h.select_rows(dk, rows, row_len, stride, k, ok, None, ov)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.select_rows(dk, rows, row_len, stride, k, ok, None, ov)
    for seed in (32, 33):
        keys = _random(gpu, n, seed, gpu.ENTROPY_PRESET_3 if seed == 33 else None)
        dk.copy_(_dev(keys))
        ok.zero_()
        ov.zero_()
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rv = gpu.topk_rows_reference(_view2d(keys, rows, row_len, stride), k, None, 2, True)
        np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint32).reshape(rows, k), rk.view(np.uint32))
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32).reshape(rows, k), rv)
    h.close()


def test_captured_loop_graph_outlives_larger_calls(gpu):
    """The LOOP route with rows and output rows off the 16-byte boundary (odd stride, odd k) goes through the handle's staging buffer.
    That buffer is allocated once, at the handle's size: a capture before it exists is refused without breaking the capture, and a
    graph captured after one plain call stays valid when later calls on the handle have longer rows and a larger k."""
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    L = LDS_ROW[4]
    rows, row_len, k = 3, 2 * L, _max_k(gpu, "pos") + 1
    stride = row_len + 1
    n = _extent(rows, row_len, stride)
    big_rows, big_len, big_k = 2, 3 * L + 5, k + 6
    big = _Case(gpu, _random(gpu, _extent(big_rows, big_len, big_len + 3), 41), big_rows, big_len, big_len + 3, "pos", 2, True)
    h = _handle(gpu, max(n, big.flat.size), big_k, "pos", 2, True)
    dk = _dev(_random(gpu, n, 31))
    ok = torch.empty(rows * k, dtype=torch.int32, device="cuda")
    ov = torch.empty(rows * k, dtype=torch.int32, device="cuda")
    small_k = torch.empty(8 * 4, dtype=torch.int32, device="cuda")
    small_v = torch.empty(8 * 4, dtype=torch.int32, device="cuda")
    # no staging yet: the capturing call is refused on the host, the capture goes on and takes a call that needs none
    refused = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp = torch.cuda.current_stream().cuda_stream
        refused = lib.gs_topk_select_rows_pairs(h._h, dk.data_ptr(), None, rows, row_len, stride, k, ok.data_ptr(), ov.data_ptr(), 2, 1, sp)
        h.select_rows(dk, 8, 64, 64, 4, small_k, None, small_v)
    assert refused == _lib.GS_ERR_MODE
    graph.replay()
    torch.cuda.synchronize()
    h.check()
    assert h.rows_last()["route"] == WAVE
    # one plain call allocates it; then the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        h.select_rows(dk, rows, row_len, stride, k, ok, None, ov)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.select_rows(dk, rows, row_len, stride, k, ok, None, ov)
    for seed in (32, 33):
        if seed == 33:  # longer rows and a larger k on the same handle in between
            big.run(h, big_k, LOOP)
        keys = _random(gpu, n, seed, gpu.ENTROPY_PRESET_3 if seed == 33 else None)
        dk.copy_(_dev(keys))
        ok.zero_()
        ov.zero_()
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rv = gpu.topk_rows_reference(_view2d(keys, rows, row_len, stride), k, None, 2, True)
        np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint32).reshape(rows, k), rk.view(np.uint32))
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32).reshape(rows, k), rv)
    h.close()


def test_select_rows_rejects_values_that_are_no_tensor(gpu):
    torch = _torch()
    h = _handle(gpu, 1024, 8, "v4")
    keys = torch.zeros(1024, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        h.select_rows(keys, 4, 100, 100, 8, out, [1, 2, 3], out.clone())
    h.close()
    # a single row: its row stride is never used, values with another one are accepted
    x = torch.from_numpy(_random(gpu, 2 * 600, 3).view(np.float32).copy()).cuda().reshape(2, 600)
    vals = torch.arange(500, dtype=torch.int32, device="cuda").reshape(1, 500) * 7  # row stride 500, the keys' is 600
    v, w = gpu.topk(x[:1, :500], 5, values=vals)
    rk, rv = gpu.topk_rows_reference(x[:1, :500].cpu().numpy().view(np.uint32), 5, vals.cpu().numpy().view(np.uint32), 2, True)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), rk.view(np.uint32))
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), rv)


def test_functional_topk_on_matrices(gpu):
    torch = _torch()
    rows, width = 6, 50257
    keys = _random(gpu, rows * width, 5).reshape(rows, width)
    x = torch.from_numpy(keys.view(np.float32).copy()).cuda()
    for largest in (True, False):
        v, i = gpu.topk(x, 50, largest=largest)
        rk, rv = gpu.topk_rows_reference(keys, 50, None, 2, largest)
        assert v.shape == (rows, 50) and i.dtype == torch.int32 and v.dtype == torch.float32
        np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), rk.view(np.uint32))
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
    # rows that are not contiguous: a view on the leading columns
    row_len = 20001
    v, i = gpu.topk(x[:, :row_len], 7)
    rk, rv = gpu.topk_rows_reference(keys[:, :row_len], 7, None, 2, True)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), rk.view(np.uint32))
    np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
    # values, int32 keys as unsigned, a short row length
    xi = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    vals = torch.arange(rows * width, dtype=torch.int64, device="cuda").reshape(rows, width) * 3
    v, w = gpu.topk(xi[:, :200], 12, largest=False, values=vals[:, :200], unsigned=True)
    rk, rv = gpu.topk_rows_reference(keys[:, :200], 12, (np.arange(rows * width, dtype=np.uint64) * 3).reshape(rows, width)[:, :200], 0, False)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), rk)
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint64), rv)
    with pytest.raises(ValueError):
        gpu.topk(x.t(), 3)  # the last dimension is not contiguous


def test_error_returns(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    keys = torch.zeros(4096, dtype=torch.int32, device="cuda")
    vals = torch.zeros(4096, dtype=torch.int32, device="cuda")
    out = torch.zeros(4096, dtype=torch.int32, device="cuda")
    outv = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, v, o, ov = keys.data_ptr(), vals.data_ptr(), out.data_ptr(), outv.data_ptr()
    hk = gpu.TopK(2048, 64)
    hp = gpu.TopK(2048, 64, mode=gpu.MODE_PAIRS, value_bytes=4)
    h8 = gpu.TopK(2048, 64, mode=gpu.MODE_PAIRS, value_bytes=8)

    def rk(h, keys_p, rows, row_len, stride, k, out_p, kt=0, order=0):
        return lib.gs_topk_select_rows_keys(h._h, keys_p, rows, row_len, stride, k, out_p, kt, order, None)

    def rp(h, keys_p, vals_p, rows, row_len, stride, k, out_p, outv_p, kt=0, order=0):
        return lib.gs_topk_select_rows_pairs(h._h, keys_p, vals_p, rows, row_len, stride, k, out_p, outv_p, kt, order, None)

    assert rk(hk, p, 4, 100, 100, 8, o) == _lib.GS_OK
    assert rp(hp, p, v, 4, 100, 100, 8, o, ov) == _lib.GS_OK
    assert rp(hp, p, None, 4, 100, 100, 8, o, ov) == _lib.GS_OK
    # sizes
    for rows, row_len, stride, k in ((0, 100, 100, 8), (4, 0, 100, 1), (4, 100, 100, 0), (4, 100, 100, 101), (4, 100, 100, 65), (21, 100, 100, 8),
                                     (2, 100, 1949, 8), (3, 100, 0x7FFFFFFF, 8)):
        assert rk(hk, p, rows, row_len, stride, k, o) == S, (rows, row_len, stride, k)
    assert rk(hk, p, 2, 100, 1948, 8, o) == _lib.GS_OK  # (rows - 1) * stride + row_len == max_keys
    # arguments
    assert rk(hk, p, 4, 100, 99, 8, o) == A                      # stride < row_len
    assert rk(hk, None, 4, 100, 100, 8, o) == A and rk(hk, p, 4, 100, 100, 8, None) == A
    assert rk(hk, p + 4, 4, 100, 100, 8, o) == A and rk(hk, p, 4, 100, 100, 8, o + 8) == A
    assert rk(hk, p, 4, 100, 100, 8, o, kt=3) == A and rk(hk, p, 4, 100, 100, 8, o, order=2) == A
    assert rk(hk, p, 4, 100, 100, 8, p + 16 * 99) == A           # the output starts inside the input
    assert rk(hk, p, 4, 100, 100, 8, p - 16) == A                # ... and ends inside it
    assert rk(hk, p, 4, 100, 100, 8, p + 4 * 400) == _lib.GS_OK  # right behind the last row
    assert rp(hp, p, v, 4, 100, 100, 8, o, None) == A and rp(hp, p, v + 4, 4, 100, 100, 8, o, ov) == A
    assert rp(hp, p, v, 4, 100, 100, 8, o, v + 16) == A          # values out overlapping values in
    assert rp(h8, p, None, 4, 100, 100, 8, o, ov) == A           # positions need a 4-byte handle
    # modes
    assert rp(hk, p, v, 4, 100, 100, 8, o, ov) == M
    assert rk(hp, p, 4, 100, 100, 8, o) == M
    buf = (__import__("ctypes").c_uint32 * 8)()
    assert lib.gs_topk_rows_last(hk._h, buf, 7, None) == A and lib.gs_topk_rows_last(hk._h, None, 8, None) == A
    torch.cuda.synchronize()
    for h in (hk, hp, h8):
        h.close()
