"""The row-wise top-k on 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 of gs_topk_select_rows_*,
gpusorting_amd/csrc/topk_rows16_kernels.hpp) on the GPU.  Built like tests/test_gpu_topk_rows.py: every case compares keys AND values
bit for bit with gpusorting_amd.topk_rows_reference (tests/test_topk_rows16_cpu.py), calls status(), asks rows_last() for the route,
checks the fill behind element rows * k of both outputs and that the inputs are unchanged.  Keys are 2-byte words cut from the
init_random output, or built against the structure of the kernels.  No counterpart in the reference project."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
KEY_TYPES = (U16, I16, F16, BF16)
VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
LDS_ROW = {0: 32768, 4: 16384, 8: 8192}  # seg_max_lds: rows up to here are sorted in LDS
NONE, WAVE, TILE, STREAM = 0, 1, 2, 3
MODES = ("keys", "pos", "v4", "v8")
FILL16, FILL = 0x5EED, 0x5EEDBEEF
LONG = 70001  # more than two stream tiles of 32 768 elements plus a peel


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def _vb(mode):
    return {"keys": 0, "v4": 4, "v8": 8, "pos": 4}[mode]


def _max_k(gpu, mode):
    from gpusorting_amd.topk import rows_max_k
    vb = _vb(mode)
    return rows_max_k(gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _random16(gpu, n, seed, preset=None):
    """n 2-byte words cut from the init_random output."""
    torch = _torch()
    dk = torch.empty((n + 1) // 2, dtype=torch.int32, device="cuda")
    gpu.init_random(dk, seed, gpu.ENTROPY_PRESET_1 if preset is None else preset)
    torch.cuda.synchronize()
    return dk.cpu().numpy().view(np.uint16)[:n].copy()


def _values(n, mode):
    """Values that differ from the position, so that a position written for a value shows."""
    if mode == "v4":
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    if mode == "v8":
        return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x1F)
    return None


def _handle(gpu, max_keys, max_k, mode, key_type=U16, descending=False):
    vb = _vb(mode)
    return gpu.TopK(max_keys, max_k, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type,
                    gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _extent(rows, row_len, stride):
    return (rows - 1) * stride + row_len


def _view2d(flat, rows, row_len, stride):
    return np.lib.stride_tricks.as_strided(flat, (rows, row_len), (stride * flat.itemsize, flat.itemsize), writeable=False)


def _route(gpu, row_len, k, mode):
    assert row_len <= LDS_ROW[_vb(mode)] or k <= _max_k(gpu, mode), "16-bit keys have no LOOP route"
    return WAVE if row_len <= 256 else TILE if row_len <= LDS_ROW[_vb(mode)] else STREAM


class _Case:
    """One matrix of 2-byte keys on the device and its full per-row reference (k = row_len), computed once: the reference for a
    smaller k is its head, by the definition of topk_reference."""

    def __init__(self, gpu, flat, rows, row_len, stride, mode, key_type=U16, descending=False):
        assert flat.dtype == np.uint16
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
        ok = torch.full((m + pad,), FILL16, dtype=torch.int16, device="cuda")
        ov = torch.full((m + pad,), FILL, dtype=torch.int32 if vb == 4 else torch.int64, device="cuda") if vb else None
        h.select_rows(self.dk, self.rows, self.row_len, self.stride, k, ok, self.dv, ov)
        assert h.status() == 0
        rep = h.rows_last()
        assert (rep["rows"], rep["row_len"], rep["k"], rep["status"]) == (self.rows, self.row_len, k, 0)
        assert rep["route"] == (route or _route(gpu, self.row_len, k, self.mode)), rep
        assert rep["reads"] in ((2, 3) if rep["route"] == STREAM else (0,)), rep
        hk = ok.cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(hk[:m].reshape(self.rows, k), self.rk[:, :k].view(np.uint16))
        assert np.all(hk[m:] == FILL16), "nothing behind element rows * k of the output keys is written"
        if vb:
            hv = ov.cpu().numpy().view(VALUE_DTYPE[vb])
            np.testing.assert_array_equal(hv[:m].reshape(self.rows, k), self.rv[:, :k].astype(VALUE_DTYPE[vb]))
            assert np.all(hv[m:] == FILL), "nothing behind element rows * k of the output values is written"
        return rep

    def inputs_unchanged(self):
        np.testing.assert_array_equal(self.dk.cpu().numpy().view(np.uint16), self.flat)
        if self.dv is not None:
            np.testing.assert_array_equal(self.dv.cpu().numpy().view(self.vals.dtype), self.vals)


def _row_lens(vb):
    L = LDS_ROW[vb]
    return (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1025, L - 1, L, L + 1, 40000, LONG)


# ---- route borders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("len_index", range(18))
def test_route_borders(gpu, mode, len_index):
    """Every row length around a route border and around the eight elements of a 16-byte load, rows 1 / 3 / 67, strides row_len,
    row_len + 1, + 3 (2-byte-only row starts) and + 13, k = 1, 2, min(64, row_len), min(gs_topk_rows_max_k, row_len)."""
    row_len = _row_lens(_vb(mode))[len_index]
    ks = sorted({1, min(2, row_len), min(64, row_len), min(_max_k(gpu, mode), row_len)})
    shapes = [(1, 0), (3, 1), (3, 3), (3, 13), (3, 0)] + ([(67, 1), (67, 0)] if row_len <= 1025 else [])
    h = _handle(gpu, _extent(67, row_len, row_len + 13), row_len, mode)
    for i, (rows, extra) in enumerate(shapes):
        stride = row_len + extra
        case = _Case(gpu, _random16(gpu, _extent(rows, row_len, stride), 100 + len_index * 8 + i), rows, row_len, stride, mode)
        for k in ks:
            case.run(h, k)
        case.inputs_unchanged()
    h.close()


# ---- types and orders ------------------------------------------------------------------------------------------------------------
FLOAT_SALT = {  # +-0, +-inf, NaNs of both signs, denormals, the largest finite values
    F16: [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF],
    BF16: [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x0001, 0x8001, 0x007F, 0x7F7F, 0xFF7F],
}
INT_SALT = [0x0000, 0xFFFF, 0x8000, 0x7FFF, 0x0001, 0x8001]


def _salted(gpu, n, seed, key_type):
    flat = _random16(gpu, n, seed)
    salt = np.array(FLOAT_SALT.get(key_type, INT_SALT), dtype=np.uint16)
    at = np.arange(0, n, 5)
    flat[at] = salt[(at // 5) % salt.size]
    return flat


@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("long_row", [False, True])
def test_types_and_orders(gpu, key_type, descending, long_row):
    mode = "pos"
    row_len, rows = (LDS_ROW[4] + 1 if long_row else 257), 5
    stride = row_len + 1
    flat = _salted(gpu, _extent(rows, row_len, stride), 40 + key_type, key_type)  # (every fifth element one of 13 or 6 values: ties)
    h = _handle(gpu, flat.size, row_len, mode, key_type, descending)
    case = _Case(gpu, flat, rows, row_len, stride, mode, key_type, descending)
    for k in (1, 50, 257):
        case.run(h, k)
    case.inputs_unchanged()
    h.close()


# ---- every bit pattern once ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_patterns():
    a = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    np.random.default_rng(16).shuffle(a)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("key_type", KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shape", ["wave", "tile", "stream"])
def test_every_bit_pattern_once(gpu, all_patterns, key_type, descending, shape):
    rows, row_len = {"wave": (256, 256), "tile": (8, 8192), "stream": (1, 65536)}[shape]
    for mode in (MODES if shape == "tile" else ("pos",)):
        k = row_len if shape != "stream" else _max_k(gpu, mode)
        h = _handle(gpu, 65536, k, mode, key_type, descending)
        case = _Case(gpu, all_patterns.copy(), rows, row_len, row_len, mode, key_type, descending)
        case.run(h, k, {"wave": WAVE, "tile": TILE, "stream": STREAM}[shape])
        case.inputs_unchanged()
        h.close()


# ---- structure of the stream select ----------------------------------------------------------------------------------------------
def _stream_case(gpu, keys2d, mode, descending, ks, key_type=U16, stride_extra=1, reads=None):
    rows, row_len = keys2d.shape
    stride = row_len + stride_extra
    flat = np.full(_extent(rows, row_len, stride), 0xA5A5, dtype=np.uint16)
    for r in range(rows):
        flat[r * stride:r * stride + row_len] = keys2d[r].view(np.uint16)
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
    """The exact level, the share taken by position (the lowest positions ascending, the highest descending) and the packed counts of
    a tile at their maximum: every element of every full tile is `equal`."""
    _stream_case(gpu, np.full((2, LONG), 0x1234, dtype=np.uint16), "pos", descending, (1, 64, 4096), reads=3)


@pytest.mark.parametrize("descending", [False, True])
def test_stream_keys_share_their_top_12_bits(gpu, descending):
    """More than gs_topk_rows_max_k elements share the top 12 bits of the k-th: the second, exact level (three reads; 16 values over
    the row: every value is a run of ties that the LDS sort puts in position order)."""
    low = _random16(gpu, 3 * LONG, 77).reshape(3, LONG) & np.uint16(0x000F)
    _stream_case(gpu, low | np.uint16(0xABC0), "pos", descending, (1, 64, 1000), reads=3)


@pytest.mark.parametrize("descending", [False, True])
def test_stream_spread_keys_take_two_reads(gpu, descending):
    """Random words: 70 001 / 4096 = 17 elements to a bin of the first level, so the elements in front of the k-th and its bin fit
    the staging for every k <= 1000."""
    _stream_case(gpu, _random16(gpu, 3 * LONG, 78).reshape(3, LONG), "pos", descending, (1, 64, 1000), reads=2)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("copies", ["few", "many"])
def test_stream_threshold_run_straddles_tile_and_chunk_borders(gpu, descending, copies):
    """The threshold value T sits on both sides of every border of an 8192-element load chunk, so of every 32 768-element tile (and,
    with an odd stride, of the peeled chunks), k takes only a part of its copies: position-rank ties.  "few": all copies are staged
    and the LDS sort decides; "many": more copies than the staging holds, the gather takes the wanted share by rank."""
    rows, row_len = 3, LONG
    T = np.uint16(0x4000)
    keys = (_random16(gpu, rows * row_len, 55).reshape(rows, row_len) >> np.uint16(2)) | np.uint16(0x8000)  # behind T (ascending)
    pos = np.arange(row_len)
    at_border = (pos % 8192 < 9) | (pos % 8192 >= 8183)
    keys[:, at_border if copies == "few" else (at_border | (pos % 3 == 0))] = T
    keys[:, 100::5000] = np.uint16(7)  # in front of T
    if descending:
        keys = ~keys
    count = int(np.count_nonzero(keys[0] == (~T if descending else T)))
    front = int(np.count_nonzero(keys[0] == (~np.uint16(7) if descending else np.uint16(7))))
    assert (count < 4096 - front) == (copies == "few")
    for mode in ("pos", "keys"):
        _stream_case(gpu, keys, mode, descending, (front + 1, front + min(count, 4000) // 2), stride_extra=1 if mode == "pos" else 2)


@pytest.mark.parametrize("descending", [False, True])
def test_stream_sorted_and_reverse_sorted_rows(gpu, descending):
    """Whole waves under one bin of the histogram: the one-add shortcut."""
    base = np.sort(_random16(gpu, LONG, 91))
    _stream_case(gpu, np.stack([base, base[::-1], np.sort(base >> np.uint16(6))]), "pos", descending, (1, 777))


# ---- against the 32-bit path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", [BF16, F16])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("rows,row_len", [(67, 257), (3, LDS_ROW[4] + 1)])
def test_against_the_32_bit_call_on_the_widened_matrix(gpu, key_type, descending, rows, row_len):
    """What a caller did before: widen to float32, call gs_topk_select_rows_pairs.  Same positions, and the same keys once narrowed.
    bfloat16: bits << 16, every pattern; float16: .float(), finite and infinite values only (NaN payloads do not survive a cast)."""
    torch = _torch()
    k = min(row_len, 300)
    flat = _salted(gpu, rows * row_len, 7, key_type)
    if key_type == F16:
        nan = ((flat & np.uint16(0x7C00)) == 0x7C00) & ((flat & np.uint16(0x03FF)) != 0)
        flat[nan] &= np.uint16(0xFC00)  # -> the infinity of its sign
    d16 = _dev(flat)
    if key_type == BF16:
        d32 = (d16.to(torch.int32) << 16)
    else:
        d32 = d16.view(torch.float16).float().view(torch.int32)
    out = {}
    for name, keys, kt in (("16", d16, key_type), ("32", d32, 2)):
        h = _handle(gpu, flat.size, k, "pos", kt, descending)
        ok = torch.empty(rows * k, dtype=keys.dtype, device="cuda")
        ov = torch.empty(rows * k, dtype=torch.int32, device="cuda")
        h.select_rows(keys, rows, row_len, row_len, k, ok, None, ov)
        assert h.status() == 0
        out[name] = (ok, ov)
        h.close()
    np.testing.assert_array_equal(out["16"][1].cpu().numpy(), out["32"][1].cpu().numpy())
    k32 = out["32"][0]
    narrowed = (k32 >> 16).to(torch.int16) if key_type == BF16 else k32.view(torch.float32).half().view(torch.int16)
    np.testing.assert_array_equal(out["16"][0].cpu().numpy(), narrowed.cpu().numpy())


# ---- the memory contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,row_len,k", [(WAVE, 200, 9), (TILE, 3002, 65), (STREAM, 16384 + 4098, 131)])
@pytest.mark.parametrize("mode", ["pos", "v4"])
def test_memory_contract_on_a_guard_arena(gpu, route, row_len, k, mode):
    """Bases with 16 bytes of alignment and no more, guard bands around the inputs and the [rows, k] outputs, an odd stride and an odd
    k (rows and output rows start at odd elements: 2-byte alignment only), a handle whose max_keys is the extent exactly.  The gaps
    between the rows hold a key that would win every selection (0, ascending) and must never come out.  The arena carves bytes for
    the 2-byte keys: it knows 1-, 4- and 8-byte elements."""
    from guard_arena import Arena
    torch = _torch()
    rows, stride = 3, row_len + 3
    assert stride % 2 == 1 and k % 2 == 1
    n = _extent(rows, row_len, stride)
    flat = np.zeros(n, dtype=np.uint16)
    body = _random16(gpu, rows * row_len, 23) | np.uint16(1)
    for r in range(rows):
        flat[r * stride:r * stride + row_len] = body[r * row_len:(r + 1) * row_len]
    vals = _values(n, mode)
    spare = 11
    m = rows * k
    specs = [(2 * n, np.uint8), (2 * (m + spare), np.uint8), (m + spare, np.uint32)] + ([(n, np.uint32)] if vals is not None else [])
    arena = Arena.for_views(specs, "cuda", fill="hash")
    dk = arena.carve(2 * n, np.uint8, 1, "keys")
    ok = arena.carve(2 * (m + spare), np.uint8, 3, "out_keys")
    ov = arena.carve(m + spare, np.uint32, 5, "out_values")
    dv = None
    if vals is not None:
        dv = arena.carve(n, np.uint32, 7, "values")
        arena.write(dv, vals)
    arena.write(dk, flat.view(np.uint8))
    arena.live(ok, 2 * m)
    arena.live(ov, m)
    h = _handle(gpu, n, k, mode)
    h.select_rows(dk.view(torch.int16), rows, row_len, stride, k, ok.view(torch.int16), dv, ov)
    assert h.status() == 0
    assert h.rows_last()["route"] == route
    h.close()
    arena.verify()
    rk, rv = gpu.topk_rows_reference(_view2d(flat, rows, row_len, stride), k, None if vals is None else _view2d(vals, rows, row_len, stride), U16)
    hk = arena.read(ok, np.uint16, 2 * m)
    assert not np.any(hk == 0), "a key of a gap between two rows was selected"
    np.testing.assert_array_equal(hk.reshape(rows, k), rk)
    np.testing.assert_array_equal(arena.read(ov, np.uint32, m).reshape(rows, k), rv)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    A, S = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE
    L = LDS_ROW[4]
    n = 2 * L + 64
    keys = torch.zeros(n, dtype=torch.int32, device="cuda")  # (as 2-byte elements: 2 n of them)
    out = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    outv = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 100], dtype=torch.int32, device="cuda")
    p, o, ov = keys.data_ptr(), out.data_ptr(), outv.data_ptr()
    max_k = _max_k(gpu, "pos")
    hk = gpu.TopK(n, max_k + 1)
    hp = gpu.TopK(n, max_k + 1, mode=gpu.MODE_PAIRS, value_bytes=4)
    sorter = gpu.OneSweep(n)
    seg = gpu.SegmentedSort(n, 4)

    def rk(keys_p, rows, row_len, stride, k, out_p, kt=U16):
        return lib.gs_topk_select_rows_keys(hk._h, keys_p, rows, row_len, stride, k, out_p, kt, 0, None)

    # the other entries do not know the 16-bit key types
    for kt in KEY_TYPES:
        assert lib.gs_topk_select_keys(hk._h, p, 4096, 8, o, kt, 0, None) == A
        assert lib.gs_topk_select_pairs(hp._h, p, None, 4096, 8, o, ov, kt, 0, None) == A
        assert lib.gs_onesweep_sort_keys(sorter._h, p, o, 4096, kt, 0, None) == A
        assert lib.gs_segsort_sort_keys(seg._h, p, o, 4096, offs.data_ptr(), 1, 0, kt, 0, None) == A
        assert rk(p, 4, 100, 100, 8, o, kt) == _lib.GS_OK
    assert rk(p, 4, 100, 100, 8, o, 10) == A and rk(p, 4, 100, 100, 8, o, -1) == A
    assert lib.gs_topk_select_rows_pairs(hp._h, p, None, 4, 100, 100, 8, o, ov, 10, 0, None) == A
    # a base pointer with 4 bytes of alignment, keys in or out
    assert rk(p + 4, 4, 100, 100, 8, o) == A and rk(p, 4, 100, 100, 8, o + 4) == A and rk(p + 2, 4, 100, 100, 8, o) == A
    # the overlap test takes 2-byte extents: 4 rows of 100 at stride 100 end at byte 800, a multiple of 16
    assert rk(p, 4, 100, 100, 8, p + 800) == _lib.GS_OK
    assert rk(p, 4, 100, 100, 8, p + 800 - 16) == A
    assert rk(p, 4, 101, 101, 8, p + 800) == A                    # 808 bytes of input
    assert rk(p, 4, 101, 101, 8, p + 816) == _lib.GS_OK           # the first 16-byte boundary behind it
    assert rk(p + 64, 4, 100, 100, 8, p) == _lib.GS_OK and rk(p + 64, 4, 100, 100, 8, p + 16) == A  # 4 x 8 x 2 = 64 bytes of output
    # max_keys counts elements
    assert rk(p, 1, n, n, 8, o) == _lib.GS_OK and rk(p, 1, n + 1, n + 1, 8, o) == S
    torch.cuda.synchronize()
    # no LOOP route: a row longer than LDS holds with k > gs_topk_rows_max_k is refused before anything is launched
    out.fill_(FILL)
    outv.fill_(FILL)
    assert lib.gs_topk_select_rows_pairs(hp._h, p, None, 2, L + 1, L + 1, max_k + 1, o, ov, BF16, 1, None) == S
    assert hp.rows_last()["route"] == NONE
    assert lib.gs_topk_select_rows_pairs(hp._h, p, None, 2, L, L, max_k + 1, o, ov, BF16, 1, None) == _lib.GS_OK  # (fits LDS: TILE, every k)
    assert hp.rows_last()["route"] == TILE
    out.fill_(FILL)
    assert rk(p, 1, 2 * L + 1, 2 * L + 1, max_k + 1, o) == S
    assert hk.rows_last()["route"] == NONE
    assert bool((out == FILL).all()), "a refused call writes nothing"
    # the Python layer: the 1-D call has no 16-bit form, and the key tensors' width follows the key type
    h16 = gpu.TopK(4096, 8, key_type=F16)
    k16 = torch.zeros(4096, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        h16.select(k16, 8, torch.zeros(8, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        h16.select_rows(keys, 4, 100, 100, 8, out)  # 4-byte tensors on a 16-bit handle
    with pytest.raises(ValueError):
        hk.select_rows(k16, 4, 100, 100, 8, k16.clone())  # 2-byte tensors on a 32-bit handle
    for h in (hk, hp, h16, sorter, seg):
        h.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_len,k", [(64, 8), (16384 + 77, 100)])
def test_captured_graph_replayed_on_new_data(gpu, row_len, k):
    """One wave-route and one stream-route call, each a single-stream, linear capture, replayed after the input was overwritten."""
    torch = _torch()
    rows, stride = 9, row_len + 1
    n = _extent(rows, row_len, stride)
    h = _handle(gpu, n, k, "pos", BF16, True)
    dk = _dev(_random16(gpu, n, 31))
    ok = torch.empty(rows * k, dtype=torch.int16, device="cuda")
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
        keys = _random16(gpu, n, seed, gpu.ENTROPY_PRESET_3 if seed == 33 else None)
        dk.copy_(_dev(keys))
        ok.zero_()
        ov.zero_()
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rv = gpu.topk_rows_reference(_view2d(keys, rows, row_len, stride), k, None, BF16, True)
        np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint16).reshape(rows, k), rk)
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32).reshape(rows, k), rv)
    h.close()


# ---- functional.topk -------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(_torch().int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("dtype_name,key_type", [("float16", F16), ("bfloat16", BF16), ("int16", I16)])
def test_functional_topk(gpu, dtype_name, key_type):
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    rows, width, k = 33, 1000, 17
    # NaN-free and tie-free: every row a permutation of 1000 distinct representable values
    if key_type == I16:
        distinct = (np.arange(width) * 61 - 30000).astype(np.int16).view(np.uint16)
    else:  # 500 positive and 500 negative finite patterns, valid in both float formats
        distinct = np.concatenate([0x3000 + np.arange(500), 0xB000 + np.arange(500)]).astype(np.uint16)
    rng = np.random.default_rng(5)
    m = np.stack([rng.permutation(distinct) for _ in range(rows)])
    x = torch.from_numpy(m.view(np.int16)).cuda().view(dtype)
    for view in (x, x[:, :777]):
        for largest in (True, False):
            v, i = gpu.topk(view, k, largest=largest)
            tv, ti = torch.topk(view, k, dim=-1, largest=largest)
            assert v.shape == (rows, k) and v.dtype == dtype and i.dtype == torch.int32
            np.testing.assert_array_equal(_bits(v), _bits(tv))
            np.testing.assert_array_equal(i.cpu().numpy(), ti.cpu().numpy().astype(np.int32))
    # with ties (and, for the floats, NaNs and both zeros): the library's order, as the reference states it
    t = _random16(gpu, rows * width, 9).reshape(rows, width) & np.uint16(0xFC07)
    xt = torch.from_numpy(t.view(np.int16).copy()).cuda().view(dtype)
    for largest in (True, False):
        v, i = gpu.topk(xt[:, :901], 40, largest=largest)
        rk, rv = gpu.topk_rows_reference(t[:, :901], 40, None, key_type, largest)
        np.testing.assert_array_equal(_bits(v), rk)
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
    if key_type == I16:  # int16 storage as unsigned keys, with carried values
        vals = torch.arange(rows * width, dtype=torch.int64, device="cuda").reshape(rows, width) * 3
        v, w = gpu.topk(xt, 12, largest=False, values=vals, unsigned=True)
        rk, rv = gpu.topk_rows_reference(t, 12, (np.arange(rows * width, dtype=np.uint64) * 3).reshape(rows, width), U16, False)
        np.testing.assert_array_equal(_bits(v), rk)
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint64), rv)
    # a 1-D tensor names the 2-D form; a shape without a route states the rule
    with pytest.raises(TypeError, match=r"x\[None, :\]"):
        gpu.topk(x[0], 5)
    long = torch.zeros((2, LDS_ROW[4] + 1), dtype=dtype, device="cuda")
    with pytest.raises(ValueError, match="k <= %d" % _max_k(gpu, "pos")):
        gpu.topk(long, _max_k(gpu, "pos") + 1)
    v, i = gpu.topk(long[:1], 3, largest=False)  # (one row of zeros: the lowest positions)
    assert i.cpu().numpy().tolist() == [[0, 1, 2]]


def test_functional_topk_on_uint16_storage(gpu):
    """int16 storage with unsigned=True, and a torch.uint16 tensor where this torch has the dtype: the same keys, the same result."""
    torch = _torch()
    t = _random16(gpu, 5 * 300, 11).reshape(5, 300)
    x = torch.from_numpy(t.view(np.int16).copy()).cuda()
    rk, rv = gpu.topk_rows_reference(t, 9, None, U16, True)
    views = [(x, True)] + ([(x.view(torch.uint16), False)] if hasattr(torch, "uint16") else [])
    for view, unsigned in views:
        v, i = gpu.topk(view, 9, unsigned=unsigned)
        assert v.dtype == view.dtype
        np.testing.assert_array_equal(_bits(v), rk)
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
