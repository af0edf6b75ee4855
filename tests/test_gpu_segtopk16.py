"""The segmented top-k on 16-bit keys (gs_segtopk16_*, gpusorting_amd/csrc/topk_seg16_kernels.hpp) on the GPU: every case compares
keys AND values bit for bit with gpusorting_amd.segmented_topk_reference on uint16 bit patterns (tests/test_segtopk16_cpu.py), on
outputs pre-filled with a pattern so that the slots the call must not write are compared too — a 2-byte slot beside a written one in
the same 32-bit word among them — calls check(), and asks last() which kernels ran.  Every input is seeded.  No counterpart in the
reference project."""
import ctypes as C

import numpy as np
import pytest

from test_segtopk16_cpu import SPECIAL, special_keys

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
LDS = {0: 32768, 4: 16384, 8: 8192}  # gs_segsort_max_lds_segment: segments up to here are selected in LDS
CLASS_MAX = (1, 32, 256, 1024, 2048, 8192, 16384, 32768)
MODES = ("keys", "pos", "v4", "v8")
FILL, FILL_V = 0x5EED, 0x0BADF00D
PAD = 37  # output elements behind num_segments * k that must keep the fill
OK, ERR_ARG, ERR_SIZE = 0, 1, 2
TILE16 = 32768  # elements per tile of the 16-bit select; a load chunk is 8192


def _torch():
    import torch
    return torch


def _dev(a):
    view = {2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return _torch().from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def _vb(mode):
    return {"keys": 0, "v4": 4, "v8": 8, "pos": 4}[mode]


def _vi(mode):
    return MODES.index(mode)


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 16, n, dtype=np.uint16)


def _values(n, mode):
    """Values that differ from the position, so that a position written for a value shows."""
    if mode == "v4":
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    if mode == "v8":
        return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x1F)
    return None


def _offsets(lens, front=3):
    return np.concatenate([[front], front + np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def _handle(gpu, n, segs, k, mode, key_type=U16, descending=False):
    vb = _vb(mode)
    return gpu.SegmentedTopK16(n, segs, k, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type,
                               gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _class_of(length, vb):
    if length > LDS[vb]:
        return 8
    return next(c for c, m in enumerate(CLASS_MAX) if length <= m) if length > 1 else 0


class _Case:
    """One array of 2-byte keys and its offsets on the device; run(h, k): a call into fresh, pre-filled outputs, compared with the
    reference."""

    def __init__(self, gpu, bits, offsets, mode, key_type=U16, descending=False, tail=5):
        self.gpu, self.mode, self.kt, self.desc = gpu, mode, key_type, descending
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.segs = self.offsets.size - 1
        self.n = int(self.offsets[-1]) + tail  # off[S] < n
        assert bits.size >= self.n and bits.dtype == np.uint16
        self.bits = np.ascontiguousarray(bits[:self.n])
        self.vals = _values(self.n, mode)
        self.dk, self.do = _dev(self.bits), _dev(self.offsets.astype(np.uint32))
        self.dv = None if self.vals is None else _dev(self.vals)

    def expected(self, k, untouched=()):
        from gpusorting_amd.segtopk import segmented_topk_reference
        vdt = VALUE_DTYPE[_vb(self.mode)] if _vb(self.mode) else None
        rk, rv, counts = segmented_topk_reference(self.bits, self.offsets, k, self.vals, self.desc, self.kt, fill_key=FILL, fill_value=FILL_V)
        for s in untouched:
            rk[s], rv[s] = FILL, FILL_V
        return rk.reshape(-1), (rv.astype(vdt).reshape(-1) if vdt else None), counts

    def outputs(self, k):
        torch = _torch()
        ok = torch.full((self.segs * k + PAD,), FILL, dtype=torch.int16, device="cuda")
        vb = _vb(self.mode)
        ov = None if not vb else torch.full((self.segs * k + PAD,), FILL_V, dtype=torch.int64 if vb == 8 else torch.int32, device="cuda")
        return ok, ov

    def compare(self, k, ok, ov, untouched=()):
        rk, rv, _ = self.expected(k, untouched)
        got = ok.cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(got[:rk.size], rk, err_msg=f"keys, k={k} mode={self.mode}")
        assert (got[rk.size:] == FILL).all(), "written behind num_segments * k"
        if ov is not None:
            gv = ov.cpu().numpy().view(rv.dtype)
            np.testing.assert_array_equal(gv[:rv.size], rv, err_msg=f"values, k={k} mode={self.mode}")
            assert (gv[rv.size:] == FILL_V).all(), "values written behind num_segments * k"

    def run(self, h, k, max_len=0, status=OK, untouched=()):
        ok, ov = self.outputs(k)
        h.select(self.dk, self.do, k, ok, self.dv, ov, n=self.n, max_segment_len=max_len)
        assert h.status() == status
        self.compare(k, ok, ov, untouched)
        return h.last()

    def inputs_unchanged(self):
        np.testing.assert_array_equal(self.dk.cpu().numpy().view(np.uint16), self.bits)
        np.testing.assert_array_equal(self.do.cpu().numpy().view(np.uint32), self.offsets.astype(np.uint32))
        if self.dv is not None:
            np.testing.assert_array_equal(self.dv.cpu().numpy().view(self.vals.dtype), self.vals)

    def check_classes(self, rep, max_len=0):
        vb = _vb(self.mode)
        lens = np.diff(self.offsets)
        want = [0] * 9
        for length in lens:
            want[0 if (max_len and length > max_len) else _class_of(int(length), vb)] += 1
        assert rep["counts"] == want, (rep, want)
        assert rep["longest"] == int(lens.max())
        assert rep["packed"] == int(np.count_nonzero((lens >= 1) & (lens <= 32) & ((lens <= max_len) | (max_len == 0))))


def _set_order(gpu, h, case, desc):
    case.desc = desc
    h.order = gpu.ORDER_DESCENDING if desc else gpu.ORDER_ASCENDING


# ---- class borders in one call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_class_borders_in_one_call(gpu, mode):
    L = LDS[_vb(mode)]
    lens = sorted({0, 1, 2, 31, 32, 33, 255, 256, 257, 1024, 1025, 2048, 2049, 8192, 8193, L, L + 1})
    np.random.default_rng(7).shuffle(lens)
    mixed = []
    for length in lens:  # empty segments between them; the front gap and the odd lengths give odd starts
        mixed += [int(length), 0]
    off = _offsets(mixed, front=3)
    assert any(int(o) % 2 for o in off) and len({int(o) % 8 for o in off}) >= 4
    case = _Case(gpu, _bits(int(off[-1]) + 5, 11), off, mode)
    h = _handle(gpu, case.n, case.segs, 300, mode)
    for k in (1, 33, 300):
        rep = case.run(h, k)
        case.check_classes(rep)
        assert rep["k"] == k and rep["status"] == 0 and rep["reads"] in (2, 3)
        want = gpu._lib.GS_SEGTOPK_F_PACKED | gpu._lib.GS_SEGTOPK_F_WAVE | gpu._lib.GS_SEGTOPK_F_STREAM | (gpu._lib.GS_SEGTOPK_F_VM << _vi(mode))
        for c in range(3, 8):
            if CLASS_MAX[c] <= L:
                want |= gpu._lib.GS_SEGTOPK_F_TILE(c, rep["rank"])
        assert rep["forms"] == want, (hex(rep["forms"]), hex(want))
    case.inputs_unchanged()
    h.close()


# ---- every compiled cell ----------------------------------------------------------------------------------------------------------
def _tile_cells():
    for c in range(3, 8):
        for mode in MODES:
            if CLASS_MAX[c] <= LDS[_vb(mode)]:
                for rank in (0, 1):
                    yield c, rank, mode


@pytest.mark.parametrize("c,rank,mode", list(_tile_cells()))
def test_every_tile_cell(gpu, c, rank, mode):
    """One segment of the class's shortest length and one of its longest on the cell's kernel: the forms word shows it ran."""
    lens = [CLASS_MAX[c - 1] + 1, CLASS_MAX[c]]
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 100 + c), off, mode, key_type=BF16, descending=bool(rank))
    h = _handle(gpu, case.n, case.segs, 64, mode, BF16, descending=bool(rank))
    h.set_rank_mode(rank)
    assert h.rank_mode == rank
    rep = case.run(h, 19, max_len=CLASS_MAX[c])
    assert rep["counts"][c] == 2 and rep["rank"] == rank
    assert rep["forms"] & gpu._lib.GS_SEGTOPK_F_TILE(c, rank) and not rep["forms"] & gpu._lib.GS_SEGTOPK_F_TILE(c, 1 - rank)
    assert rep["forms"] >> 16 == 1 << _vi(mode) and not rep["forms"] & gpu._lib.GS_SEGTOPK_F_STREAM
    h.close()


@pytest.mark.parametrize("mode", MODES)
def test_packed_wave_and_stream_cells(gpu, mode):
    L = LDS[_vb(mode)]
    for form, lens in (("PACKED", [1, 5, 0, 32, 2]), ("WAVE", [34, 256, 33, 100]), ("STREAM", [L + 1, L + 2, 2 * L + 5])):
        off = _offsets(lens, front=1)
        case = _Case(gpu, _bits(int(off[-1]) + 5, 200 + len(form)), off, mode)
        h = _handle(gpu, case.n, case.segs, 16, mode)
        rep = case.run(h, 7)
        case.check_classes(rep)
        assert rep["forms"] & getattr(gpu._lib, "GS_SEGTOPK_F_" + form) and rep["forms"] >> 16 == 1 << _vi(mode)
        assert (rep["reads"] >= 2) == (form == "STREAM") and rep["reads"] <= 3
        h.close()


# ---- 2-byte stores ------------------------------------------------------------------------------------------------------------------
# With k odd, row s + 1 begins in the 32-bit word in which row s ends; a segment shorter than k leaves the end of its row unwritten
# beside the written beginning of the next row, and its own written slots beside its unwritten ones.
def _store_lens(L):
    """Per kernel form: segments of that form between segments shorter than every k below (L: the LDS limit of the value mode)."""
    return {"PACKED": [2, 1, 0, 7, 2, 32, 1, 4], "WAVE": [2, 40, 1, 256, 0, 33, 2], "TILE": [1, 257, 2, 3001, 0, 1024, 2, 2049, 1],
            "STREAM": [2, L + 4099, 1, L + 1, 0, 2]}


@pytest.mark.parametrize("k", [3, 5, 9])
@pytest.mark.parametrize("mode", MODES)
def test_unwritten_slots_beside_written_ones_keep_the_sentinel(gpu, k, mode):
    lens = [x for form_lens in _store_lens(LDS[_vb(mode)]).values() for x in form_lens]
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 250 + k), off, mode, key_type=F16)
    h = _handle(gpu, case.n, case.segs, k, mode, F16)
    for desc in (False, True):
        _set_order(gpu, h, case, desc)
        rep = case.run(h, k)  # compares every slot: the sentinel in slots m_s .. k included
        assert rep["forms"] & 7 == 7 and rep["forms"] & gpu._lib.GS_SEGTOPK_F_TILE(3, rep["rank"])  # packed, wave, stream, tile
    h.close()


@pytest.mark.parametrize("k", [3, 5, 9])
@pytest.mark.parametrize("form", ["PACKED", "WAVE", "TILE", "STREAM"])
def test_memory_contract_on_a_guard_arena(gpu, form, k):
    """The same on 16-byte-only aligned inputs and outputs inside one arena, guard bands around both outputs, n below the buffers'
    length: nothing outside [0, S * k) of the outputs is written, nothing inside it that the reference does not write, and nothing
    in the inputs."""
    from guard_arena import Arena
    from gpusorting_amd.segtopk import segmented_topk_reference
    lens = _store_lens(LDS[4])[form]
    off = _offsets(lens, front=3)
    n, segs = int(off[-1]) + 2, len(lens)
    room = n + 101
    bits = _bits(room, 300 + k)
    arena = Arena.for_views([(2 * room, np.uint8), (segs + 1, np.uint32), (2 * (segs * k + 51), np.uint8), (segs * k + 50, np.uint32)], "cuda", "hash")
    dk = arena.carve(2 * room, np.uint8, 1, "keys")
    do = arena.carve(segs + 1, np.uint32, 5, "offsets")
    ok = arena.carve(2 * (segs * k + 51), np.uint8, 7, "out_keys")
    ov = arena.carve(segs * k + 50, np.uint32, 9, "out_values")
    arena.write(dk, bits.view(np.uint8))
    arena.write(do, off.astype(np.uint32))
    arena.write(ok, np.full(segs * k, FILL, dtype=np.uint16).view(np.uint8))
    arena.write(ov, np.full(segs * k, FILL_V, dtype=np.uint32))
    arena.live(ok, 2 * segs * k)
    arena.live(ov, segs * k)
    h = _handle(gpu, room, segs, k, "pos", I16)
    h.select(dk.view(_torch().int16), do, k, ok.view(_torch().int16), None, ov, n=n)
    h.check()
    rep = h.last()
    assert rep["forms"] & (gpu._lib.GS_SEGTOPK_F_TILE(3, rep["rank"]) if form == "TILE" else getattr(gpu._lib, "GS_SEGTOPK_F_" + form))
    arena.verify()
    rk, rv, _ = segmented_topk_reference(bits[:n], off, k, None, False, I16, fill_key=FILL, fill_value=FILL_V)
    np.testing.assert_array_equal(arena.read(ok, np.uint16, 2 * segs * k), rk.reshape(-1))
    np.testing.assert_array_equal(arena.read(ov, np.uint32, segs * k), rv.reshape(-1))
    h.close()


# ---- the all-one dummies -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type,pattern", [(U16, 0xFFFF), (F16, 0x7FFF), (U16, 0x0000), (BF16, 0xFFFF)])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("rank", [0, 1])
def test_a_real_key_that_ties_with_the_dummies(gpu, key_type, pattern, descending, rank):
    """A key whose sortable pattern is 0xFFFF (and its mirror image, 0x0000) at the last positions of segments that do not fill their
    slots: the dummies of the slots behind the segment must stay behind it.  k = the longest length: every element is emitted."""
    lens = [33, 100, 255, 1023, 2047]
    off = _offsets(lens, front=1)
    bits = _bits(int(off[-1]) + 5, 350)
    for s in range(len(lens)):
        seg = bits[off[s]:off[s + 1]]
        seg[-5:] = pattern
        seg[3::17] = pattern
    case = _Case(gpu, bits, off, "pos", key_type, descending)
    h = _handle(gpu, case.n, case.segs, 2047, "pos", key_type, descending)
    h.set_rank_mode(rank)
    rep = case.run(h, 2047)
    assert rep["counts"][2] == 3 and rep["counts"][3] == 1 and rep["counts"][4] == 1 and rep["rank"] == rank
    h.close()


# ---- types and orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", [U16, I16, F16, BF16])
@pytest.mark.parametrize("descending", [False, True])
def test_types_and_orders(gpu, key_type, descending):
    L = LDS[4]
    lens = [7, 0, 40, 300, 1, 2500, L + 300, 20, 200, 64, 64, 9000]
    off = _offsets(lens, front=1)
    n = int(off[-1]) + 5
    rng = np.random.default_rng(31 + key_type)
    bits = special_keys(rng, n, 0.3)
    bits[off[8]:off[9]] = SPECIAL[rng.integers(0, 2, 200)]    # a segment of zeros of both signs
    bits[off[9]:off[10]] = SPECIAL[rng.integers(2, 6, 64)]    # of infinities
    bits[off[10]:off[11]] = SPECIAL[rng.integers(6, 12, 64)]  # of NaNs
    case = _Case(gpu, bits, off, "pos", key_type, descending)
    h = _handle(gpu, case.n, case.segs, 128, "pos", key_type, descending)
    for k in (3, 100):
        rep = case.run(h, k)
        assert rep["counts"][8] == 1
    case.inputs_unchanged()
    h.close()


# ---- stream route -------------------------------------------------------------------------------------------------------------------
def _residue_lens(L):
    """Long segments of L + 1 .. L + 9 elements and one of two full tiles and a tail, each brought to its start residue mod 8 by a
    short filler in front of it; the residues are chosen so that the starts take all eight values and the ends do too (start = i
    cannot: start + length would take the odd values only)."""
    lens, at = [], 8
    longs = [L + 1 + i for i in range(9)] + [2 * TILE16 + 5]
    for long_len, start in zip(longs, (6, 0, 2, 5, 6, 1, 7, 4, 5, 3)):
        filler = (start - at) % 8
        lens += [filler, long_len]
        at += filler + long_len
    return lens, longs


@pytest.mark.parametrize("descending", [False, True])
def test_stream_every_start_and_end_residue(gpu, descending):
    L = LDS[4]
    lens, longs = _residue_lens(L)
    off = _offsets(lens, front=8)
    starts = [int(off[s]) % 8 for s, length in enumerate(lens) if length > L]
    ends = [int(off[s + 1]) % 8 for s, length in enumerate(lens) if length > L]
    assert set(starts) == set(range(8)) and set(ends) == set(range(8))
    case = _Case(gpu, _bits(int(off[-1]) + 5, 41), off, "pos", descending=descending)
    h = _handle(gpu, case.n, case.segs, 4096, "pos", descending=descending)
    for k in (1, 777, 4096):
        rep = case.run(h, k)
        assert rep["counts"][8] == len(longs)
        # uniform keys: a 12-bit bin holds a handful of them, so the first level ends the narrowing — unless k is the whole staging,
        # where the elements in front of the bin and those in it need not fit it together
        assert rep["reads"] == 2 or (k == 4096 and rep["reads"] == 3)
    case.inputs_unchanged()
    h.close()


@pytest.mark.parametrize("descending", [False, True])
def test_stream_keys_share_their_top_12_bits(gpu, descending):
    """Every key of a segment lies in one bin of the first level: the second, exact level is needed (three reads)."""
    L = LDS[4]
    lens = [L + 1, 3, 2 * L + 1, L + 9]
    off = _offsets(lens, front=1)
    bits = (_bits(int(off[-1]) + 5, 77) & np.uint16(0xF)) | np.uint16(0xABC0)
    case = _Case(gpu, bits, off, "pos", descending=descending)
    h = _handle(gpu, case.n, case.segs, 4096, "pos", descending=descending)
    for k in (1, 64, 4096):
        assert case.run(h, k)["reads"] == 3
    h.close()


@pytest.mark.parametrize("descending", [False, True])
def test_stream_threshold_repeated_across_chunk_and_tile_borders(gpu, descending):
    """The threshold key T sits on both sides of every border of a load chunk (8192 elements) and of a tile (32 768), in more copies
    than the staging holds, so k takes only a part of them (take < equal): the position rank decides, in both orders."""
    seg_len = 2 * TILE16 + 5
    lens = [seg_len, 3, seg_len]
    off = _offsets(lens, front=1)
    T = np.uint16(0x4000)
    bits = (_bits(int(off[-1]) + 5, 55) >> np.uint16(2)) | np.uint16(0x8000)  # behind T (ascending)
    pos = np.arange(seg_len)
    mark = (pos % 8192 < 9) | (pos % 8192 >= 8183) | (pos % 3 == 0)  # (the borders lie at most 7 elements off a multiple: the peel)
    for s in (0, 2):
        seg = bits[off[s]:off[s + 1]]
        seg[mark] = T
        seg[100::5000] = np.uint16(7)  # in front of T
    if descending:
        bits = ~bits
    count, front = int(np.count_nonzero(mark & (pos % 5000 != 100))), len(range(100, seg_len, 5000))
    assert count > 4096
    case = _Case(gpu, bits, off, "pos", descending=descending)
    h = _handle(gpu, case.n, case.segs, 4096, "pos", descending=descending)
    for k in (front + 1, front + 2000, 4096):
        assert case.run(h, k)["reads"] == 3
    h.close()


@pytest.mark.parametrize("descending", [False, True])
def test_stream_all_equal_segment_of_two_tiles_and_a_tail(gpu, descending):
    """65 541 equal keys: every element of a tile counts as equal, which is what the tile's 16-bit packed counts must hold."""
    lens = [3, 2 * TILE16 + 5, 1]
    off = _offsets(lens, front=5)
    bits = _bits(int(off[-1]) + 5, 66)
    bits[off[1]:off[2]] = 0xBEEF
    for mode in ("keys", "pos"):
        case = _Case(gpu, bits, off, mode, key_type=I16, descending=descending)
        h = _handle(gpu, case.n, case.segs, 4096, mode, I16, descending)
        for k in (1, 4096):
            rep = case.run(h, k)
            assert rep["counts"][8] == 1 and rep["reads"] == 3
        h.close()


# ---- parity with what exists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,row_len", [(64, 200), (8, 3001), (3, LDS[4] + 77)])
@pytest.mark.parametrize("descending", [False, True])
def test_uniform_offsets_equal_the_16_bit_row_wise_top_k(gpu, rows, row_len, descending):
    torch = _torch()
    k = 50
    bits = _bits(rows * row_len, 61) >> np.uint16(6)  # ties
    dk = _dev(bits)
    do = _dev((np.arange(rows + 1, dtype=np.int64) * row_len).astype(np.uint32))
    order = gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING
    seg = gpu.SegmentedTopK16(bits.size, rows, k, order, U16, gpu.MODE_PAIRS, 4)
    row = gpu.TopK(bits.size, k, order, U16, gpu.MODE_PAIRS, 4)
    sk, sv = torch.zeros(rows * k, dtype=torch.int16, device="cuda"), torch.zeros(rows * k, dtype=torch.int32, device="cuda")
    rk, rv = torch.ones(rows * k, dtype=torch.int16, device="cuda"), torch.ones(rows * k, dtype=torch.int32, device="cuda")
    seg.select(dk, do, k, sk, None, sv)
    seg.check()
    row.select_rows(dk, rows, row_len, row_len, k, rk, None, rv)
    row.check()
    assert torch.equal(sk, rk)
    starts = (torch.arange(rows, dtype=torch.int32, device="cuda") * row_len).repeat_interleave(k)
    assert torch.equal(sv, rv + starts)
    seg.close()
    row.close()


@pytest.mark.parametrize("largest", [False, True])
def test_ragged_mix_equals_the_heads_of_the_16_bit_segmented_sort(gpu, largest):
    torch = _torch()
    L = LDS[4]
    lens = [5, 0, 1, 33, 700, 3000, L + 50, 12, 256, 9000]
    off = _offsets(lens, front=1)
    n, k = int(off[-1]) + 3, 40
    keys = _dev(_bits(n, 71) >> np.uint16(4)).view(torch.float16)
    do = _dev(off.astype(np.uint32))
    hk, hi, counts = gpu.segmented_topk16(keys, do, k, largest=largest)
    sk = gpu.segmented_sort(keys, do, descending=largest)
    si = gpu.segmented_argsort(keys, do, descending=largest)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [min(k, x) for x in lens]
    for s, length in enumerate(lens):
        m, a = min(k, length), int(off[s])
        assert torch.equal(hk[s, :m].view(torch.int16), sk[a:a + m].view(torch.int16)) and torch.equal(hi[s, :m], si[a:a + m].to(torch.int32)), s
        assert (hk[s, m:].view(torch.int16) == 0).all() and (hi[s, m:] == -1).all()


# ---- the promise ----------------------------------------------------------------------------------------------------------------------
def test_a_large_k_needs_the_promise(gpu):
    L = LDS[4]
    lens = [L, 3, 6000, 0, L - 1, 200, 5001]
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5 + 1, 81), off, "v4", tail=6)
    h = _handle(gpu, case.n, case.segs, 5000, "v4")
    rep = case.run(h, 5000, max_len=L)
    case.check_classes(rep, L)
    assert not rep["forms"] & gpu._lib.GS_SEGTOPK_F_STREAM
    # one segment of L + 1: GS_ERR_SIZE at check, that row untouched, every other row right
    off2 = off.copy()
    off2[1:] += 1
    broken = _Case(gpu, case.bits, off2, "v4", tail=5)
    rep = broken.run(h, 5000, max_len=L, status=ERR_SIZE, untouched=(0,))
    broken.check_classes(rep, L)
    assert rep["status"] == 2
    # no promise: refused before any launch, the outputs untouched
    ok, ov = case.outputs(5000)
    for max_len in (0, L + 1):
        with pytest.raises(gpu.GpuSortError) as e:
            h.select(case.dk, case.do, 5000, ok, case.dv, ov, n=case.n, max_segment_len=max_len)
        assert e.value.status == ERR_SIZE
    _torch().cuda.synchronize()
    assert (ok.cpu().numpy().view(np.uint16) == FILL).all() and (ov.cpu().numpy().view(np.uint32) == FILL_V).all()
    case.run(h, 4096)  # the stream route's largest k needs none
    h.close()


# ---- bad offsets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["decreasing", "beyond_n"])
def test_bad_offsets_write_nothing(gpu, what):
    L = LDS[0]
    lens = [10, 300, 2000, L + 9, 1, 40]
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 91), off, "keys")
    h = _handle(gpu, case.n, case.segs, 64, "keys")
    bad = off.copy()
    if what == "decreasing":
        bad[3] = bad[2] - 1
    else:
        bad[-1] = case.n + 1
    case.do.copy_(_dev(bad.astype(np.uint32)))
    ok, _ = case.outputs(9)
    h.select(case.dk, case.do, 9, ok, n=case.n)
    assert h.status() == ERR_ARG and h.last()["status"] & 1
    assert (ok.cpu().numpy().view(np.uint16) == FILL).all()
    case.do.copy_(_dev(off.astype(np.uint32)))
    case.run(h, 9)  # the handle works on the next call
    h.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------
def _hip():
    """The HIP runtime this process already runs on (the one torch loaded), for the graph calls torch does not bind."""
    path = next((line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line), None)
    assert path, "no HIP runtime is loaded"
    return C.CDLL(path)


def test_one_capture_replayed_on_new_keys_and_new_offsets(gpu):
    """max_segment_len = 0 and long segments present: one call captured on one stream — every node a kernel launch, no more nodes
    than the 32-bit call has — and replayed on new keys and on new offsets (same n and number of segments, other lengths and classes)
    written into the same buffers."""
    torch = _torch()
    hip = _hip()
    L = LDS[4]
    lens = [L + 300, 5, 0, 700, 40, 2 * L + 1, 1, 3000, 256]
    other = [9, L + 5, 2 * L + 296, 0, 2, 700, 3000, 290, 1]
    assert sum(lens) == sum(other)
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 400), off, "pos", key_type=BF16, descending=True)
    h = _handle(gpu, case.n, case.segs, 64, "pos", BF16, descending=True)
    k = 47
    ok, ov = case.outputs(k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.select(case.dk, case.do, k, ok, None, ov, n=case.n)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.select(case.dk, case.do, k, ok, None, ov, n=case.n)
    for seed, off_lens in ((401, lens), (402, other), (403, lens)):
        case.offsets = _offsets(off_lens, front=1)
        case.bits = _bits(case.n, seed)
        case.dk.copy_(_dev(case.bits))
        case.do.copy_(_dev(case.offsets.astype(np.uint32)))
        ok.fill_(FILL)
        ov.fill_(FILL_V)
        graph.replay()
        torch.cuda.synchronize()
        assert h.status() == OK
        case.compare(k, ok, ov)
        case.check_classes(h.last())
    # the nodes of one call, counted on a capture of our own on the same stream
    with torch.cuda.stream(side):
        side.synchronize()
        stream, g = C.c_void_p(side.cuda_stream), C.c_void_p()
        assert hip.hipStreamBeginCapture(stream, 2) == 0          # hipStreamCaptureModeRelaxed
        try:
            h.select(case.dk, case.do, k, ok, None, ov, n=case.n)
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(g)) == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(count)) == 0
    nodes = (C.c_void_p * count.value)()
    assert hip.hipGraphGetNodes(g, nodes, C.byref(count)) == 0
    kinds = []
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
        kinds.append(kind.value)
    assert hip.hipGraphDestroy(g) == 0
    # reset, classify, fill, packed, wave, the tile classes that hold 4-byte values, stream: at most the 32-bit call's 11
    assert 0 < len(kinds) <= 11 and all(x == 0 for x in kinds), kinds    # hipGraphNodeTypeKernel = 0
    case.run(h, k)  # nothing ran during the capture; the handle is as usable as before
    h.close()


# ---- handle reuse, error returns, the functional layer -----------------------------------------------------------------------------
def test_handle_reuse_across_shapes_k_orders_and_classes(gpu):
    L = LDS[8]
    h = _handle(gpu, 1 << 17, 64, 512, "v8", F16)
    for i, (lens, k, desc) in enumerate([([5, 0, 31], 3, False), ([L + 9, 40], 512, True), ([300, 300, 2048, 1], 77, False),
                                         ([L, L + 1, 7], 1, True), ([1] * 64, 2, False), ([33], 33, True)]):
        case = _Case(gpu, _bits(sum(lens) + 8, 500 + i) >> np.uint16(5), _offsets(lens, front=i % 4), "v8", F16, descending=desc)
        h.order = gpu.ORDER_DESCENDING if desc else gpu.ORDER_ASCENDING
        case.check_classes(case.run(h, k))
    h.close()


def test_error_returns(gpu):
    torch = _torch()
    lib = gpu._lib.load()
    A, S, M = gpu._lib.GS_ERR_ARG, gpu._lib.GS_ERR_SIZE, gpu._lib.GS_ERR_MODE
    n, segs, k = 4096, 8, 16
    keys = torch.zeros(n + 1024, dtype=torch.int16, device="cuda")  # (one call below puts the output right behind the n keys)
    vals = torch.zeros(n + 1024, dtype=torch.int32, device="cuda")
    off = _dev((np.arange(segs + 1) * 512).astype(np.uint32))
    ok = torch.zeros(segs * k + 64, dtype=torch.int16, device="cuda")
    ov = torch.zeros(segs * k + 64, dtype=torch.int32, device="cuda")
    K, V, O, OK_, OV = keys.data_ptr(), vals.data_ptr(), off.data_ptr(), ok.data_ptr(), ov.data_ptr()
    hk, hp, hp8 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.gs_segtopk16_create(C.byref(hk), n, segs, k, 0, 0) == 0 and lib.gs_segtopk16_create(C.byref(hp), n, segs, k, 1, 4) == 0
    assert lib.gs_segtopk16_create(C.byref(hp8), n, segs, k, 1, 8) == 0

    def keys_call(h=hk, d_keys=K, n_=n, d_off=O, segs_=segs, k_=k, max_len=0, d_out=OK_, kt=U16, order=0):
        return lib.gs_segtopk16_select_keys(h, d_keys, n_, d_off, segs_, k_, max_len, d_out, kt, order, None)

    def pairs_call(h=hp, d_keys=K, d_vals=V, n_=n, d_off=O, segs_=segs, k_=k, max_len=0, d_out=OK_, d_outv=OV, kt=U16, order=0):
        return lib.gs_segtopk16_select_pairs(h, d_keys, d_vals, n_, d_off, segs_, k_, max_len, d_out, d_outv, kt, order, None)

    assert keys_call() == 0 and pairs_call() == 0 and pairs_call(d_vals=None) == 0
    assert all(keys_call(kt=t) == 0 and pairs_call(kt=t) == 0 for t in (U16, I16, F16, BF16))
    assert keys_call(h=None) == A and pairs_call(h=None) == A
    assert keys_call(d_keys=None) == A and keys_call(d_off=None) == A and keys_call(d_out=None) == A
    assert keys_call(d_keys=K + 2) == A and keys_call(d_keys=K + 8) == A and keys_call(d_out=OK_ + 8) == A and keys_call(d_off=O + 2) == A
    assert all(keys_call(kt=t) == A and pairs_call(kt=t) == A for t in (0, 1, 2, 3, 4, 5, 10, 99)) and keys_call(order=2) == A
    assert keys_call(d_out=K + 16) == A and keys_call(d_out=K + 2 * n - 16) == A  # the output overlaps the keys
    assert keys_call(d_out=K + 2 * n) == 0                                        # right behind the n 2-byte keys: no overlap
    assert keys_call(d_out=O) == A                                                # the output overlaps the offsets
    assert pairs_call(d_outv=None) == A and pairs_call(d_outv=OV + 4) == A and pairs_call(d_vals=V + 4) == A
    assert pairs_call(d_outv=V + 32) == A and pairs_call(d_outv=OK_ + 16) == A and pairs_call(d_outv=K + 32) == A and pairs_call(d_outv=O) == A
    assert pairs_call(d_out=V + 32) == A
    assert pairs_call(h=hp8, d_vals=None) == A  # positions are 4-byte values
    assert keys_call(h=hp) == M and pairs_call(h=hk) == M
    assert keys_call(n_=0) == S and keys_call(n_=n + 1) == S and keys_call(segs_=0) == S and keys_call(segs_=segs + 1) == S
    assert keys_call(k_=0) == S and keys_call(k_=k + 1) == S
    torch.cuda.synchronize()
    rep = (C.c_uint32 * 16)()
    assert lib.gs_segtopk16_last(hk, None, 16, None) == A and lib.gs_segtopk16_last(hk, rep, 15, None) == A and lib.gs_segtopk16_last(hk, rep, 16, None) == 0
    assert lib.gs_segtopk16_set_rank_mode(hk, 2) == A and lib.gs_segtopk16_set_rank_mode(hk, 0) == 0 and lib.gs_segtopk16_get_rank_mode(hk) == 0
    for h in (hk, hp, hp8):
        assert lib.gs_segtopk16_check(h, None) == 0 and lib.gs_segtopk16_destroy(h) == 0
    # the class refuses 32-bit key types, and a fresh handle answers check before any call
    with pytest.raises(ValueError):
        gpu.SegmentedTopK16(64, 2, 2, key_type=0)
    h = gpu.SegmentedTopK16(64, 2, 2)
    assert h.status() == OK and h.temp_bytes == 512 and h.max_lds_segment == LDS[0] and h.class_of(257) == 3
    with pytest.raises(ValueError):
        h.select(torch.zeros(64, dtype=torch.int32, device="cuda"), off, 2, torch.zeros(64, dtype=torch.int32, device="cuda"))
    h.close()


def test_functional_segmented_topk16(gpu):
    torch = _torch()
    from gpusorting_amd import functional
    from gpusorting_amd.segtopk import segmented_topk_reference
    functional._segtopk_cache.clear()
    L = LDS[4]
    lens = [4, 0, 50, 1, 600, L + 10, 33]
    off = _offsets(lens, front=1)
    n = int(off[-1]) + 2
    do = _dev(off.astype(np.uint32))
    bits = special_keys(np.random.default_rng(600), n, 0.3)
    cases = [(torch.int16, I16, False), (torch.int16, U16, True), (torch.float16, F16, False), (torch.bfloat16, BF16, False)]
    if hasattr(torch, "uint16"):
        cases.append((torch.uint16, U16, False))
    for dtype, kt, unsigned in cases:
        keys = _dev(bits).view(dtype)
        for largest in (True, False):
            hk, hi, counts = functional.segmented_topk16(keys, do, 9, largest=largest, unsigned=unsigned)
            rk, rv, rc = segmented_topk_reference(bits, off, 9, None, largest, kt, fill_key=0, fill_value=0xFFFFFFFF)
            assert hk.dtype == dtype and hi.dtype == torch.int32 and counts.dtype == torch.int32 and hk.shape == hi.shape == (len(lens), 9)
            np.testing.assert_array_equal(hk.cpu().view(torch.int16).numpy().view(np.uint16), rk)
            np.testing.assert_array_equal(hi.cpu().numpy().view(np.uint32), rv)
            np.testing.assert_array_equal(counts.cpu().numpy(), rc)
    keys = _dev(bits)
    for vdtype, vals in ((torch.int32, _values(n, "v4")), (torch.int64, _values(n, "v8"))):
        hk, hv, counts = functional.segmented_topk16(keys, do, 5, largest=False, values=_dev(vals), unsigned=True)
        rk, rv, rc = segmented_topk_reference(bits, off, 5, vals, False, U16)
        assert hv.dtype == vdtype
        np.testing.assert_array_equal(hk.cpu().numpy().view(np.uint16), rk)
        np.testing.assert_array_equal(hv.cpu().numpy().view(vals.dtype), rv)
    # the cached handle is a SegmentedTopK16, re-created when n, the segments or k outgrow it
    key = next(k for k in functional._segtopk_cache if k[2] == U16 and k[3] == gpu.ORDER_ASCENDING and k[4] == 4)
    first = functional._segtopk_cache[key]
    assert isinstance(first, gpu.SegmentedTopK16) and (first.max_keys, first.max_segments, first.max_k) == (1 << 16, 1 << 16, 64)
    functional.segmented_topk16(keys, do, 64, largest=False, values=_dev(_values(n, "v4")), unsigned=True)
    assert functional._segtopk_cache[key] is first
    functional.segmented_topk16(keys, do, 65, largest=False, values=_dev(_values(n, "v4")), unsigned=True)
    second = functional._segtopk_cache[key]
    assert second is not first and second.max_k == 128 and first._h is None
    big_n = (1 << 16) + 1
    big_bits = _bits(big_n, 601)
    big = _dev(big_bits)
    big_off = _dev(np.array([0, 10, big_n], dtype=np.uint32))
    hk, _, counts = functional.segmented_topk16(big, big_off, 3, largest=False, values=torch.zeros(big_n, dtype=torch.int32, device="cuda"), unsigned=True)
    third = functional._segtopk_cache[key]
    assert third is not second and third.max_keys == 1 << 17 and counts.cpu().tolist() == [3, 3]
    many = (1 << 16) + 1
    many_off = torch.arange(many + 1, dtype=torch.int32, device="cuda").clamp(max=big_n)
    hk, _, counts = functional.segmented_topk16(big, many_off, 2, largest=False, values=torch.zeros(big_n, dtype=torch.int32, device="cuda"), unsigned=True)
    fourth = functional._segtopk_cache[key]
    assert fourth is not third and fourth.max_segments == 1 << 17 and int(counts.sum()) == big_n
    np.testing.assert_array_equal(hk[:, 0].cpu().numpy().view(np.uint16)[:big_n], big_bits)
    # argument errors follow segmented_topk
    with pytest.raises(ValueError):
        functional.segmented_topk16(keys, do, 0)
    with pytest.raises(ValueError):
        functional.segmented_topk16(keys, do, 5000)  # above rows_max_k without a promise that fits LDS
    assert functional.segmented_topk16(keys, do, 5000, max_segment_len=L)[0].shape == (len(lens), 5000)  # (a broken promise: check's business)
    with pytest.raises(TypeError, match="segmented_topk"):
        functional.segmented_topk16(keys.to(torch.int32), do, 2)
    with pytest.raises(TypeError, match="segmented_topk16"):
        functional.segmented_topk(keys, do, 2)
    with pytest.raises(ValueError):
        functional.segmented_topk16(keys, do.to(torch.int64), 2)
    torch.cuda.synchronize()
    functional._segtopk_cache.clear()
