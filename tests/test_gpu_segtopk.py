"""The segmented top-k (gs_segtopk_*, gpusorting_amd/csrc/topk_seg_kernels.hpp) on the GPU: every case compares keys AND values bit
for bit with gpusorting_amd.segmented_topk_reference (tests/test_segtopk_cpu.py), on outputs pre-filled with a pattern so that the
slots the call must not write are compared too, calls check(), and asks last() which kernels ran.  Every input is seeded.  No
counterpart in the reference project."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32, I32, F32 = 0, 1, 2
VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
LDS = {0: 32768, 4: 16384, 8: 8192}  # seg_max_lds: segments up to here are selected in LDS
CLASS_MAX = (1, 32, 256, 1024, 2048, 8192, 16384, 32768)
MODES = ("keys", "pos", "v4", "v8")
FILL, FILL_V = 0x5EEDBEEF, 0x0BADF00D
PAD = 37  # output elements behind num_segments * k that must keep the fill
OK, ERR_ARG, ERR_SIZE = 0, 1, 2


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).cuda()


def _vb(mode):
    return {"keys": 0, "v4": 4, "v8": 8, "pos": 4}[mode]


def _vi(mode):
    return MODES.index(mode)


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)


def _values(n, mode):
    """Values that differ from the position, so that a position written for a value shows."""
    if mode == "v4":
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    if mode == "v8":
        return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x1F)
    return None


def _offsets(lens, front=3):
    return np.concatenate([[front], front + np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def _handle(gpu, n, segs, k, mode, key_type=U32, descending=False):
    vb = _vb(mode)
    return gpu.SegmentedTopK(n, segs, k, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type,
                             gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


def _class_of(length, vb):
    if length > LDS[vb]:
        return 8
    return next(c for c, m in enumerate(CLASS_MAX) if length <= m) if length > 1 else 0


class _Case:
    """One array and its offsets on the device; run(h, k): a call into fresh, pre-filled outputs, compared with the reference."""

    def __init__(self, gpu, bits, offsets, mode, key_type=U32, descending=False, tail=5):
        self.gpu, self.mode, self.kt, self.desc = gpu, mode, key_type, descending
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.segs = self.offsets.size - 1
        self.n = int(self.offsets[-1]) + tail  # off[S] < n
        assert bits.size >= self.n
        self.bits = np.ascontiguousarray(bits[:self.n]).view(np.uint32)
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
        ok = torch.full((self.segs * k + PAD,), FILL, dtype=torch.int32, device="cuda")
        vb = _vb(self.mode)
        ov = None if not vb else torch.full((self.segs * k + PAD,), FILL_V, dtype=torch.int64 if vb == 8 else torch.int32, device="cuda")
        return ok, ov

    def compare(self, k, ok, ov, untouched=()):
        rk, rv, _ = self.expected(k, untouched)
        got = ok.cpu().numpy().view(np.uint32)
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
        np.testing.assert_array_equal(self.dk.cpu().numpy().view(np.uint32), self.bits)
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
        # length 1 is the sort's class 0, and the packed kernel's work here
        assert rep["packed"] == int(np.count_nonzero((lens >= 1) & (lens <= 32) & ((lens <= max_len) | (max_len == 0))))


# ---- class borders in one call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_class_borders_in_one_call(gpu, mode):
    L = LDS[_vb(mode)]
    lens = sorted({0, 1, 2, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 8192, 8193, 16384, 16385, L - 1, L, L + 1, L + 4099})
    rng = np.random.default_rng(7)
    rng.shuffle(lens)
    mixed = []
    for length in lens:  # empty segments between them; the odd lengths give odd starts
        mixed += [int(length), 0]
    off = _offsets(mixed, front=3)
    assert off[0] > 0 and len({int(o) % 4 for o in off}) == 4
    case = _Case(gpu, _bits(int(off[-1]) + 5, 11), off, mode)
    h = _handle(gpu, case.n, case.segs, 300, mode)
    for k in (1, 8, 33, 300):
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


# ---- k against the length ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pos", "v8"])
def test_k_against_the_length(gpu, mode):
    """Segments of length k - 1, k and k + 1 in the packed, wave and tile classes; k = 1 and k = the length are among them."""
    ks = (1, 2, 20, 32, 33, 100, 256, 257, 700, 1024, 1025, 3000)
    lens = sorted({x for k in ks for x in (k - 1, k, k + 1)} | {1})
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 21) >> np.uint32(22), off, mode)  # 1024 distinct keys: ties in every longer segment
    h = _handle(gpu, case.n, case.segs, max(ks), mode)
    for desc in (False, True):
        case.desc = desc
        h.order = gpu.ORDER_DESCENDING if desc else gpu.ORDER_ASCENDING
        for k in ks:
            case.run(h, k)
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
    """Two segments of the class's minimum length + 1 and one of its maximum, on the cell's kernel: the forms word shows it ran."""
    lens = [CLASS_MAX[c - 1] + 2, CLASS_MAX[c], CLASS_MAX[c - 1] + 2]
    off = _offsets(lens, front=1)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 100 + c), off, mode, descending=bool(rank))
    h = _handle(gpu, case.n, case.segs, 64, mode, descending=bool(rank))
    h.set_rank_mode(rank)
    assert h.rank_mode == rank
    rep = case.run(h, 19, max_len=CLASS_MAX[c])
    assert rep["counts"][c] == 3 and rep["rank"] == rank
    assert rep["forms"] & gpu._lib.GS_SEGTOPK_F_TILE(c, rank) and not rep["forms"] & gpu._lib.GS_SEGTOPK_F_TILE(c, 1 - rank)
    assert rep["forms"] >> 16 == 1 << _vi(mode) and not rep["forms"] & gpu._lib.GS_SEGTOPK_F_STREAM
    h.close()


@pytest.mark.parametrize("mode", MODES)
def test_packed_wave_and_stream_cells(gpu, mode):
    L = LDS[_vb(mode)]
    for form, lens in (("PACKED", [1, 5, 0, 32, 2]), ("WAVE", [34, 256, 34, 100]), ("STREAM", [L + 1, L + 2, 2 * L + 5])):
        off = _offsets(lens, front=2)
        case = _Case(gpu, _bits(int(off[-1]) + 5, 200 + len(form)), off, mode)
        h = _handle(gpu, case.n, case.segs, 16, mode)
        rep = case.run(h, 7)
        case.check_classes(rep)
        assert rep["forms"] & getattr(gpu._lib, "GS_SEGTOPK_F_" + form) and rep["forms"] >> 16 == 1 << _vi(mode)
        assert (rep["reads"] >= 2) == (form == "STREAM")
        h.close()


# ---- types and orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", [U32, I32, F32])
@pytest.mark.parametrize("descending", [False, True])
def test_types_and_orders(gpu, key_type, descending):
    L = LDS[4]
    lens = [7, 0, 40, 300, 1, 2500, L + 300, 20, 200, 64, 64, 9000]
    off = _offsets(lens, front=1)
    n = int(off[-1]) + 5
    rng = np.random.default_rng(31 + key_type)
    if key_type == F32:
        f = rng.standard_normal(n).astype(np.float32)
        pool = np.array([0.0, -0.0, np.inf, -np.inf], dtype=np.float32).view(np.uint32)
        nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)
        bits = f.view(np.uint32).copy()
        sel = rng.random(n) < 0.3
        bits[sel] = np.concatenate([pool, nans])[rng.integers(0, 8, int(sel.sum()))]
        bits[off[8]:off[9]] = pool[rng.integers(0, 2, 200)]   # a segment of zeros of both signs
        bits[off[9]:off[10]] = pool[rng.integers(2, 4, 64)]   # of infinities
        bits[off[10]:off[11]] = nans[rng.integers(0, 4, 64)]  # of NaNs
    else:
        bits = _bits(n, 31 + key_type)
        bits[::3] &= np.uint32(0x8000000F)  # ties, of both signs
    case = _Case(gpu, bits, off, "pos", key_type, descending)
    h = _handle(gpu, case.n, case.segs, 128, "pos", key_type, descending)
    for k in (3, 100):
        rep = case.run(h, k)
        assert rep["counts"][8] == 1
    case.inputs_unchanged()
    h.close()


# ---- stream route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_stream_alignments_lengths_and_equal_segment(gpu, descending):
    """Long segments that start at each of the four alignments off[s] % 4; length L + 1 and lengths that are no multiple of the
    4096-element chunk; an all-equal long segment beside random ones; k up to 4096."""
    for mode in ("pos", "keys"):
        L = LDS[_vb(mode)]
        lens, at = [], 4
        for long_len, start in ((L + 1, 0), (L + 4099, 1), (L + 7, 2), (2 * L + 1, 3), (L + 1, 1)):
            lens += [(start - at) % 4, long_len]  # a short (or empty) segment in front brings the long one to its alignment
            at += lens[-2] + long_len
        off = _offsets(lens, front=4)
        assert [int(off[s]) % 4 for s, length in enumerate(lens) if length > L] == [0, 1, 2, 3, 1]
        bits = _bits(int(off[-1]) + 5, 41)
        bits[off[5]:off[6]] = 0x12345678  # every key of the third long segment equal: four reads, the position rank decides
        case = _Case(gpu, bits, off, mode, descending=descending)
        h = _handle(gpu, case.n, case.segs, 4096, mode, descending=descending)
        for k in (1, 777, 4096):
            rep = case.run(h, k)
            assert rep["counts"][8] == 5 and rep["reads"] == 4
        case.inputs_unchanged()
        h.close()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shared_bits,reads", [(16, 3), (24, 4)])
def test_stream_keys_share_their_top_bits(gpu, descending, shared_bits, reads):
    """All keys share their top 16 bits: the second level is needed (three reads); their top 24: the third, exact level (four)."""
    L = LDS[4]
    lens = [2 * L, 3, 2 * L + 1, 2 * L + 2]
    off = _offsets(lens, front=1)
    low = _bits(int(off[-1]) + 5, 77) & np.uint32((1 << (32 - shared_bits)) - 1)
    case = _Case(gpu, low | np.uint32(0xABCDEF00 & ~((1 << (32 - shared_bits)) - 1)), off, "pos", descending=descending)
    h = _handle(gpu, case.n, case.segs, 1000, "pos", descending=descending)
    for k in (1, 64, 1000):
        assert case.run(h, k)["reads"] == reads
    h.close()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("copies", ["few", "many"])
def test_stream_threshold_repeated_across_chunk_borders(gpu, descending, copies):
    """The threshold value T sits on both sides of every border of a 4096-element load chunk, in segments at every alignment; k takes
    only a part of its copies.  "few": all copies are staged and the LDS sort decides; "many": more than the staging holds."""
    L = LDS[4]
    seg_len = 3 * L
    lens = [seg_len, 1, seg_len, 2, seg_len]
    off = _offsets(lens, front=1)
    T = np.uint32(0x40000000)
    bits = (_bits(int(off[-1]) + 5, 55) >> np.uint32(2)) | np.uint32(0x80000000)  # behind T (ascending)
    pos = np.arange(seg_len)
    at_border = (pos % 4096 < 5) | (pos % 4096 >= 4091)
    mark = at_border if copies == "few" else (at_border | (pos % 3 == 0))
    for s in (0, 2, 4):
        seg = bits[off[s]:off[s + 1]]
        seg[mark] = T
        seg[100::5000] = np.uint32(7)  # in front of T
    if descending:
        bits = ~bits
    count, front = int(np.count_nonzero(mark & (pos % 5000 != 100))), len(range(100, seg_len, 5000))
    assert (count < 4096 - front) == (copies == "few")
    case = _Case(gpu, bits, off, "pos", descending=descending)
    h = _handle(gpu, case.n, case.segs, 4096, "pos", descending=descending)
    for k in (front + 1, front + min(count, 4000) // 2):
        case.run(h, k)
    h.close()


# ---- parity with what exists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,row_len", [(64, 200), (8, 3001), (3, LDS[4] + 77)])
@pytest.mark.parametrize("descending", [False, True])
def test_uniform_offsets_equal_the_row_wise_top_k(gpu, rows, row_len, descending):
    torch = _torch()
    k = 50
    bits = _bits(rows * row_len, 61) >> np.uint32(20)  # ties
    dk = _dev(bits)
    do = _dev((np.arange(rows + 1, dtype=np.int64) * row_len).astype(np.uint32))
    order = gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING
    seg = gpu.SegmentedTopK(bits.size, rows, k, order, U32, gpu.MODE_PAIRS, 4)
    row = gpu.TopK(bits.size, k, order, U32, gpu.MODE_PAIRS, 4)
    sk, sv = torch.zeros(rows * k, dtype=torch.int32, device="cuda"), torch.zeros(rows * k, dtype=torch.int32, device="cuda")
    rk, rv = torch.ones(rows * k, dtype=torch.int32, device="cuda"), torch.ones(rows * k, dtype=torch.int32, device="cuda")
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
def test_ragged_mix_equals_the_heads_of_the_segmented_sort(gpu, largest):
    torch = _torch()
    L = LDS[4]
    lens = [5, 0, 1, 33, 700, 3000, L + 50, 12, 256, 9000]
    off = _offsets(lens, front=2)
    n, k = int(off[-1]) + 3, 40
    keys = _dev(_bits(n, 71) >> np.uint32(18))
    do = _dev(off.astype(np.uint32))
    hk, hi, counts = gpu.segmented_topk(keys, do, k, largest=largest)
    sk = gpu.segmented_sort(keys, do, descending=largest)
    si = gpu.segmented_argsort(keys, do, descending=largest)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [min(k, x) for x in lens]
    for s, length in enumerate(lens):
        m, a = min(k, length), int(off[s])
        assert torch.equal(hk[s, :m], sk[a:a + m]) and torch.equal(hi[s, :m], si[a:a + m]), s
        assert (hk[s, m:] == 0).all() and (hi[s, m:] == -1).all()


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
    assert (ok.cpu().numpy().view(np.uint32) == FILL).all() and (ov.cpu().numpy().view(np.uint32) == FILL_V).all()
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
    assert (ok.cpu().numpy().view(np.uint32) == FILL).all()
    case.do.copy_(_dev(off.astype(np.uint32)))
    case.run(h, 9)  # the handle works on the next call
    h.close()


# ---- memory contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,lens,k", [("PACKED", [1, 0, 32, 7, 19, 2], 9), ("WAVE", [33, 256, 100, 0, 255], 40),
                                         ("TILE", [257, 3001, 1024, 0, 2049], 65), ("STREAM", [LDS[4] + 4099, 1, LDS[4] + 1], 130)])
@pytest.mark.parametrize("mode", ["pos", "v4"])
def test_memory_contract_on_a_guard_arena(gpu, form, lens, k, mode):
    """16-byte-only aligned inputs and outputs inside one arena, guard bands around both outputs, n below the buffers' length: nothing
    outside [0, S * k) of the outputs is written, and nothing in the inputs."""
    from guard_arena import Arena
    from gpusorting_amd.segtopk import segmented_topk_reference
    off = _offsets(lens, front=3)
    n, segs = int(off[-1]) + 2, len(lens)
    room = n + 100
    bits = _bits(room, 300 + k)
    vals = _values(room, mode)
    arena = Arena.for_views([(room, np.uint32), (room, np.uint32), (segs + 1, np.uint32), (segs * k + 50, np.uint32), (segs * k + 50, np.uint32)], "cuda", "hash")
    dk = arena.carve(room, np.uint32, 1, "keys")
    dv = arena.carve(room, np.uint32, 3, "values")
    do = arena.carve(segs + 1, np.uint32, 5, "offsets")
    ok = arena.carve(segs * k + 50, np.uint32, 7, "out_keys")
    ov = arena.carve(segs * k + 50, np.uint32, 9, "out_values")
    arena.write(dk, bits)
    if vals is not None:
        arena.write(dv, vals)
    arena.write(do, off.astype(np.uint32))
    arena.write(ok, np.full(segs * k, FILL, dtype=np.uint32))
    arena.write(ov, np.full(segs * k, FILL_V, dtype=np.uint32))
    arena.live(ok, segs * k)
    arena.live(ov, segs * k)
    h = _handle(gpu, room, segs, k, mode)
    h.select(dk, do, k, ok, dv if vals is not None else None, ov, n=n)
    h.check()
    rep = h.last()
    assert rep["forms"] & (gpu._lib.GS_SEGTOPK_F_TILE(3, rep["rank"]) if form == "TILE" else getattr(gpu._lib, "GS_SEGTOPK_F_" + form))
    arena.verify()
    rk, rv, _ = segmented_topk_reference(bits[:n], off, k, None if vals is None else vals[:n], fill_key=FILL, fill_value=FILL_V)
    np.testing.assert_array_equal(arena.read(ok, np.uint32, segs * k), rk.reshape(-1))
    np.testing.assert_array_equal(arena.read(ov, np.uint32, segs * k), rv.reshape(-1))
    h.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------
def _hip():
    """The HIP runtime this process already runs on (the one torch loaded), for the graph calls torch does not bind."""
    path = next((line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line), None)
    assert path, "no HIP runtime is loaded"
    return C.CDLL(path)


def test_graph_capture_replayed_on_new_keys_and_new_offsets(gpu):
    """max_segment_len = 0 and long segments present: one call captured on a side stream, replayed on new keys and on new offsets
    (same n and number of segments, other lengths and classes) written into the same buffers."""
    torch = _torch()
    L = LDS[4]
    lens = [L + 300, 5, 0, 700, 40, 2 * L + 1, 1, 3000, 256]
    other = [9, L + 5, 2 * L + 296, 0, 2, 700, 3000, 290, 1]
    assert sum(lens) == sum(other)
    off = _offsets(lens, front=2)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 400), off, "pos", descending=True)
    h = _handle(gpu, case.n, case.segs, 64, "pos", descending=True)
    k = 48
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
        case.offsets = _offsets(off_lens, front=2)
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
    h.close()


def test_every_captured_node_is_a_kernel_launch(gpu):
    torch = _torch()
    hip = _hip()
    L = LDS[0]
    lens = [L + 300, 5, 0, 700, 40, 2 * L + 1, 1, 3000, 256, 20000]
    off = _offsets(lens, front=2)
    case = _Case(gpu, _bits(int(off[-1]) + 5, 410), off, "keys")
    h = _handle(gpu, case.n, case.segs, 64, "keys")
    ok, _ = case.outputs(16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.select(case.dk, case.do, 16, ok, n=case.n)
        side.synchronize()
        stream, graph = C.c_void_p(side.cuda_stream), C.c_void_p()
        assert hip.hipStreamBeginCapture(stream, 2) == 0          # hipStreamCaptureModeRelaxed
        try:
            h.select(case.dk, case.do, 16, ok, n=case.n)
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0
    nodes = (C.c_void_p * count.value)()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(count)) == 0
    kinds = []
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
        kinds.append(kind.value)
    assert hip.hipGraphDestroy(graph) == 0
    # reset, classify, fill, packed, wave, five tile classes, stream
    assert len(kinds) == 11 and all(x == 0 for x in kinds), kinds    # hipGraphNodeTypeKernel = 0
    case.run(h, 16)  # nothing ran during the capture; the handle is as usable as before
    h.close()


# ---- handle reuse, error returns, the functional layer -----------------------------------------------------------------------------
def test_handle_reuse_across_shapes_k_orders_and_classes(gpu):
    L = LDS[8]
    h = _handle(gpu, 1 << 17, 64, 512, "v8")
    for i, (lens, k, desc) in enumerate([([5, 0, 31], 3, False), ([L + 9, 40], 512, True), ([300, 300, 2048, 1], 77, False),
                                         ([L, L + 1, 7], 1, True), ([1] * 64, 2, False), ([33], 33, True)]):
        case = _Case(gpu, _bits(sum(lens) + 8, 500 + i) >> np.uint32(16), _offsets(lens, front=i % 4), "v8", descending=desc)
        h.order = gpu.ORDER_DESCENDING if desc else gpu.ORDER_ASCENDING
        case.check_classes(case.run(h, k))
    h.close()


def test_error_returns(gpu):
    torch = _torch()
    lib = gpu._lib.load()
    A, S, M = gpu._lib.GS_ERR_ARG, gpu._lib.GS_ERR_SIZE, gpu._lib.GS_ERR_MODE
    n, segs, k = 4096, 8, 16
    keys = torch.zeros(n + 1024, dtype=torch.int32, device="cuda")  # (one call below puts the output right behind the n keys)
    vals = torch.zeros(n + 1024, dtype=torch.int32, device="cuda")
    off = _dev((np.arange(segs + 1) * 512).astype(np.uint32))
    ok = torch.zeros(segs * k + 64, dtype=torch.int32, device="cuda")
    ov = torch.zeros(segs * k + 64, dtype=torch.int32, device="cuda")
    K, V, O, OK_, OV = keys.data_ptr(), vals.data_ptr(), off.data_ptr(), ok.data_ptr(), ov.data_ptr()
    hk, hp, hp8 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.gs_segtopk_create(C.byref(hk), n, segs, k, 0, 0) == 0 and lib.gs_segtopk_create(C.byref(hp), n, segs, k, 1, 4) == 0
    assert lib.gs_segtopk_create(C.byref(hp8), n, segs, k, 1, 8) == 0

    def keys_call(h=hk, d_keys=K, n_=n, d_off=O, segs_=segs, k_=k, max_len=0, d_out=OK_, kt=U32, order=0):
        return lib.gs_segtopk_select_keys(h, d_keys, n_, d_off, segs_, k_, max_len, d_out, kt, order, None)

    def pairs_call(h=hp, d_keys=K, d_vals=V, n_=n, d_off=O, segs_=segs, k_=k, max_len=0, d_out=OK_, d_outv=OV, kt=U32, order=0):
        return lib.gs_segtopk_select_pairs(h, d_keys, d_vals, n_, d_off, segs_, k_, max_len, d_out, d_outv, kt, order, None)

    assert keys_call() == 0 and pairs_call() == 0 and pairs_call(d_vals=None) == 0
    assert keys_call(h=None) == A and pairs_call(h=None) == A
    assert keys_call(d_keys=None) == A and keys_call(d_off=None) == A and keys_call(d_out=None) == A
    assert keys_call(d_keys=K + 4) == A and keys_call(d_out=OK_ + 8) == A and keys_call(d_off=O + 2) == A
    assert keys_call(kt=3) == A and keys_call(kt=6) == A and keys_call(kt=9) == A and keys_call(kt=99) == A and keys_call(order=2) == A
    assert keys_call(d_out=K + 16) == A and keys_call(d_out=K + 4 * n - 16) == A  # the output overlaps the keys
    assert keys_call(d_out=K + 4 * n) == 0                                        # right behind them: no overlap
    assert pairs_call(d_outv=None) == A and pairs_call(d_outv=OV + 4) == A and pairs_call(d_vals=V + 4) == A
    assert pairs_call(d_outv=V + 32) == A and pairs_call(d_outv=OK_ + 16) == A
    assert pairs_call(h=hp8, d_vals=None) == A  # positions are 4-byte values
    assert keys_call(h=hp) == M and pairs_call(h=hk) == M
    assert keys_call(n_=0) == S and keys_call(n_=n + 1) == S and keys_call(segs_=0) == S and keys_call(segs_=segs + 1) == S
    assert keys_call(k_=0) == S and keys_call(k_=k + 1) == S
    torch.cuda.synchronize()
    rep = (C.c_uint32 * 16)()
    assert lib.gs_segtopk_last(hk, None, 16, None) == A and lib.gs_segtopk_last(hk, rep, 15, None) == A and lib.gs_segtopk_last(hk, rep, 16, None) == 0
    assert lib.gs_segtopk_set_rank_mode(hk, 2) == A and lib.gs_segtopk_set_rank_mode(hk, 0) == 0 and lib.gs_segtopk_get_rank_mode(hk) == 0
    for h in (hk, hp, hp8):
        assert lib.gs_segtopk_check(h, None) == 0 and lib.gs_segtopk_destroy(h) == 0
    # a fresh handle answers check before any call
    h = gpu.SegmentedTopK(64, 2, 2)
    assert h.status() == OK and h.temp_bytes == 512
    h.close()


def test_functional_segmented_topk(gpu):
    torch = _torch()
    from gpusorting_amd import functional
    from gpusorting_amd.segtopk import segmented_topk_reference
    functional._segtopk_cache.clear()
    L = LDS[4]
    lens = [4, 0, 50, 1, 600, L + 10, 33]
    off = _offsets(lens, front=1)
    n = int(off[-1]) + 2
    do = _dev(off.astype(np.uint32))
    bits = _bits(n, 600)
    bits[::4] &= np.uint32(0x800000FF)
    for dtype, kt, unsigned in ((torch.int32, I32, False), (torch.int32, U32, True), (torch.float32, F32, False)):
        keys = _dev(bits).view(dtype)
        for largest in (True, False):
            hk, hi, counts = functional.segmented_topk(keys, do, 9, largest=largest, unsigned=unsigned)
            rk, rv, rc = segmented_topk_reference(bits, off, 9, None, largest, kt, fill_key=0, fill_value=0xFFFFFFFF)
            assert hk.dtype == dtype and hi.dtype == torch.int32 and counts.dtype == torch.int32 and hk.shape == hi.shape == (len(lens), 9)
            np.testing.assert_array_equal(hk.cpu().view(torch.int32).numpy().view(np.uint32), rk)
            np.testing.assert_array_equal(hi.cpu().numpy().view(np.uint32), rv)
            np.testing.assert_array_equal(counts.cpu().numpy(), rc)
    keys = _dev(bits)
    for vdtype, vals in ((torch.int32, _values(n, "v4")), (torch.int64, _values(n, "v8"))):
        hk, hv, counts = functional.segmented_topk(keys, do, 5, largest=False, values=_dev(vals), unsigned=True)
        rk, rv, rc = segmented_topk_reference(bits, off, 5, vals, False, U32)
        assert hv.dtype == vdtype
        np.testing.assert_array_equal(hk.cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(hv.cpu().numpy().view(vals.dtype), rv)
    # the cached handle is re-created when n, the segments or k outgrow it
    key = next(k for k in functional._segtopk_cache if k[2] == U32 and k[3] == gpu.ORDER_ASCENDING and k[4] == 4)
    first = functional._segtopk_cache[key]
    assert (first.max_keys, first.max_segments, first.max_k) == (1 << 16, 1 << 16, 64)
    functional.segmented_topk(keys, do, 64, largest=False, values=_dev(_values(n, "v4")), unsigned=True)
    assert functional._segtopk_cache[key] is first
    functional.segmented_topk(keys, do, 65, largest=False, values=_dev(_values(n, "v4")), unsigned=True)
    second = functional._segtopk_cache[key]
    assert second is not first and second.max_k == 128 and first._h is None
    big_n = (1 << 16) + 1
    big = _dev(_bits(big_n, 601))
    big_off = _dev(np.array([0, 10, big_n], dtype=np.uint32))
    hk, _, counts = functional.segmented_topk(big, big_off, 3, largest=False, values=torch.zeros(big_n, dtype=torch.int32, device="cuda"), unsigned=True)
    third = functional._segtopk_cache[key]
    assert third is not second and third.max_keys == 1 << 17 and counts.cpu().tolist() == [3, 3]
    many = (1 << 16) + 1
    many_off = torch.arange(many + 1, dtype=torch.int32, device="cuda").clamp(max=big_n)
    hk, _, counts = functional.segmented_topk(big, many_off, 2, largest=False, values=torch.zeros(big_n, dtype=torch.int32, device="cuda"), unsigned=True)
    fourth = functional._segtopk_cache[key]
    assert fourth is not third and fourth.max_segments == 1 << 17 and int(counts.sum()) == big_n
    np.testing.assert_array_equal(hk[:, 0].cpu().numpy().view(np.uint32)[:big_n], _bits(big_n, 601))
    # argument errors follow the other helpers
    with pytest.raises(ValueError):
        functional.segmented_topk(keys, do, 0)
    with pytest.raises(ValueError):
        functional.segmented_topk(keys, do, 5000)  # above rows_max_k without a promise that fits LDS
    with pytest.raises(TypeError):
        functional.segmented_topk(keys.to(torch.int16), do, 2)
    with pytest.raises(ValueError):
        functional.segmented_topk(keys, do.to(torch.int64), 2)
    torch.cuda.synchronize()
    functional._segtopk_cache.clear()
