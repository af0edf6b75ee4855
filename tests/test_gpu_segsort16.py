"""GPU tests of the segmented sort of 16-bit keys (gs_segsort16_* in include/gpusort.h; segsort16_kernels.hpp): many segments of one
array of uint16 / int16 / float16 / bfloat16 keys, each sorted on its own, in place — keys only, as an argsort, with 4- and 8-byte
values — in the LDS classes (packed, wave, workgroup) and on the long route (a work list built on the device, two passes of count, scan,
scatter over all long segments at once).  Everything is compared bit for bit with segmented_sort16_reference, the numpy statement of the
semantics (tests/test_segsort16_cpu.py checks that one on the CPU); the comparison runs over the WHOLE array, so the elements in front of
the first and behind the last offset are guards of every case.  After every call gs_segsort16_check is GS_OK and gs_segsort16_last_classes
matches the classes computed from the lengths.  The last test asserts that the cases of this file reached every kernel form the build
compiles (gs_segsort16_last's form words).  All arrays stay below 2^19 elements."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
KEY_TYPES = (U16, I16, F16, BF16)
KEYS, PAIRS = 0, 1
ENTRIES = ("keys", "argsort", "pairs4", "pairs8")
BORDER_LENGTHS = (0, 1, 2, 32, 33, 256, 257, 1024, 1025, 2048, 2049, 8192, 8193, 16384, 16385, 32768, 32769)
_FORMS_SEEN = [0]   # union of SegmentedSort16.last()["forms"] over the file's cases


def _torch():
    import torch
    return torch


def _mode(entry):
    return (KEYS, 0) if entry == "keys" else (PAIRS, 8 if entry == "pairs8" else 4)


def _lds(entry):
    from gpusorting_amd import _lib
    return int(_lib.load().gs_segsort_max_lds_segment(*_mode(entry)))


def _part():
    from gpusorting_amd import _lib
    return _lib.GS_SEGSORT16_PART


def _tile():
    from gpusorting_amd import _lib
    return _lib.GS_SORT_ROWS_TILE


def _values(n, vb):
    """value = array index (8 bytes: spread over both halves, a high bit on top): equal keys must come out in rising index."""
    idx = np.arange(n, dtype=np.uint32)
    return idx if vb == 4 else idx.astype(np.uint64) * np.uint64(0x100000001) | np.uint64(1 << 63)


def _offsets(lens, front=1):
    return (front + np.concatenate(([0], np.cumsum(np.asarray(lens, dtype=np.int64))))).astype(np.uint32)


def _odd_starts(lens, filler=1):
    """The lengths with a filler segment in front of every one that would start at an even element index (offsets[0] = 1)."""
    out, at = [], 1
    for length in lens:
        if at % 2 == 0:
            out.append(filler)
            at += filler
        out.append(length)
        at += length
    return out


def _handle(gpu, entry, max_keys, max_segments, kt=U16, desc=False, rank=None):
    mode, vb = _mode(entry)
    h = gpu.SegmentedSort16(max_keys, max_segments, order=1 if desc else 0, key_type=kt, mode=mode, value_bytes=vb)
    if rank is not None:
        h.set_rank_mode(rank)
        assert h.rank_mode == rank
    return h


def _classes(h, lens, max_len=0):
    counts = [0] * 9
    for length in lens:
        counts[0 if (max_len and length > max_len) else h.class_of(int(length))] += 1
    return counts


def _units(entry, lens, max_len=0):
    lds, part = _lds(entry), _part()
    return sum(-(-int(x) // part) for x in lens if x > lds and not (max_len and x > max_len))


def _note(h, entry, offsets, n, max_len=0, status=0):
    """gs_segsort16_check, gs_segsort16_last_classes and gs_segsort16_last agree with the lengths; the form words join the file's union."""
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort16 import segsort16_units
    lens = np.diff(offsets.astype(np.int64))
    assert h.status() == status
    cls = h.last_classes()
    assert cls["counts"] == _classes(h, lens, max_len) and cls["longest"] == int(lens.max()), (cls, lens.tolist())
    last = h.last()
    long_allowed = (max_len == 0 or max_len > _lds(entry)) and n > _lds(entry)
    assert last["n"] == n and last["units"] == (_units(entry, lens, max_len) if long_allowed else 0), last
    assert last["long_segments"] == cls["counts"][8]
    assert last["unit_cap"] == (segsort16_units(n, len(lens), *_mode(entry)) if long_allowed else 0) and last["units"] <= max(last["unit_cap"], 0)
    assert last["status"] == (2 if status == _lib.GS_ERR_SIZE else 0)
    assert bool(last["forms"] & _lib.GS_SEGSORT16_F_UNITS) == long_allowed
    _FORMS_SEEN[0] |= last["forms"]
    return last


def _run(gpu, h, entry, bits, offsets, kt, desc, max_len=0):
    """One call on fresh device copies of the uint16 array `bits`, compared with the reference over the whole array."""
    torch = _torch()
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    n, vb = bits.size, _mode(entry)[1]
    dk = torch.from_numpy(bits.view(np.int16).copy()).cuda()
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    if entry == "keys":
        h.sort(dk, do, max_segment_len=max_len)
        rk, _ = segmented_sort16_reference(bits, offsets, None, kt, desc)
        rv = dv = None
    elif entry == "argsort":
        dv = torch.full((n,), -1, dtype=torch.int32, device="cuda")   # output only: what it holds is never read
        h.argsort(dk, do, dv, max_segment_len=max_len)
        rk, rv = segmented_sort16_reference(bits, offsets, None, kt, desc)
        rv = rv.copy()
        lens = np.diff(offsets.astype(np.int64))
        inside = np.zeros(n, dtype=bool)
        inside[int(offsets[0]):int(offsets[-1])] = np.repeat(lens > 0, lens)    # (every non-empty segment is written, one-element ones too)
        rv[~inside] = 0xFFFFFFFF                                               # d_pos outside the segments is untouched
    else:
        vals = _values(n, vb)
        dv = torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()).cuda()
        h.sort(dk, do, dv, max_segment_len=max_len)
        rk, rv = segmented_sort16_reference(bits, offsets, vals, kt, desc)
    last = _note(h, entry, offsets, n, max_len)
    where = f"{entry} n={n} segments={offsets.size - 1} kt={kt} desc={desc} rank={last['rank_mode']} units={last['units']}"
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), rk, err_msg=where)
    if rv is not None:
        np.testing.assert_array_equal(dv.cpu().numpy().view(rv.dtype), rv, err_msg=where)
    np.testing.assert_array_equal(do.cpu().numpy().view(np.uint32), offsets, err_msg="the offsets were written")
    return last


def _random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 65536, n, dtype=np.uint16)


# ±0, ±inf, quiet and signalling NaNs of both signs, subnormals, ±1, the extremes — of float16 and of bfloat16
_SPECIALS = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400,
                      0x3C00, 0xBC00, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x007F, 0x807F, 0x0080, 0x3F80, 0xBF80], dtype=np.uint16)


def _float_bits(n, seed):
    """Uniform bit patterns with the special values strewn in, each many times."""
    rng = np.random.default_rng(seed)
    bits = _random_bits(n, seed)
    hit = rng.random(n) < 0.25
    bits[hit] = _SPECIALS[rng.integers(0, _SPECIALS.size, int(hit.sum()))]
    return bits


def _mix(entry, long_extra=9):
    """Lengths that fill every class the entry has, one long segment among them, short ones in between."""
    lds = _lds(entry)
    lens = [0, 1, 5, 32, 33, 0, 200, 256, 1, 257, 1000, 1024, 2, 1025, 2048, 2049, 5000, 8192]
    if lds >= 16384:
        lens += [8193, 7, 12000, 16384]
    if lds >= 32768:
        lens += [16385, 1, 20000, 32768]
    return lens + [3, lds + long_extra, 40, 1]


@pytest.mark.parametrize("entry", ENTRIES)
def test_class_borders(gpu, entry):
    """Every border of the length classes in one array, every segment starting at an odd element index; what lies above the entry's LDS
    limit takes the long route."""
    lens = _odd_starts(BORDER_LENGTHS)
    offsets = _offsets(lens)
    assert all(int(a) % 2 == 1 for a, length in zip(offsets[:-1], lens) if length in BORDER_LENGTHS and length != 1)
    n = int(offsets[-1]) + 3
    h = _handle(gpu, entry, n, len(lens), BF16)
    last = _run(gpu, h, entry, _float_bits(n, 1), offsets, BF16, False)
    assert last["units"] == _units(entry, BORDER_LENGTHS) > 0
    h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_alignment(gpu, entry):
    """A packed, a wave, a workgroup and a long segment at every residue 0 .. 7 of the start index mod 8, neighbours of another class on
    both sides (they share the dword and the 16-byte line at the boundary), guards in front and behind."""
    lds = _lds(entry)
    lens, at = [], 5
    for target, filler in ((7, 40), (100, 3), (300, 3), (lds + 5, 40)):
        for residue in range(8):
            pad = (residue - at) % 8
            pad += 8 if pad < 2 else 0       # a neighbour of at least two elements, of the other class
            pad = pad if filler == 3 or pad > 32 else pad + 32     # (the filler of 40 is a wave segment: 33 .. 47 elements)
            lens += [pad, target]
            at += pad
            assert at % 8 == residue
            at += target
    lens.append(3)
    offsets = _offsets(lens, front=5)
    n = int(offsets[-1]) + 11
    h = _handle(gpu, entry, n, len(lens), F16, True)
    _run(gpu, h, entry, _float_bits(n, 2), offsets, F16, True)
    h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ENTRIES)
def test_long_route(gpu, entry, rank):
    """The borders of the long route — the LDS limit + 1, one tile more than the limit, a part less one, a part, a part and one, two parts
    and a tile and three — several long segments of different lengths interleaved with short ones in one call; gs_segsort16_last reports
    the unit count computed here."""
    lds, part, tile = _lds(entry), _part(), _tile()
    longs = [lds + 1, part - 1, part, part + 1, 2 * part + tile + 3, lds + tile]
    lens = []
    for i, length in enumerate(longs):
        lens += [length, (1, 20, 300, 0, 2000, 33)[i]]
    offsets = _offsets(lens, front=3)
    n = int(offsets[-1]) + 5
    h = _handle(gpu, entry, n, len(lens), I16, rank == 1, rank)
    last = _run(gpu, h, entry, _random_bits(n, 3 + rank), offsets, I16, rank == 1)
    assert last["units"] == sum(-(-x // part) for x in longs if x > lds) >= 8 and last["rank_mode"] == rank
    h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_dummies_tie_with_all_one_keys_in_the_last_partial_tile(gpu, entry):
    """A last partial tile whose real keys have the sortable bits 0xFFFF (the dummies' pattern), in the ballot ranking, where the dummies
    are ranked: they must stay behind the real keys.  Long segments and LDS segments with a partial last row of slots."""
    lds, tile = _lds(entry), _tile()
    lens = [lds + tile + 100, 100, 300, 5000, lds + 1]
    offsets = _offsets(lens)
    n = int(offsets[-1]) + 1
    for kt, ones, desc in ((U16, 0xFFFF, False), (I16, 0x7FFF, True), (F16, 0x7FFF, False), (BF16, 0x7FFF, True)):
        bits = _random_bits(n, kt)
        bits[::7] = ones
        for a, length in zip(offsets[:-1], lens):
            tail = length % tile if length > lds else min(length, 50)
            bits[int(a) + length - tail:int(a) + length] = ones
        h = _handle(gpu, entry, n, len(lens), kt, desc, rank=0)
        _run(gpu, h, entry, bits, offsets, kt, desc)
        h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("desc", (False, True))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_orders_and_rank_modes(gpu, kt, desc, rank):
    for entry in ENTRIES:
        lens = _mix(entry)
        offsets = _offsets(lens, front=2)
        n = int(offsets[-1]) + 2
        h = _handle(gpu, entry, n, len(lens), kt, desc, rank)
        _run(gpu, h, entry, _float_bits(n, 10 * kt + rank), offsets, kt, desc)
        h.close()


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_every_pattern_once(gpu, kt):
    """A segment of 65 536 elements holding every bit pattern once (NaNs, ±0, infinities), shuffled, beside a short one."""
    rng = np.random.default_rng(kt)
    offsets = _offsets([10, 65536, 300], front=1)
    n = int(offsets[-1]) + 1
    bits = _random_bits(n, kt)
    bits[11:11 + 65536] = rng.permutation(65536).astype(np.uint16)
    for entry, desc in (("keys", False), ("argsort", True), ("pairs8", False)):
        h = _handle(gpu, entry, n, 3, kt, desc)
        _run(gpu, h, entry, bits, offsets, kt, desc)
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_distributions_and_stability(gpu, entry):
    """All equal, two values, sorted, reverse, and heavy duplicates on a mix of classes: values are array indices, so the comparison with
    the stable reference is the stability check, for 4- and 8-byte values and for the argsort."""
    lens = _mix(entry, long_extra=_tile() + 1)
    offsets = _offsets(lens)
    n = int(offsets[-1]) + 4
    rng = np.random.default_rng(6)
    ramp = np.arange(n, dtype=np.uint32)
    cases = {"equal": np.full(n, 0x3C00, dtype=np.uint16), "two": np.where(rng.random(n) < 0.5, 0x8000, 0x0000).astype(np.uint16),
             "sorted": (ramp // 3).astype(np.uint16), "reverse": (65535 - ramp // 3 % 65536).astype(np.uint16),
             "duplicates": (rng.integers(0, 5, n, dtype=np.uint16) << np.uint16(13)) | rng.integers(0, 2, n, dtype=np.uint16)}
    h = _handle(gpu, entry, n, len(lens), U16, False)
    hd = _handle(gpu, entry, n, len(lens), F16, True)
    for name, bits in cases.items():
        _run(gpu, h, entry, bits, offsets, U16, False)
        _run(gpu, hd, entry, bits, offsets, F16, True)
    h.close()
    hd.close()


def test_argsort_positions_are_array_indices(gpu):
    """Positions are array indices (segment start + position in the segment), segments of one element get their own index, and d_pos in
    front of, between (empty segments) and behind the segments keeps what it held."""
    torch = _torch()
    lens = [1, 0, 1, 3, 1, 0, 40, 1, 300, 1]
    offsets = _offsets(lens, front=6)
    n = int(offsets[-1]) + 6
    bits = _random_bits(n, 8)
    h = _handle(gpu, "argsort", n, len(lens), U16)
    dk = torch.from_numpy(bits.view(np.int16).copy()).cuda()
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    dp = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for max_len in (0, 300, 1):    # a promise of one element: only the packed kernel runs, and it still writes the lone elements
        dp.fill_(-7)
        dk.copy_(torch.from_numpy(bits.view(np.int16).copy()))
        h.argsort(dk, do, dp, max_segment_len=max_len)
        pos = dp.cpu().numpy()
        assert h.status() == (0 if max_len != 1 else 2)
        assert (pos[:6] == -7).all() and (pos[int(offsets[-1]):] == -7).all()
        for a, length in zip(offsets[:-1], lens):
            a = int(a)
            if max_len == 1 and length > 1:
                assert (pos[a:a + length] == -7).all()      # longer than promised: left alone
                continue
            got = pos[a:a + length]
            assert sorted(got.tolist()) == list(range(a, a + length))
            np.testing.assert_array_equal(bits[got], np.sort(bits[a:a + length], kind="stable"))
            if length == 1:
                assert got[0] == a
    _FORMS_SEEN[0] |= h.last()["forms"]
    h.close()


def test_promises(gpu):
    """A promise within LDS needs no alt buffers; a segment longer than promised is left unsorted with GS_ERR_SIZE while every other one is
    sorted; a promise above the LDS limit lets long segments up to it through."""
    torch = _torch()
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    lib = _lib.load()
    for entry in ("keys", "pairs4"):
        lds, vb = _lds(entry), _mode(entry)[1]
        lens = [5, 300, 2000, 40, lds + 10, 1000, 33, lds + 4000]
        offsets = _offsets(lens)
        n = int(offsets[-1]) + 2
        bits = _random_bits(n, 9)
        h = _handle(gpu, entry, n, len(lens), BF16)
        do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
        for max_len, size_err in ((2000, True), (1999, True), (lds, True), (lds + 10, True), (lds + 4000, False)):
            dk = torch.from_numpy(bits.view(np.int16).copy()).cuda()
            vals = _values(n, 4)
            dv = torch.from_numpy(vals.view(np.int32).copy()).cuda()
            within = max_len <= lds
            tk, tv = torch.empty(n, dtype=torch.int16, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
            ak, av = (None, None) if within else (tk.data_ptr(), tv.data_ptr())
            if entry == "keys":
                st = lib.gs_segsort16_sort_keys(h._h, dk.data_ptr(), ak, n, do.data_ptr(), len(lens), max_len, BF16, 0, None)
            else:
                st = lib.gs_segsort16_sort_pairs(h._h, dk.data_ptr(), dv.data_ptr(), ak, av, n, do.data_ptr(), len(lens), max_len, BF16, 0, None)
            assert st == 0      # d_alt = NULL is taken when the promise fits LDS
            _note(h, entry, offsets, n, max_len, status=_lib.GS_ERR_SIZE if size_err else 0)
            rk, rv = segmented_sort16_reference(bits, offsets, vals, BF16, False)
            for a, length in zip(offsets[:-1], lens):   # the segments that broke the promise are as they were
                if length > max_len:
                    rk[int(a):int(a) + length] = bits[int(a):int(a) + length]
                    rv[int(a):int(a) + length] = vals[int(a):int(a) + length]
            np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), rk, err_msg=f"{entry} max_len={max_len}")
            if vb:
                np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), rv, err_msg=f"{entry} max_len={max_len}")
        h.close()


def test_bad_offsets_write_nothing(gpu):
    """Decreasing offsets and a last offset beyond n: found on the device before anything is loaded through them; GS_ERR_ARG from the
    check, keys, values and positions untouched — with long segments among the good ones."""
    torch = _torch()
    from gpusorting_amd import _lib
    lds = _lds("pairs4")
    lens = [5, 300, lds + 100, 40, 2000]
    good = _offsets(lens)
    n = int(good[-1]) + 2
    down = good.copy()
    down[2] = down[1] - 1                    # decreasing
    beyond = good.copy()
    beyond[-1] = n + 1                       # the last offset lies beyond n
    wild = good.copy()
    wild[3] = 0xFFFFFFF0                     # far outside, and decreasing behind it
    bits = _random_bits(n, 12)
    for entry in ("pairs4", "argsort", "keys"):
        h = _handle(gpu, entry, n, len(lens), F16)
        for offsets in (down, beyond, wild):
            dk = torch.from_numpy(bits.view(np.int16).copy()).cuda()
            do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
            dv = torch.full((n,), 1234567, dtype=torch.int32, device="cuda")
            if entry == "keys":
                h.sort(dk, do)
            elif entry == "argsort":
                h.argsort(dk, do, dv)
            else:
                h.sort(dk, do, dv)
            assert h.status() == _lib.GS_ERR_ARG
            last = h.last()
            assert last["status"] & 1 and last["units"] == 0
            _FORMS_SEEN[0] |= last["forms"]
            np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), bits)
            assert (dv == 1234567).all()
        # the handle recovers: every call resets the status
        _run(gpu, h, entry, bits, good, F16, False)
        h.close()


def test_error_returns(gpu):
    """GS_ERR_ARG / GS_ERR_MODE / GS_ERR_SIZE in the order the header lists them; a refused call writes nothing; gs_segsort_sort_keys
    keeps refusing the 16-bit key types."""
    torch = _torch()
    from gpusorting_amd import _lib
    lib = _lib.load()
    long = _lds("pairs4") + 1
    n, segs = 2 * long, 2
    back = lambda nbytes: nbytes - (nbytes % 16 or 16)   # noqa: E731 (an aligned offset inside a buffer's last 16 bytes: refused for the overlap alone)
    k = torch.full((n + 64,), 0x1234, dtype=torch.int16, device="cuda")
    v = torch.full((n + 64,), 77, dtype=torch.int32, device="cuda")
    ak = torch.full((n + 64,), 0x4321, dtype=torch.int16, device="cuda")
    av = torch.full((n + 64,), 88, dtype=torch.int32, device="cuda")
    v8 = torch.full((n + 64,), 99, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, long, n, n], dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (k, v, ak, av, v8, off)]
    hk, hp, h8 = _handle(gpu, "keys", n, 4), _handle(gpu, "pairs4", n, 4), _handle(gpu, "pairs8", n, 4)
    kp, vp, akp, avp, v8p, op = (t.data_ptr() for t in (k, v, ak, av, v8, off))
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    keys = lib.gs_segsort16_sort_keys
    assert keys(None, kp, akp, n, op, segs, 0, U16, 0, None) == A
    assert keys(hk._h, None, akp, n, op, segs, 0, U16, 0, None) == A
    assert keys(hk._h, kp + 2, akp, n, op, segs, 0, U16, 0, None) == A        # element-aligned only
    assert keys(hk._h, kp, akp, n, None, segs, 0, U16, 0, None) == A
    assert keys(hk._h, kp, akp, n, op + 2, segs, 0, U16, 0, None) == A
    for kt in (0, 1, 2, 3, 4, 5, 10, -1):                                     # the 32- and 64-bit key types
        assert keys(hk._h, kp, akp, n, op, segs, 0, kt, 0, None) == A
    assert keys(hk._h, kp, akp, n, op, segs, 0, U16, 2, None) == A
    assert keys(hp._h, kp, akp, n, op, segs, 0, 0, 0, None) == A              # ARG (key type) comes before MODE
    assert keys(hp._h, kp, akp, n, op, segs, 0, U16, 0, None) == M            # keys call on a pairs handle
    assert keys(hp._h, kp, akp, 0, op, segs, 0, U16, 0, None) == M            # MODE comes before SIZE
    assert keys(hk._h, kp, akp, 0, op, segs, 0, U16, 0, None) == S
    assert keys(hk._h, kp, akp, n + 1, op, segs, 0, U16, 0, None) == S        # sizes beyond the handle
    assert keys(hk._h, kp, akp, n, op, 0, 0, U16, 0, None) == S
    assert keys(hk._h, kp, akp, n, op, 5, 0, U16, 0, None) == S
    assert keys(hk._h, kp, None, n + 1, op, segs, 0, U16, 0, None) == S       # SIZE comes before the alt pointers
    assert keys(hk._h, kp, None, n, op, segs, 0, U16, 0, None) == A           # NULL alt where long segments are allowed
    assert keys(hk._h, kp, None, n, op, segs, 32769, U16, 0, None) == A
    assert keys(hk._h, kp, akp + 2, n, op, segs, 0, U16, 0, None) == A
    assert keys(hk._h, kp, kp + back(2 * n), n, op, segs, 0, U16, 0, None) == A   # overlapping
    for call in (lib.gs_segsort16_sort_pairs, lib.gs_segsort16_argsort):
        assert call(None, kp, vp, akp, avp, n, op, segs, 0, BF16, 0, None) == A
        assert call(hp._h, None, vp, akp, avp, n, op, segs, 0, BF16, 0, None) == A
        assert call(hp._h, kp, vp, akp, avp, n, op, segs, 0, 2, 0, None) == A
        assert call(hp._h, kp, vp, akp, avp, n, op, segs, 0, BF16, 3, None) == A
        assert call(hk._h, kp, None, akp, avp, n, op, segs, 0, BF16, 0, None) == M             # on a keys-only handle; MODE before the value pointer
        assert call(hp._h, kp, None, akp, avp, n, op, segs, 0, BF16, 0, None) == A
        assert call(hp._h, kp, vp + 4, akp, avp, n, op, segs, 0, BF16, 0, None) == A
        assert call(hp._h, kp, None, akp, avp, 0, op, segs, 0, BF16, 0, None) == A             # the value pointer before SIZE
        assert call(hp._h, kp, vp, akp, avp, 0, op, segs, 0, BF16, 0, None) == S
        assert call(hp._h, kp, vp, akp, avp, n + 1, op, segs, 0, BF16, 0, None) == S
        assert call(hp._h, kp, vp, None, avp, n, op, segs, 0, BF16, 0, None) == A              # NULL alt where long segments are allowed
        assert call(hp._h, kp, vp, akp, None, n, op, segs, 0, BF16, 0, None) == A
        assert call(hp._h, kp, vp, akp + 8, avp, n, op, segs, 0, BF16, 0, None) == A
        assert call(hp._h, kp, vp, kp + back(2 * n), avp, n, op, segs, 0, BF16, 0, None) == A  # any two buffers overlapping
        assert call(hp._h, kp, vp, akp, vp + back(4 * n), n, op, segs, 0, BF16, 0, None) == A
    assert lib.gs_segsort16_argsort(h8._h, kp, v8p, akp, avp, n, op, segs, 0, BF16, 0, None) == M   # argsort needs 4-byte values
    assert lib.gs_segsort16_set_rank_mode(hp._h, 2) == A
    r = (C.c_uint32 * 16)()
    assert lib.gs_segsort16_last(hp._h, r, 7, None) == A and lib.gs_segsort16_last(hp._h, None, 8, None) == A
    assert lib.gs_segsort16_last_classes(hp._h, r, 9, None) == A and lib.gs_segsort16_last_classes(hp._h, None, 10, None) == A
    # the 32-bit segmented sort keeps refusing the 16-bit key types
    h32 = gpu.SegmentedSort(n, 4)
    for kt in KEY_TYPES:
        assert lib.gs_segsort_sort_keys(h32._h, kp, akp, n // 2, op, 1, 0, kt, 0, None) == A
    h32.close()
    torch.cuda.synchronize()
    for t, b in zip((k, v, ak, av, v8, off), before):
        assert torch.equal(t, b), "a refused call wrote to a buffer"
    # the same arguments, in order, are taken
    assert lib.gs_segsort16_sort_pairs(hp._h, kp, vp, akp, avp, n, op, 3, 0, BF16, 0, None) == 0
    hp.check()
    assert lib.gs_segsort16_argsort(hp._h, kp, vp, akp, avp, n, op, 3, 0, BF16, 1, None) == 0
    hp.check()
    assert keys(hk._h, kp, akp, n, op, 3, 0, U16, 0, None) == 0
    hk.check()
    for h in (hk, hp, h8):
        h.close()


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_memory_contract(gpu, entry, fill):
    """16-byte-only aligned views with guard bands, n smaller than the allocation: nothing in front of offsets[0] or at or behind
    offsets[-1] of the keys and values changes (the 2-byte neighbours included), the offsets are read-only, the alt buffers are written
    on [0, n) only — and not at all when the promise fits LDS — and what d_pos and the scratch hold on entry does not influence the result."""
    from guard_arena import Arena
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    lib = _lib.load()
    mode, vb = _mode(entry)
    vdt = np.uint64 if vb == 8 else np.uint32
    lds = _lds(entry)
    for lens, max_len in (([7, 100, lds + _tile() + 3, 300, 1, 33], 0), ([7, 100, 300, 1, 2049, 33], 4000)):
        offsets = _offsets(lens, front=3)
        n = int(offsets[-1]) + 3
        count = n + 21
        long = max_len == 0
        arena = Arena.for_views([(2 * count, np.uint8)] * 2 + [(len(offsets), np.uint32)] + ([(count, vdt)] * 2 if mode == PAIRS else []), "cuda", fill)
        dk = arena.carve(2 * count, np.uint8, 1, "keys")
        ak = arena.carve(2 * count, np.uint8, 3, "alt_keys")
        do = arena.carve(len(offsets), np.uint32, 9, "offsets")
        bits = _random_bits(count, n)
        arena.write(dk, bits.view(np.uint8))
        arena.write(do, offsets)
        arena.read_only(do)
        arena.live(dk, 2 * int(offsets[-1]), 2 * int(offsets[0]))
        arena.live(ak, 2 * n if long else 0)
        desc = not long
        h = _handle(gpu, entry, count, len(lens), F16, desc)
        if mode == PAIRS:
            dv = arena.carve(count, vdt, 5, "values")
            av = arena.carve(count, vdt, 7, "alt_values")
            vals = _values(count, vb).astype(vdt)
            if entry != "argsort":
                arena.write(dv, vals)       # argsort: d_pos keeps the arena's fill — it is output only
            arena.live(dv, int(offsets[-1]), int(offsets[0]))
            arena.live(av, n if long else 0)
            call = lib.gs_segsort16_argsort if entry == "argsort" else lib.gs_segsort16_sort_pairs
            st = call(h._h, dk.data_ptr(), dv.data_ptr(), ak.data_ptr(), av.data_ptr(), n, do.data_ptr(), len(lens), max_len, F16, h.order, None)
        else:
            st = lib.gs_segsort16_sort_keys(h._h, dk.data_ptr(), ak.data_ptr(), n, do.data_ptr(), len(lens), max_len, F16, h.order, None)
        assert st == 0
        _note(h, entry, offsets, n, max_len)
        arena.verify()
        carried = None if entry in ("keys", "argsort") else vals[:n]
        rk, rv = segmented_sort16_reference(bits[:n], offsets, carried, F16, desc)
        np.testing.assert_array_equal(arena.read(dk, np.uint16, 2 * n), rk, err_msg=f"{entry} {lens}")
        if mode == PAIRS:
            a, b = int(offsets[0]), int(offsets[-1])
            np.testing.assert_array_equal(arena.read(dv, vdt, n)[a:b], rv.astype(vdt)[a:b], err_msg=f"{entry} {lens}")
        h.close()


def test_graph_capture(gpu):
    """A call with max_segment_len = 0 and long segments present, captured once into a graph on one linear stream and replayed on new data
    with the same offsets: no host wait, whatever the segment lengths."""
    torch = _torch()
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    lds, part = _lds("argsort"), _part()
    lens = [5, lds + 77, 300, part + _tile() + 9, 1, 2000, lds + 1, 40]
    offsets = _offsets(lens, front=2)
    n = int(offsets[-1]) + 2
    h = _handle(gpu, "argsort", n, len(lens), BF16, True)
    dk = torch.empty(n, dtype=torch.int16, device="cuda")
    dp = torch.empty(n, dtype=torch.int32, device="cuda")
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()

    def load(seed):
        bits = _float_bits(n, seed)
        dk.copy_(torch.from_numpy(bits.view(np.int16).copy()))
        dp.fill_(-1)
        return bits

    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.argsort(dk, do, dp)         # warm-up outside the capture (the alt buffers are allocated here)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.argsort(dk, do, dp)
    for seed in (11, 12):
        bits = load(seed)
        graph.replay()
        torch.cuda.synchronize()
        last = _note(h, "argsort", offsets, n)
        assert last["units"] == _units("argsort", lens) >= 4
        rk, rp = segmented_sort16_reference(bits, offsets, None, BF16, True)
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), rk)
        inside = slice(int(offsets[0]), int(offsets[-1]))
        np.testing.assert_array_equal(dp.cpu().numpy().view(np.uint32)[inside], rp[inside])
        assert (dp[:2] == -1).all() and (dp[int(offsets[-1]):] == -1).all()
    h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_offset_sets_alternating_on_one_handle(gpu, entry):
    """Different offsets on one handle — long segments, none, long segments again — the state is reset by every call."""
    lds, part = _lds(entry), _part()
    sets = ([3, lds + part + 9, 300, lds + 1], [7, 300, 33, 2000, 1], [lds + 5, 5, 2 * part + 1, 0, 40], [100] * 50)
    h = _handle(gpu, entry, lds + 2 * part + 4096, 64, BF16, True)
    for i, lens in enumerate(sets + sets[:2]):
        offsets = _offsets(lens, front=i)
        n = int(offsets[-1]) + i
        _run(gpu, h, entry, _float_bits(n, 50 + i), offsets, BF16, True)
    h.close()


def test_tensor_convenience_layer(gpu):
    """gpusorting_amd.segmented_sort / segmented_sort_ / segmented_argsort on bfloat16, float16 and int16 (signed and unsigned=True)
    tensors against the library's reference; bfloat16 and float16 without NaNs are identical to widening to float32 and calling the
    32-bit functions; the 32-bit paths are unchanged; the input is not written."""
    torch = _torch()
    from gpusorting_amd.segsort import segmented_sort_reference
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    for lens in ([1], [5, 300, 0, 33, 2000], [40, _lds("argsort") + 100, 7, 9000], [3] * 70000):   # the cached handle grows
        offsets = _offsets(lens, front=2)
        n = int(offsets[-1]) + 3
        do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
        bits = _float_bits(n, n % 1000)
        for dtype, kt, unsigned in ((torch.bfloat16, BF16, False), (torch.float16, F16, False), (torch.int16, I16, False), (torch.int16, U16, True)):
            t = torch.from_numpy(bits.view(np.int16).copy()).cuda().view(dtype)
            for desc in (False, True):
                out = gpu.segmented_sort(t, do, descending=desc, unsigned=unsigned)
                assert out.dtype == dtype and out.shape == t.shape
                rk, rp = segmented_sort16_reference(bits, offsets, None, kt, desc)
                np.testing.assert_array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), rk)
                perm = gpu.segmented_argsort(t, do, descending=desc, unsigned=unsigned)
                assert perm.dtype == torch.int32 and perm.shape == t.shape
                np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), rp)      # identity outside the segments
                assert torch.equal(t.view(torch.int16).cpu(), torch.from_numpy(bits.view(np.int16)))   # the input is not written
            v8 = torch.arange(n, dtype=torch.int64, device="cuda")
            k2, v2 = gpu.segmented_sort(t, do, v8, unsigned=unsigned)
            rk, rv = segmented_sort16_reference(bits, offsets, np.arange(n, dtype=np.int64), kt, False)
            np.testing.assert_array_equal(k2.view(torch.int16).cpu().numpy().view(np.uint16), rk)
            np.testing.assert_array_equal(v2.cpu().numpy(), rv)
            k3, v4 = t.clone(), torch.arange(n, dtype=torch.int32, device="cuda")
            gpu.segmented_sort_(k3, do, v4, descending=True, unsigned=unsigned, max_segment_len=max(lens))
            rk, rp = segmented_sort16_reference(bits, offsets, None, kt, True)
            np.testing.assert_array_equal(k3.view(torch.int16).cpu().numpy().view(np.uint16), rk)
            np.testing.assert_array_equal(v4.cpu().numpy().view(np.uint32), rp)
        # without NaNs: the same result as widening to float32, the 32-bit functions, and narrowing
        for dtype in (torch.bfloat16, torch.float16):
            t = torch.from_numpy(bits.view(np.int16).copy()).cuda().view(dtype)
            t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
            for desc in (False, True):
                wide = gpu.segmented_sort(t.float(), do, descending=desc).to(dtype)
                assert torch.equal(gpu.segmented_sort(t, do, descending=desc).view(torch.int16), wide.view(torch.int16))
                assert torch.equal(gpu.segmented_argsort(t, do, descending=desc), gpu.segmented_argsort(t.float(), do, descending=desc))
    # the 32-bit paths are unchanged
    b32 = np.random.default_rng(3).integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    o32 = np.array([3, 100, 100, 2500, 4990], dtype=np.uint32)
    t32, d32 = torch.from_numpy(b32.view(np.int32).copy()).cuda(), torch.from_numpy(o32.view(np.int32).copy()).cuda()
    for desc in (False, True):
        np.testing.assert_array_equal(gpu.segmented_sort(t32, d32, descending=desc).cpu().numpy().view(np.uint32),
                                      segmented_sort_reference(b32, o32, None, 1, desc))
    np.testing.assert_array_equal(gpu.segmented_sort(t32.view(torch.float32), d32).view(torch.int32).cpu().numpy().view(np.uint32),
                                  segmented_sort_reference(b32, o32, None, 2, False))
    with pytest.raises(TypeError):
        gpu.segmented_sort(torch.zeros(8, dtype=torch.int64, device="cuda"), d32)
    with pytest.raises(ValueError):
        gpu.segmented_sort(torch.zeros((4, 4), dtype=torch.float16, device="cuda"), d32)                     # 2-D
    with pytest.raises(ValueError):
        gpu.segmented_sort(torch.zeros(8, dtype=torch.float16, device="cuda"), d32.long())                   # 8-byte offsets
    with pytest.raises(TypeError):
        gpu.segmented_sort(torch.zeros(8, dtype=torch.float16, device="cuda"), d32[:2], torch.zeros(8, dtype=torch.int16, device="cuda"))


def test_zz_every_compiled_kernel_form_was_reached(gpu):
    """gs_segsort16_last reports the kernel forms a call launched; their union over this file's cases must be every form the build
    compiles: classify, fill, the packed and the wave kernel for keys only, positions, 4- and 8-byte values, the 32 workgroup-class
    kernels, units, count, scan and the scatter's eight forms (run the whole file: this test stands last)."""
    from gpusorting_amd.segsort16 import SEGSORT16_FORMS
    assert len(SEGSORT16_FORMS) == 53
    missing = [name for name, bit in SEGSORT16_FORMS.items() if not _FORMS_SEEN[0] & bit]
    assert not missing, f"kernel forms no case of this file launched: {missing}"
    assert _FORMS_SEEN[0] == sum(SEGSORT16_FORMS.values())
