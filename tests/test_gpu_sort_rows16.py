"""GPU tests of the row-wise sort of 16-bit keys (gs_sort_rows16_* in include/gpusort.h; sortrows16_kernels.hpp): every row of a
[rows, row_len] matrix of uint16 / int16 / float16 / bfloat16 keys sorted on its own — keys only, as an argsort, with 4- and 8-byte
values — on the LDS route (the row-wise top-k's 2-byte LDS sorts with k = row_len, in place) and on the pass route (two passes of
count, scan, scatter over all rows at once).  Everything is compared bit for bit with sort_rows16_reference, the numpy statement of
the semantics (tests/test_sort_rows16_cpu.py checks that one on the CPU).  The LDS limit and the tile come from
gs_segsort_max_lds_segment and gs_sort_rows16_plan.  The last test asserts that the cases of this file reached every kernel form the
build compiles (gs_sort_rows16_last's form mask).  All shapes stay below 2^19 elements.

With a tile of 4096 elements the shortest pass-route row is two tiles + 1 (8-byte values: the LDS limit is 8192), so "one tile + 1" of
a row is run as "whole tiles + 1": the LDS limit + 1, whose last tile holds one element.  A plan of ONE part with several tiles needs
rows x (tiles / 2) >= 1024 or a row of fewer than four tiles; below 2^19 elements only 8-byte values reach it (a row of 8193 .. 16383
elements), in both rank modes; the other forms walk several tiles per part in plans of several parts."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
KEY_TYPES = (U16, I16, F16, BF16)
KEYS, PAIRS = 0, 1
ENTRIES = ("keys", "argsort", "pairs4", "pairs8")
ROUTE_LDS, ROUTE_PASSES = 1, 2
F_CLEAR, F_WAVE, F_TILE, F_COUNT, F_SCAN, F_SCATTER = 1, 2, 4, 8, 16, 32
_FORMS_SEEN = [0]   # union of gs_sort_rows16_last's form masks over the file's cases


def _torch():
    import torch
    return torch


def _mode(entry):
    return (KEYS, 0) if entry == "keys" else (PAIRS, 8 if entry == "pairs8" else 4)


def _lds(entry):
    from gpusorting_amd import _lib
    return int(_lib.load().gs_segsort_max_lds_segment(*_mode(entry)))


def _plan(entry, rows, row_len):
    from gpusorting_amd.rowsort16 import sort_rows16_plan
    return sort_rows16_plan(rows, row_len, *_mode(entry))


def _tile(entry):
    return _plan(entry, 1, _lds(entry) + 1)["tile"]


def _values(rows, row_len, vb):
    """value = position within the row (8 bytes: the row number and a high bit on top): equal keys must come out in rising position."""
    pos = np.tile(np.arange(row_len, dtype=np.uint32), (rows, 1))
    if vb == 4:
        return pos
    return pos.astype(np.uint64) | (np.arange(rows, dtype=np.uint64)[:, None] << np.uint64(40)) | np.uint64(1 << 63)


def _dev16(bits):
    return _torch().from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).cuda()


def _handle(gpu, entry, max_keys, kt=U16, desc=False, rank=None):
    mode, vb = _mode(entry)
    h = gpu.RowSort16(max_keys, order=1 if desc else 0, key_type=kt, mode=mode, value_bytes=vb)
    if rank is not None:
        h.set_rank_mode(rank)
        assert h.rank_mode == rank
    return h


def _scatter_forms(entry, rank):
    """The scatter instantiations a pass-route call of this form launches: v = 0 keys, 1 positions (argsort's first pass), 2 / 3 values."""
    vs = {"keys": (0,), "argsort": (1, 2), "pairs4": (2,), "pairs8": (3,)}[entry]
    return sum(F_SCATTER << (2 * v + rank) for v in vs)


def _note(h, entry, rows, row_len):
    """gs_sort_rows16_check is GS_OK, gs_sort_rows16_last agrees with gs_sort_rows16_plan; the form mask joins the file's union."""
    h.check()
    last, p = h.last(), _plan(entry, rows, row_len)
    assert last["status"] == 0 and (last["rows"], last["row_len"]) == (rows, row_len)
    assert (last["route"], last["parts"], last["per_part"]) == (p["route"], p["parts"], p["per_part"])
    assert last["route"] == (ROUTE_LDS if row_len <= _lds(entry) else ROUTE_PASSES)
    if last["route"] == ROUTE_PASSES:   # clear, count, scan and exactly the scatter forms of the entry and the rank mode: 7 launches
        assert last["forms"] == F_CLEAR | F_COUNT | F_SCAN | _scatter_forms(entry, last["rank_mode"]), last
    else:                               # the clear and ONE launch: the wave kernel up to 256 elements, the tile kernel above
        assert last["forms"] == F_CLEAR | (F_WAVE if row_len <= 256 else F_TILE), last
    _FORMS_SEEN[0] |= last["forms"]
    return last


def _run(gpu, h, entry, bits, kt, desc):
    """One call on fresh device copies of the [rows, row_len] uint16 array `bits`, compared with the reference."""
    torch = _torch()
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    rows, row_len = bits.shape
    dk = _dev16(bits)
    vb = _mode(entry)[1]
    if entry == "keys":
        h.sort(dk)
        rk, _ = sort_rows16_reference(bits, None, kt, desc)
        rv = dv = None
    elif entry == "argsort":
        dv = torch.full((rows, row_len), -1, dtype=torch.int32, device="cuda")   # output only: what it holds is never read
        h.argsort(dk, dv)
        rk, rv = sort_rows16_reference(bits, None, kt, desc)
    else:
        vals = _values(rows, row_len, vb)
        dv = torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()).cuda()
        h.sort(dk, dv)
        rk, rv = sort_rows16_reference(bits, vals, kt, desc)
    last = _note(h, entry, rows, row_len)
    where = f"{entry} rows={rows} row_len={row_len} kt={kt} desc={desc} rank={last['rank_mode']} parts={last['parts']}"
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), rk, err_msg=where)
    if rv is not None:
        np.testing.assert_array_equal(dv.cpu().numpy().view(rv.dtype), rv, err_msg=where)
    return last


def _random_bits(rows, row_len, seed):
    return np.random.default_rng(seed).integers(0, 65536, (rows, row_len), dtype=np.uint16)


# ±0, ±inf, quiet and signalling NaNs of both signs, subnormals, ±1, the extremes — of float16 and of bfloat16
_SPECIALS = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400,
                      0x3C00, 0xBC00, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x007F, 0x807F, 0x0080, 0x3F80, 0xBF80], dtype=np.uint16)


def _float_bits(rows, row_len, seed):
    """Uniform bit patterns with the special values strewn in, each many times."""
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
        h = _handle(gpu, entry, rows * (lds + 1), BF16, desc)
        last = _run(gpu, h, entry, _random_bits(rows, row_len, 10 * rows + i), BF16, desc)
        assert last["route"] == route
        h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ENTRIES)
def test_row_alignment(gpu, entry, rank):
    """9 rows of an odd length: with the LDS limit a multiple of 8, rows of limit + 1 elements start at all eight 2-byte offsets within
    16 bytes (the count kernel's peel), and so do rows of 257 and 1025 on the LDS route."""
    lds = _lds(entry)
    assert lds % 8 == 0
    for row_len in (lds + 1, 257, 1025):
        assert sorted((r * row_len * 2 % 16) // 2 for r in range(8)) == list(range(8))
        for desc in (False, True):
            h = _handle(gpu, entry, 9 * row_len, F16, desc, rank)
            _run(gpu, h, entry, _float_bits(9, row_len, row_len + rank), F16, desc)
            h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_lds_route_in_place(gpu, entry):
    """The LDS route at every class border it crosses (wave kernel up to 256, then the tile kernel's classes), 5 rows — a wave kernel's
    second workgroup has three dead waves — and 65 rows of 300."""
    lds = _lds(entry)
    lens = [n for n in (1, 2, 255, 256, 257, 1024, 1025, 2048, 2049, 8192, 8193, 16384, 16385) if n < lds] + [lds]
    for i, row_len in enumerate(lens):
        desc, kt = bool(i & 1), KEY_TYPES[i % 4]
        h = _handle(gpu, entry, 5 * row_len, kt, desc, rank=(i >> 1) & 1)
        last = _run(gpu, h, entry, _float_bits(5, row_len, 200 + i), kt, desc)
        assert last["route"] == ROUTE_LDS
        h.close()
    for rank in (0, 1):
        h = _handle(gpu, entry, 65 * 300, I16, bool(rank), rank)
        _run(gpu, h, entry, _float_bits(65, 300, 300 + rank), I16, bool(rank))
        h.close()


def _pass_shapes(entry):
    """(rows, row_len, what) on the pass route — see the module's note on the tile and the LDS limit."""
    lds, tile = _lds(entry), _tile(entry)
    uneven = lds + 3 * tile + 77
    shapes = [(1, lds + 1, "tiles+1"), (1, lds + 2 * tile, "k tiles"), (1, lds + 2 * tile - 1, "k tiles - 1"), (3, uneven, "uneven last part"),
              (3, lds + tile + 1, "odd rows"), (2, lds + 5, "short tail")]
    p = _plan(entry, 3, uneven)
    assert p["parts"] > 1 and p["per_part"] >= 2 * tile and 0 < uneven - (p["parts"] - 1) * p["per_part"] < p["per_part"] and uneven % tile, p
    assert all(r * n < (1 << 19) and _plan(entry, r, n)["route"] == ROUTE_PASSES for r, n, _ in shapes)
    if entry == "pairs8":
        assert _plan(entry, 1, lds + 1)["parts"] == 1 and _plan(entry, 1, lds + 1)["per_part"] == 3 * tile   # one part, several tiles
    return shapes


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ENTRIES)
def test_pass_route_shapes(gpu, entry, rank):
    shapes = _pass_shapes(entry)
    for desc in (False, True):
        h = _handle(gpu, entry, max(r * n for r, n, _ in shapes), U16, desc, rank)
        for i, (rows, row_len, _) in enumerate(shapes):
            last = _run(gpu, h, entry, _random_bits(rows, row_len, 100 + 7 * i + rank), U16, desc)
            assert last["route"] == ROUTE_PASSES and last["rank_mode"] == rank
        h.close()


@pytest.mark.parametrize("desc", (False, True))
def test_argsort_positions_are_relative_to_the_row(gpu, desc):
    """3 and 4 rows on both routes: the positions the kernels make equal the reference's and what a pairs call carries when it is fed an
    explicit in-row arange."""
    torch = _torch()
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    lds = _lds("argsort")
    for rows, row_len in ((3, 300), (4, 5000), (3, lds + _tile("argsort") + 7)):
        bits = _float_bits(rows, row_len, rows + row_len) & np.uint16(0xF00F)   # heavy ties
        ha, hp = _handle(gpu, "argsort", rows * row_len, F16, desc), _handle(gpu, "pairs4", rows * row_len, F16, desc)
        ka, kp = _dev16(bits), _dev16(bits)
        pos = torch.full((rows, row_len), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        ar = torch.arange(row_len, dtype=torch.int32, device="cuda").repeat(rows, 1).contiguous()
        ha.argsort(ka, pos)
        hp.sort(kp, ar)
        _note(ha, "argsort", rows, row_len)
        _note(hp, "pairs4", rows, row_len)
        rk, rp = sort_rows16_reference(bits, None, F16, desc)
        assert int(pos.max()) < row_len and int(pos.min()) >= 0
        np.testing.assert_array_equal(pos.cpu().numpy().view(np.uint32), rp)
        assert torch.equal(pos, ar) and torch.equal(ka, kp)
        np.testing.assert_array_equal(ka.cpu().numpy().view(np.uint16), rk)
        ha.close()
        hp.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("desc", (False, True))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_orders_and_rank_modes(gpu, kt, desc, rank):
    """The four key types on bit patterns strewn with ±0, ±inf, NaNs and subnormals (as integers they are just extremes)."""
    for entry in ENTRIES:
        rows, row_len = 3, _lds(entry) + _tile(entry) + 5
        h = _handle(gpu, entry, rows * row_len, kt, desc, rank)
        _run(gpu, h, entry, _float_bits(rows, row_len, 31 * kt + rank), kt, desc)
        _run(gpu, h, entry, _float_bits(65, 300, 32 * kt + rank), kt, desc)     # and the LDS route's tile kernel
        h.close()


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_every_pattern_once(gpu, kt):
    """Rows that hold every one of the 65 536 bit patterns exactly once, each in another order."""
    rng = np.random.default_rng(kt)
    bits = np.stack([rng.permutation(65536).astype(np.uint16) for _ in range(2)])
    for entry in ("keys", "argsort"):
        for desc in (False, True):
            h = _handle(gpu, entry, bits.size, kt, desc)
            _run(gpu, h, entry, bits, kt, desc)
            h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_distributions(gpu, entry):
    torch = _torch()
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    rows, row_len = 2, _lds(entry) + 2 * _tile(entry) + 9
    vb = _mode(entry)[1]
    for kt, desc in ((BF16, False), (I16, True)):
        h = _handle(gpu, entry, rows * row_len, kt, desc)
        rnd = _random_bits(rows, row_len, 5)
        equal = np.full((rows, row_len), 0x3F80, dtype=np.uint16)
        _run(gpu, h, entry, rnd, kt, desc)
        _run(gpu, h, entry, equal, kt, desc)
        if entry == "pairs4":   # all equal: the values stay where they are, descending turns the row round
            dk = _dev16(equal)
            dv = torch.from_numpy(_values(rows, row_len, 4).view(np.int32).copy()).cuda()
            h.sort(dk, dv)
            want = np.tile(np.arange(row_len, dtype=np.int32), (rows, 1))
            np.testing.assert_array_equal(dv.cpu().numpy(), want[:, ::-1] if desc else want)
        mixed = rnd.copy()
        mixed[0, :] = 0xBF80                                   # one row all equal beside a uniform one
        _run(gpu, h, entry, mixed, kt, desc)
        _run(gpu, h, entry, np.where(rnd & 4, np.uint16(0x8001), np.uint16(0x7FFF)).astype(np.uint16), kt, desc)   # two values
        _run(gpu, h, entry, (rnd & np.uint16(0x0303)) | np.uint16(0xFC00), kt, desc)    # four values per digit: every base moves far
        srt = sort_rows16_reference(rnd, None, kt, desc)[0]
        _run(gpu, h, entry, srt, kt, desc)                     # already sorted
        _run(gpu, h, entry, np.ascontiguousarray(srt[:, ::-1]), kt, desc)   # reverse sorted
        h.close()


@pytest.mark.parametrize("entry", ("argsort", "pairs4"))
def test_dummies_tie_with_all_one_keys_in_the_last_partial_tile(gpu, entry):
    """Rank mode 0 ranks the all-one dummies of a partial tile's slots >= m under digit 255 on both bytes, where real keys whose sortable
    bits are 0xFFFF lie as well: the last partial tile holds nothing but such keys (and more of them are strewn over the row), with
    positions as values — a dummy that overtook a real key, or a wrong count of digit 255, would show."""
    lds, tile = _lds(entry), _tile(entry)
    rows, row_len = 3, lds + tile + 100
    assert row_len % tile == 100 + lds % tile and 0 < row_len % tile < tile
    for kt, ones, desc in ((U16, 0xFFFF, False), (I16, 0x7FFF, True), (F16, 0x7FFF, False), (BF16, 0x7FFF, True)):
        bits = _random_bits(rows, row_len, kt)
        bits[:, ::7] = ones
        bits[:, row_len - row_len % tile:] = ones
        h = _handle(gpu, entry, rows * row_len, kt, desc, rank=0)
        last = _run(gpu, h, entry, bits, kt, desc)
        assert last["route"] == ROUTE_PASSES and last["rank_mode"] == 0
        h.close()


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_memory_contract(gpu, entry, fill):
    """16-byte-only aligned views with guard bands, rows * row_len smaller than the allocation and odd rows, on both routes: nothing at
    or behind element rows * row_len of the keys, the values and both alt buffers changes — the 2-byte neighbour of the last key
    included — the LDS route leaves the alt buffers alone altogether, and what d_pos and the scratch hold on entry does not influence
    the result."""
    from guard_arena import Arena
    from gpusorting_amd import _lib
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    lib = _lib.load()
    mode, vb = _mode(entry)
    vdt = np.uint64 if vb == 8 else np.uint32
    for rows, row_len in ((3, _lds(entry) + _tile(entry) + 3), (5, 257), (3, 7)):
        n = rows * row_len
        count = n + 21
        passes = row_len > _lds(entry)
        arena = Arena.for_views([(2 * count, np.uint8)] * 2 + ([(count, vdt)] * 2 if mode == PAIRS else []), "cuda", fill)
        dk = arena.carve(2 * count, np.uint8, 1, "keys")
        ak = arena.carve(2 * count, np.uint8, 3, "alt_keys")
        bits = _random_bits(1, count, n)[0]
        arena.write(dk, bits.view(np.uint8))
        arena.live(dk, 2 * n)
        arena.live(ak, 2 * n if passes else 0)
        desc = rows == 5
        h = _handle(gpu, entry, count, F16, desc)
        if mode == PAIRS:
            dv = arena.carve(count, vdt, 5, "values")
            av = arena.carve(count, vdt, 7, "alt_values")
            vals = np.zeros(count, dtype=vdt)
            vals[:n] = _values(rows, row_len, vb).reshape(-1)
            if entry != "argsort":
                arena.write(dv, vals)       # argsort: d_pos keeps the arena's fill — it is output only
            arena.live(dv, n)
            arena.live(av, n if passes else 0)
            call = lib.gs_sort_rows16_argsort if entry == "argsort" else lib.gs_sort_rows16_pairs
            st = call(h._h, dk.data_ptr(), dv.data_ptr(), ak.data_ptr(), av.data_ptr(), rows, row_len, F16, h.order, None)
        else:
            st = lib.gs_sort_rows16_keys(h._h, dk.data_ptr(), ak.data_ptr(), rows, row_len, F16, h.order, None)
        assert st == 0
        _note(h, entry, rows, row_len)
        arena.verify()
        carried = None if entry in ("keys", "argsort") else vals[:n].reshape(rows, row_len)
        rk, rv = sort_rows16_reference(bits[:n].reshape(rows, row_len), carried, F16, desc)
        np.testing.assert_array_equal(arena.read(dk, np.uint16, 2 * n).reshape(rows, row_len), rk, err_msg=f"{entry} {rows}x{row_len}")
        if mode == PAIRS:
            np.testing.assert_array_equal(arena.read(dv, vdt, n).reshape(rows, row_len), rv.astype(vdt), err_msg=f"{entry} {rows}x{row_len}")
        h.close()


def test_error_returns(gpu):
    """GS_ERR_ARG / GS_ERR_MODE / GS_ERR_SIZE in the order the header lists them; a refused call writes nothing."""
    torch = _torch()
    from gpusorting_amd import _lib
    lib = _lib.load()
    rows, long = 2, _lds("pairs4") + 1          # a pass-route shape for 4-byte values; short rows of 100 take the LDS route
    n = rows * long
    back = lambda nbytes: nbytes - (nbytes % 16 or 16)   # noqa: E731 (an aligned offset inside a buffer's last 16 bytes: refused for the overlap alone)
    k = torch.full((n + 64,), 0x1234, dtype=torch.int16, device="cuda")
    v = torch.full((n + 64,), 77, dtype=torch.int32, device="cuda")
    ak = torch.full((n + 64,), 0x4321, dtype=torch.int16, device="cuda")
    av = torch.full((n + 64,), 88, dtype=torch.int32, device="cuda")
    v8 = torch.full((n + 64,), 99, dtype=torch.int64, device="cuda")
    before = [t.clone() for t in (k, v, ak, av, v8)]
    hk, hp, h8 = _handle(gpu, "keys", 2 * (_lds("keys") + 1)), _handle(gpu, "pairs4", n), _handle(gpu, "pairs8", n)
    kp, vp, akp, avp, v8p = (t.data_ptr() for t in (k, v, ak, av, v8))
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    lk = _lds("keys") + 1
    # keys entry
    keys = lib.gs_sort_rows16_keys
    assert keys(None, kp, akp, 4, 100, U16, 0, None) == A
    assert keys(hk._h, None, akp, 4, 100, U16, 0, None) == A
    assert keys(hk._h, kp + 2, akp, 4, 100, U16, 0, None) == A        # element-aligned only
    for kt in (0, 1, 2, 3, 4, 5, 10, -1):                             # the 32- and 64-bit key types
        assert keys(hk._h, kp, akp, 4, 100, kt, 0, None) == A
    assert keys(hk._h, kp, akp, 4, 100, U16, 2, None) == A
    assert keys(hp._h, kp, akp, 4, 100, 0, 0, None) == A              # ARG (key type) comes before MODE
    assert keys(hp._h, kp, akp, 4, 100, U16, 0, None) == M            # keys call on a pairs handle
    assert keys(hp._h, kp, akp, 0, 100, U16, 0, None) == M            # MODE comes before SIZE
    assert keys(hk._h, kp, akp, 0, 100, U16, 0, None) == S            # zero rows
    assert keys(hk._h, kp, akp, 4, 0, U16, 0, None) == S
    assert keys(hk._h, kp, akp, 3, lk, U16, 0, None) == S             # rows * row_len > max_keys
    assert keys(hk._h, kp, akp, 1 << 16, 1 << 16, U16, 0, None) == S  # the product wraps to 0 in 32 bits
    assert keys(hk._h, kp, None, 3, lk, U16, 0, None) == S            # SIZE comes before the alt pointers
    assert keys(hk._h, kp, None, 1, lk, U16, 0, None) == A            # NULL alt on the pass route
    assert keys(hk._h, kp, akp + 2, 1, lk, U16, 0, None) == A
    assert keys(hk._h, kp, kp + back(2 * lk), 1, lk, U16, 0, None) == A   # overlapping
    # pairs and argsort entries
    for call in (lib.gs_sort_rows16_pairs, lib.gs_sort_rows16_argsort):
        assert call(None, kp, vp, akp, avp, rows, long, BF16, 0, None) == A
        assert call(hp._h, None, vp, akp, avp, rows, long, BF16, 0, None) == A
        assert call(hp._h, kp, vp, akp, avp, rows, long, 2, 0, None) == A
        assert call(hp._h, kp, vp, akp, avp, rows, long, BF16, 3, None) == A
        assert call(hk._h, kp, None, akp, avp, 4, 100, BF16, 0, None) == M             # on a keys-only handle; MODE before the value pointer
        assert call(hp._h, kp, None, akp, avp, rows, long, BF16, 0, None) == A
        assert call(hp._h, kp, vp + 4, akp, avp, rows, long, BF16, 0, None) == A
        assert call(hp._h, kp, None, akp, avp, 0, long, BF16, 0, None) == A             # the value pointer before SIZE
        assert call(hp._h, kp, vp, akp, avp, 0, long, BF16, 0, None) == S
        assert call(hp._h, kp, vp, akp, avp, rows + 1, long, BF16, 0, None) == S
        assert call(hp._h, kp, vp, None, avp, rows, long, BF16, 0, None) == A           # NULL alt on the pass route
        assert call(hp._h, kp, vp, akp, None, rows, long, BF16, 0, None) == A
        assert call(hp._h, kp, vp, akp + 8, avp, rows, long, BF16, 0, None) == A
        assert call(hp._h, kp, vp, kp + back(2 * n), avp, rows, long, BF16, 0, None) == A   # any two buffers overlapping
        assert call(hp._h, kp, vp, akp, vp + back(4 * n), rows, long, BF16, 0, None) == A
    assert lib.gs_sort_rows16_argsort(h8._h, kp, v8p, akp, avp, 4, 100, BF16, 0, None) == M   # argsort needs 4-byte values
    assert lib.gs_sort_rows16_set_rank_mode(hp._h, 2) == A
    r = (C.c_uint32 * 8)()
    assert lib.gs_sort_rows16_last(hp._h, r, 7, None) == A and lib.gs_sort_rows16_last(hp._h, None, 8, None) == A
    torch.cuda.synchronize()
    for t, b in zip((k, v, ak, av, v8), before):
        assert torch.equal(t, b), "a refused call wrote to a buffer"
    # the same arguments, in order, are taken; on the LDS route the alt pointers may be NULL
    assert lib.gs_sort_rows16_pairs(hp._h, kp, vp, akp, avp, rows, long, BF16, 0, None) == 0
    hp.check()
    assert lib.gs_sort_rows16_argsort(hp._h, kp, vp, akp, avp, rows, long, BF16, 1, None) == 0
    hp.check()
    assert lib.gs_sort_rows16_pairs(hp._h, kp, vp, None, None, 4, 100, BF16, 0, None) == 0 and keys(hk._h, kp, None, 4, 100, U16, 0, None) == 0
    assert lib.gs_sort_rows16_argsort(hp._h, kp, vp, None, None, 4, 100, BF16, 0, None) == 0
    hp.check()
    hk.check()
    for h in (hk, hp, h8):
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_shapes_alternating_on_one_handle(gpu, entry):
    """Different shapes on one handle — pass route, LDS route, pass route — the state is reset by every call."""
    lds, tile = _lds(entry), _tile(entry)
    h = _handle(gpu, entry, 3 * (lds + 3 * tile), BF16, True)
    for i, (rows, row_len) in enumerate(((3, lds + 2 * tile + 9), (7, 300), (1, lds + 1), (65, 20), (2, lds + 3 * tile))):
        _run(gpu, h, entry, _float_bits(rows, row_len, 50 + i), BF16, True)
        assert h.status() == 0
    h.close()


def test_graph_capture(gpu):
    """One pass-route argsort captured into a graph on one linear stream, replayed on fresh data."""
    torch = _torch()
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    rows, row_len = 3, _lds("argsort") + 2 * _tile("argsort") + 77
    h = _handle(gpu, "argsort", rows * row_len, BF16, True)
    dk = torch.empty((rows, row_len), dtype=torch.int16, device="cuda")
    dp = torch.empty((rows, row_len), dtype=torch.int32, device="cuda")

    def load(seed):
        bits = _float_bits(rows, row_len, seed)
        dk.copy_(torch.from_numpy(bits.view(np.int16).copy()))
        dp.fill_(-1)
        return bits

    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.argsort(dk, dp)         # warm-up outside the capture (the alt buffers are allocated here)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.argsort(dk, dp)
    for seed in (11, 12):
        bits = load(seed)
        graph.replay()
        torch.cuda.synchronize()
        _note(h, "argsort", rows, row_len)
        rk, rp = sort_rows16_reference(bits, None, BF16, True)
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), rk)
        np.testing.assert_array_equal(dp.cpu().numpy().view(np.uint32), rp)
    h.close()


def test_tensor_convenience_layer(gpu):
    """gpusorting_amd.sort_rows / sort_rows_ / argsort_rows on bfloat16, float16 and int16 (signed and unsigned=True) 2-D tensors:
    against the library's reference, integer keys also against torch.sort(dim=-1, stable=True); 32-bit tensors are forwarded; the
    input is not written; sort / argsort keep refusing 2-D half tensors."""
    torch = _torch()
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    from gpusorting_amd.rowsort import sort_rows_reference
    for rows, row_len in ((1, 1), (5, 300), (3, _lds("argsort") + _tile("argsort") + 1), (2, _lds("keys") + 5), (70, 33)):  # the cached handle grows
        bits = _float_bits(rows, row_len, rows + row_len)
        for dtype, kt, unsigned in ((torch.bfloat16, BF16, False), (torch.float16, F16, False), (torch.int16, I16, False), (torch.int16, U16, True)):
            t = torch.from_numpy(bits.view(np.int16).copy()).cuda().view(dtype)
            for desc in (False, True):
                out = gpu.sort_rows(t, descending=desc, unsigned=unsigned)
                assert out.dtype == dtype and out.shape == t.shape
                rk, rp = sort_rows16_reference(bits, None, kt, desc)
                np.testing.assert_array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), rk)
                perm = gpu.argsort_rows(t, descending=desc, unsigned=unsigned)
                assert perm.dtype == torch.int32 and perm.shape == t.shape
                np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), rp)
                if dtype == torch.int16 and not unsigned:
                    want, widx = torch.sort(t, dim=-1, descending=desc, stable=True)
                    assert torch.equal(out, want)
                    if not desc:    # ascending, ties in rising position: torch's stable order
                        assert torch.equal(perm.long(), widx)
                assert torch.equal(t.view(torch.int16).cpu(), torch.from_numpy(bits.view(np.int16)))   # the input is not written
            # 8-byte values out of place, 4-byte values in place
            v8 = torch.arange(rows * row_len, dtype=torch.int64, device="cuda").reshape(rows, row_len)
            k2, v2 = gpu.sort_rows(t, v8, unsigned=unsigned)
            rk, rv = sort_rows16_reference(bits, np.arange(rows * row_len, dtype=np.int64).reshape(rows, row_len), kt, False)
            np.testing.assert_array_equal(k2.view(torch.int16).cpu().numpy().view(np.uint16), rk)
            np.testing.assert_array_equal(v2.cpu().numpy(), rv)
            k3 = t.clone()
            v4 = torch.arange(row_len, dtype=torch.int32, device="cuda").repeat(rows, 1)
            gpu.sort_rows_(k3, v4, descending=True, unsigned=unsigned)
            rk, rp = sort_rows16_reference(bits, None, kt, True)
            np.testing.assert_array_equal(k3.view(torch.int16).cpu().numpy().view(np.uint16), rk)
            np.testing.assert_array_equal(v4.cpu().numpy().view(np.uint32), rp)
    # 32-bit tensors are forwarded to the 32-bit row-wise sort
    b32 = np.random.default_rng(3).integers(0, 1 << 32, (5, 700), dtype=np.uint64).astype(np.uint32)
    t32 = torch.from_numpy(b32.view(np.int32).copy()).cuda()
    for desc in (False, True):
        rk, rp = sort_rows_reference(b32, None, 1, desc)
        np.testing.assert_array_equal(gpu.sort_rows(t32, descending=desc).cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(gpu.argsort_rows(t32, descending=desc).cpu().numpy().view(np.uint32), rp)
    f32 = t32.view(torch.float32)
    np.testing.assert_array_equal(gpu.sort_rows(f32).view(torch.int32).cpu().numpy().view(np.uint32), sort_rows_reference(b32, None, 2, False)[0])
    # what the new names refuse, and what the old ones keep refusing
    with pytest.raises(ValueError):
        gpu.sort_rows(torch.zeros(8, dtype=torch.float16, device="cuda"))                                   # 1-D
    with pytest.raises(ValueError):
        gpu.sort_rows_(torch.zeros((4, 8), dtype=torch.bfloat16, device="cuda")[:, :4])                     # strided rows
    with pytest.raises(TypeError):
        gpu.sort_rows(torch.zeros((4, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        gpu.sort_rows(torch.zeros((4, 4), dtype=torch.float16, device="cuda"), torch.zeros((4, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        gpu.sort_rows(torch.zeros((4, 4), dtype=torch.float16, device="cuda"), torch.zeros((4, 4), dtype=torch.int16, device="cuda"))
    for dtype in (torch.float16, torch.bfloat16, torch.int16):
        with pytest.raises(TypeError, match="int32, uint32, float32"):
            gpu.sort(torch.zeros((4, 4), dtype=dtype, device="cuda"))
        with pytest.raises(TypeError, match="int32, uint32, float32"):
            gpu.argsort(torch.zeros((4, 4), dtype=dtype, device="cuda"))


def test_zz_every_compiled_kernel_form_was_reached(gpu):
    """The forms this build compiles: the clear, the LDS route's wave and tile kernels; count, scan; the scatter for keys only, positions,
    4- and 8-byte values, each in both rank modes.  gs_sort_rows16_last reports the forms a call launched; their union over this file's
    cases must be all of them (run the whole file: this test stands last)."""
    from gpusorting_amd.rowsort16 import SORT_ROWS16_FORMS
    from gpusorting_amd import _lib
    assert len(SORT_ROWS16_FORMS) == 13 and sum(SORT_ROWS16_FORMS.values()) == _lib.GS_SORT_ROWS16_F_ALL
    missing = [name for name, bit in SORT_ROWS16_FORMS.items() if not _FORMS_SEEN[0] & bit]
    assert not missing, f"kernel forms no case of this file reached: {missing}"
