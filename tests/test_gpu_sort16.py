"""GPU tests of the 16-bit sort (gs_sort16_* in include/gpusort.h; sort16_kernels.hpp): keys only (histogram, scan, fill), pairs with
4- and 8-byte values and argsort (two passes of count, scan, scatter).  Everything is compared bit for bit with sort16_reference, the
numpy statement of the semantics (tests/test_sort16_cpu.py checks that one on the CPU).  Sizes come from gs_sort16_plan.  The last
test asserts that the cases of this file reached every kernel form the build compiles (gs_sort16_last's form mask)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U16, I16, F16, BF16 = 6, 7, 8, 9
KEY_TYPES = (U16, I16, F16, BF16)
KEYS, PAIRS = 0, 1
ENTRIES = ("keys", "pairs4", "pairs8", "argsort")
_FORMS_SEEN = [0]   # union of gs_sort16_last's form masks over the file's cases


def _torch():
    import torch
    return torch


def _mode(entry):
    return (KEYS, 0) if entry == "keys" else (PAIRS, 8 if entry == "pairs8" else 4)


def _plan(entry, n=1):
    from gpusorting_amd.sort16 import sort16_plan
    return sort16_plan(n, *_mode(entry))


def _multi_tile_sizes(entry):
    """Sizes above the range cap, where the plan gives a range more than one tile: cap * tile + tile + 3 (two tiles per range, the last
    range ends in a partial tile: the running per-digit bases of the scatter, its barriers between tiles); keys only also
    cap * 4 * tile + tile + 3 (five tiles per range: a second trip of the histogram's unrolled loop, which holds four)."""
    p = _plan(entry)
    tile, cap = p["tile"], p["cap"]
    sizes = [cap * tile + tile + 3] + ([cap * 4 * tile + tile + 3] if entry == "keys" else [])
    for n, tiles in zip(sizes, (2, 5)):
        q = _plan(entry, n)
        assert q["per_range"] == tiles * tile and n % q["per_range"] not in (0, tile) and n % tile != 0, (n, q)
    return sizes


def _sizes(entry):
    """The issue's list: small and odd sizes, around a tile, around one range and behind two (below the cap a range is one tile, so
    these fall together with the tile's neighbours and 2 * tile + 3), 2^20 + 5, the smallest n that reaches the range cap + 1 — and
    _multi_tile_sizes, the sizes at which a range holds several tiles."""
    p = _plan(entry)
    tile, cap = p["tile"], p["cap"]
    reach = (cap - 1) * tile + 1
    assert _plan(entry, reach)["ranges"] == cap and _plan(entry, reach - 1)["ranges"] == cap - 1
    per = _plan(entry, tile)["per_range"]
    return [1, 2, 7, 8, 9, 63, 64, 65, tile - 1, tile, tile + 1, per - 1, per + 1, 2 * per + 3, (1 << 20) + 5, reach + 1] + _multi_tile_sizes(entry)


def _dev16(bits):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).cuda()


def _values(n, vb, seed=0):
    if vb == 8:
        return (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(seed)
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(seed)


def _handle(gpu, entry, max_keys, kt=U16, desc=False, rank=None):
    mode, vb = _mode(entry)
    h = gpu.Sort16(max_keys, order=1 if desc else 0, key_type=kt, mode=mode, value_bytes=vb)
    if rank is not None:
        h.set_rank_mode(rank)
        assert h.rank_mode == rank
    return h


def _note(h, entry, n):
    """gs_sort16_check is GS_OK, gs_sort16_last agrees with gs_sort16_plan; the form mask joins the file's union."""
    h.check()
    last, p = h.last(), _plan(entry, n)
    assert last["status"] == 0 and last["n"] == n
    assert (last["ranges"], last["per_range"], last["tile"]) == (p["ranges"], p["per_range"], p["tile"])
    assert last["route"] == (1 if entry == "keys" else 2)
    _FORMS_SEEN[0] |= last["forms"]
    return last


def _run(gpu, h, entry, bits, kt, desc, seed=0):
    """One call on fresh device copies of `bits`, compared with the reference."""
    torch = _torch()
    from gpusorting_amd.sort16 import sort16_reference
    n = bits.size
    dk = _dev16(bits)
    if entry == "keys":
        h.sort(dk)
        rk, _ = sort16_reference(bits, None, kt, desc)
        rv = dv = None
    elif entry == "argsort":
        dv = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        h.argsort(dk, dv)
        rk, rv = sort16_reference(bits, None, kt, desc)
    else:
        vals = _values(n, _mode(entry)[1], seed)
        dv = torch.from_numpy(vals.view(np.int64 if vals.itemsize == 8 else np.int32).copy()).cuda()
        h.sort(dk, dv)
        rk, rv = sort16_reference(bits, vals, kt, desc)
    last = _note(h, entry, n)
    where = f"{entry} n={n} kt={kt} desc={desc} rank={last['rank_mode']}"
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), rk, err_msg=where)
    if rv is not None:
        np.testing.assert_array_equal(dv.cpu().numpy().view(rv.dtype), rv, err_msg=where)
    return last


def _random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 65536, n, dtype=np.uint16)


@pytest.mark.parametrize("entry", ENTRIES)
def test_sizes(gpu, entry):
    sizes = _sizes(entry)
    h = {d: _handle(gpu, entry, max(sizes), U16, d) for d in (False, True)}
    for i, n in enumerate(sizes):
        _run(gpu, h[bool(i & 1)], entry, _random_bits(n, 100 + i), U16, bool(i & 1), seed=i)
    for x in h.values():
        x.close()


@pytest.mark.parametrize("kt", KEY_TYPES)
@pytest.mark.parametrize("desc", (False, True))
def test_key_types_and_orders(gpu, kt, desc):
    for entry in ("keys", "pairs4", "argsort"):
        p = _plan(entry)
        sizes = (9, p["tile"] + 1, 2 * p["tile"] + 3)
        h = _handle(gpu, entry, max(sizes), kt, desc)
        for n in sizes:
            _run(gpu, h, entry, _random_bits(n, 7 * kt + n), kt, desc)
        h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ("pairs4", "pairs8", "argsort"))
def test_both_rank_modes(gpu, entry, rank):
    tile = _plan(entry)["tile"]
    sizes = (1, 65, tile - 1, tile + 1, 2 * tile + 3, 5 * tile + 77)
    for desc in (False, True):
        h = _handle(gpu, entry, max(sizes), F16, desc, rank)
        for n in sizes:
            last = _run(gpu, h, entry, _random_bits(n, 31 * rank + n), F16, desc)
            assert last["rank_mode"] == rank
            v = {"argsort": 0, "pairs4": 1, "pairs8": 2}[entry]
            assert last["forms"] & (32 << (2 * v + rank))
        # heavy ties under this ranking: two values
        bits = np.where(_random_bits(3 * tile + 5, 5) & 1, np.uint16(0x3C00), np.uint16(0xBC00)).astype(np.uint16)
        _run(gpu, h, entry, bits, F16, desc)
        h.close()


@pytest.mark.parametrize("desc", (False, True))
@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ("pairs4", "pairs8", "argsort"))
def test_ranges_of_several_tiles(gpu, entry, rank, desc):
    """Every scatter form (positions, 4- and 8-byte values; both rank modes), both orders, on ranges of two tiles with a partial last
    one: the bases that run from tile to tile, the ballot form's dummy correction, the positions of a later tile.  Uniform bits, and
    few distinct values so that every digit's base moves by a large count."""
    n = _multi_tile_sizes(entry)[0]
    h = _handle(gpu, entry, n, I16, desc, rank)
    for bits in (_random_bits(n, 77 + rank), (_random_bits(n, 78) & np.uint16(0x0303)) | np.uint16(0xFC00)):
        last = _run(gpu, h, entry, bits, I16, desc, seed=5)
        assert last["per_range"] == 2 * last["tile"] and last["rank_mode"] == rank
    h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ("pairs4", "pairs8", "argsort"))
def test_all_ones_keys_tie_with_the_dummies_of_a_partial_tile(gpu, entry, rank):
    """Real keys whose sortable bits are 0xFFFF, in the partial last tile of a range, under both ranking forms: on both bytes they share
    digit 255 with the tile's dummies and must come out in front of them, in input order.  With them 0xFF00 and 0x00FF (the tie on one
    byte only) and a key of digits below.  Three one-tile ranges with 37 elements in the last, both orders; and the size at which a
    range holds two tiles and the last one three elements, descending (the running bases and the reverse index)."""
    tile = _plan(entry)["tile"]
    pool = np.array([0xFFFF, 0xFF00, 0x00FF, 0x1234], dtype=np.uint16)
    for n, orders in ((2 * tile + 37, (False, True)), (_multi_tile_sizes(entry)[0], (True,))):
        bits = pool[np.random.default_rng(n + rank).integers(0, 4, n)]
        bits[-3:] = (0xFFFF, 0x1234, 0xFFFF)
        assert np.count_nonzero(bits[-(n % tile):] == 0xFFFF) >= 2 and 0 < n % tile < tile
        for desc in orders:
            h = _handle(gpu, entry, n, U16, desc, rank)
            assert _run(gpu, h, entry, bits, U16, desc, seed=3)["rank_mode"] == rank
            h.close()


@pytest.mark.parametrize("desc", (False, True))
def test_keys_ranges_of_several_tiles(gpu, desc):
    """Keys only above the cap: two and five tiles per range (the histogram's unrolled loop makes a second trip), partial last tile;
    uniform bits, all equal (the wave-aggregated add on every trip) and sorted input."""
    for n in _multi_tile_sizes("keys"):
        h = _handle(gpu, "keys", n, BF16, desc)
        rnd = _random_bits(n, n & 0xFFFF)
        for bits in (rnd, np.full(n, 0xBF80, dtype=np.uint16), np.sort(rnd)):
            _run(gpu, h, "keys", bits, BF16, desc)
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_distributions(gpu, entry):
    torch = _torch()
    tile = _plan(entry)["tile"]
    n = 3 * tile + 11
    for kt, desc in ((BF16, False), (I16, True)):
        h = _handle(gpu, entry, 131072, kt, desc)
        # all equal: argsort is the identity, descending n - 1 .. 0
        bits = np.full(n, 0x3F80, dtype=np.uint16)
        _run(gpu, h, entry, bits, kt, desc)
        if entry == "argsort":
            dk, dv = _dev16(bits), torch.empty(n, dtype=torch.int32, device="cuda")
            h.argsort(dk, dv)
            want = np.arange(n, dtype=np.int32)
            np.testing.assert_array_equal(dv.cpu().numpy(), want[::-1] if desc else want)
        # two values (stability under heavy ties)
        _run(gpu, h, entry, np.where(_random_bits(n, 3) & 4, np.uint16(0x8001), np.uint16(0x7FFF)).astype(np.uint16), kt, desc)
        # every bit pattern exactly once and exactly twice: the fill's inverse transform, NaN payloads, subnormals, -0
        once = np.random.default_rng(9).permutation(65536).astype(np.uint16)
        _run(gpu, h, entry, once, kt, desc)
        _run(gpu, h, entry, np.concatenate([once, once[::-1]]), kt, desc)
        # three far-apart bins at n = 1000: long runs of empty bins for the fill
        _run(gpu, h, entry, np.array([0x0003, 0x8000, 0xFFF0], dtype=np.uint16)[np.random.default_rng(4).integers(0, 3, 1000)], kt, desc)
        # already sorted and reverse sorted
        from gpusorting_amd.sort16 import sort16_reference
        srt = sort16_reference(_random_bits(n, 6), None, kt, desc)[0]
        _run(gpu, h, entry, srt, kt, desc)
        _run(gpu, h, entry, srt[::-1].copy(), kt, desc)
        h.close()


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_memory_contract(gpu, entry, fill):
    """16-byte-only aligned views with guard bands, n smaller than the allocation and odd: nothing at or behind element n changes — the
    2-byte neighbour of the last key included — and what d_pos and the scratch hold on entry does not influence the result."""
    from guard_arena import Arena
    from gpusorting_amd import _lib
    from gpusorting_amd.sort16 import sort16_reference
    lib = _lib.load()
    mode, vb = _mode(entry)
    tile = _plan(entry)["tile"]
    vdt = np.uint64 if vb == 8 else np.uint32
    for n in (1, 7, tile + 3, 2 * tile + 5):
        count = n + 21
        specs = [(2 * count, np.uint8)] + ([(2 * count, np.uint8), (count, vdt), (count, vdt)] if mode == PAIRS else [])
        arena = Arena.for_views(specs, "cuda", fill)
        dk = arena.carve(2 * count, np.uint8, 1, "keys")
        bits = _random_bits(count, n)
        arena.write(dk, bits.view(np.uint8))
        arena.live(dk, 2 * n)
        h = _handle(gpu, entry, count, F16, n % 2 == 0)
        if mode == PAIRS:
            ak = arena.carve(2 * count, np.uint8, 3, "alt_keys")
            dv = arena.carve(count, vdt, 5, "values")
            av = arena.carve(count, vdt, 7, "alt_values")
            vals = _values(count, vb, 3)
            if entry != "argsort":
                arena.write(dv, vals)   # argsort: d_pos keeps the arena's fill — it is output only
            for v in (ak, dv, av):
                arena.live(v, 2 * n if v is ak else n)
            call = lib.gs_sort16_argsort if entry == "argsort" else lib.gs_sort16_sort_pairs
            st = call(h._h, dk.data_ptr(), dv.data_ptr(), ak.data_ptr(), av.data_ptr(), n, F16, h.order, None)
        else:
            st = lib.gs_sort16_sort_keys(h._h, dk.data_ptr(), n, F16, h.order, None)
        assert st == 0
        _note(h, entry, n)
        arena.verify()
        rk, rv = sort16_reference(bits[:n], None if entry in ("keys", "argsort") else vals[:n], F16, bool(h.order))
        np.testing.assert_array_equal(arena.read(dk, np.uint16, 2 * n), rk, err_msg=f"{entry} n={n}")
        if mode == PAIRS:
            np.testing.assert_array_equal(arena.read(dv, vdt, n), rv.astype(vdt), err_msg=f"{entry} n={n}")
        h.close()


def test_error_returns(gpu):
    """GS_ERR_ARG / GS_ERR_MODE / GS_ERR_SIZE as the header lists them; a refused call writes nothing."""
    torch = _torch()
    from gpusorting_amd import _lib
    lib = _lib.load()
    n = 1000
    k = torch.full((2 * n,), 0x1234, dtype=torch.int16, device="cuda")
    v = torch.full((2 * n,), 77, dtype=torch.int32, device="cuda")
    ak = torch.full((2 * n,), 0x4321, dtype=torch.int16, device="cuda")
    av = torch.full((2 * n,), 88, dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (k, v, ak, av)]
    hk, hp, h8 = _handle(gpu, "keys", n), _handle(gpu, "pairs4", n), _handle(gpu, "pairs8", n)
    kp, vp, akp, avp = (t.data_ptr() for t in (k, v, ak, av))
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    # keys entry
    assert lib.gs_sort16_sort_keys(None, kp, n, U16, 0, None) == A
    assert lib.gs_sort16_sort_keys(hk._h, None, n, U16, 0, None) == A
    assert lib.gs_sort16_sort_keys(hk._h, kp + 2, n, U16, 0, None) == A       # element-aligned only
    for kt in (0, 1, 2, 3, 5, 10, -1):
        assert lib.gs_sort16_sort_keys(hk._h, kp, n, kt, 0, None) == A
    assert lib.gs_sort16_sort_keys(hk._h, kp, n, U16, 2, None) == A
    assert lib.gs_sort16_sort_keys(hk._h, kp, 0, U16, 0, None) == S
    assert lib.gs_sort16_sort_keys(hk._h, kp, n + 1, U16, 0, None) == S
    assert lib.gs_sort16_sort_keys(hp._h, kp, n, U16, 0, None) == M          # keys call on a pairs handle
    # pairs entry and argsort
    for call, h in ((lib.gs_sort16_sort_pairs, hp), (lib.gs_sort16_argsort, hp)):
        assert call(None, kp, vp, akp, avp, n, U16, 0, None) == A
        assert call(h._h, None, vp, akp, avp, n, U16, 0, None) == A
        assert call(h._h, kp, None, akp, avp, n, U16, 0, None) == A
        assert call(h._h, kp, vp, None, avp, n, U16, 0, None) == A
        assert call(h._h, kp, vp, akp, None, n, U16, 0, None) == A
        assert call(h._h, kp, vp + 4, akp, avp, n, U16, 0, None) == A
        assert call(h._h, kp, vp, akp + 8, avp, n, U16, 0, None) == A
        assert call(h._h, kp, vp, akp, avp, n, 2, 0, None) == A
        assert call(h._h, kp, vp, akp, avp, 0, U16, 0, None) == S
        assert call(h._h, kp, vp, akp, avp, n + 1, U16, 0, None) == S
        assert call(hk._h, kp, vp, akp, avp, n, U16, 0, None) == M           # pairs call on a keys-only handle
        # any two buffers overlapping
        assert call(h._h, kp, vp, kp + 2 * n - 16, avp, n, U16, 0, None) == A
        assert call(h._h, kp, vp, akp, vp + 4 * n - 16, n, U16, 0, None) == A
        assert call(h._h, kp, vp, akp, avp, n, U16, 0, None) == 0            # (the same arguments, disjoint, are taken)
        h.check()
        k.copy_(before[0]); v.copy_(before[1]); ak.copy_(before[2]); av.copy_(before[3])
    assert lib.gs_sort16_argsort(h8._h, kp, vp, akp, avp, n // 2, U16, 0, None) == M   # argsort needs 4-byte values
    assert lib.gs_sort16_set_rank_mode(hp._h, 2) == A
    r = (C.c_uint32 * 8)()
    assert lib.gs_sort16_last(hp._h, r, 7, None) == A and lib.gs_sort16_last(hp._h, None, 8, None) == A
    torch.cuda.synchronize()
    for t, b in zip((k, v, ak, av), before):
        assert torch.equal(t, b), "a refused call wrote to a buffer"
    for h in (hk, hp, h8):
        h.close()


def test_the_32_bit_entries_still_refuse_16_bit_key_types(gpu):
    torch = _torch()
    from gpusorting_amd import _lib
    lib = _lib.load()
    s = gpu.OneSweep(1024)
    k = torch.zeros(1024, dtype=torch.int32, device="cuda")
    a = torch.zeros(1024, dtype=torch.int32, device="cuda")
    for kt in KEY_TYPES:
        assert lib.gs_onesweep_sort_keys(s._h, k.data_ptr(), a.data_ptr(), 1024, kt, 0, None) == _lib.GS_ERR_ARG
    s.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_call_twice_on_one_handle(gpu, entry):
    """Different n on one handle, larger then smaller then larger: the state is reset by every call."""
    tile = _plan(entry)["tile"]
    h = _handle(gpu, entry, 6 * tile, BF16, True)
    for i, n in enumerate((5 * tile + 9, 3, 2 * tile + 1, 5 * tile + 9)):
        _run(gpu, h, entry, _random_bits(n, 50 + i), BF16, True)
        assert h.status() == 0
    h.close()


def test_graph_capture(gpu):
    """One keys call and one argsort call captured into a graph, replayed on fresh input."""
    torch = _torch()
    from gpusorting_amd.sort16 import sort16_reference
    n = 3 * 8192 + 77
    hk, ha = _handle(gpu, "keys", n, F16, False), _handle(gpu, "argsort", n, F16, True)
    dk, da = _dev16(_random_bits(n, 1)), _dev16(_random_bits(n, 2))
    pos = torch.empty(n, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hk.sort(dk)            # warm-up outside the capture (and the argsort's alt buffers are allocated here)
        ha.argsort(da, pos)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hk.sort(dk)
        ha.argsort(da, pos)
    for seed in (11, 12):
        a, b = _random_bits(n, seed), _random_bits(n, seed + 100)
        dk.copy_(_dev16(a))
        da.copy_(_dev16(b))
        pos.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        _note(hk, "keys", n)
        _note(ha, "argsort", n)
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint16), sort16_reference(a, None, F16, False)[0])
        rk, rp = sort16_reference(b, None, F16, True)
        np.testing.assert_array_equal(da.cpu().numpy().view(np.uint16), rk)
        np.testing.assert_array_equal(pos.cpu().numpy().view(np.uint32), rp)
    hk.close()
    ha.close()


def test_tensor_convenience_layer(gpu):
    """gpusorting_amd.sort / sort_ / argsort on bfloat16, float16 and int16 tensors, unsigned=True and 8-byte values included."""
    torch = _torch()
    from gpusorting_amd.sort16 import sort16_reference
    for n in (1, 5, 40000, 70000, 1000):  # the cached handle grows and is reused
        bits = _random_bits(n, n)
        for dtype, kt in ((torch.bfloat16, BF16), (torch.float16, F16), (torch.int16, I16)):
            t = _dev16(bits).view(dtype)
            for desc in (False, True):
                out = gpu.sort(t, descending=desc)
                assert out.dtype == dtype
                rk, rp = sort16_reference(bits, None, kt, desc)
                np.testing.assert_array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), rk, err_msg=f"n={n} {dtype} desc={desc}")
                perm = gpu.argsort(t, descending=desc)
                assert perm.dtype == torch.int32
                np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), rp)
                np.testing.assert_array_equal(t.view(torch.int16).cpu().numpy().view(np.uint16), bits)  # the input is not written
        t = _dev16(bits)
        vals = torch.arange(n, dtype=torch.int64, device="cuda")
        k2, v2 = gpu.sort(t, vals, unsigned=True)
        rk, rp = sort16_reference(bits, None, U16, False)
        np.testing.assert_array_equal(k2.cpu().numpy().view(np.uint16), rk)
        np.testing.assert_array_equal(v2.cpu().numpy().astype(np.uint32), rp)
        np.testing.assert_array_equal(gpu.argsort(t, unsigned=True).cpu().numpy().view(np.uint32), rp)
        v4 = torch.arange(n, dtype=torch.int32, device="cuda")
        k3 = t.clone()
        gpu.sort_(k3, v4, descending=True)       # in place, int16 keys, 4-byte values
        rk, rp = sort16_reference(bits, None, I16, True)
        np.testing.assert_array_equal(k3.cpu().numpy().view(np.uint16), rk)
        np.testing.assert_array_equal(v4.cpu().numpy().view(np.uint32), rp)
    with pytest.raises(ValueError):
        gpu.sort(torch.zeros((4, 4), dtype=torch.float16, device="cuda"))
    with pytest.raises(TypeError):
        gpu.sort(torch.zeros(8, dtype=torch.float16, device="cuda"), torch.zeros(8, dtype=torch.int16, device="cuda"))


def test_zz_every_compiled_kernel_form_was_reached(gpu):
    """The forms this build compiles: histogram, scan, fill; count, pairs scan; the scatter for positions made in registers, 4- and
    8-byte values, each in both rank modes.  gs_sort16_last reports the forms a call launched; their union over this file's cases must
    be all of them (run the whole file: this test stands last)."""
    from gpusorting_amd.sort16 import SORT16_FORMS
    from gpusorting_amd import _lib
    assert len(SORT16_FORMS) == 11 and sum(SORT16_FORMS.values()) == _lib.GS_SORT16_F_ALL
    missing = [name for name, bit in SORT16_FORMS.items() if not _FORMS_SEEN[0] & bit]
    assert not missing, f"kernel forms no case of this file reached: {missing}"
