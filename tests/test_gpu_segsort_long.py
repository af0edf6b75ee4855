"""GPU tests of the segmented sort's device route for long 32-bit segments (gs_segsort_set_long_route(h, GS_SEGSORT_LONG_DEVICE) in
include/gpusort.h; segsort_long_kernels.hpp): a work list built on the device, then four passes of count, scan, scatter over all long
segments at once, with no host wait.  Every result is compared bit for bit with segmented_sort_reference, the numpy statement of the
semantics, over the WHOLE array (the elements in front of the first and behind the last offset are guards of every case), and with the
host route on the same handle and input.  After every call gs_segsort_check is GS_OK, gs_segsort_last reports the unit count computed
here, and gs_segsort_last_classes is the same on both routes.  The last test asserts that the cases of this file reached every kernel
form of the route (gs_segsort_last's forms word)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32, I32, F32 = 0, 1, 2
KEYS, PAIRS = 0, 1
ENTRIES = ("keys", "pairs4", "pairs8")
_FORMS_SEEN = [0]   # union of SegmentedSort.last()["forms"] over the file's cases


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
    return _lib.GS_SEGSORT_LONG_PART


def _tile():
    from gpusorting_amd import _lib
    return _lib.GS_SORT_ROWS_TILE


def _values(n, vb):
    """value = array index (8 bytes: spread over both halves, a high bit on top): equal keys must come out in rising index."""
    idx = np.arange(n, dtype=np.uint32)
    return idx if vb == 4 else idx.astype(np.uint64) * np.uint64(0x100000001) | np.uint64(1 << 63)


def _offsets(lens, front=0):
    return (front + np.concatenate(([0], np.cumsum(np.asarray(lens, dtype=np.int64))))).astype(np.uint32)


def _edge_lengths(entry):
    lds, part, tile = _lds(entry), _part(), _tile()
    return [5, lds + 1, 300, part, 1, part + 1, 0, part + tile + 9, 2 * part + 1, 40, lds]


def _units(entry, lens, max_len=0):
    lds, part = _lds(entry), _part()
    return sum(-(-int(x) // part) for x in lens if x > lds and not (max_len and x > max_len))


def _handle(gpu, entry, max_keys, max_segments, kt=U32, desc=False, rank=None, long_route="device"):
    mode, vb = _mode(entry)
    h = gpu.SegmentedSort(max_keys, max_segments, order=1 if desc else 0, key_type=kt, mode=mode, value_bytes=vb, long_route=long_route)
    assert h.long_route == long_route
    if rank is not None:
        h.engine.set_rank_mode(rank)
        assert h.engine.rank_mode == rank
    return h


def _note(h, entry, offsets, n, max_len=0, status=0):
    """gs_segsort_check and gs_segsort_last agree with the lengths and the route; the forms word joins the file's union."""
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort import segsort_long_units
    lens = np.diff(offsets.astype(np.int64))
    assert h.status() == status
    last = h.last()
    lds = _lds(entry)
    device = h.long_route == "device"
    assert last["route"] == (1 if device else 0) and last["n"] == n and last["rank"] == h.engine.rank_mode, last
    assert last["long"] == sum(1 for x in lens if x > lds and not (max_len and x > max_len)), last
    assert last["status"] == (2 if status == _lib.GS_ERR_SIZE else 0), last
    ran = device and (max_len == 0 or max_len > lds) and n > lds
    assert last["units"] == (_units(entry, lens, max_len) if ran else 0), last
    assert last["unit_cap"] == (segsort_long_units(n, len(lens), *_mode(entry)) if ran else 0) and last["units"] <= last["unit_cap"], last
    assert bool(last["forms"] & _lib.GS_SEGSORT_LF_UNITS) == ran and (device or last["forms"] == 0), last
    _FORMS_SEEN[0] |= last["forms"]
    return last


def _run(h, entry, bits, offsets, kt, desc, max_len=0, host_too=True):
    """One device-route call on fresh device copies of the uint32 array `bits`, compared with the reference over the whole array and, on
    the same handle and input, with the host route."""
    torch = _torch()
    from gpusorting_amd.segsort import segmented_sort_reference
    n, vb = bits.size, _mode(entry)[1]
    vals = _values(n, vb) if vb else None
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    got = {}
    for route in (("device", "host") if host_too else ("device",)):
        h.set_long_route(route)
        dk = torch.from_numpy(bits.view(np.int32).copy()).cuda()
        dv = None if vals is None else torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()).cuda()
        h.sort(dk, do, dv, max_segment_len=max_len)
        last = _note(h, entry, offsets, n, max_len)
        got[route] = (dk.cpu().numpy().view(np.uint32), None if dv is None else dv.cpu().numpy().view(vals.dtype), h.last_classes(), last)
    h.set_long_route("device")
    where = f"{entry} n={n} segments={offsets.size - 1} kt={kt} desc={desc} rank={got['device'][3]['rank']} units={got['device'][3]['units']}"
    ref = segmented_sort_reference(bits, offsets, vals, kt, desc)
    rk, rv = ref if vb else (ref, None)
    np.testing.assert_array_equal(got["device"][0], rk, err_msg=where)
    if vb:
        np.testing.assert_array_equal(got["device"][1], rv, err_msg=where)
    if host_too:
        np.testing.assert_array_equal(got["host"][0], got["device"][0], err_msg="host route: " + where)
        if vb:
            np.testing.assert_array_equal(got["host"][1], got["device"][1], err_msg="host route: " + where)
        assert got["host"][2] == got["device"][2], "last_classes differs between the routes"
    np.testing.assert_array_equal(do.cpu().numpy().view(np.uint32), offsets, err_msg="the offsets were written")
    return got["device"][3]


def _random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


# ±0, ±inf, quiet and signalling NaNs of both signs, the all-one pattern, subnormals, ±1, the extremes
_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0xFFFFFFFF, 0x7FFFFFFF,
                      0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)


def _float_bits(n, seed):
    """Uniform bit patterns with the special values strewn in, each many times."""
    rng = np.random.default_rng(seed)
    bits = _random_bits(n, seed)
    hit = rng.random(n) < 0.25
    bits[hit] = _SPECIALS[rng.integers(0, _SPECIALS.size, int(hit.sum()))]
    return bits


@pytest.mark.parametrize("entry", ENTRIES)
def test_edges_of_the_cut(gpu, entry):
    """The LDS limit and one more, a part, a part and one, a part and a tile and nine, two parts and one, short segments in between, two
    untouched elements in front and three behind: uint32 ascending, int32 descending, float32 both orders with -0, infinities and NaNs."""
    lens = _edge_lengths(entry)
    offsets = _offsets(lens, front=2)
    n = int(offsets[-1]) + 3
    for kt, desc, bits in ((U32, False, _random_bits(n, 1)), (I32, True, _random_bits(n, 2)), (F32, False, _float_bits(n, 3)),
                           (F32, True, _float_bits(n, 4))):
        h = _handle(gpu, entry, n, len(lens), kt, desc)
        last = _run(h, entry, bits, offsets, kt, desc)
        assert last["units"] == _units(entry, lens) >= 6
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_start_residue(gpu, entry):
    """The long lengths with 0, 1, 2 and 3 elements in front: the host route needs its head merge here, the device route must not care
    (8-byte values start at odd element indices)."""
    lds, part, tile = _lds(entry), _part(), _tile()
    lens = [lds + 1, part + 1, 3, part + tile + 9, 2 * part + 1]
    for front in range(4):
        offsets = _offsets(lens, front=front)
        n = int(offsets[-1]) + 1
        h = _handle(gpu, entry, n, len(lens), F32, front % 2 == 1)
        _run(h, entry, _float_bits(n, 10 + front), offsets, F32, front % 2 == 1)
        h.close()


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("entry", ENTRIES)
def test_stability_and_the_dummies(gpu, entry, rank):
    """A segment of two distinct keys, one of them all ones (the dummies' pattern), whose partial last tile holds all-one keys only:
    the dummies must stay behind the real keys, under both rankings; and a segment of all-equal keys (the count's one-add shortcut) of
    two parts — a tile more than the LDS limit where two parts still fit LDS, so that it takes the long route for every entry.
    Values are positions, so the comparison with the stable reference is the stability check."""
    lds, part, tile = _lds(entry), _part(), _tile()
    assert lds % tile == 0
    lens = [lds + tile // 2 + 3, 7, max(2 * part, lds + tile)]
    offsets = _offsets(lens, front=1)
    n = int(offsets[-1]) + 2
    rng = np.random.default_rng(20 + rank)
    bits = _random_bits(n, 21)
    a = int(offsets[0])
    bits[a:a + lens[0]] = np.where(rng.random(lens[0]) < 0.5, 0xFFFFFFFF, 0x00C0FFEE).astype(np.uint32)
    bits[a + lds:a + lens[0]] = 0xFFFFFFFF
    b = int(offsets[2])
    bits[b:b + lens[2]] = 0x3F800000
    for desc in (False, True):
        h = _handle(gpu, entry, n, len(lens), U32, desc, rank)
        last = _run(h, entry, bits, offsets, U32, desc)
        assert last["rank"] == rank
        h.close()


def test_more_long_segments_than_the_read_back_chunk(gpu):
    """1100 long segments just above the LDS limit with 8-byte values: more than the host route reads back at a time, one launch
    sequence on the device route."""
    lds = _lds("pairs8")
    lens = [lds + 1 + i % 9 for i in range(1100)]
    offsets = _offsets(lens, front=1)
    n = int(offsets[-1]) + 1
    h = _handle(gpu, "pairs8", n, len(lens), U32, False)
    last = _run(h, "pairs8", _random_bits(n, 30), offsets, U32, False, host_too=False)
    assert last["long"] == 1100 and last["units"] == 1100
    h.close()


def _raw_call(lib, h, entry, dk, dv, ak, av, n, do, segs, max_len, kt, order):
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    if entry == "keys":
        return lib.gs_segsort_sort_keys(h._h, ptr(dk), ptr(ak), n, ptr(do), segs, max_len, kt, order, None)
    return lib.gs_segsort_sort_pairs(h._h, ptr(dk), ptr(dv), ptr(ak), ptr(av), n, ptr(do), segs, max_len, kt, order, None)


def test_status(gpu):
    """Decreasing offsets: GS_ERR_ARG from the check and nothing written, the alternates included.  A segment longer than promised is left
    unsorted with GS_ERR_SIZE while every other one, long ones among them, is sorted.  Overlapping buffers and a NULL alternate where long
    segments are allowed are refused by the call itself."""
    torch = _torch()
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort import segmented_sort_reference
    lib = _lib.load()
    for entry in ENTRIES:
        lds, vb = _lds(entry), _mode(entry)[1]
        vdt = torch.int64 if vb == 8 else torch.int32
        lens = [5, 300, lds + 50, 40, lds + 200, 2000, lds + 100]
        good = _offsets(lens, front=1)
        n = int(good[-1]) + 2
        bits = _random_bits(n, 40)
        vals = _values(n, vb) if vb else None
        h = _handle(gpu, entry, n, len(lens), I32)

        def fresh():
            dk = torch.from_numpy(bits.view(np.int32).copy()).cuda()
            dv = None if vals is None else torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()).cuda()
            ak = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            av = None if vals is None else torch.full((n,), 77, dtype=vdt, device="cuda")
            return dk, dv, ak, av

        def untouched(dk, dv, ak, av):
            torch.cuda.synchronize()
            np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), bits)
            assert (ak == 0x5A5A5A5A).all()
            if vb:
                np.testing.assert_array_equal(dv.cpu().numpy().view(vals.dtype), vals)
                assert (av == 77).all()

        # decreasing offsets
        down = good.copy()
        down[2] = down[1] - 1
        do = torch.from_numpy(down.view(np.int32).copy()).cuda()
        dk, dv, ak, av = fresh()
        assert _raw_call(lib, h, entry, dk, dv, ak, av, n, do, len(lens), 0, I32, 0) == 0
        assert h.status() == _lib.GS_ERR_ARG
        last = h.last()
        assert last["status"] & 1 and last["units"] == 0 and last["route"] == 1
        _FORMS_SEEN[0] |= last["forms"]
        untouched(dk, dv, ak, av)
        # a promise of lds + 100 with one segment of lds + 200
        do = torch.from_numpy(good.view(np.int32).copy()).cuda()
        dk, dv, ak, av = fresh()
        assert _raw_call(lib, h, entry, dk, dv, ak, av, n, do, len(lens), lds + 100, I32, 0) == 0
        _note(h, entry, good, n, lds + 100, status=_lib.GS_ERR_SIZE)
        ref = segmented_sort_reference(bits, good, vals, I32, False)
        rk, rv = ref if vb else (ref, None)
        a = int(good[4])
        rk[a:a + lens[4]] = bits[a:a + lens[4]]
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), rk, err_msg=entry)
        if vb:
            rv[a:a + lens[4]] = vals[a:a + lens[4]]
            np.testing.assert_array_equal(dv.cpu().numpy().view(vals.dtype), rv, err_msg=entry)
        # overlapping keys / alternate keys: refused on the device route, nothing written
        dk, dv, ak, av = fresh()
        big = torch.from_numpy(np.concatenate((bits, bits)).view(np.int32).copy()).cuda()
        inside = big.data_ptr() + (4 * n - 16) // 16 * 16    # an aligned address inside the last 16 bytes of [0, n)
        assert _raw_call(lib, h, entry, big, dv, inside, av, n, do, len(lens), 0, I32, 0) == _lib.GS_ERR_ARG
        torch.cuda.synchronize()
        np.testing.assert_array_equal(big.cpu().numpy().view(np.uint32), np.concatenate((bits, bits)))
        if vb:
            assert _raw_call(lib, h, entry, dk, dv, ak, dv.data_ptr() + (vb * n - 16) // 16 * 16, n, do, len(lens), 0, I32, 0) == _lib.GS_ERR_ARG
        # a NULL alternate where long segments are allowed
        assert _raw_call(lib, h, entry, dk, dv, None, av, n, do, len(lens), 0, I32, 0) == _lib.GS_ERR_ARG
        assert _raw_call(lib, h, entry, dk, dv, None, av, n, do, len(lens), lds + 1, I32, 0) == _lib.GS_ERR_ARG
        untouched(dk, dv, ak, av)
        # a promise within LDS needs no alternates and keeps the long launches off
        assert _raw_call(lib, h, entry, dk, dv, None, None, n, do, len(lens), lds, I32, 0) == 0
        _note(h, entry, good, n, lds, status=_lib.GS_ERR_SIZE)
        # unknown routes are refused and change nothing
        assert lib.gs_segsort_set_long_route(h._h, 2) == _lib.GS_ERR_ARG and h.long_route == "device"
        h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_handle_alternating(gpu, entry):
    """Host, device, host, device on different offsets — long segments, none, long segments again — the state is reset by every call."""
    torch = _torch()
    from gpusorting_amd.segsort import segmented_sort_reference
    lds, part, vb = _lds(entry), _part(), _mode(entry)[1]
    sets = ([3, lds + part + 9, 300, lds + 1], [7, 300, 33, 2000, 1], [lds + 5, 5, 2 * part + 1, 0, 40], [100] * 50)
    h = _handle(gpu, entry, max(sum(lens) for lens in sets) + 16, 64, F32, True, long_route="host")
    for i, lens in enumerate(sets + sets[:2]):
        offsets = _offsets(lens, front=i)
        n = int(offsets[-1]) + i
        bits = _float_bits(n, 50 + i)
        vals = _values(n, vb) if vb else None
        h.set_long_route(("host", "device")[i % 2])
        dk = torch.from_numpy(bits.view(np.int32).copy()).cuda()
        dv = None if vals is None else torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()).cuda()
        do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
        h.sort(dk, do, dv)
        _note(h, entry, offsets, n)
        ref = segmented_sort_reference(bits, offsets, vals, F32, True)
        rk, rv = ref if vb else (ref, None)
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), rk, err_msg=f"{entry} call {i}")
        if vb:
            np.testing.assert_array_equal(dv.cpu().numpy().view(vals.dtype), rv, err_msg=f"{entry} call {i}")
    h.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_graph_capture(gpu, entry):
    """A device-route call with max_segment_len = 0 and long segments present, captured once into a graph on one linear stream, replayed
    on new keys and once after the offsets were rewritten in place to other lengths (same n, same number of segments): no host wait,
    whatever the segment lengths.  The elements outside the segments keep their fill."""
    torch = _torch()
    from gpusorting_amd.segsort import segmented_sort_reference
    lens = _edge_lengths(entry)
    other = lens[::-1]
    offsets = _offsets(lens, front=2)
    n = int(offsets[-1]) + 3
    vb = _mode(entry)[1]
    h = _handle(gpu, entry, n, len(lens), F32, True)
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    dv = None if not vb else torch.empty(n, dtype=torch.int64 if vb == 8 else torch.int32, device="cuda")
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    vals = _values(n, vb) if vb else None

    def load(seed):
        bits = _float_bits(n, seed)
        bits[:2] = 0xDEADBEEF
        bits[int(offsets[-1]):] = 0xDEADBEEF
        dk.copy_(torch.from_numpy(bits.view(np.int32).copy()))
        if vb:
            dv.copy_(torch.from_numpy(vals.view(np.int64 if vb == 8 else np.int32).copy()))
        return bits

    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.sort(dk, do, dv)            # warm-up outside the capture (the alt buffers are allocated here)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    load(2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.sort(dk, do, dv)
    for seed, off_lens in ((11, lens), (12, lens), (13, other)):
        offs = _offsets(off_lens, front=2)
        assert int(offs[-1]) == int(offsets[-1])
        do.copy_(torch.from_numpy(offs.view(np.int32).copy()))
        bits = load(seed)
        graph.replay()
        torch.cuda.synchronize()
        last = _note(h, entry, offs, n)
        assert last["units"] == _units(entry, off_lens) >= 6
        ref = segmented_sort_reference(bits, offs, vals, F32, True)
        rk, rv = ref if vb else (ref, None)
        got = dk.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, rk)
        assert (got[:2] == 0xDEADBEEF).all() and (got[int(offs[-1]):] == 0xDEADBEEF).all()
        if vb:
            np.testing.assert_array_equal(dv.cpu().numpy().view(vals.dtype), rv)
    h.close()


def _hip():
    """The HIP runtime this process already runs on (the one torch loaded), for the graph calls torch does not bind."""
    import ctypes as C
    path = next((line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line), None)
    assert path, "no HIP runtime is loaded"
    return C.CDLL(path)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_captured_node_is_a_kernel_launch(gpu, entry):
    """The device-route call with max_segment_len = 0 and long segments present, captured on one stream: the graph holds kernel nodes
    only — no copy, no memset, no host node — and at least the 13 launches of the long route behind reset, classify and fill."""
    import ctypes as C
    torch = _torch()
    hip = _hip()
    lens = _edge_lengths(entry)
    offsets = _offsets(lens, front=2)
    n = int(offsets[-1]) + 3
    vb = _mode(entry)[1]
    h = _handle(gpu, entry, n, len(lens), U32, False)
    dk = torch.from_numpy(_random_bits(n, 60).view(np.int32).copy()).cuda()
    dv = None if not vb else torch.arange(n, dtype=torch.int64 if vb == 8 else torch.int32, device="cuda")
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.sort(dk, do, dv)            # warm-up outside the capture (the alt buffers are allocated here)
        side.synchronize()
        stream, graph = C.c_void_p(side.cuda_stream), C.c_void_p()
        assert hip.hipStreamBeginCapture(stream, 2) == 0          # hipStreamCaptureModeRelaxed
        try:
            h.sort(dk, do, dv)
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
    assert len(kinds) >= 3 + 13 and all(k == 0 for k in kinds), kinds    # hipGraphNodeTypeKernel = 0
    # nothing ran during the capture; the handle is as usable as before
    _run(h, entry, _random_bits(n, 61), offsets, U32, False)
    h.close()


@pytest.mark.parametrize("fill", (0x00, 0xFF, "hash"))
@pytest.mark.parametrize("entry", ENTRIES)
def test_memory_contract(gpu, entry, fill):
    """16-byte-only aligned views with guard bands, n smaller than the allocation: nothing in front of offsets[0] or at or behind
    offsets[-1] of the keys and values changes, the offsets are read-only, the alt buffers are written on [0, n) only, and what the
    scratch holds on entry does not influence the result."""
    from guard_arena import Arena
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort import segmented_sort_reference
    lib = _lib.load()
    mode, vb = _mode(entry)
    vdt = np.uint64 if vb == 8 else np.uint32
    lds = _lds(entry)
    lens = [7, 100, lds + _tile() + 3, 300, 1, _part() + 1, 33]
    offsets = _offsets(lens, front=3)
    n = int(offsets[-1]) + 3
    count = n + 21
    arena = Arena.for_views([(count, np.uint32)] * 2 + [(len(offsets), np.uint32)] + ([(count, vdt)] * 2 if mode == PAIRS else []), "cuda", fill)
    dk = arena.carve(count, np.uint32, 1, "keys")
    ak = arena.carve(count, np.uint32, 3, "alt_keys")
    do = arena.carve(len(offsets), np.uint32, 9, "offsets")
    bits = _random_bits(count, n)
    arena.write(dk, bits)
    arena.write(do, offsets)
    arena.read_only(do)
    arena.live(dk, int(offsets[-1]), int(offsets[0]))
    arena.live(ak, n)
    h = _handle(gpu, entry, count, len(lens), F32, True)
    vals = None
    if mode == PAIRS:
        dv = arena.carve(count, vdt, 5, "values")
        av = arena.carve(count, vdt, 7, "alt_values")
        vals = _values(count, vb).astype(vdt)
        arena.write(dv, vals)
        arena.live(dv, int(offsets[-1]), int(offsets[0]))
        arena.live(av, n)
        st = lib.gs_segsort_sort_pairs(h._h, dk.data_ptr(), dv.data_ptr(), ak.data_ptr(), av.data_ptr(), n, do.data_ptr(), len(lens), 0, F32, h.order, None)
    else:
        st = lib.gs_segsort_sort_keys(h._h, dk.data_ptr(), ak.data_ptr(), n, do.data_ptr(), len(lens), 0, F32, h.order, None)
    assert st == 0
    _note(h, entry, offsets, n)
    arena.verify()
    ref = segmented_sort_reference(bits[:n], offsets, None if vals is None else vals[:n], F32, True)
    rk, rv = ref if vb else (ref, None)
    np.testing.assert_array_equal(arena.read(dk, np.uint32, n), rk, err_msg=f"{entry} {lens}")
    if mode == PAIRS:
        np.testing.assert_array_equal(arena.read(dv, vdt, n), rv, err_msg=f"{entry} {lens}")
    h.close()


def test_tensor_convenience_layer(gpu):
    """gpusorting_amd.segmented_sort / segmented_sort_ / segmented_argsort with long_route="device" on int32, uint32 (unsigned=True) and
    float32 tensors against the reference and equal to long_route="host"; the default argument still takes the host route."""
    torch = _torch()
    from gpusorting_amd import functional
    from gpusorting_amd.segsort import segmented_sort_reference
    lens = [40, _lds("keys") + 100, 7, _lds("pairs4") + _part() + 5, 9000]
    offsets = _offsets(lens, front=2)
    n = int(offsets[-1]) + 3
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    bits = _float_bits(n, 70)
    for dtype, kt, unsigned in ((torch.int32, I32, False), (torch.int32, U32, True), (torch.float32, F32, False)):
        t = torch.from_numpy(bits.view(np.int32).copy()).cuda().view(dtype)
        for desc in (False, True):
            out = gpu.segmented_sort(t, do, descending=desc, unsigned=unsigned, long_route="device")
            assert out.dtype == dtype and out.shape == t.shape
            np.testing.assert_array_equal(out.view(torch.int32).cpu().numpy().view(np.uint32), segmented_sort_reference(bits, offsets, None, kt, desc))
            assert torch.equal(out.view(torch.int32), gpu.segmented_sort(t, do, descending=desc, unsigned=unsigned, long_route="host").view(torch.int32))
            perm = gpu.segmented_argsort(t, do, descending=desc, unsigned=unsigned, long_route="device")
            rk, rp = segmented_sort_reference(bits, offsets, np.arange(n, dtype=np.uint32), kt, desc)
            np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), rp)
            assert torch.equal(perm, gpu.segmented_argsort(t, do, descending=desc, unsigned=unsigned))
            assert torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(bits.view(np.int32)))   # the input is not written
        k, v8 = t.clone(), torch.arange(n, dtype=torch.int64, device="cuda")
        gpu.segmented_sort_(k, do, v8, unsigned=unsigned, long_route="device")
        rk, rv = segmented_sort_reference(bits, offsets, np.arange(n, dtype=np.int64), kt, False)
        np.testing.assert_array_equal(k.view(torch.int32).cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(v8.cpu().numpy(), rv)
        # the cached handles: one per route, and the default argument's reports the host route
        dev = functional._seg_sorter(t.device, n, len(lens), kt, 0, 8, "device")
        assert dev.long_route == "device" and dev.last()["route"] == 1 and dev.last()["units"] > 0
        _FORMS_SEEN[0] |= dev.last()["forms"]
        gpu.segmented_sort_(k, do, v8, unsigned=unsigned)
        host = functional._seg_sorter(t.device, n, len(lens), kt, 0, 8)
        assert host is not dev and host.long_route == "host" and host.last()["route"] == 0 and host.last()["forms"] == 0
    with pytest.raises(ValueError):
        gpu.segmented_sort(t, do, long_route="both")
    # 16-bit keys ignore the argument
    t16 = torch.from_numpy(bits[:5000].view(np.int16)[:5000].copy()).cuda()
    o16 = torch.tensor([0, 100, 5000], dtype=torch.int32, device="cuda")
    assert torch.equal(gpu.segmented_sort(t16, o16, long_route="device"), gpu.segmented_sort(t16, o16))


def test_zz_every_kernel_form_of_the_route_was_reached(gpu):
    """gs_segsort_last reports the kernel forms of the long route a call launched; their union over this file's cases must be all of
    them: units, count, scan and the scatter for keys only, 4- and 8-byte values under both rankings (run the whole file: this test
    stands last)."""
    from gpusorting_amd import _lib
    assert _FORMS_SEEN[0] == _lib.GS_SEGSORT_LF_ALL, hex(_FORMS_SEEN[0])
