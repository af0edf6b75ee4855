"""The segmented sort (gs_segsort_*, gpusorting_amd/csrc/segsort_kernels.hpp) on the GPU: every case compares keys AND values bit
for bit with gpusorting_amd.segmented_sort_reference (itself checked against the oracle in tests/test_segsort_cpu.py), with
value = index so that stability is visible, and calls check().  Keys come from init_random with seeds, entropy presets 1 and 5
(preset 5 gives the duplicates).  Stands in for the reference's TestAllRandomSegmentLengths / TestAllFixedSegmentLengths
(GPUSortingCUDA/SegSort/SplitSort/SplitSortVariantTests.cuh)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
LDS_LIMIT = {0: 32768, 4: 16384, 8: 8192}
# upper length bound of every class below the long one, by value width (gs_segsort_class_of)
CLASS_BOUNDS = {0: (1, 32, 256, 1024, 2048, 8192, 16384, 32768), 4: (1, 32, 256, 1024, 2048, 8192, 16384), 8: (1, 32, 256, 1024, 2048, 8192)}


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()


def _keys(gpu, n, seed, preset):
    """n keys of InitRandom on the device, as a host uint32 array."""
    torch = _torch()
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.init_random(dk, seed, preset)
    torch.cuda.synchronize()
    return dk.cpu().numpy().view(np.uint32).copy()


def _offsets(lengths, head=0):
    return (head + np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])).astype(np.uint32)


def _run(gpu, keys, offsets, vb=0, key_type=0, descending=False, max_segment_len=0, sorter=None, expect_status=0, reference=None):
    """Sorts on the GPU, compares with the reference (or `reference`, a (keys, values) pair), returns the sorter's class counts."""
    n = keys.size
    vals = np.arange(n, dtype=VALUE_DTYPE[vb]) if vb else None
    s = sorter or gpu.SegmentedSort(n, offsets.size - 1, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type,
                                    gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)
    dk, do = _dev(keys), _dev(offsets)
    dv = _dev(vals) if vb else None
    s.sort(dk, do, dv, max_segment_len=max_segment_len)
    assert s.status() == expect_status
    classes = s.last_classes()
    if sorter is None:
        s.close()
    ok = dk.cpu().numpy().view(np.uint32)
    ov = dv.cpu().numpy().view(VALUE_DTYPE[vb]) if vb else None
    if reference is None:
        reference = gpu.segmented_sort_reference(keys, offsets, vals, key_type, descending)
        if not vb:
            reference = (reference, None)
    np.testing.assert_array_equal(ok, reference[0])
    if vb:
        np.testing.assert_array_equal(ov, reference[1])
    return classes


@pytest.mark.parametrize("vb", [0, 4, 8])
def test_fixed_lengths(gpu, vb):
    lengths = {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, LDS_LIMIT[vb]}
    for b in CLASS_BOUNDS[vb]:
        lengths |= {b - 1, b, b + 1}
    total = 1 << 20
    for i, length in enumerate(sorted(lengths)):
        count = max(total // max(length, 1), 3) if length else 1 << 16
        n = max(count * length, 1)
        for preset in (gpu.ENTROPY_PRESET_1, gpu.ENTROPY_PRESET_5):
            keys = _keys(gpu, n, 100 + i, preset)
            promise = max(length, 1) if length <= LDS_LIMIT[vb] else 0  # (limit + 1 is the long class: no promise fits it)
            classes = _run(gpu, keys, _offsets([length] * count), vb, max_segment_len=promise)
            assert sum(classes["counts"]) == count and classes["longest"] == length


@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("max_len", [32, 256, 2048, 8192, "lds-limit"])
def test_random_lengths(gpu, vb, max_len):
    """TestAllRandomSegmentLengths: lengths uniform in [0, max], total 2^22."""
    max_len = LDS_LIMIT[vb] if max_len == "lds-limit" else max_len
    if max_len > LDS_LIMIT[vb]:
        max_len = LDS_LIMIT[vb]
    total = 1 << 22
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed * 7919 + max_len)
        lengths = rng.integers(0, max_len + 1, size=2 * total // max_len + 64)
        lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), total))]
        offsets = _offsets(lengths)
        keys = _keys(gpu, int(offsets[-1]), seed, gpu.ENTROPY_PRESET_5 if seed == 2 else gpu.ENTROPY_PRESET_1)
        _run(gpu, keys, offsets, vb, descending=seed == 3, max_segment_len=max_len if seed != 1 else 0)


def test_random_lengths_max_32_at_2_pow_27(gpu):
    """The reference's own shipping case: 2^27 elements, lengths uniform in [0, 32]; keys-only and 4-byte values."""
    total = 1 << 27
    rng = np.random.default_rng(27)
    lengths = rng.integers(0, 33, size=total // 16 + (1 << 16))
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), total))]
    offsets = _offsets(lengths)
    n = int(offsets[-1])
    keys = _keys(gpu, n, 27, gpu.ENTROPY_PRESET_1)
    vals = np.arange(n, dtype=np.uint32)
    ref = gpu.segmented_sort_reference(keys, offsets, vals, 0, False)
    _run(gpu, keys, offsets, 0, max_segment_len=32, reference=(ref[0], None))
    _run(gpu, keys, offsets, 4, max_segment_len=32, reference=ref)


@pytest.mark.parametrize("vb", [0, 4, 8])
def test_heavy_tailed_mix(gpu, vb):
    """Most segments below 16, a few hundred around 1000, a few at the LDS limit, three long ones; empty segments at the start, in
    the middle and at the end; every class is non-empty."""
    rng = np.random.default_rng(5 + vb)
    limit = LDS_LIMIT[vb]
    parts = [rng.integers(0, 16, size=20000), rng.integers(900, 1100, size=300), [limit] * 3, [limit + 1, (1 << 20) + 5, 3 << 22]]
    parts += [[b] for b in CLASS_BOUNDS[vb]] + [[40, 200, 1500, 5000]] + ([[12000]] if vb != 8 else []) + ([[20000]] if vb == 0 else [])
    lengths = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    rng.shuffle(lengths)
    mid = lengths.size // 2
    lengths = np.concatenate([np.zeros(5, dtype=np.int64), lengths[:mid], np.zeros(1000, dtype=np.int64), lengths[mid:], np.zeros(7, dtype=np.int64)])
    offsets = _offsets(lengths, head=3)
    n = int(offsets[-1]) + 2
    keys = _keys(gpu, n, 77, gpu.ENTROPY_PRESET_1)
    for descending in (False, True):
        classes = _run(gpu, keys, offsets, vb, descending=descending, max_segment_len=0)
        assert sum(classes["counts"]) == lengths.size
        expected = [c for c in range(9) if c == 8 or c < len(CLASS_BOUNDS[vb])]
        assert all(classes["counts"][c] > 0 for c in expected), classes
        assert classes["counts"][8] == 3 and classes["longest"] == 3 << 22


@pytest.mark.parametrize("key_type", [0, 1, 2])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("vb", [0, 4, 8])
def test_types_orders_and_value_widths(gpu, key_type, descending, vb):
    rng = np.random.default_rng(11)
    lengths = np.concatenate([rng.integers(0, 40, size=5000), rng.integers(0, 300, size=1000), rng.integers(0, 3000, size=100),
                              [LDS_LIMIT[vb], LDS_LIMIT[vb] + 3, 8192, 0, 1]])
    rng.shuffle(lengths)
    offsets = _offsets(lengths)
    n = int(offsets[-1])
    for preset in (gpu.ENTROPY_PRESET_1, gpu.ENTROPY_PRESET_5):
        keys = _keys(gpu, n, 31 + key_type, preset)
        if key_type == 2:  # -0 / +0, infinities and NaN patterns of both signs among the floats
            specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0xFFFFFFFF], dtype=np.uint32)
            where = rng.integers(0, 4, size=n) == 0
            keys[where] = specials[rng.integers(0, specials.size, size=int(where.sum()))]
        _run(gpu, keys, offsets, vb, key_type, descending)


@pytest.mark.parametrize("vb", [0, 4])
def test_head_and_tail_are_not_touched(gpu, vb):
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 500, size=2000)
    head, tail = 1001, 777
    offsets = _offsets(lengths, head=head)
    n = int(offsets[-1]) + tail
    keys = _keys(gpu, n, 9, gpu.ENTROPY_PRESET_1)
    keys[:head] = np.arange(head, 0, -1, dtype=np.uint32) | np.uint32(0xABC00000)  # descending patterns: any sort would move them
    keys[n - tail:] = np.arange(tail, 0, -1, dtype=np.uint32) | np.uint32(0xDEF00000)
    _run(gpu, keys, offsets, vb)   # (the reference leaves head and tail as they are)
    _run(gpu, keys, offsets, vb, max_segment_len=499)


@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("n", [1000, "lds-limit", (1 << 24) + 12345])
def test_one_segment_covering_everything(gpu, vb, n):
    """num_segments = 1: equals gs_onesweep_sort_* on the same data."""
    n = LDS_LIMIT[vb] if n == "lds-limit" else n
    keys = _keys(gpu, n, 5, gpu.ENTROPY_PRESET_1)
    vals = np.arange(n, dtype=VALUE_DTYPE[vb]) if vb else None
    for descending in (False, True):
        one = gpu.OneSweep(n, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, 0, gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)
        dk, dv = _dev(keys), (_dev(vals) if vb else None)
        one.sort(dk, dv)
        one.check()
        ref = (dk.cpu().numpy().view(np.uint32), dv.cpu().numpy().view(VALUE_DTYPE[vb]) if vb else None)
        one.close()
        _run(gpu, keys, _offsets([n]), vb, descending=descending, reference=ref)
        _run(gpu, keys, _offsets([n]), vb, descending=descending)


def test_all_segments_empty_and_single_element(gpu):
    keys = _keys(gpu, 4096, 1, gpu.ENTROPY_PRESET_1)
    for vb in (0, 4):
        classes = _run(gpu, keys, np.full(1001, 77, dtype=np.uint32), vb)
        assert classes["counts"][0] == 1000 and classes["longest"] == 0
        _run(gpu, keys, np.zeros(2, dtype=np.uint32), vb, max_segment_len=32)
        _run(gpu, keys[:1], np.array([0, 1], dtype=np.uint32), vb)
        _run(gpu, keys[:1], np.array([0, 1], dtype=np.uint32), vb, max_segment_len=1)


@pytest.mark.parametrize("vb", [0, 4])
def test_promise_broken(gpu, vb):
    """max_segment_len = 64 with one segment of 65: GS_ERR_SIZE, every other segment sorted, that one unchanged."""
    from gpusorting_amd import _lib
    rng = np.random.default_rng(64)
    lengths = rng.integers(0, 65, size=3000)
    lengths[1234] = 65
    offsets = _offsets(lengths)
    n = int(offsets[-1])
    keys = _keys(gpu, n, 64, gpu.ENTROPY_PRESET_1)
    vals = np.arange(n, dtype=VALUE_DTYPE[vb]) if vb else None
    rk = gpu.segmented_sort_reference(keys, offsets, vals)
    rk, rv = rk if vb else (rk, None)
    a, b = int(offsets[1234]), int(offsets[1235])
    rk[a:b] = keys[a:b]
    if vb:
        rv[a:b] = vals[a:b]
    _run(gpu, keys, offsets, vb, max_segment_len=64, expect_status=_lib.GS_ERR_SIZE, reference=(rk, rv))


@pytest.mark.parametrize("bad", ["decreasing-pair", "last-beyond-n"])
def test_bad_offsets_write_nothing(gpu, bad):
    """The offsets are validated on the device before anything is loaded through them: GS_ERR_ARG, keys and values untouched; a good
    call on the same handle succeeds afterwards (every call resets the status word)."""
    from gpusorting_amd import _lib
    rng = np.random.default_rng(8)
    lengths = np.concatenate([rng.integers(0, 300, size=4000), [5000, 16000]])
    rng.shuffle(lengths)
    good = _offsets(lengths)
    n = int(good[-1])
    offsets = good.copy()
    if bad == "decreasing-pair":
        offsets[2000] = offsets[1999] - 1 if offsets[1999] > 0 else 0
        assert offsets[2000] < offsets[1999]
    else:
        offsets[-1] = n + 1
    keys = _keys(gpu, n, 8, gpu.ENTROPY_PRESET_1)
    vals = np.arange(n, dtype=np.uint32)
    for max_segment_len in (0, 16384):
        s = gpu.SegmentedSort(n, offsets.size - 1, mode=gpu.MODE_PAIRS, value_bytes=4)
        _run(gpu, keys, offsets, 4, max_segment_len=max_segment_len, sorter=s, expect_status=_lib.GS_ERR_ARG, reference=(keys, vals))
        _run(gpu, keys, good, 4, max_segment_len=max_segment_len, sorter=s)
        s.close()


@pytest.mark.parametrize("vb", [0, 4])
def test_graph_capture_with_a_fitting_promise(gpu, vb):
    """With a fitting max_segment_len the call has no host round trip: it can be captured (a captured host wait fails the capture),
    and the graph replays on fresh data."""
    torch = _torch()
    rng = np.random.default_rng(21)
    lengths = np.concatenate([rng.integers(0, 100, size=20000), rng.integers(0, 4000, size=200), [LDS_LIMIT[vb]]])
    rng.shuffle(lengths)
    offsets = _offsets(lengths)
    n = int(offsets[-1])
    s = gpu.SegmentedSort(n, offsets.size - 1, mode=gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, value_bytes=vb)
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    dv = torch.empty(n, dtype=torch.int32, device="cuda") if vb else None
    do = _dev(offsets)
    vals = np.arange(n, dtype=np.uint32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.sort(dk, do, dv, max_segment_len=LDS_LIMIT[vb])  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.sort(dk, do, dv, max_segment_len=LDS_LIMIT[vb])
    for seed in (1, 2):
        keys = _keys(gpu, n, 40 + seed, gpu.ENTROPY_PRESET_1)
        dk.copy_(_dev(keys))
        if vb:
            dv.copy_(_dev(vals))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        s.check()
        ref = gpu.segmented_sort_reference(keys, offsets, vals if vb else None)
        rk, rv = ref if vb else (ref, None)
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), rk)
        if vb:
            np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), rv)
    s.close()


def test_functional_layer(gpu):
    torch = _torch()
    rng = np.random.default_rng(2)
    lengths = np.concatenate([rng.integers(0, 200, size=3000), [40000, 0, 1]])
    rng.shuffle(lengths)
    offsets = _offsets(lengths, head=4)
    n = int(offsets[-1]) + 4
    do = _dev(offsets)
    for dtype, key_type in ((torch.int32, 1), (torch.float32, 2)):
        raw = _keys(gpu, n, 12, gpu.ENTROPY_PRESET_1)
        keys = _dev(raw).view(dtype)
        for descending in (False, True):
            rk, rv = gpu.segmented_sort_reference(raw, offsets, np.arange(n, dtype=np.uint32), key_type, descending)
            out = gpu.segmented_sort(keys, do, descending=descending)
            np.testing.assert_array_equal(out.view(torch.int32).cpu().numpy().view(np.uint32), rk)
            np.testing.assert_array_equal(keys.view(torch.int32).cpu().numpy().view(np.uint32), raw)  # out of place
            perm = gpu.segmented_argsort(keys, do, descending=descending)
            np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), rv)
            assert torch.equal(keys.view(torch.int32)[perm.long()], out.view(torch.int32))
            ok, ov = gpu.segmented_sort(keys, do, torch.arange(n, dtype=torch.int64, device="cuda"), descending=descending, max_segment_len=40000)
            np.testing.assert_array_equal(ov.cpu().numpy().astype(np.uint32), rv)
            inplace = keys.clone()
            gpu.segmented_sort_(inplace, do, descending=descending)
            assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))
    # uint32 keys in int32 storage
    raw = _keys(gpu, n, 13, gpu.ENTROPY_PRESET_1)
    out = gpu.segmented_sort(_dev(raw), do, unsigned=True)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), gpu.segmented_sort_reference(raw, offsets))
