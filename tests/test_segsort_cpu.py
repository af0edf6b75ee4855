"""CPU tests of the segmented sort's boundary (gs_segsort_* in include/gpusort.h, gpusorting_amd/segsort.py): the host-only entry
points (length classes, LDS limit, temp memory) and the numpy reference the GPU tests compare against, itself checked segment for
segment against the oracle's std_sort.  Nothing here runs on a GPU."""
import ctypes as C

import numpy as np
import pytest

KEYS_ONLY, PAIRS = 0, 1
MODES = ((KEYS_ONLY, 0, 32768), (PAIRS, 4, 16384), (PAIRS, 8, 8192))  # (mode, value bytes, longest segment sorted in LDS)


@pytest.fixture(scope="module")
def lib():
    from gpusorting_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("mode,vb,limit", MODES)
def test_max_lds_segment_and_classes(lib, mode, vb, limit):
    from gpusorting_amd import _lib
    assert lib.gs_segsort_max_lds_segment(mode, vb) == limit
    classes = [lib.gs_segsort_class_of(length, mode, vb) for length in range(0, limit + 2)]
    assert all(a <= b for a, b in zip(classes, classes[1:])), "the class is monotone in the length"
    assert classes[0] == classes[1] == 0, "lengths 0 and 1 fall in the class that does no work"
    long_class = _lib.GS_SEGSORT_CLASSES - 1
    assert max(classes[:limit + 1]) < long_class, "every length up to the limit has an LDS class"
    assert classes[limit + 1] == long_class and lib.gs_segsort_class_of(1 << 29, mode, vb) == long_class
    assert classes[2] == 1 and classes[32] == 1 and classes[33] == 2 and classes[256] == 2 and classes[257] == 3
    assert all(0 <= c < _lib.GS_SEGSORT_CLASSES for c in classes)


def test_temp_bytes_formula_and_bound(lib):
    sizes = (1 << 10, 1 << 16, 1 << 20, 1 << 24, 1 << 28, (1 << 30) - 1)
    segs = (1, 1000, 1 << 14, 1 << 20, 1 << 26)
    for i, n in enumerate(sizes):
        for j, m in enumerate(segs):
            t = lib.gs_segsort_temp_bytes(n, m)
            assert t == lib.gs_onesweep_temp_bytes(n) + 4 * m + 256, "the formula the header states"
            assert t <= lib.gs_onesweep_temp_bytes(n) + 16 * m + 64 * 1024
            if j:
                assert t > lib.gs_segsort_temp_bytes(n, segs[j - 1]), "grows with max_segments"
            if i:
                assert t >= lib.gs_segsort_temp_bytes(sizes[i - 1], m), "grows with max_keys"
    assert lib.gs_segsort_temp_bytes(sizes[-1], 1) > lib.gs_segsort_temp_bytes(sizes[0], 1)


def test_argument_errors_without_touching_the_gpu(lib):
    from gpusorting_amd import _lib
    h = C.c_void_p()
    assert lib.gs_segsort_create(None, 1024, 16, 0, 0) == _lib.GS_ERR_ARG
    assert lib.gs_segsort_create(C.byref(h), 1024, 0, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_segsort_create(C.byref(h), 0, 16, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_segsort_create(C.byref(h), 1024, 16, 0, 4) == _lib.GS_ERR_MODE
    assert lib.gs_segsort_create(C.byref(h), 1024, 16, 1, 2) == _lib.GS_ERR_MODE
    assert lib.gs_segsort_destroy(None) == _lib.GS_ERR_ARG
    assert lib.gs_segsort_check(None, None) == _lib.GS_ERR_ARG
    assert lib.gs_segsort_sort_keys(None, None, None, 4, None, 1, 0, 0, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_segsort_last_classes(None, None, 0, None) == _lib.GS_ERR_ARG


def _special_keys(rng, n, key_type):
    """Seeded keys with duplicates and, for floats, -0 / +0, infinities and NaN patterns of both signs."""
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    dup = rng.integers(0, 2, size=n) == 1
    keys[dup] &= np.uint32(0x80000007) if key_type else np.uint32(7)  # few distinct values (both signs): duplicates in every segment
    if key_type == 2:
        specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF],
                            dtype=np.uint32)
        where = rng.integers(0, 3, size=n) == 0
        keys[where] = specials[rng.integers(0, specials.size, size=int(where.sum()))]
    return keys


@pytest.mark.parametrize("key_type", [0, 1, 2])
@pytest.mark.parametrize("descending", [False, True])
def test_reference_matches_the_oracle_segment_by_segment(oracle, key_type, descending):
    from gpusorting_amd import segmented_sort_reference
    rng = np.random.default_rng(1000 + 10 * key_type + int(descending))
    lengths = np.concatenate([rng.integers(0, 40, size=300), rng.integers(0, 700, size=60), [0, 0, 1, 2, 3000]])
    rng.shuffle(lengths)
    head, tail = 5, 7
    offsets = head + np.concatenate([[0], np.cumsum(lengths)])
    n = int(offsets[-1]) + tail
    keys = _special_keys(rng, n, key_type)
    vals = np.arange(n, dtype=np.uint32)
    rk, rv = segmented_sort_reference(keys, offsets, vals, key_type, descending)
    assert rk.dtype == keys.dtype and rv.dtype == vals.dtype
    np.testing.assert_array_equal(rk[:head], keys[:head])
    np.testing.assert_array_equal(rk[n - tail:], keys[n - tail:])
    np.testing.assert_array_equal(rv[:head], vals[:head])
    np.testing.assert_array_equal(rv[n - tail:], vals[n - tail:])
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            ok, ov = oracle.std_sort(keys[a:b], key_type, 1 if descending else 0, vals[a:b])
            np.testing.assert_array_equal(rk[a:b], ok)
            np.testing.assert_array_equal(rv[a:b], ov)
    only_keys = segmented_sort_reference(keys, offsets, None, key_type, descending)
    np.testing.assert_array_equal(only_keys, rk)


def test_reference_rejects_bad_offsets():
    from gpusorting_amd import segmented_sort_reference
    keys = np.arange(10, dtype=np.uint32)
    with pytest.raises(ValueError):
        segmented_sort_reference(keys, np.array([0, 5, 4, 10]))
    with pytest.raises(ValueError):
        segmented_sort_reference(keys, np.array([0, 5, 11]))
