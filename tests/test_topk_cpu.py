"""CPU tests of the top-k selection's boundary (gs_topk_* in include/gpusort.h, gpusorting_amd/topk.py): the numpy reference the GPU
tests compare against, itself checked against the head of the oracle's std_sort, and the host-only entry points (argument errors,
the temp-memory formula and its bound against sort-and-slice).  Nothing here runs on a GPU."""
import ctypes as C

import numpy as np
import pytest

F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF,
                         0x3F800000, 0xBF800000], dtype=np.uint32)  # +0 -0 +inf -inf NaNs of both signs, +1 -1


@pytest.fixture(scope="module")
def lib():
    from gpusorting_amd import _lib
    return _lib.load()


def _against_oracle(oracle, keys, key_type, descending, ks):
    from gpusorting_amd import topk_reference
    n = keys.size
    idx = np.arange(n, dtype=np.uint32)
    ok, ov = oracle.std_sort(keys, key_type, 1 if descending else 0, idx)
    for k in ks:
        rk, rv = topk_reference(keys, k, None, key_type, descending)
        assert rk.dtype == keys.dtype and rv.dtype == np.uint32 and rk.size == k and rv.size == k
        np.testing.assert_array_equal(rk, ok[:k])
        np.testing.assert_array_equal(rv, ov[:k])
        vals = (idx.astype(np.uint64) << np.uint64(32)) | np.uint64(7)
        rk2, rv2 = topk_reference(keys, k, vals, key_type, descending)
        np.testing.assert_array_equal(rk2, ok[:k])
        np.testing.assert_array_equal(rv2, vals[ov[:k]])


@pytest.mark.parametrize("key_type", [0, 1, 2])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("preset", [1, 5])
def test_reference_is_the_head_of_the_oracles_sort(oracle, key_type, descending, preset):
    n = 50_000
    keys = oracle.init_random(n, 77 + preset, preset - 1)
    _against_oracle(oracle, keys, key_type, descending, (1, 2, 63, 1000, n // 2, n - 1, n))


@pytest.mark.parametrize("key_type", [0, 1, 2])
@pytest.mark.parametrize("descending", [False, True])
def test_reference_on_hand_made_inputs(oracle, key_type, descending):
    rng = np.random.default_rng(5)
    n = 257
    inputs = [np.full(n, 0x80000001, dtype=np.uint32),                                          # all keys equal
              np.where(rng.integers(0, 2, size=n) == 1, 0x00000005, 0xFFFF0005).astype(np.uint32),  # two distinct keys
              F32_SPECIALS[rng.integers(0, F32_SPECIALS.size, size=n)]]                         # -0 / +0 / infinities / NaNs
    for keys in inputs:
        _against_oracle(oracle, keys, key_type, descending, (1, 2, n - 1, n))


def test_reference_tie_rule_and_errors():
    from gpusorting_amd import topk_reference
    keys = np.array([3, 1, 3, 1, 3], dtype=np.uint32)
    k, v = topk_reference(keys, 3)
    assert k.tolist() == [1, 1, 3] and v.tolist() == [1, 3, 0]           # ascending: lowest positions, increasing
    k, v = topk_reference(keys, 2, descending=True)
    assert k.tolist() == [3, 3] and v.tolist() == [4, 2]                 # descending: highest positions, decreasing
    f = np.array([0x80000000, 0x00000000], dtype=np.uint32)              # -0 < +0
    assert topk_reference(f, 1, key_type=2)[1].tolist() == [0]
    for bad in (0, 6):
        with pytest.raises(ValueError):
            topk_reference(keys, bad)


def test_argument_errors_without_touching_the_gpu(lib):
    from gpusorting_amd import _lib
    h = C.c_void_p()
    assert lib.gs_topk_create(None, 1024, 16, 0, 0) == _lib.GS_ERR_ARG
    assert lib.gs_topk_create(C.byref(h), 0, 16, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_topk_create(C.byref(h), 1024, 0, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_topk_create(C.byref(h), 1024, 1025, 0, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_topk_create(C.byref(h), 1 << 30, 16, 0, 0) == _lib.GS_ERR_SIZE
    assert h.value is None
    assert lib.gs_topk_destroy(None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_check(None, None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_select_keys(None, None, 4, 1, None, 0, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_select_pairs(None, None, None, 4, 1, None, None, 0, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_last(None, None, 0, None) == _lib.GS_ERR_ARG


def _up(x):
    return (x + 255) // 256 * 256


def _formula(lib, n, k, vb):
    """The formula include/gpusort.h states."""
    e, c = 4 + vb, max(k, min(n, 32768))
    return (_up(n * 4) + _up(n * vb) + _up(c * 4) + _up(c * vb) + lib.gs_onesweep_temp_bytes(c) + 256 * 131088 + 3 * 262144 + 4096 + 256), e


def test_temp_bytes_formula_monotone_and_below_sort_and_slice(lib):
    sizes = (1 << 10, 1 << 16, 1 << 20, 1 << 24, 1 << 28, (1 << 30) - 1)
    for vb in (0, 4, 8):
        for i, n in enumerate(sizes):
            ks = [k for k in (1, 64, 1 << 10, 1 << 16, 1 << 20, n) if k <= n]
            for j, k in enumerate(ks):
                t = lib.gs_topk_temp_bytes(n, k, vb)
                assert t == _formula(lib, n, k, vb)[0], "the formula the header states"
                if j:
                    assert t >= lib.gs_topk_temp_bytes(n, ks[j - 1], vb), "grows with max_k"
                if i and k <= sizes[i - 1]:
                    assert t >= lib.gs_topk_temp_bytes(sizes[i - 1], k, vb), "grows with max_keys"
        assert lib.gs_topk_temp_bytes(sizes[-1], 1, vb) > lib.gs_topk_temp_bytes(sizes[0], 1, vb)
        # what sort-and-slice needs: the engine for n, a scratch copy and the sort's second buffer
        n, k, e = 1 << 28, 1 << 20, 4 + vb
        assert lib.gs_topk_temp_bytes(n, k, vb) < lib.gs_onesweep_temp_bytes(n) + 2 * n * e
