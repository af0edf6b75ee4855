"""The row-wise top-k without a GPU: topk_rows_reference is topk_reference applied to every row, and the new C entries answer a null
handle and the host-only capacity question.  No counterpart in the reference project."""
import ctypes as C

import numpy as np
import pytest

from gpusorting_amd.topk import KEY_FLOAT32, KEY_INT32, KEY_UINT32, topk_reference, topk_rows_reference

DTYPE = {KEY_UINT32: np.uint32, KEY_INT32: np.int32, KEY_FLOAT32: np.float32}


def _rows(kind, key_type, rows, row_len, seed):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        bits = np.full((rows, row_len), 0x3F800000, dtype=np.uint32)
    elif key_type == KEY_FLOAT32:
        special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x3F800000, 0xBF800000], dtype=np.uint32)
        bits = np.where(rng.random((rows, row_len)) < 0.5, special[rng.integers(0, special.size, (rows, row_len))],
                        rng.integers(0, 1 << 32, (rows, row_len), dtype=np.uint64).astype(np.uint32))
    else:
        bits = rng.integers(0, 1 << 32, (rows, row_len), dtype=np.uint64).astype(np.uint32)  # both signs as int32
        bits[:, ::3] = bits[:, :1]  # ties
    return bits.view(DTYPE[key_type])


@pytest.mark.parametrize("key_type", [KEY_UINT32, KEY_INT32, KEY_FLOAT32])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kind", ["random", "equal"])
def test_rows_reference_is_the_reference_of_every_row(key_type, descending, kind):
    rows, row_len = 5, 37
    keys = _rows(kind, key_type, rows, row_len, 7 + key_type)
    vals = (np.arange(rows * row_len, dtype=np.uint64).reshape(rows, row_len) << np.uint64(20)) | np.uint64(5)
    for k in (1, 6, row_len):
        for v in (None, vals):
            rk, rv = topk_rows_reference(keys, k, v, key_type, descending)
            assert rk.shape == (rows, k) and rv.shape == (rows, k)
            assert rv.dtype == (np.uint32 if v is None else np.uint64)
            for r in range(rows):
                ek, ev = topk_reference(keys[r], k, None if v is None else v[r], key_type, descending)
                np.testing.assert_array_equal(rk[r].view(np.uint32), ek.view(np.uint32))
                np.testing.assert_array_equal(rv[r], ev)
                if v is None:
                    assert ev.max() < row_len  # positions within the row


def test_rows_reference_takes_a_strided_view():
    flat = np.random.default_rng(3).integers(0, 1 << 32, 4 * 11, dtype=np.uint64).astype(np.uint32)
    view = np.lib.stride_tricks.as_strided(flat, (4, 9), (11 * 4, 4))
    rk, rv = topk_rows_reference(view, 3)
    for r in range(4):
        ek, ev = topk_reference(flat[r * 11:r * 11 + 9], 3)
        np.testing.assert_array_equal(rk[r], ek)
        np.testing.assert_array_equal(rv[r], ev)
    with pytest.raises(ValueError):
        topk_rows_reference(flat, 3)


def test_null_handle_is_an_argument_error():
    from gpusorting_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint32 * _lib.GS_TOPK_ROWS_REPORT_WORDS)()
    assert lib.gs_topk_select_rows_keys(None, 16, 2, 8, 8, 1, 4096, 0, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_select_rows_pairs(None, 16, 32, 2, 8, 8, 1, 4096, 8192, 0, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_rows_last(None, buf, _lib.GS_TOPK_ROWS_REPORT_WORDS, None) == _lib.GS_ERR_ARG


def test_rows_max_k_meets_the_minima():
    from gpusorting_amd import _lib
    from gpusorting_amd.topk import MODE_KEYS_ONLY, MODE_PAIRS, rows_max_k
    assert rows_max_k(MODE_KEYS_ONLY, 0) >= 2048
    assert rows_max_k(MODE_PAIRS, 4) >= 2048
    assert rows_max_k(MODE_PAIRS, 8) >= 1024
    assert _lib.load().gs_topk_rows_max_k(MODE_PAIRS, 3) == 0
