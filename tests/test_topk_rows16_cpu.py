"""The 16-bit key types of the row-wise top-k (GS_KEY_UINT16 .. GS_KEY_BFLOAT16) on the host: the numpy statement of their order
(sortable_bits, and through it topk_reference / topk_rows_reference) and the constants.  No GPU and no library needed."""
import importlib
import os
import re

import numpy as np
import pytest

from gpusorting_amd import _lib
from gpusorting_amd.segsort import sortable_bits
from gpusorting_amd.topk import topk_reference, topk_rows_reference

U16, I16, F16, BF16 = 6, 7, 8, 9
ALL = np.arange(65536, dtype=np.uint32).astype(np.uint16)  # every bit pattern once
topk = importlib.import_module("gpusorting_amd.topk")  # (the package's attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_equal_the_header():
    text = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    enum = {name: int(value) for name, value in re.findall(r"\b(GS_KEY_[A-Z0-9]+)\s*=\s*(\d+)", text)}
    want = {"KEY_UINT16": 6, "KEY_INT16": 7, "KEY_FLOAT16": 8, "KEY_BFLOAT16": 9}
    for name, value in want.items():
        assert enum["GS_" + name] == value
        assert getattr(_lib, name) == value and getattr(topk, name) == value


def test_float16_is_strictly_monotone_against_numpy():
    bits = sortable_bits(ALL.view(np.float16), F16)
    assert bits.dtype == np.uint16 and np.unique(bits).size == 65536
    f = ALL.view(np.float16)
    finite = ALL[~np.isnan(f)]
    order = finite[np.argsort(sortable_bits(finite, F16), kind="stable")].view(np.float16).astype(np.float64)
    step = np.diff(order)
    zero_pair = (order[:-1] == 0) & (order[1:] == 0)
    assert np.all(step[~zero_pair] > 0) and np.count_nonzero(zero_pair) == 1  # (inf - inf never meets: one -inf, one +inf)
    assert sortable_bits(np.array([0x8000], np.uint16), F16)[0] + 1 == sortable_bits(np.array([0x0000], np.uint16), F16)[0]  # -0 < +0


def test_bfloat16_follows_the_float32_transform_nans_included():
    b16 = sortable_bits(ALL, BF16)
    b32 = sortable_bits((ALL.astype(np.uint32) << np.uint32(16)).view(np.float32), 2)
    assert np.unique(b16).size == 65536
    np.testing.assert_array_equal(np.argsort(b16, kind="stable"), np.argsort(b32, kind="stable"))
    np.testing.assert_array_equal(b16, (b32 >> np.uint32(16)).astype(np.uint16))
    # float16 arrays and their uint16 patterns are the same keys
    np.testing.assert_array_equal(sortable_bits(ALL.view(np.float16), F16), sortable_bits(ALL, F16))


def test_integer_types_agree_with_the_32_bit_transforms():
    u = sortable_bits(ALL, U16)
    np.testing.assert_array_equal(u, ALL)
    np.testing.assert_array_equal(np.argsort(u, kind="stable"), np.argsort(sortable_bits(ALL.astype(np.uint32), 0), kind="stable"))
    s = ALL.view(np.int16)
    np.testing.assert_array_equal(np.argsort(sortable_bits(s, I16), kind="stable"),
                                  np.argsort(sortable_bits(s.astype(np.int32), 1), kind="stable"))
    np.testing.assert_array_equal(np.argsort(sortable_bits(s, I16), kind="stable"), np.argsort(s.astype(np.int32), kind="stable"))
    with pytest.raises(ValueError):
        sortable_bits(ALL.astype(np.uint32), U16)  # 4-byte elements under a 16-bit key type


def test_topk_reference_on_16_bit_arrays_against_a_hand_built_list():
    #                 0    1     2    3    4    5     6    7
    f = np.array([1.5, -2.0, 1.5, 0.0, -0.0, 7.0, -2.0, 1.5], dtype=np.float16)
    k, v = topk_reference(f, 4, None, F16, False)  # -2 (1), -2 (6), -0 (4), +0 (3)
    assert v.tolist() == [1, 6, 4, 3] and k.dtype == np.float16
    np.testing.assert_array_equal(k.view(np.uint16), f[[1, 6, 4, 3]].view(np.uint16))
    k, v = topk_reference(f, 5, None, F16, True)  # the exact reverse of the stable ascending order: 7, then 1.5 by falling position
    assert v.tolist() == [5, 7, 2, 0, 3]
    assert topk_reference(f, 1, None, F16, False)[1].tolist() == [1] and topk_reference(f, 1, None, F16, True)[1].tolist() == [5]
    assert topk_reference(f, 8, None, F16, False)[1].tolist() == [1, 6, 4, 3, 0, 2, 7, 5]  # k = n
    assert topk_reference(f, 8, None, F16, True)[1].tolist() == [5, 7, 2, 0, 3, 4, 6, 1]
    # bfloat16 as bit patterns: 1.0, -1.0, 1.0, +inf, NaN (0x7FC0 sorts behind +inf), -NaN (0xFFC0 in front of everything)
    b = np.array([0x3F80, 0xBF80, 0x3F80, 0x7F80, 0x7FC0, 0xFFC0], dtype=np.uint16)
    assert topk_reference(b, 6, None, BF16, False)[1].tolist() == [5, 1, 0, 2, 3, 4]
    assert topk_reference(b, 3, None, BF16, True)[1].tolist() == [4, 3, 2]
    # integers, with carried values
    i = np.array([-32768, 32767, 0, -1, 32767], dtype=np.int16)
    vals = np.array([10, 11, 12, 13, 14], dtype=np.uint64)
    k, v = topk_reference(i, 2, vals, I16, True)
    assert k.tolist() == [32767, 32767] and v.tolist() == [14, 11]
    assert topk_reference(i.view(np.uint16), 2, vals, U16, True)[1].tolist() == [13, 10]  # 0xFFFF, 0x8000


def test_topk_rows_reference_on_16_bit_arrays():
    m = np.array([[3, 1, 3, 2], [0, 0, 65535, 1]], dtype=np.uint16)
    k, v = topk_rows_reference(m, 2, None, U16, False)
    assert k.tolist() == [[1, 2], [0, 0]] and v.tolist() == [[1, 3], [0, 1]] and k.dtype == np.uint16
    k, v = topk_rows_reference(m, 2, None, U16, True)
    assert k.tolist() == [[3, 3], [65535, 1]] and v.tolist() == [[2, 0], [2, 3]]
    k, v = topk_rows_reference(m.view(np.int16), 4, None, I16, False)  # k = n; 65535 is -1
    assert v.tolist() == [[1, 3, 0, 2], [2, 0, 1, 3]]
    assert topk_rows_reference(m, 1, None, U16, True)[1].tolist() == [[2], [2]]
