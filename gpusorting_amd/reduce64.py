"""Reduce by key on 64-bit keys over the C-ABI (``gs_reduce64_*`` in include/gpusort.h): ``reduce`` restated for 8-byte keys (uint64,
int64, float64): one sum, minimum or maximum per distinct key: the library's stable sort of (key, value) pairs followed by one
segmented reduction, or that stage alone on runs of equal neighbouring keys of the input as it lies.  Counts stay 32-bit.

Key equality is BITWISE on all 64 bits.  Integer sums wrap.  MIN / MAX on floats use this library's TOTAL ORDER of floats
(``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN``) and return one of the inputs bit for bit: this DIFFERS from ``torch.amin`` /
``amax`` (which propagate NaNs) and from ``fmin`` / ``fmax`` (which drop them).  A float sum is combined in the tree of ``reduce``,
fixed by n and the run's place in the sorted array: two calls give bitwise identical output, and on keys that are zero-extended 32-bit
keys the values are bit for bit those of ``ReduceByKey``; it is not the left-to-right sequential sum.  No counterpart in the reference
project.  PyTorch is used only for device memory and the current HIP stream.  The numpy statement of the semantics is
``reduce_by_key64_reference``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .onesweep import KEY_FLOAT64, KEY_INT64, KEY_UINT64  # noqa: F401
from .reduce import (OP_MAX, OP_MIN, OP_SUM, VALUE_DTYPES, VALUE_FLOAT32, VALUE_FLOAT64, VALUE_INT32, ReduceByKey,  # noqa: F401
                     _reference_runs, _reference_values, value_from_order_bits, value_order_bits)
from .unique64 import KEY64_TYPES, sorted_perm64


def reduce_by_key64_reference(keys: np.ndarray, values: np.ndarray, key_type: int = KEY_UINT64, descending: bool = False,
                              value_type: int = VALUE_INT32, op: int = OP_SUM, consecutive: bool = False):
    """What ``gs_reduce64_by_key`` (or, with ``consecutive=True``, ``gs_reduce64_by_key_consecutive``) delivers for the 8-byte array
    ``keys`` and the array ``values`` of ``value_type``'s width: ``(out_keys, out_values, counts)``: the distinct key bit patterns in
    the order of the library's sort (uint64), the reduction of each key's values, the multiplicities (uint32).  Integer sums wrap and
    come in the value's dtype; FLOAT SUMS ARE SUMMED IN float64 and returned as float64 for the comparison (the device's order of
    combination is its own); MIN / MAX go through ``value_order_bits`` and return one of the inputs bit for bit, in the value's dtype."""
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize != 8 or k.ndim != 1:
        raise ValueError("keys must be a 1-D array of 8-byte elements")
    v = _reference_values(k, values, value_type, op)
    dtype = v.dtype
    bits = k.view(np.uint64)
    n = bits.size
    is_float = value_type in (VALUE_FLOAT32, VALUE_FLOAT64)
    if n == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.float64 if is_float and op == OP_SUM else dtype), np.zeros(0, np.uint32)
    perm = sorted_perm64(bits, key_type, descending, consecutive)
    return _reference_runs(bits, v, perm, value_type, op)


def temp_bytes(max_keys: int, value_bytes: int = 4) -> int:
    """``gs_reduce64_temp_bytes`` (host only); 0 for invalid sizes or value width."""
    return int(_lib.load().gs_reduce64_temp_bytes(max_keys, value_bytes))


class ReduceByKey64(ReduceByKey):
    """One ``gs_reduce64`` handle: ``ReduceByKey`` for 8-byte keys (``key_type`` KEY_UINT64, the default, KEY_INT64 or KEY_FLOAT64).
    The methods, their arguments and what they return are ``ReduceByKey``'s: the key tensors hold 8-byte elements (int64, float64,
    uint64 where torch has it), counts and ``num`` stay int32 tensors."""

    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_reduce64_", 8, KEY64_TYPES
    _KEYS_WANTED = "ReduceByKey64 takes 64-bit keys (KEY_UINT64, KEY_INT64, KEY_FLOAT64)"
