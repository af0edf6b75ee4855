"""Unique / run-length encode of 64-bit keys over the C-ABI (``gs_unique64_*`` in include/gpusort.h): ``unique`` restated for 8-byte
keys (uint64, int64, float64): the distinct keys of an array in sorted order, how often each occurs, the lowest input position of each,
and the inverse map: the library's sort of 64-bit keys followed by the run-length stage on 8-byte loads, or that stage alone on the
input as it lies.  Counts, positions and the inverse stay 32-bit.

Equality is BITWISE on all 64 bits: ``-0.0`` and ``+0.0`` are two keys and every NaN pattern is a key of its own, unlike
``torch.unique`` / ``numpy.unique``, which compare values.  No counterpart in the reference project.  PyTorch is used only for device
memory and the current HIP stream.  The numpy statement of the semantics is ``unique64_reference``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .onesweep import KEY_FLOAT64, KEY_INT64, KEY_UINT64
from .topk import MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING  # noqa: F401
from ._handle import KEY64_TYPES
from .unique import Unique, _runs


def sortable_bits64(keys: np.ndarray, key_type: int = KEY_UINT64) -> np.ndarray:
    """The uint64 pattern whose unsigned order is the order of the library's sort of 64-bit keys: signed keys flip the sign bit, floats
    flip all bits of negatives too (``-0.0 < +0.0``, NaNs by bit pattern): ``segsort.sortable_bits`` on 64 bits."""
    u = np.ascontiguousarray(keys).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    if key_type == KEY_INT64:
        return u ^ top
    if key_type == KEY_FLOAT64:
        return u ^ np.where(u & top != 0, np.uint64(0xFFFFFFFFFFFFFFFF), top).astype(np.uint64)
    if key_type != KEY_UINT64:
        raise ValueError("64-bit key types only (KEY_UINT64, KEY_INT64, KEY_FLOAT64)")
    return u


def sorted_perm64(bits: np.ndarray, key_type: int, descending: bool, consecutive: bool) -> np.ndarray:
    """The permutation the references work on: the stable argsort on the sortable bits, reversed for descending; the identity for the
    input as it lies."""
    if consecutive:
        return np.arange(bits.size, dtype=np.int64)
    if key_type not in KEY64_TYPES:
        raise ValueError("64-bit key types only (KEY_UINT64, KEY_INT64, KEY_FLOAT64)")
    perm = np.argsort(sortable_bits64(bits, key_type), kind="stable")
    return perm[::-1] if descending else perm


def unique64_reference(keys: np.ndarray, key_type: int = KEY_UINT64, descending: bool = False, consecutive: bool = False):
    """What ``gs_unique64_positions`` (or, with ``consecutive=True``, ``gs_unique64_consecutive``) delivers for the 8-byte array
    ``keys``: ``(out_keys, counts, first, inverse)``: the distinct bit patterns (uint64) in the order of the library's sort (a stable
    argsort on the sortable bits, reversed for descending), and as uint32 arrays their multiplicities, the lowest input position of
    each, and for every input the index of its key.  ``consecutive=True``: runs of bitwise-equal neighbours of the input as it lies
    (``key_type`` and ``descending`` are not looked at; ``first`` is where each run starts)."""
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize != 8 or k.ndim != 1:
        raise ValueError("keys must be a 1-D array of 8-byte elements")
    bits = k.view(np.uint64)
    n = bits.size
    empty = np.zeros(0, np.uint32)
    if n == 0:
        return np.zeros(0, np.uint64), empty, empty.copy(), empty.copy()
    perm = sorted_perm64(bits, key_type, descending, consecutive)
    return _runs(bits, perm)


def temp_bytes(max_keys: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_unique64_temp_bytes`` (host only); 0 for invalid sizes, mode or value width."""
    return int(_lib.load().gs_unique64_temp_bytes(max_keys, mode, value_bytes))


class Unique64(Unique):
    """One ``gs_unique64`` handle: ``Unique`` for 8-byte keys (``key_type`` KEY_UINT64, the default, KEY_INT64 or KEY_FLOAT64).  The
    methods, their arguments and what they return are ``Unique``'s: the key tensors hold 8-byte elements (int64, float64, uint64 where
    torch has it), counts, positions, the inverse and ``num`` stay int32 tensors.  The stage's plan is ``unique.unique_plan``."""

    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_unique64_", 8, KEY64_TYPES
    _KEYS_WANTED = "Unique64 takes 64-bit keys (KEY_UINT64, KEY_INT64, KEY_FLOAT64)"
