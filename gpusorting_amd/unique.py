"""Unique / run-length encode of 32-bit keys over the C-ABI (``gs_unique_*`` in include/gpusort.h): the distinct keys of an array in
sorted order, how often each occurs, the lowest input position of each, and the inverse map — the library's sort followed by one
streaming run-length stage, or that stage alone on the input as it lies (``unique_consecutive``).

Equality is BITWISE: ``-0.0`` and ``+0.0`` are two keys and every NaN pattern is a key of its own, unlike ``torch.unique`` /
``numpy.unique``, which compare values.  No counterpart in the reference project.  PyTorch is used only for device memory and the
current HIP stream.  The numpy statement of the semantics is ``unique_reference``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle, _lib
from ._handle import _ptr, _require_room, _stream_ptr
from ._lib import check
from .segsort import sortable_bits
from .topk import KEY_FLOAT32, KEY_INT32, KEY_UINT32, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING  # noqa: F401

ROUTE_NONE, ROUTE_KEYS, ROUTE_POSITIONS, ROUTE_CONSECUTIVE = 0, 1, 2, 3
_REPORT = ("route", "n", "u", "ranges", "per_range", "tile", "status", "rank")
_KEY_TYPES = _handle.KEY32_TYPES


def unique_reference(keys: np.ndarray, key_type: int = KEY_UINT32, descending: bool = False, consecutive: bool = False):
    """What ``gs_unique_positions`` (or, with ``consecutive=True``, ``gs_unique_consecutive``) delivers for the 4-byte array ``keys``:
    ``(out_keys, counts, first, inverse)`` as uint32 arrays — the distinct bit patterns in the order of the library's sort (a stable
    argsort on the sortable bits, reversed for descending), their multiplicities, the lowest input position of each, and for every
    input the index of its key.  ``consecutive=True``: runs of bitwise-equal neighbours of the input as it lies (``key_type`` and
    ``descending`` are not looked at; ``first`` is where each run starts)."""
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize != 4 or k.ndim != 1:
        raise ValueError("keys must be a 1-D array of 4-byte elements")
    bits = k.view(np.uint32)
    n = bits.size
    empty = np.zeros(0, np.uint32)
    if n == 0:
        return empty, empty.copy(), empty.copy(), empty.copy()
    if consecutive:
        perm = np.arange(n, dtype=np.int64)
    else:
        if key_type not in _KEY_TYPES:
            raise ValueError("unique takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)")
        perm = np.argsort(sortable_bits(bits, key_type), kind="stable")
        if descending:
            perm = perm[::-1]
    return _runs(bits, perm)


def _runs(bits: np.ndarray, perm: np.ndarray):
    """The references' run-length stage on ``bits[perm]`` (at least one element): ``(out_keys, counts, first, inverse)``."""
    n = bits.size
    s = bits[perm]
    head = np.ones(n, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    starts = np.flatnonzero(head)
    rank = np.cumsum(head) - 1  # the run of every sorted element
    counts = np.diff(np.append(starts, n))
    first = np.minimum.reduceat(perm, starts)  # ascending: the run's head; descending: its tail
    inverse = np.empty(n, dtype=np.int64)
    inverse[perm] = rank
    return s[starts].copy(), counts.astype(np.uint32), first.astype(np.uint32), inverse.astype(np.uint32)


def temp_bytes(max_keys: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_unique_temp_bytes`` (host only); 0 for invalid sizes, mode or value width."""
    return int(_lib.load().gs_unique_temp_bytes(max_keys, mode, value_bytes))


def unique_plan(n: int) -> tuple:
    """``gs_unique_plan`` (host only): ``(ranges, per_range, tile)`` of the run-length stage for ``n`` elements."""
    plan = (C.c_uint32 * 3)()
    check(_lib.load().gs_unique_plan(int(n), plan), "gs_unique_plan")
    return int(plan[0]), int(plan[1]), int(plan[2])


def _out(keys, count: int, want: bool = True, dtype=None):
    """An output tensor of ``count`` elements (int32 unless ``dtype``) on the device of ``keys``, or None for one not wanted."""
    import torch
    return torch.empty(count, dtype=dtype or torch.int32, device=keys.device) if want else None


class Unique(_handle.Checked, _handle.Handle):
    """One ``gs_unique`` handle: an embedded sorter of capacity ``max_keys`` and the buffers it sorts in.

    ``positions=False`` makes a handle for keys and counts; ``positions=True`` one that also delivers first positions and the inverse
    (its sorter sorts (key, position) pairs).  Every call returns full-capacity tensors (``n`` elements; only the first ``u`` of keys,
    counts and first are written) plus the one-element count tensor ``num`` on the device, and does not wait on the host."""

    # the family of entries behind the class, its key width and key types (unique64.Unique64 states its own)
    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_unique_", 4, _KEY_TYPES
    _KEYS_WANTED = "Unique takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)"

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int | None = None, positions: bool = False, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.order = int(max_keys), order
        self.mode, self.value_bytes = (MODE_PAIRS, 4) if positions else (MODE_KEYS_ONLY, 0)
        self._create(device, self.max_keys, self.mode, self.value_bytes)

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_keys, self.mode, self.value_bytes))

    def _keys(self, keys, n):
        if keys.element_size() != self._KEY_BYTES:
            raise ValueError("keys must be %d-bit" % (8 * self._KEY_BYTES))
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        return n

    def unique(self, keys, n: int | None = None, counts: bool = True, stream=None):
        """``gs_unique_keys``: ``(out_keys, out_counts | None, num)``.  ``keys`` is not written."""
        n = self._keys(keys, n)
        out_k, out_c, num = _out(keys, n, dtype=keys.dtype), _out(keys, n, counts), _out(keys, 1)
        self._call("keys", keys.data_ptr(), n, out_k.data_ptr(), _ptr(out_c), num.data_ptr(), self.key_type, self.order, _stream_ptr(stream))
        return out_k, out_c, num

    def unique_positions(self, keys, n: int | None = None, counts: bool = True, first: bool = True, inverse: bool = True, stream=None):
        """``gs_unique_positions`` (a handle with ``positions=True``): ``(out_keys, out_counts | None, out_first | None, out_inverse | None,
        num)``; positions and the inverse are int32 tensors holding uint32 values."""
        n = self._keys(keys, n)
        out_k = _out(keys, n, dtype=keys.dtype)
        out_c, out_f, out_i, num = _out(keys, n, counts), _out(keys, n, first), _out(keys, n, inverse), _out(keys, 1)
        self._call("positions", keys.data_ptr(), n, out_k.data_ptr(), _ptr(out_c), _ptr(out_f), _ptr(out_i), num.data_ptr(), self.key_type,
                   self.order, _stream_ptr(stream))
        return out_k, out_c, out_f, out_i, num

    def unique_consecutive(self, keys, n: int | None = None, counts: bool = True, inverse: bool = True, stream=None):
        """``gs_unique_consecutive``: the run-length encode of ``keys`` as it lies: ``(out_keys, out_counts | None, out_inverse | None,
        num)``."""
        n = self._keys(keys, n)
        out_k, out_c, out_i, num = _out(keys, n, dtype=keys.dtype), _out(keys, n, counts), _out(keys, n, inverse), _out(keys, 1)
        self._call("consecutive", keys.data_ptr(), n, out_k.data_ptr(), _ptr(out_c), _ptr(out_i), num.data_ptr(), _stream_ptr(stream))
        return out_k, out_c, out_i, num

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, n, u, ranges, per_range, tile, status, rank (the sorter's rank mode)."""
        return self._report("last", _lib.GS_UNIQUE_REPORT_WORDS, _handle._indexed(_REPORT), stream)
