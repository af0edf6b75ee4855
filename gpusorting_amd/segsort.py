"""Segmented sort over the C-ABI (``gs_segsort_*`` in include/gpusort.h): many independent segments of one array, given by CSR
offsets, each sorted on its own, in place, in one call.

Stands in for the reference's SplitSort (GPUSortingCUDA/SegSort/SplitSort/SplitSort.cuh:674-709: SplitSortAllocateTempMemory /
SplitSortPairs / SplitSortFreeTempMemory); the reference takes segment starts plus a total length, this takes CSR offsets.
PyTorch is used only for device memory and the current HIP stream.  ``segmented_sort_reference`` is the pure-numpy statement of
the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import numpy as np

from . import _handle, _lib
from ._handle import (KEY16_TYPES, KEY_FLOAT32, KEY_INT32, KEY_UINT32, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING,  # noqa: F401
                      ORDER_DESCENDING, _require_cuda, _require_room, _stream_ptr)
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401

SEGSORT_CLASSES = _lib.GS_SEGSORT_CLASSES
LONG_ROUTES = {"host": _lib.GS_SEGSORT_LONG_HOST, "device": _lib.GS_SEGSORT_LONG_DEVICE}
_REPORT = ("route", "units", "long", "unit_cap", "forms", "status", "rank", "n")  # GS_SEGSORT_R_*


def segsort_long_units(n: int, num_segments: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_segsort_long_units``: the bound on the (segment, part) units of a device-route call, the fixed grid of its passes (host
    only; 0 for sizes or a mode / value width the sort refuses)."""
    return int(_lib.load().gs_segsort_long_units(int(n), int(num_segments), mode, value_bytes))


def sortable_bits(keys: np.ndarray, key_type: int = KEY_UINT32) -> np.ndarray:
    """The uint32 pattern whose unsigned order is the key order (GPUSortingD3D12/Shaders/SortCommon.hlsl:134-154): signed keys flip
    the sign bit, floats flip all bits of negatives too (-0 < +0, NaNs by bit pattern).  The 16-bit key types of the row-wise top-k
    (6 .. 9: uint16, int16, float16, bfloat16) take 2-byte arrays, bfloat16 as its uint16 bit patterns, and return the same rule on
    16 bits as uint16."""
    if key_type in KEY16_TYPES:
        k = np.ascontiguousarray(keys)
        if k.dtype.itemsize != 2:
            raise ValueError("the 16-bit key types take 2-byte elements (bfloat16 as its uint16 bit patterns)")
        h = k.view(np.uint16)
        if key_type == KEY_UINT16:
            return h
        if key_type == KEY_INT16:
            return h ^ np.uint16(0x8000)
        return h ^ np.where(h >> 15 != 0, np.uint16(0xFFFF), np.uint16(0x8000)).astype(np.uint16)
    u = np.ascontiguousarray(keys).view(np.uint32)
    if key_type == KEY_INT32:
        return u ^ np.uint32(0x80000000)
    if key_type == KEY_FLOAT32:
        return u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)
    if key_type != KEY_UINT32:
        raise ValueError("32-bit key types only")
    return u


def segmented_sort_reference(keys: np.ndarray, offsets: np.ndarray, values: np.ndarray | None = None, key_type: int = KEY_UINT32,
                             descending: bool = False):
    """Every segment ``[offsets[s], offsets[s + 1])`` sorted on its own: stable argsort on the sortable bit pattern, reversed per
    segment for descending.  Elements outside ``[offsets[0], offsets[-1])`` are returned as they are.  Returns ``keys`` or
    ``(keys, values)`` (new arrays, dtypes kept)."""
    keys = np.ascontiguousarray(keys)
    offsets = np.asarray(offsets).astype(np.int64)
    if offsets.ndim != 1 or offsets.size < 1 or np.any(np.diff(offsets) < 0) or offsets[0] < 0 or offsets[-1] > keys.size:
        raise ValueError("offsets must be non-decreasing and end within the keys")
    bits = sortable_bits(keys, key_type)
    perm = np.arange(keys.size, dtype=np.int64)
    lo, hi = int(offsets[0]), int(offsets[-1])
    if hi > lo:
        # one stable argsort on (segment number, sortable bits) is the per-segment stable argsort of every segment at once
        lens = np.diff(offsets)
        seg = np.repeat(np.arange(lens.size, dtype=np.uint64), lens)
        p = np.argsort((seg << np.uint64(32)) | bits[lo:hi].astype(np.uint64), kind="stable") + lo
        if descending:  # reversal per segment: position i of [a, b) takes what the ascending order has at a + b - 1 - i
            p = p[np.repeat(offsets[:-1] + offsets[1:] - 1, lens) - np.arange(lo, hi, dtype=np.int64) - lo]
        perm[lo:hi] = p
    out = keys[perm]
    if values is None:
        return out
    return out, np.ascontiguousarray(values)[perm]


class _SegmentedSortCalls(_handle.Checked, _handle.AltBuffers, _handle.Handle):
    """What ``SegmentedSort`` and ``SegmentedSort16`` (segsort16.py) share: the constructor's frame, ``sort``, the class counts."""

    _KEY_BYTES = 4

    def _open(self, max_keys, max_segments, order, key_type, mode, value_bytes, device) -> None:
        self.max_keys, self.max_segments = int(max_keys), int(max_segments)
        self.key_type = key_type
        self._pairs_mode(order, mode, value_bytes)
        self._create(device, self.max_keys, self.max_segments, mode, self.value_bytes)

    @property
    def max_lds_segment(self) -> int:
        """Longest segment sorted in LDS; a ``max_segment_len`` up to it needs no alt buffers and, on 32-bit keys, keeps ``sort`` free
        of host waits."""
        return int(self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes))

    def class_of(self, length: int) -> int:
        return int(self._lib.gs_segsort_class_of(int(length), self.mode, self.value_bytes))

    def _args(self, keys, offsets, n):
        _require_cuda(keys, "keys")
        _require_cuda(offsets, "offsets")
        if keys.element_size() != self._KEY_BYTES or offsets.element_size() != 4 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError(f"keys must be {8 * self._KEY_BYTES}-bit and offsets a 1-D tensor of num_segments + 1 32-bit words")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        return n, offsets.numel() - 1

    def _alt_for(self, n: int, max_segment_len: int):
        """The alternate buffers of a call, unless the promised segment length keeps every segment in LDS."""
        if max_segment_len != 0 and max_segment_len <= self.max_lds_segment:
            return None, None
        return self._alt(n)

    def sort(self, keys, offsets, values=None, n: int | None = None, max_segment_len: int = 0, stream=None) -> None:
        """Sort every segment of ``keys[:n]`` (and ``values[:n]``) in place on the current stream.  ``offsets``: int32 device tensor of
        ``num_segments + 1`` CSR offsets.  ``max_segment_len``: a promise (0 = unknown).  16-bit keys: the call never waits on the host.
        32-bit keys: non-zero and at most ``max_lds_segment`` the call never waits on the host; otherwise it waits once for the list of
        long segments on the ``"host"`` long route and never on the ``"device"`` one."""
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        n, num_segments = self._args(keys, offsets, n)
        _require_room(values, n, "values")
        if values is not None and values.element_size() != self.value_bytes:
            raise ValueError(f"values must be {self.value_bytes} bytes wide for this sorter")
        max_segment_len = int(max_segment_len)
        alt_k, alt_v = self._alt_for(n, max_segment_len)
        tail = (n, offsets.data_ptr(), num_segments, max_segment_len, self.key_type, self.order, _stream_ptr(stream))
        if values is None:
            self._call("sort_keys", keys.data_ptr(), alt_k, *tail, where="sort")
        else:
            self._call("sort_pairs", keys.data_ptr(), values.data_ptr(), alt_k, alt_v, *tail, where="sort")

    def last_classes(self, stream=None) -> dict:
        """Segments per length class in the last call and the longest segment seen (synchronises)."""
        w = self._words("last_classes", SEGSORT_CLASSES + 1, stream)
        return {"counts": w[:SEGSORT_CLASSES], "longest": w[SEGSORT_CLASSES]}


class SegmentedSort(_SegmentedSortCalls):
    """One ``gs_segsort`` handle (class lists + an embedded OneSweep engine for long segments) + lazily sized alt buffers.
    ``long_route``: ``"host"`` (the default: one host wait for the list of long segments, the engine sorts them one by one) or
    ``"device"`` (four passes over all long segments at once, no host wait: ``gs_segsort_set_long_route``)."""

    _PREFIX, _KEY_TYPES, _KEYS_WANTED = "gs_segsort_", _handle.KEY32_TYPES, "the segmented sort takes 32-bit keys only"

    def __init__(self, max_keys: int, max_segments: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT32,
                 mode: int = MODE_KEYS_ONLY, value_bytes: int = 0, device: int | None = None, long_route: str = "host"):
        key_type = self._check_key_type(key_type)
        if long_route not in LONG_ROUTES:
            raise ValueError('long_route must be "host" or "device"')
        self._open(max_keys, max_segments, order, key_type, mode, value_bytes, device)
        if long_route != "host":
            self.set_long_route(long_route)

    @property
    def engine(self):
        """The embedded OneSweep engine, borrowed (``gs_segsort_engine``): it sorts the long segments and its rank mode is the one the
        workgroup classes run with.  For ``set_rank_mode`` / ``rank_mode`` / ``check``, with no call in flight; it lives as long as
        this handle."""
        from .onesweep import OneSweep
        return OneSweep._borrow(self._lib.gs_segsort_engine(self._h), self.max_keys, self.mode, self.value_bytes, self.key_type)

    @property
    def long_route(self) -> str:
        """The route of the long segments: ``"host"`` or ``"device"``."""
        r = int(self._lib.gs_segsort_get_long_route(self._h))
        return next(name for name, code in LONG_ROUTES.items() if code == r)

    def set_long_route(self, long_route: str) -> None:
        """``gs_segsort_set_long_route``, with no call in flight and not during a capture: the first switch to ``"device"`` allocates
        that route's buffers (synchronously); they stay until ``close``."""
        if long_route not in LONG_ROUTES:
            raise ValueError('long_route must be "host" or "device"')
        self._call("set_long_route", LONG_ROUTES[long_route])

    def last(self, stream=None) -> dict:
        """``gs_segsort_last`` (synchronises): the report words of the last call as a dict: ``route``, ``units``, ``long``,
        ``unit_cap``, ``forms`` (``GS_SEGSORT_LF_*``), ``status``, ``rank``, ``n``."""
        return self._report("last", _lib.GS_SEGSORT_REPORT_WORDS, _handle._indexed(_REPORT), stream)
