"""Segmented sort over the C-ABI (``gs_segsort_*`` in include/gpusort.h): many independent segments of one array, given by CSR
offsets, each sorted on its own, in place, in one call.

Stands in for the reference's SplitSort (GPUSortingCUDA/SegSort/SplitSort/SplitSort.cuh:674-709: SplitSortAllocateTempMemory /
SplitSortPairs / SplitSortFreeTempMemory); the reference takes segment starts plus a total length, this takes CSR offsets.
PyTorch is used only for device memory and the current HIP stream.  ``segmented_sort_reference`` is the pure-numpy statement of
the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check

MODE_KEYS_ONLY, MODE_PAIRS = 0, 1
ORDER_ASCENDING, ORDER_DESCENDING = 0, 1
KEY_UINT32, KEY_INT32, KEY_FLOAT32 = 0, 1, 2
KEY16_TYPES = (KEY_UINT16, KEY_INT16, KEY_FLOAT16, KEY_BFLOAT16)  # 2-byte keys: the row-wise top-k only (gs_topk_select_rows_*)
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


class SegmentedSort:
    """One ``gs_segsort`` handle (class lists + an embedded OneSweep engine for long segments) + lazily sized alt buffers.
    ``long_route``: ``"host"`` (the default: one host wait for the list of long segments, the engine sorts them one by one) or
    ``"device"`` (four passes over all long segments at once, no host wait: ``gs_segsort_set_long_route``)."""

    def __init__(self, max_keys: int, max_segments: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT32,
                 mode: int = MODE_KEYS_ONLY, value_bytes: int = 0, device: int | None = None, long_route: str = "host"):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type not in (KEY_UINT32, KEY_INT32, KEY_FLOAT32):
            raise ValueError("the segmented sort takes 32-bit keys only")
        if long_route not in LONG_ROUTES:
            raise ValueError('long_route must be "host" or "device"')
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys, self.max_segments = int(max_keys), int(max_segments)
        self.order, self.key_type, self.mode = order, key_type, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0
        h = C.c_void_p()
        check(self._lib.gs_segsort_create(C.byref(h), self.max_keys, self.max_segments, mode, self.value_bytes), "gs_segsort_create")
        self._h = h
        self._alt_keys = self._alt_vals = None
        if long_route != "host":
            self.set_long_route(long_route)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gs_segsort_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def max_lds_segment(self) -> int:
        """Longest segment sorted in LDS; a ``max_segment_len`` up to it keeps ``sort`` free of host waits."""
        return int(self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes))

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
        check(self._lib.gs_segsort_set_long_route(self._h, LONG_ROUTES[long_route]), "gs_segsort_set_long_route")

    def class_of(self, length: int) -> int:
        return int(self._lib.gs_segsort_class_of(int(length), self.mode, self.value_bytes))

    def sort(self, keys, offsets, values=None, n: int | None = None, max_segment_len: int = 0, stream=None) -> None:
        """Sort every segment of ``keys[:n]`` (and ``values[:n]``) in place on the current stream.  ``offsets``: int32 device tensor of
        ``num_segments + 1`` CSR offsets.  ``max_segment_len``: a promise (0 = unknown); non-zero and at most ``max_lds_segment`` the
        call never waits on the host; otherwise it waits once for the list of long segments on the ``"host"`` long route and never
        on the ``"device"`` one."""
        import torch
        from .onesweep import _require_cuda, _require_room, _stream_ptr
        _require_cuda(keys, "keys")
        _require_cuda(offsets, "offsets")
        if keys.element_size() != 4 or offsets.element_size() != 4 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError("keys must be 32-bit and offsets a 1-D tensor of num_segments + 1 32-bit words")
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        _require_room(values, n, "values")
        if values is not None and values.element_size() != self.value_bytes:
            raise ValueError(f"values must be {self.value_bytes} bytes wide for this sorter")
        num_segments = offsets.numel() - 1
        max_segment_len = int(max_segment_len)
        alt_k = alt_v = None
        if max_segment_len == 0 or max_segment_len > self.max_lds_segment:
            if self._alt_keys is None or self._alt_keys.numel() < n:
                self._alt_keys = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
            alt_k = self._alt_keys.data_ptr()
            if values is not None:
                if self._alt_vals is None or self._alt_vals.numel() < n:
                    self._alt_vals = torch.empty(max(n, 1), dtype=torch.int32 if self.value_bytes == 4 else torch.int64, device=self.device)
                alt_v = self._alt_vals.data_ptr()
        s = _stream_ptr(stream)
        if values is None:
            st = self._lib.gs_segsort_sort_keys(self._h, keys.data_ptr(), alt_k, n, offsets.data_ptr(), num_segments, max_segment_len,
                                                self.key_type, self.order, s)
        else:
            st = self._lib.gs_segsort_sort_pairs(self._h, keys.data_ptr(), values.data_ptr(), alt_k, alt_v, n, offsets.data_ptr(),
                                                 num_segments, max_segment_len, self.key_type, self.order, s)
        check(st, "gs_segsort_sort")

    def status(self, stream=None) -> int:
        """``gs_segsort_check`` as a status code (synchronises): GS_OK, GS_ERR_ARG (bad offsets), GS_ERR_SIZE (promise broken) ..."""
        from .onesweep import _stream_ptr
        return int(self._lib.gs_segsort_check(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), "gs_segsort_check")

    def last_classes(self, stream=None) -> dict:
        """Segments per length class in the last call and the longest segment seen (synchronises)."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * (SEGSORT_CLASSES + 1))()
        check(self._lib.gs_segsort_last_classes(self._h, buf, SEGSORT_CLASSES + 1, _stream_ptr(stream)), "gs_segsort_last_classes")
        return {"counts": [int(x) for x in buf[:SEGSORT_CLASSES]], "longest": int(buf[SEGSORT_CLASSES])}

    def last(self, stream=None) -> dict:
        """``gs_segsort_last`` (synchronises): the report words of the last call as a dict: ``route``, ``units``, ``long``,
        ``unit_cap``, ``forms`` (``GS_SEGSORT_LF_*``), ``status``, ``rank``, ``n``."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_SEGSORT_REPORT_WORDS)()
        check(self._lib.gs_segsort_last(self._h, buf, _lib.GS_SEGSORT_REPORT_WORDS, _stream_ptr(stream)), "gs_segsort_last")
        return {name: int(buf[i]) for i, name in enumerate(_REPORT)}
