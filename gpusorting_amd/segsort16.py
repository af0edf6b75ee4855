"""Segmented sort of 16-bit keys over the C-ABI (``gs_segsort16_*`` in include/gpusort.h): many independent segments of one array of
float16, bfloat16, int16 or uint16 keys, given by CSR offsets, each sorted on its own, in place, in one call, at the keys' own width —
keys only, with 4- or 8-byte values, or as an argsort whose array indices the kernels make themselves.  Segments that fit LDS are sorted
there in two ranking passes; longer ones take two stable 8-bit passes over all long segments at once on a work list built on the device,
so a call never waits on the host, whatever the segment lengths, and can be captured into a graph.

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.
``segmented_sort16_reference`` is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch and
no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .segsort import KEY16_TYPES, SEGSORT_CLASSES, segmented_sort_reference

MODE_KEYS_ONLY, MODE_PAIRS = 0, 1
ORDER_ASCENDING, ORDER_DESCENDING = 0, 1
SEGSORT16_PART = _lib.GS_SEGSORT16_PART
_VM_NAMES = ("keys", "pos", "v4", "v8")
# every kernel form a call can launch -> its bit in ``SegmentedSort16.last()["forms"]`` (report word FORMS, with WG_FORMS << 32)
SEGSORT16_FORMS = {"classify": _lib.GS_SEGSORT16_F_CLASSIFY, "fill": _lib.GS_SEGSORT16_F_FILL, "units": _lib.GS_SEGSORT16_F_UNITS,
                   "count": _lib.GS_SEGSORT16_F_COUNT, "scan": _lib.GS_SEGSORT16_F_SCAN}
for _v, _name in enumerate(_VM_NAMES):
    SEGSORT16_FORMS[f"packed_{_name}"] = _lib.GS_SEGSORT16_F_PACKED << _v
    SEGSORT16_FORMS[f"wave_{_name}"] = _lib.GS_SEGSORT16_F_WAVE << _v
    for _r in (0, 1):
        SEGSORT16_FORMS[f"scatter_{_name}_rank{_r}"] = _lib.GS_SEGSORT16_F_SCATTER << (2 * _v + _r)
        for _c in (3, 4, 5, 6, 7):  # class 6 takes no 8-byte values, class 7 keys only: what 160 KiB of LDS hold
            if _c <= 5 or (_c == 6 and _name != "v8") or _name == "keys":
                SEGSORT16_FORMS[f"wg{_c}_{_name}_rank{_r}"] = _lib.GS_SEGSORT16_WG_FORM(_c, _v, _r) << 32


def segmented_sort16_reference(keys: np.ndarray, offsets: np.ndarray, values: np.ndarray | None = None, key_type: int = KEY_UINT16,
                               descending: bool = False):
    """Every segment ``[offsets[s], offsets[s + 1])`` of the 1-D array ``keys`` (2-byte elements, bfloat16 as its uint16 bit patterns)
    sorted on its own: ``segmented_sort_reference`` on a 16-bit key type.  Returns ``(keys, positions)`` — positions: uint32 ARRAY
    indices, ``positions[i]`` = where the element the order puts at ``i`` came from; identity outside the segments — or, with
    ``values``, ``(keys, values)``; new arrays, dtypes kept."""
    if key_type not in KEY16_TYPES:
        raise ValueError("16-bit key types only")
    keys = np.ascontiguousarray(keys)
    if keys.ndim != 1 or keys.dtype.itemsize != 2:
        raise ValueError("keys must be a 1-D array of 2-byte elements")
    if values is None:
        out, pos = segmented_sort_reference(keys, offsets, np.arange(keys.size, dtype=np.uint32), key_type, descending)
        return out, pos
    values = np.ascontiguousarray(values)
    if values.shape != keys.shape:
        raise ValueError("values must have the shape of keys")
    return segmented_sort_reference(keys, offsets, values, key_type, descending)


def segsort16_units(n: int, num_segments: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_segsort16_units`` (host only): the bound on (segment, part) units of a call, which sizes the tables and the fixed grids."""
    return int(_lib.load().gs_segsort16_units(int(n), int(num_segments), mode, value_bytes))


class SegmentedSort16:
    """One ``gs_segsort16`` handle + lazily sized alt buffers (the long route's scratch; the LDS classes need none)."""

    def __init__(self, max_keys: int, max_segments: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type not in KEY16_TYPES:
            raise ValueError("SegmentedSort16 takes 16-bit key types only")
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys, self.max_segments = int(max_keys), int(max_segments)
        self.order, self.key_type, self.mode = order, key_type, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0
        h = C.c_void_p()
        check(self._lib.gs_segsort16_create(C.byref(h), self.max_keys, self.max_segments, mode, self.value_bytes), "gs_segsort16_create")
        self._h = h
        self._alt_keys = self._alt_vals = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gs_segsort16_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def max_lds_segment(self) -> int:
        """Longest segment sorted in LDS; a ``max_segment_len`` up to it needs no alt buffers."""
        return int(self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes))

    @property
    def rank_mode(self) -> int:
        return int(self._lib.gs_segsort16_get_rank_mode(self._h))

    def set_rank_mode(self, mode: int) -> None:
        check(self._lib.gs_segsort16_set_rank_mode(self._h, int(mode)), "gs_segsort16_set_rank_mode")

    def class_of(self, length: int) -> int:
        return int(self._lib.gs_segsort_class_of(int(length), self.mode, self.value_bytes))

    def _alt(self, n: int, max_segment_len: int):
        import torch
        if max_segment_len != 0 and max_segment_len <= self.max_lds_segment:
            return None, None
        if self._alt_keys is None or self._alt_keys.numel() < n:
            self._alt_keys = torch.empty(max(n, 1), dtype=torch.int16, device=self.device)
        if self.value_bytes == 0:
            return self._alt_keys.data_ptr(), None
        if self._alt_vals is None or self._alt_vals.numel() < n:
            self._alt_vals = torch.empty(max(n, 1), dtype=torch.int32 if self.value_bytes == 4 else torch.int64, device=self.device)
        return self._alt_keys.data_ptr(), self._alt_vals.data_ptr()

    def _args(self, keys, offsets, n):
        from .onesweep import _require_cuda, _require_room
        _require_cuda(keys, "keys")
        _require_cuda(offsets, "offsets")
        if keys.element_size() != 2 or offsets.element_size() != 4 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError("keys must be 16-bit and offsets a 1-D tensor of num_segments + 1 32-bit words")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        return n, offsets.numel() - 1

    def sort(self, keys, offsets, values=None, n: int | None = None, max_segment_len: int = 0, stream=None) -> None:
        """Sort every segment of ``keys[:n]`` (2-byte elements; and carry ``values[:n]``) in place on the current stream.  ``offsets``:
        int32 device tensor of ``num_segments + 1`` CSR offsets.  ``max_segment_len``: a promise (0 = unknown).  The call never waits on
        the host."""
        from .onesweep import _require_room, _stream_ptr
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        n, num_segments = self._args(keys, offsets, n)
        _require_room(values, n, "values")
        if values is not None and values.element_size() != self.value_bytes:
            raise ValueError(f"values must be {self.value_bytes} bytes wide for this sorter")
        max_segment_len = int(max_segment_len)
        alt_k, alt_v = self._alt(n, max_segment_len)
        s = _stream_ptr(stream)
        if values is None:
            st = self._lib.gs_segsort16_sort_keys(self._h, keys.data_ptr(), alt_k, n, offsets.data_ptr(), num_segments, max_segment_len,
                                                  self.key_type, self.order, s)
        else:
            st = self._lib.gs_segsort16_sort_pairs(self._h, keys.data_ptr(), values.data_ptr(), alt_k, alt_v, n, offsets.data_ptr(), num_segments,
                                                   max_segment_len, self.key_type, self.order, s)
        check(st, "gs_segsort16_sort")

    def argsort(self, keys, offsets, positions, n: int | None = None, max_segment_len: int = 0, stream=None) -> None:
        """Sort every segment of ``keys[:n]`` in place and write, for every ``i`` inside the segments, the array index of the element the
        order puts at ``i`` to ``positions[i]`` (4-byte elements, output only: never read, and not written outside the segments).  Needs a
        handle with 4-byte values."""
        from .onesweep import _require_cuda, _require_room, _stream_ptr
        if self.mode != MODE_PAIRS or self.value_bytes != 4:
            raise ValueError("argsort needs a sorter built with MODE_PAIRS and 4-byte values")
        n, num_segments = self._args(keys, offsets, n)
        _require_cuda(positions, "positions")
        _require_room(positions, n, "positions")
        if positions.element_size() != 4:
            raise ValueError("positions must have 4-byte elements")
        max_segment_len = int(max_segment_len)
        alt_k, alt_v = self._alt(n, max_segment_len)
        check(self._lib.gs_segsort16_argsort(self._h, keys.data_ptr(), positions.data_ptr(), alt_k, alt_v, n, offsets.data_ptr(), num_segments,
                                             max_segment_len, self.key_type, self.order, _stream_ptr(stream)), "gs_segsort16_argsort")

    def status(self, stream=None) -> int:
        """``gs_segsort16_check`` as a status code (synchronises): GS_OK, GS_ERR_ARG (bad offsets), GS_ERR_SIZE (promise broken) ..."""
        from .onesweep import _stream_ptr
        return int(self._lib.gs_segsort16_check(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), "gs_segsort16_check")

    def last_classes(self, stream=None) -> dict:
        """Segments per length class in the last call and the longest segment seen (synchronises)."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * (SEGSORT_CLASSES + 1))()
        check(self._lib.gs_segsort16_last_classes(self._h, buf, SEGSORT_CLASSES + 1, _stream_ptr(stream)), "gs_segsort16_last_classes")
        return {"counts": [int(x) for x in buf[:SEGSORT_CLASSES]], "longest": int(buf[SEGSORT_CLASSES])}

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): the units counted on the device, the kernel forms it launched (the bits of
        ``SEGSORT16_FORMS``), status, rank mode."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_SEGSORT16_REPORT_WORDS)()
        check(self._lib.gs_segsort16_last(self._h, buf, _lib.GS_SEGSORT16_REPORT_WORDS, _stream_ptr(stream)), "gs_segsort16_last")
        r = [int(x) for x in buf]
        return {"units": r[_lib.GS_SEGSORT16_R_UNITS], "forms": r[_lib.GS_SEGSORT16_R_FORMS] | (r[_lib.GS_SEGSORT16_R_WG_FORMS] << 32),
                "status": r[_lib.GS_SEGSORT16_R_STATUS], "rank_mode": r[_lib.GS_SEGSORT16_R_RANK], "long_segments": r[_lib.GS_SEGSORT16_R_LONG],
                "unit_cap": r[_lib.GS_SEGSORT16_R_UNIT_CAP], "n": r[_lib.GS_SEGSORT16_R_N]}
