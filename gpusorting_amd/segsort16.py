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

import numpy as np

from . import _handle, _lib
from ._handle import MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING, _require_cuda, _require_room, _stream_ptr  # noqa: F401
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .segsort import KEY16_TYPES, SEGSORT_CLASSES, _SegmentedSortCalls, segmented_sort_reference  # noqa: F401

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


_REPORT = (("units", _lib.GS_SEGSORT16_R_UNITS), ("forms", _lib.GS_SEGSORT16_R_FORMS), ("wg_forms", _lib.GS_SEGSORT16_R_WG_FORMS),
           ("status", _lib.GS_SEGSORT16_R_STATUS), ("rank_mode", _lib.GS_SEGSORT16_R_RANK), ("long_segments", _lib.GS_SEGSORT16_R_LONG),
           ("unit_cap", _lib.GS_SEGSORT16_R_UNIT_CAP), ("n", _lib.GS_SEGSORT16_R_N))


class SegmentedSort16(_handle.RankMode, _SegmentedSortCalls):
    """One ``gs_segsort16`` handle + lazily sized alt buffers (the long route's scratch; the LDS classes need none): the ``sort``,
    ``last_classes``, ``class_of`` and ``max_lds_segment`` of ``SegmentedSort`` on 2-byte key tensors, a rank mode of its own, and
    ``argsort``."""

    _PREFIX, _KEY_BYTES, _KEY_TYPES, _ALT_DTYPE = "gs_segsort16_", 2, KEY16_TYPES, "int16"
    _KEYS_WANTED = "SegmentedSort16 takes 16-bit key types only"

    def __init__(self, max_keys: int, max_segments: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        self._open(max_keys, max_segments, order, self._check_key_type(key_type), mode, value_bytes, device)

    def argsort(self, keys, offsets, positions, n: int | None = None, max_segment_len: int = 0, stream=None) -> None:
        """Sort every segment of ``keys[:n]`` in place and write, for every ``i`` inside the segments, the array index of the element the
        order puts at ``i`` to ``positions[i]`` (4-byte elements, output only: never read, and not written outside the segments).  Needs a
        handle with 4-byte values."""
        if self.mode != MODE_PAIRS or self.value_bytes != 4:
            raise ValueError("argsort needs a sorter built with MODE_PAIRS and 4-byte values")
        n, num_segments = self._args(keys, offsets, n)
        _require_cuda(positions, "positions")
        _require_room(positions, n, "positions")
        if positions.element_size() != 4:
            raise ValueError("positions must have 4-byte elements")
        max_segment_len = int(max_segment_len)
        alt_k, alt_v = self._alt_for(n, max_segment_len)
        self._call("argsort", keys.data_ptr(), positions.data_ptr(), alt_k, alt_v, n, offsets.data_ptr(), num_segments, max_segment_len,
                   self.key_type, self.order, _stream_ptr(stream))

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): the units counted on the device, the kernel forms it launched (the bits of
        ``SEGSORT16_FORMS``), status, rank mode."""
        r = self._report("last", _lib.GS_SEGSORT16_REPORT_WORDS, _REPORT, stream)
        r["forms"] |= r.pop("wg_forms") << 32
        return r
