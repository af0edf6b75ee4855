"""Row-wise sort over the C-ABI (``gs_sort_rows_*`` in include/gpusort.h): every row of a contiguous ``[rows, row_len]`` matrix of
32-bit keys sorted on its own in one call, keys only or with 4- or 8-byte values — ``torch.sort(x, dim=-1)`` with the library's
semantics.  Rows that fit LDS run on the segmented sort's kernels; longer rows take four stable 8-bit passes over all rows at once
(13 launches whatever the number of rows, no host wait, capturable into a graph).

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.
``sort_rows_reference`` is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle, _lib
from ._handle import (KEY32_TYPES, KEY_FLOAT32, KEY_INT32, KEY_UINT32, MODE_KEYS_ONLY, MODE_PAIRS,  # noqa: F401
                      ORDER_ASCENDING, ORDER_DESCENDING, _require_cuda, _stream_ptr)
from ._lib import check
from .segsort import sortable_bits

ROUTE_NONE, ROUTE_LDS, ROUTE_PASSES = _lib.GS_SORT_ROWS_ROUTE_NONE, _lib.GS_SORT_ROWS_ROUTE_LDS, _lib.GS_SORT_ROWS_ROUTE_PASSES
SORT_ROWS_FORMS = {"clear": _lib.GS_SORT_ROWS_F_CLEAR, "offsets": _lib.GS_SORT_ROWS_F_OFFSETS, "lds": _lib.GS_SORT_ROWS_F_LDS,
                   "count": _lib.GS_SORT_ROWS_F_COUNT, "scan": _lib.GS_SORT_ROWS_F_SCAN}
for _v, _name in enumerate(("keys", "v4", "v8")):
    for _r in (0, 1):
        SORT_ROWS_FORMS[f"scatter_{_name}_rank{_r}"] = _lib.GS_SORT_ROWS_F_SCATTER << (2 * _v + _r)
_PLAN = (("route", _lib.GS_SORT_ROWS_P_ROUTE), ("parts", _lib.GS_SORT_ROWS_P_PARTS), ("per_part", _lib.GS_SORT_ROWS_P_PER_PART),
         ("tile", _lib.GS_SORT_ROWS_P_TILE), ("passes", _lib.GS_SORT_ROWS_P_PASSES), ("cap", _lib.GS_SORT_ROWS_P_CAP))
_REPORT = (("route", _lib.GS_SORT_ROWS_R_ROUTE), ("rows", _lib.GS_SORT_ROWS_R_ROWS), ("row_len", _lib.GS_SORT_ROWS_R_ROW_LEN),
           ("parts", _lib.GS_SORT_ROWS_R_PARTS), ("per_part", _lib.GS_SORT_ROWS_R_PER_PART), ("forms", _lib.GS_SORT_ROWS_R_FORMS),
           ("status", _lib.GS_SORT_ROWS_R_STATUS), ("rank_mode", _lib.GS_SORT_ROWS_R_RANK))


def _rows_reference(keys, values, key_type, descending, key_bytes: int):
    """``sort_rows_reference`` / ``sort_rows16_reference`` behind their key-type checks."""
    keys = np.ascontiguousarray(keys)
    if keys.ndim != 2 or keys.dtype.itemsize != key_bytes:
        raise ValueError(f"keys must be a 2-D array of {key_bytes}-byte elements")
    bits = sortable_bits(keys.reshape(-1), key_type).reshape(keys.shape)
    perm = np.argsort(bits, axis=1, kind="stable")
    if descending:
        perm = perm[:, ::-1]
    out = np.take_along_axis(keys, perm, axis=1)
    if values is None:
        return out, np.ascontiguousarray(perm).astype(np.uint32)
    values = np.ascontiguousarray(values)
    if values.shape != keys.shape:
        raise ValueError("values must have the shape of keys")
    return out, np.take_along_axis(values, perm, axis=1)


def sort_rows_reference(keys: np.ndarray, values: np.ndarray | None = None, key_type: int = KEY_UINT32, descending: bool = False):
    """Every row of the 2-D array ``keys`` (4-byte elements) sorted on its own: stable argsort on the sortable bits per row, the row
    reversed as a whole for descending.  Returns ``(keys, positions)`` (positions: uint32 positions within the row of the sorted
    order) or, with ``values`` (same shape), ``(keys, values)``; new arrays, dtypes kept."""
    if key_type not in KEY32_TYPES:
        raise ValueError("32-bit key types only")
    return _rows_reference(keys, values, key_type, descending, 4)


def _plan(entry: str, rows: int, row_len: int, mode: int, value_bytes: int) -> dict:
    p = (C.c_uint32 * _lib.GS_SORT_ROWS_PLAN_WORDS)()
    check(getattr(_lib.load(), entry)(int(rows), int(row_len), mode, value_bytes, p), entry)
    return {name: int(p[i]) for name, i in _PLAN}


def sort_rows_plan(rows: int, row_len: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> dict:
    """``gs_sort_rows_plan`` (host only): the route of a call and how its rows are cut."""
    return _plan("gs_sort_rows_plan", rows, row_len, mode, value_bytes)


class RowSort(_handle.Checked, _handle.RankMode, _handle.AltBuffers, _handle.Handle):
    """One ``gs_sort_rows`` handle + lazily sized alt buffers (the pass route's scratch; the LDS route needs none)."""

    # what the key width decides (RowSort16, rowsort16.py, states its own)
    _PREFIX, _KEY_BYTES, _KEY_TYPES, _ALT_DTYPE = "gs_sort_rows_", 4, KEY32_TYPES, "int32"
    _KEYS_WANTED = "RowSort takes 32-bit key types only"

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT32, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys = int(max_keys)
        self._pairs_mode(order, mode, value_bytes)
        self._create(device, self.max_keys, mode, self.value_bytes)

    def _shape(self, keys):
        """``(rows, row_len, (alt_keys, alt_values))`` of a call on ``keys``; the alternate buffers only where the rows take the passes."""
        _require_cuda(keys, "keys")
        if keys.dim() != 2 or not keys.is_contiguous() or keys.element_size() != self._KEY_BYTES:
            raise ValueError(f"keys must be a contiguous 2-D tensor of {self._KEY_BYTES}-byte elements")
        rows, row_len = keys.shape
        passes = row_len > self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes)
        return rows, row_len, (self._alt(rows * row_len) if passes else (None, None))

    def sort(self, keys, values=None, stream=None) -> None:
        """Sort every row of the contiguous 2-D tensor ``keys`` (elements of the handle's key width; and carry ``values``, same shape)
        in place on the current stream."""
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        rows, row_len, (alt_k, alt_v) = self._shape(keys)
        s = _stream_ptr(stream)
        if values is None:
            return self._call("keys", keys.data_ptr(), alt_k, rows, row_len, self.key_type, self.order, s)
        _require_cuda(values, "values")
        if values.shape != keys.shape or not values.is_contiguous() or values.element_size() != self.value_bytes:
            raise ValueError(f"values must be a contiguous tensor of the shape of keys with {self.value_bytes}-byte elements")
        self._call("pairs", keys.data_ptr(), values.data_ptr(), alt_k, alt_v, rows, row_len, self.key_type, self.order, s)

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, shape, parts per row, the kernel forms it launched, status."""
        return self._report("last", _lib.GS_SORT_ROWS_REPORT_WORDS, _REPORT, stream)
