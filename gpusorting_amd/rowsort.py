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

from . import _lib
from ._lib import check
from .segsort import KEY_FLOAT32, KEY_INT32, KEY_UINT32, sortable_bits

MODE_KEYS_ONLY, MODE_PAIRS = 0, 1
ORDER_ASCENDING, ORDER_DESCENDING = 0, 1
KEY32_TYPES = (KEY_UINT32, KEY_INT32, KEY_FLOAT32)
ROUTE_NONE, ROUTE_LDS, ROUTE_PASSES = _lib.GS_SORT_ROWS_ROUTE_NONE, _lib.GS_SORT_ROWS_ROUTE_LDS, _lib.GS_SORT_ROWS_ROUTE_PASSES
SORT_ROWS_FORMS = {"clear": _lib.GS_SORT_ROWS_F_CLEAR, "offsets": _lib.GS_SORT_ROWS_F_OFFSETS, "lds": _lib.GS_SORT_ROWS_F_LDS,
                   "count": _lib.GS_SORT_ROWS_F_COUNT, "scan": _lib.GS_SORT_ROWS_F_SCAN}
for _v, _name in enumerate(("keys", "v4", "v8")):
    for _r in (0, 1):
        SORT_ROWS_FORMS[f"scatter_{_name}_rank{_r}"] = _lib.GS_SORT_ROWS_F_SCATTER << (2 * _v + _r)


def sort_rows_reference(keys: np.ndarray, values: np.ndarray | None = None, key_type: int = KEY_UINT32, descending: bool = False):
    """Every row of the 2-D array ``keys`` (4-byte elements) sorted on its own: stable argsort on the sortable bits per row, the row
    reversed as a whole for descending.  Returns ``(keys, positions)`` (positions: uint32 positions within the row of the sorted
    order) or, with ``values`` (same shape), ``(keys, values)``; new arrays, dtypes kept."""
    if key_type not in KEY32_TYPES:
        raise ValueError("32-bit key types only")
    keys = np.ascontiguousarray(keys)
    if keys.ndim != 2 or keys.dtype.itemsize != 4:
        raise ValueError("keys must be a 2-D array of 4-byte elements")
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


def sort_rows_plan(rows: int, row_len: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> dict:
    """``gs_sort_rows_plan`` (host only): the route of a call and how its rows are cut."""
    p = (C.c_uint32 * _lib.GS_SORT_ROWS_PLAN_WORDS)()
    check(_lib.load().gs_sort_rows_plan(int(rows), int(row_len), mode, value_bytes, p), "gs_sort_rows_plan")
    return {"route": int(p[_lib.GS_SORT_ROWS_P_ROUTE]), "parts": int(p[_lib.GS_SORT_ROWS_P_PARTS]), "per_part": int(p[_lib.GS_SORT_ROWS_P_PER_PART]),
            "tile": int(p[_lib.GS_SORT_ROWS_P_TILE]), "passes": int(p[_lib.GS_SORT_ROWS_P_PASSES]), "cap": int(p[_lib.GS_SORT_ROWS_P_CAP])}


class RowSort:
    """One ``gs_sort_rows`` handle + lazily sized alt buffers (the pass route's scratch; the LDS route needs none)."""

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT32, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type not in KEY32_TYPES:
            raise ValueError("RowSort takes 32-bit key types only")
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys = int(max_keys)
        self.order, self.key_type, self.mode = order, key_type, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0
        h = C.c_void_p()
        check(self._lib.gs_sort_rows_create(C.byref(h), self.max_keys, mode, self.value_bytes), "gs_sort_rows_create")
        self._h = h
        self._alt_keys = self._alt_vals = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gs_sort_rows_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rank_mode(self) -> int:
        return int(self._lib.gs_sort_rows_get_rank_mode(self._h))

    def set_rank_mode(self, mode: int) -> None:
        check(self._lib.gs_sort_rows_set_rank_mode(self._h, int(mode)), "gs_sort_rows_set_rank_mode")

    def _alt(self, n: int):
        import torch
        if self._alt_keys is None or self._alt_keys.numel() < n:
            self._alt_keys = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        if self.value_bytes == 0:
            return self._alt_keys.data_ptr(), None
        if self._alt_vals is None or self._alt_vals.numel() < n:
            self._alt_vals = torch.empty(max(n, 1), dtype=torch.int32 if self.value_bytes == 4 else torch.int64, device=self.device)
        return self._alt_keys.data_ptr(), self._alt_vals.data_ptr()

    def sort(self, keys, values=None, stream=None) -> None:
        """Sort every row of the contiguous 2-D tensor ``keys`` (4-byte elements; and carry ``values``, same shape) in place on the
        current stream."""
        from .onesweep import _require_cuda, _stream_ptr
        _require_cuda(keys, "keys")
        if keys.dim() != 2 or not keys.is_contiguous() or keys.element_size() != 4:
            raise ValueError("keys must be a contiguous 2-D tensor of 4-byte elements")
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        rows, row_len = keys.shape
        s = _stream_ptr(stream)
        passes = row_len > self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes)
        alt_k, alt_v = self._alt(rows * row_len) if passes else (None, None)
        if values is None:
            check(self._lib.gs_sort_rows_keys(self._h, keys.data_ptr(), alt_k, rows, row_len, self.key_type, self.order, s), "gs_sort_rows_keys")
            return
        _require_cuda(values, "values")
        if values.shape != keys.shape or not values.is_contiguous() or values.element_size() != self.value_bytes:
            raise ValueError(f"values must be a contiguous tensor of the shape of keys with {self.value_bytes}-byte elements")
        check(self._lib.gs_sort_rows_pairs(self._h, keys.data_ptr(), values.data_ptr(), alt_k, alt_v, rows, row_len, self.key_type, self.order, s),
              "gs_sort_rows_pairs")

    def status(self, stream=None) -> int:
        """``gs_sort_rows_check`` as a status code (synchronises)."""
        from .onesweep import _stream_ptr
        return int(self._lib.gs_sort_rows_check(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), "gs_sort_rows_check")

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, shape, parts per row, the kernel forms it launched, status."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_SORT_ROWS_REPORT_WORDS)()
        check(self._lib.gs_sort_rows_last(self._h, buf, _lib.GS_SORT_ROWS_REPORT_WORDS, _stream_ptr(stream)), "gs_sort_rows_last")
        r = [int(x) for x in buf]
        return {"route": r[_lib.GS_SORT_ROWS_R_ROUTE], "rows": r[_lib.GS_SORT_ROWS_R_ROWS], "row_len": r[_lib.GS_SORT_ROWS_R_ROW_LEN],
                "parts": r[_lib.GS_SORT_ROWS_R_PARTS], "per_part": r[_lib.GS_SORT_ROWS_R_PER_PART], "forms": r[_lib.GS_SORT_ROWS_R_FORMS],
                "status": r[_lib.GS_SORT_ROWS_R_STATUS], "rank_mode": r[_lib.GS_SORT_ROWS_R_RANK]}
