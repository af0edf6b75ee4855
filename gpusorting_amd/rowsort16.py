"""Row-wise sort of 16-bit keys over the C-ABI (``gs_sort_rows16_*`` in include/gpusort.h): every row of a contiguous
``[rows, row_len]`` matrix of float16, bfloat16, int16 or uint16 keys sorted on its own in one call, at the keys' own width — keys
only, with 4- or 8-byte values, or as an argsort whose positions within the row the kernels make themselves:
``torch.sort(x, dim=-1)`` on half tensors with the library's semantics.  Rows that fit LDS take one launch of the row-wise top-k's
2-byte LDS sorts, in place; longer rows take two stable 8-bit passes over all rows at once (7 launches whatever the number of rows, no
host wait, capturable into a graph).

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.
``sort_rows16_reference`` is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .segsort import KEY16_TYPES, sortable_bits

MODE_KEYS_ONLY, MODE_PAIRS = 0, 1
ORDER_ASCENDING, ORDER_DESCENDING = 0, 1
ROUTE_NONE, ROUTE_LDS, ROUTE_PASSES = _lib.GS_SORT_ROWS_ROUTE_NONE, _lib.GS_SORT_ROWS_ROUTE_LDS, _lib.GS_SORT_ROWS_ROUTE_PASSES
SORT_ROWS16_FORMS = {"clear": _lib.GS_SORT_ROWS16_F_CLEAR, "lds_wave": _lib.GS_SORT_ROWS16_F_LDS_WAVE, "lds_tile": _lib.GS_SORT_ROWS16_F_LDS_TILE,
                     "count": _lib.GS_SORT_ROWS16_F_COUNT, "scan": _lib.GS_SORT_ROWS16_F_SCAN}
for _v, _name in enumerate(("keys", "pos", "v4", "v8")):
    for _r in (0, 1):
        SORT_ROWS16_FORMS[f"scatter_{_name}_rank{_r}"] = _lib.GS_SORT_ROWS16_F_SCATTER << (2 * _v + _r)


def sort_rows16_reference(keys: np.ndarray, values: np.ndarray | None = None, key_type: int = KEY_UINT16, descending: bool = False):
    """Every row of the 2-D array ``keys`` (2-byte elements, bfloat16 as its uint16 bit patterns) sorted on its own: stable argsort on
    the sortable 16 bits per row, the row reversed as a whole for descending.  Returns ``(keys, positions)`` (positions: uint32 positions
    within the row of the sorted order) or, with ``values`` (same shape), ``(keys, values)``; new arrays, dtypes kept."""
    if key_type not in KEY16_TYPES:
        raise ValueError("16-bit key types only")
    keys = np.ascontiguousarray(keys)
    if keys.ndim != 2 or keys.dtype.itemsize != 2:
        raise ValueError("keys must be a 2-D array of 2-byte elements")
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


def sort_rows16_plan(rows: int, row_len: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> dict:
    """``gs_sort_rows16_plan`` (host only): the route of a call and how its rows are cut."""
    p = (C.c_uint32 * _lib.GS_SORT_ROWS_PLAN_WORDS)()
    check(_lib.load().gs_sort_rows16_plan(int(rows), int(row_len), mode, value_bytes, p), "gs_sort_rows16_plan")
    return {"route": int(p[_lib.GS_SORT_ROWS_P_ROUTE]), "parts": int(p[_lib.GS_SORT_ROWS_P_PARTS]), "per_part": int(p[_lib.GS_SORT_ROWS_P_PER_PART]),
            "tile": int(p[_lib.GS_SORT_ROWS_P_TILE]), "passes": int(p[_lib.GS_SORT_ROWS_P_PASSES]), "cap": int(p[_lib.GS_SORT_ROWS_P_CAP])}


class RowSort16:
    """One ``gs_sort_rows16`` handle + lazily sized alt buffers (the pass route's scratch; the LDS route needs none)."""

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type not in KEY16_TYPES:
            raise ValueError("RowSort16 takes 16-bit key types only")
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys = int(max_keys)
        self.order, self.key_type, self.mode = order, key_type, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0
        h = C.c_void_p()
        check(self._lib.gs_sort_rows16_create(C.byref(h), self.max_keys, mode, self.value_bytes), "gs_sort_rows16_create")
        self._h = h
        self._alt_keys = self._alt_vals = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gs_sort_rows16_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rank_mode(self) -> int:
        return int(self._lib.gs_sort_rows16_get_rank_mode(self._h))

    def set_rank_mode(self, mode: int) -> None:
        check(self._lib.gs_sort_rows16_set_rank_mode(self._h, int(mode)), "gs_sort_rows16_set_rank_mode")

    def _alt(self, n: int):
        import torch
        if self._alt_keys is None or self._alt_keys.numel() < n:
            self._alt_keys = torch.empty(max(n, 1), dtype=torch.int16, device=self.device)
        if self.value_bytes == 0:
            return self._alt_keys.data_ptr(), None
        if self._alt_vals is None or self._alt_vals.numel() < n:
            self._alt_vals = torch.empty(max(n, 1), dtype=torch.int32 if self.value_bytes == 4 else torch.int64, device=self.device)
        return self._alt_keys.data_ptr(), self._alt_vals.data_ptr()

    def _shape(self, keys):
        from .onesweep import _require_cuda
        _require_cuda(keys, "keys")
        if keys.dim() != 2 or not keys.is_contiguous() or keys.element_size() != 2:
            raise ValueError("keys must be a contiguous 2-D tensor of 2-byte elements")
        rows, row_len = keys.shape
        passes = row_len > self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes)
        return rows, row_len, (self._alt(rows * row_len) if passes else (None, None))

    def sort(self, keys, values=None, stream=None) -> None:
        """Sort every row of the contiguous 2-D tensor ``keys`` (2-byte elements; and carry ``values``, same shape) in place on the
        current stream."""
        from .onesweep import _require_cuda, _stream_ptr
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        rows, row_len, (alt_k, alt_v) = self._shape(keys)
        s = _stream_ptr(stream)
        if values is None:
            check(self._lib.gs_sort_rows16_keys(self._h, keys.data_ptr(), alt_k, rows, row_len, self.key_type, self.order, s), "gs_sort_rows16_keys")
            return
        _require_cuda(values, "values")
        if values.shape != keys.shape or not values.is_contiguous() or values.element_size() != self.value_bytes:
            raise ValueError(f"values must be a contiguous tensor of the shape of keys with {self.value_bytes}-byte elements")
        check(self._lib.gs_sort_rows16_pairs(self._h, keys.data_ptr(), values.data_ptr(), alt_k, alt_v, rows, row_len, self.key_type, self.order, s),
              "gs_sort_rows16_pairs")

    def argsort(self, keys, positions, stream=None) -> None:
        """Sort every row of ``keys`` in place and write the positions within the row of the sorted order to ``positions`` (same shape,
        4-byte elements, output only: never read).  Needs a handle with 4-byte values."""
        from .onesweep import _require_cuda, _stream_ptr
        if self.mode != MODE_PAIRS or self.value_bytes != 4:
            raise ValueError("argsort needs a sorter built with MODE_PAIRS and 4-byte values")
        rows, row_len, (alt_k, alt_v) = self._shape(keys)
        _require_cuda(positions, "positions")
        if positions.shape != keys.shape or not positions.is_contiguous() or positions.element_size() != 4:
            raise ValueError("positions must be a contiguous tensor of the shape of keys with 4-byte elements")
        check(self._lib.gs_sort_rows16_argsort(self._h, keys.data_ptr(), positions.data_ptr(), alt_k, alt_v, rows, row_len, self.key_type, self.order,
                                               _stream_ptr(stream)), "gs_sort_rows16_argsort")

    def status(self, stream=None) -> int:
        """``gs_sort_rows16_check`` as a status code (synchronises)."""
        from .onesweep import _stream_ptr
        return int(self._lib.gs_sort_rows16_check(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), "gs_sort_rows16_check")

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, shape, parts per row, the kernel forms it launched, status."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_SORT_ROWS_REPORT_WORDS)()
        check(self._lib.gs_sort_rows16_last(self._h, buf, _lib.GS_SORT_ROWS_REPORT_WORDS, _stream_ptr(stream)), "gs_sort_rows16_last")
        r = [int(x) for x in buf]
        return {"route": r[_lib.GS_SORT_ROWS_R_ROUTE], "rows": r[_lib.GS_SORT_ROWS_R_ROWS], "row_len": r[_lib.GS_SORT_ROWS_R_ROW_LEN],
                "parts": r[_lib.GS_SORT_ROWS_R_PARTS], "per_part": r[_lib.GS_SORT_ROWS_R_PER_PART], "forms": r[_lib.GS_SORT_ROWS_R_FORMS],
                "status": r[_lib.GS_SORT_ROWS_R_STATUS], "rank_mode": r[_lib.GS_SORT_ROWS_R_RANK]}
