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

import numpy as np

from . import _lib, rowsort
from ._handle import KEY16_TYPES, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING, _require_cuda, _stream_ptr  # noqa: F401
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .rowsort import ROUTE_LDS, ROUTE_NONE, ROUTE_PASSES, _plan, _rows_reference  # noqa: F401
from .segsort import sortable_bits  # noqa: F401

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
    return _rows_reference(keys, values, key_type, descending, 2)


def sort_rows16_plan(rows: int, row_len: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> dict:
    """``gs_sort_rows16_plan`` (host only): the route of a call and how its rows are cut."""
    return _plan("gs_sort_rows16_plan", rows, row_len, mode, value_bytes)


class RowSort16(rowsort.RowSort):
    """One ``gs_sort_rows16`` handle + lazily sized alt buffers (the pass route's scratch; the LDS route needs none): ``RowSort`` on
    2-byte key tensors, and ``argsort``."""

    _PREFIX, _KEY_BYTES, _KEY_TYPES, _ALT_DTYPE = "gs_sort_rows16_", 2, KEY16_TYPES, "int16"
    _KEYS_WANTED = "RowSort16 takes 16-bit key types only"

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        super().__init__(max_keys, order, key_type, mode, value_bytes, device)

    def argsort(self, keys, positions, stream=None) -> None:
        """Sort every row of ``keys`` in place and write the positions within the row of the sorted order to ``positions`` (same shape,
        4-byte elements, output only: never read).  Needs a handle with 4-byte values."""
        if self.mode != MODE_PAIRS or self.value_bytes != 4:
            raise ValueError("argsort needs a sorter built with MODE_PAIRS and 4-byte values")
        rows, row_len, (alt_k, alt_v) = self._shape(keys)
        _require_cuda(positions, "positions")
        if positions.shape != keys.shape or not positions.is_contiguous() or positions.element_size() != 4:
            raise ValueError("positions must be a contiguous tensor of the shape of keys with 4-byte elements")
        self._call("argsort", keys.data_ptr(), positions.data_ptr(), alt_k, alt_v, rows, row_len, self.key_type, self.order, _stream_ptr(stream))
