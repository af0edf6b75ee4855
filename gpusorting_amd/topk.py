"""Top-k selection over the C-ABI (``gs_topk_*`` in include/gpusort.h): the first k elements of the sorted order — keys, and values or
input positions — without sorting the rest.

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.  ``topk_reference`` (and
``topk_rows_reference`` for the row-wise calls, ``gs_topk_select_rows_*``) is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import numpy as np

from . import _handle, _lib
from ._handle import (KEY16_TYPES, KEY_FLOAT32, KEY_INT32, KEY_UINT32, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING,  # noqa: F401
                      _require_cuda, _require_room, _ptr, _stream_ptr)
from ._lib import check  # noqa: F401
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16  # noqa: F401
from .segsort import sortable_bits

ROUTE_NONE, ROUTE_SELECT, ROUTE_FULL_SORT, ROUTE_SINGLE_TILE = 0, 1, 2, 3
_REPORT = ("route", "threshold", "in_front", "equal", "taken", "candidates", "level2", "ranges")
ROWS_ROUTE_NONE, ROWS_ROUTE_WAVE, ROWS_ROUTE_TILE, ROWS_ROUTE_STREAM, ROWS_ROUTE_LOOP = 0, 1, 2, 3, 4
_ROWS_REPORT = ("route", "rows", "row_len", "k", "status", "reads")


def topk_reference(keys: np.ndarray, k: int, values: np.ndarray | None = None, key_type: int = KEY_UINT32, descending: bool = False):
    """The first ``k`` elements of the library's sorted order: stable argsort on the sortable bit pattern, reversed as a whole for
    descending (so ties go to the lowest positions ascending, to the highest descending), first ``k``.  Floats follow the
    order-preserving bit flip: -0 < +0, NaNs by bit pattern (not ``torch.topk``'s NaN rule).  Returns ``(keys_k, values_k)``;
    ``values=None`` returns the input positions (uint32) as values.  The 16-bit key types (``KEY_UINT16`` .. ``KEY_BFLOAT16``, row-wise
    calls only on the device) take 2-byte arrays, bfloat16 as its uint16 bit patterns."""
    keys = np.ascontiguousarray(keys)
    if keys.ndim != 1 or not 1 <= k <= keys.size:
        raise ValueError("keys must be 1-D and 1 <= k <= n")
    perm = np.argsort(sortable_bits(keys, key_type), kind="stable")
    if descending:
        perm = perm[::-1]
    perm = perm[:k]
    vals = perm.astype(np.uint32) if values is None else np.ascontiguousarray(values)[perm]
    return keys[perm], vals


def topk_rows_reference(keys2d: np.ndarray, k: int, values2d: np.ndarray | None = None, key_type: int = KEY_UINT32,
                        descending: bool = False):
    """``topk_reference`` applied to every row of a 2-D array: returns ``(keys[rows, k], values[rows, k])``; ``values2d=None``
    returns the positions within the row (uint32)."""
    keys2d = np.asarray(keys2d)
    if keys2d.ndim != 2 or keys2d.shape[0] == 0:
        raise ValueError("keys must be 2-D with at least one row")
    if values2d is not None and np.asarray(values2d).shape != keys2d.shape:
        raise ValueError("values must match keys in shape")
    rows = [topk_reference(keys2d[r], k, None if values2d is None else np.asarray(values2d)[r], key_type, descending)
            for r in range(keys2d.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def rows_max_k(mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_topk_rows_max_k``: the largest k the one-launch routes take for rows longer than LDS holds (host only)."""
    return int(_lib.load().gs_topk_rows_max_k(mode, value_bytes))


class _TopKCalls(_handle.Checked, _handle.Handle):
    """What ``TopK`` and ``TopK16`` (topk16.py) share: the constructor's frame and the 1-D ``select``."""

    _KEY_BYTES = 4

    def _open(self, max_keys, max_k, order, key_type, mode, value_bytes, device) -> None:
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.max_k = int(max_keys), int(max_k)
        self._pairs_mode(order, mode, value_bytes)
        self._create(device, self.max_keys, self.max_k, mode, self.value_bytes)

    def select(self, keys, k: int, out_keys, values=None, out_values=None, n: int | None = None, stream=None) -> None:
        """The first ``k`` of ``keys[:n]`` in this handle's order into ``out_keys[:k]`` (and ``out_values[:k]``) on the current stream.
        ``values=None`` with ``out_values`` given (4-byte handle): the values are the input positions.  Inputs are not written."""
        _require_cuda(keys, "keys")
        _require_cuda(out_keys, "out_keys")
        if keys.element_size() != self._KEY_BYTES or out_keys.element_size() != self._KEY_BYTES:
            raise ValueError(f"keys must be {8 * self._KEY_BYTES}-bit")
        if (out_values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("out_values must be given exactly when the handle was built with MODE_PAIRS")
        n = keys.numel() if n is None else int(n)
        k = int(k)
        _require_room(keys, n, "keys")
        _require_room(values, n, "values")
        _require_room(out_keys, k, "out_keys")
        _require_room(out_values, k, "out_values")
        for t, name in ((values, "values"), (out_values, "out_values")):
            if t is not None:
                _require_cuda(t, name)
                if t.element_size() != self.value_bytes:
                    raise ValueError(f"{name} must be {self.value_bytes} bytes wide for this handle")
        s = _stream_ptr(stream)
        if out_values is None:
            self._call("select_keys", keys.data_ptr(), n, k, out_keys.data_ptr(), self.key_type, self.order, s, where="select")
        else:
            self._call("select_pairs", keys.data_ptr(), _ptr(values), n, k, out_keys.data_ptr(), out_values.data_ptr(), self.key_type,
                       self.order, s, where="select")


class TopK(_TopKCalls):
    """One ``gs_topk`` handle: the selection's scratch and an embedded OneSweep engine for the final sort of k elements.

    ``value_bytes`` 0 selects keys only; 4 or 8 carries values; on a 4-byte handle ``select(keys, k, out_keys, None, out_vals)``
    delivers the input positions as values."""

    _PREFIX, _KEY_TYPES = "gs_topk_", _handle.KEY32_TYPES + KEY16_TYPES
    _KEYS_WANTED = "the selection takes 32-bit keys, and 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16) in select_rows"

    def __init__(self, max_keys: int, max_k: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT32, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        self._open(max_keys, max_k, order, key_type, mode, value_bytes, device)

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_keys, self.max_k, self.value_bytes))

    @property
    def engine(self):
        """The embedded OneSweep engine, borrowed (``gs_topk_engine``): it runs the single-tile route and the final sort of k, and its
        rank mode is the one the row-wise tile kernels run with.  For ``set_rank_mode`` / ``rank_mode`` / ``check``, with no call in
        flight; it lives as long as this handle."""
        from .onesweep import OneSweep
        cap = max(self.max_k, min(self.max_keys, 32768))
        kt = self.key_type if self.key_type in _handle.KEY32_TYPES else KEY_UINT32
        return OneSweep._borrow(self._entry("engine")(self._h), cap, self.mode, self.value_bytes, kt)

    def select(self, keys, k: int, out_keys, values=None, out_values=None, n: int | None = None, stream=None) -> None:
        """The first ``k`` of ``keys[:n]`` in this handle's order into ``out_keys[:k]`` (and ``out_values[:k]``) on the current stream.
        ``values=None`` with ``out_values`` given (4-byte handle): the values are the input positions.  Inputs are not written."""
        if self.key_type in KEY16_TYPES:
            raise ValueError("the 1-D selection takes 32-bit keys only: 16-bit keys go through select_rows (one row: rows=1)")
        super().select(keys, k, out_keys, values, out_values, n, stream)

    def select_rows(self, keys, rows: int, row_len: int, row_stride: int, k: int, out_keys, values=None, out_values=None, stream=None) -> None:
        """The first ``k`` of every row ``keys[r * row_stride : r * row_stride + row_len]`` (a 2-D or flat tensor; ``row_stride`` in
        elements, any value >= ``row_len``) into ``out_keys[r * k : (r + 1) * k]`` (and ``out_values``) on the current stream.
        ``values=None`` with ``out_values`` given (4-byte handle): the values are the positions within the row.  A handle of a 16-bit
        key type takes 2-byte key tensors (float16, bfloat16, int16, uint16); a row longer than LDS holds with
        ``k > rows_max_k`` is ``GS_ERR_SIZE`` there (no LOOP route)."""
        import torch

        def strided(t, name):  # an input: 1-D, or 2-D with any row stride; the last dimension contiguous
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() not in (1, 2) or t.stride(-1) != 1:
                raise ValueError(f"{name} must be a 1-D or 2-D tensor on the GPU whose last dimension is contiguous")
        strided(keys, "keys")
        if values is not None:
            strided(values, "values")
        _require_cuda(out_keys, "out_keys")
        if out_values is not None:
            _require_cuda(out_values, "out_values")
        key_bytes = 2 if self.key_type in KEY16_TYPES else 4
        if keys.element_size() != key_bytes or out_keys.element_size() != key_bytes:
            raise ValueError(f"keys must be {8 * key_bytes}-bit for this handle's key type")
        if (out_values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("out_values must be given exactly when the handle was built with MODE_PAIRS")
        rows, row_len, row_stride, k = int(rows), int(row_len), int(row_stride), int(k)
        extent = (rows - 1) * row_stride + row_len if rows > 0 else 0

        def room(t):  # elements reachable from the tensor's first one
            return 0 if t.numel() == 0 else 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
        for t, need, name in ((keys, extent, "keys"), (values, extent, "values"), (out_keys, rows * k, "out_keys"),
                              (out_values, rows * k, "out_values")):
            if t is not None and room(t) < need:
                raise ValueError(f"{name} holds {room(t)} elements, {need} are needed")
        for t, name in ((values, "values"), (out_values, "out_values")):
            if t is not None and t.element_size() != self.value_bytes:
                raise ValueError(f"{name} must be {self.value_bytes} bytes wide for this handle")
        s = _stream_ptr(stream)
        if out_values is None:
            self._call("select_rows_keys", keys.data_ptr(), rows, row_len, row_stride, k, out_keys.data_ptr(), self.key_type, self.order, s,
                       where="select_rows")
        else:
            self._call("select_rows_pairs", keys.data_ptr(), _ptr(values), rows, row_len, row_stride, k, out_keys.data_ptr(),
                       out_values.data_ptr(), self.key_type, self.order, s, where="select_rows")

    def rows_last(self, stream=None) -> dict:
        """Diagnostics of the last row-wise call (synchronises): route, rows, row_len, k, status, reads (stream route: the most reads
        of its row any row took)."""
        return self._report("rows_last", _lib.GS_TOPK_ROWS_REPORT_WORDS, _handle._indexed(_ROWS_REPORT), stream)

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, threshold (the k-th key as sortable bits), in_front, equal, taken,
        candidates (left after the first level), level2, ranges."""
        return self._report("last", _lib.GS_TOPK_REPORT_WORDS, _handle._indexed(_REPORT), stream)
