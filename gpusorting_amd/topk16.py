"""1-D top-k on 16-bit keys over the C-ABI (``gs_topk16_*`` in include/gpusort.h): the first k elements of the sorted order of one
array of float16, bfloat16, int16 or uint16 keys — keys, and values or input positions — read at their own width, without sorting the
rest and without any scratch that grows with the array.

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.  The numpy statement of
the semantics is ``topk_reference`` (topk.py) on ``uint16`` bit patterns with a 16-bit key type.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check
from .topk import MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING, topk_reference  # noqa: F401

ROUTE_NONE, ROUTE_TILE, ROUTE_COUNT, ROUTE_SELECT = 0, 1, 2, 3
HIST_AUTO, HIST_SLICES, HIST_GLOBAL = 0, 1, 2  # the COUNT route's histogram (gs_topk16_set_count_histogram)
COUNT_SLICES_MIN = _lib.GS_TOPK16_COUNT_SLICES_MIN
_REPORT = ("route", "threshold", "in_front", "equal", "taken", "ranges", "status", "per_range", "hist")
_KEY_TYPES = (KEY_UINT16, KEY_INT16, KEY_FLOAT16, KEY_BFLOAT16)


def temp_bytes(max_keys: int, max_k: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_topk16_temp_bytes`` (host only): independent of ``max_keys``; 0 for invalid sizes, mode or value width."""
    return int(_lib.load().gs_topk16_temp_bytes(max_keys, max_k, mode, value_bytes))


class TopK16:
    """One ``gs_topk16`` handle: the histogram scratch and, with values, an embedded ``gs_sort16`` handle for the final sort of k.

    ``value_bytes`` 0 selects keys only; 4 or 8 carries values; on a 4-byte handle ``select(keys, k, out_keys, None, out_vals)``
    delivers the input positions as values."""

    def __init__(self, max_keys: int, max_k: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type not in _KEY_TYPES:
            raise ValueError("TopK16 takes 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16); 32-bit keys go to TopK")
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys, self.max_k = int(max_keys), int(max_k)
        self.order, self.key_type, self.mode = order, key_type, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0
        h = C.c_void_p()
        check(self._lib.gs_topk16_create(C.byref(h), self.max_keys, self.max_k, mode, self.value_bytes), "gs_topk16_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gs_topk16_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def temp_bytes(self) -> int:
        return temp_bytes(self.max_keys, self.max_k, self.mode, self.value_bytes)

    def select(self, keys, k: int, out_keys, values=None, out_values=None, n: int | None = None, stream=None) -> None:
        """The first ``k`` of ``keys[:n]`` in this handle's order into ``out_keys[:k]`` (and ``out_values[:k]``) on the current stream.
        ``values=None`` with ``out_values`` given (4-byte handle): the values are the input positions.  Inputs are not written."""
        from .onesweep import _require_cuda, _require_room, _stream_ptr
        _require_cuda(keys, "keys")
        _require_cuda(out_keys, "out_keys")
        if keys.element_size() != 2 or out_keys.element_size() != 2:
            raise ValueError("keys must be 16-bit")
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
            st = self._lib.gs_topk16_select_keys(self._h, keys.data_ptr(), n, k, out_keys.data_ptr(), self.key_type, self.order, s)
        else:
            st = self._lib.gs_topk16_select_pairs(self._h, keys.data_ptr(), None if values is None else values.data_ptr(), n, k,
                                                  out_keys.data_ptr(), out_values.data_ptr(), self.key_type, self.order, s)
        check(st, "gs_topk16_select")

    def set_count_histogram(self, which: int) -> None:
        """Which histogram the COUNT route runs from the next call on: ``HIST_AUTO`` (by n, the default), ``HIST_SLICES`` or
        ``HIST_GLOBAL``; the result is the same bit for bit."""
        check(self._lib.gs_topk16_set_count_histogram(self._h, which), "gs_topk16_set_count_histogram")

    def status(self, stream=None) -> int:
        """``gs_topk16_check`` as a status code (synchronises)."""
        from .onesweep import _stream_ptr
        return int(self._lib.gs_topk16_check(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), "gs_topk16_check")

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, threshold (the k-th key as sortable 16 bits), in_front, equal, taken,
        ranges, status, per_range, hist (the histogram a COUNT call ran: ``HIST_SLICES`` or ``HIST_GLOBAL``)."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_TOPK16_REPORT_WORDS)()
        check(self._lib.gs_topk16_last(self._h, buf, _lib.GS_TOPK16_REPORT_WORDS, _stream_ptr(stream)), "gs_topk16_last")
        return {name: int(buf[i]) for i, name in enumerate(_REPORT)}
