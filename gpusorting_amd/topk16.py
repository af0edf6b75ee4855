"""1-D top-k on 16-bit keys over the C-ABI (``gs_topk16_*`` in include/gpusort.h): the first k elements of the sorted order of one
array of float16, bfloat16, int16 or uint16 keys — keys, and values or input positions — read at their own width, without sorting the
rest and without any scratch that grows with the array.

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.  The numpy statement of
the semantics is ``topk_reference`` (topk.py) on ``uint16`` bit patterns with a 16-bit key type.
"""
from __future__ import annotations

from . import _handle, _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .topk import MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING, _TopKCalls, topk_reference  # noqa: F401

ROUTE_NONE, ROUTE_TILE, ROUTE_COUNT, ROUTE_SELECT = 0, 1, 2, 3
HIST_AUTO, HIST_SLICES, HIST_GLOBAL = 0, 1, 2  # the COUNT route's histogram (gs_topk16_set_count_histogram)
COUNT_SLICES_MIN = _lib.GS_TOPK16_COUNT_SLICES_MIN
_REPORT = ("route", "threshold", "in_front", "equal", "taken", "ranges", "status", "per_range", "hist")


def temp_bytes(max_keys: int, max_k: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_topk16_temp_bytes`` (host only): independent of ``max_keys``; 0 for invalid sizes, mode or value width."""
    return int(_lib.load().gs_topk16_temp_bytes(max_keys, max_k, mode, value_bytes))


class TopK16(_TopKCalls):
    """One ``gs_topk16`` handle: the histogram scratch and, with values, an embedded ``gs_sort16`` handle for the final sort of k.

    ``value_bytes`` 0 selects keys only; 4 or 8 carries values; on a 4-byte handle ``select(keys, k, out_keys, None, out_vals)``
    delivers the input positions as values."""

    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_topk16_", 2, _handle.KEY16_TYPES
    _KEYS_WANTED = "TopK16 takes 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16); 32-bit keys go to TopK"

    def __init__(self, max_keys: int, max_k: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        self._open(max_keys, max_k, order, key_type, mode, value_bytes, device)

    @property
    def temp_bytes(self) -> int:
        return temp_bytes(self.max_keys, self.max_k, self.mode, self.value_bytes)

    def set_count_histogram(self, which: int) -> None:
        """Which histogram the COUNT route runs from the next call on: ``HIST_AUTO`` (by n, the default), ``HIST_SLICES`` or
        ``HIST_GLOBAL``; the result is the same bit for bit."""
        self._call("set_count_histogram", which)

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, threshold (the k-th key as sortable 16 bits), in_front, equal, taken,
        ranges, status, per_range, hist (the histogram a COUNT call ran: ``HIST_SLICES`` or ``HIST_GLOBAL``)."""
        return self._report("last", _lib.GS_TOPK16_REPORT_WORDS, _handle._indexed(_REPORT), stream)
