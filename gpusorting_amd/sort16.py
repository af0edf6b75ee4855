"""Sort of 16-bit keys over the C-ABI (``gs_sort16_*`` in include/gpusort.h): float16, bfloat16, int16 and uint16 keys sorted at
their own width — keys only (a counting sort, in place), pairs with 4- or 8-byte values, and argsort (two stable 8-bit passes).

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.
``sort16_reference`` is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle, _lib
from ._handle import KEY16_TYPES, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING, _require_cuda, _require_room, _stream_ptr  # noqa: F401
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .segsort import sortable_bits

SORT16_FORMS = {"hist": _lib.GS_SORT16_F_HIST, "scan": _lib.GS_SORT16_F_SCAN, "fill": _lib.GS_SORT16_F_FILL, "count": _lib.GS_SORT16_F_COUNT,
                "pscan": _lib.GS_SORT16_F_PSCAN}
for _v, _name in enumerate(("pos", "v4", "v8")):
    for _r in (0, 1):
        SORT16_FORMS[f"scatter_{_name}_rank{_r}"] = _lib.GS_SORT16_F_SCATTER << (2 * _v + _r)


def sort16_reference(keys: np.ndarray, values: np.ndarray | None = None, key_type: int = KEY_UINT16, descending: bool = False):
    """Stable argsort on the sortable 16-bit pattern, reversed as a whole for descending.  ``keys``: 2-byte elements (bfloat16 as its
    uint16 bit patterns).  Returns ``(keys, positions)`` (positions: uint32 input positions of the sorted order) or, with ``values``,
    ``(keys, values)``; new arrays, dtypes kept."""
    if key_type not in KEY16_TYPES:
        raise ValueError("16-bit key types only")
    keys = np.ascontiguousarray(keys)
    perm = np.argsort(sortable_bits(keys, key_type), kind="stable")
    if descending:
        perm = perm[::-1]
    return keys[perm], (perm.astype(np.uint32) if values is None else np.ascontiguousarray(values)[perm])


def sort16_plan(n: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> dict:
    """``gs_sort16_plan`` (host only): how a sort of n elements is cut."""
    p = (C.c_uint32 * 4)()
    check(_lib.load().gs_sort16_plan(int(n), mode, value_bytes, p), "gs_sort16_plan")
    return {"ranges": int(p[0]), "per_range": int(p[1]), "tile": int(p[2]), "cap": int(p[3])}


_REPORT = (("route", _lib.GS_SORT16_R_ROUTE), ("ranges", _lib.GS_SORT16_R_RANGES), ("per_range", _lib.GS_SORT16_R_PER_RANGE),
           ("tile", _lib.GS_SORT16_R_TILE), ("forms", _lib.GS_SORT16_R_FORMS), ("status", _lib.GS_SORT16_R_STATUS), ("n", _lib.GS_SORT16_R_N),
           ("rank_mode", _lib.GS_SORT16_R_RANK))


class Sort16(_handle.Checked, _handle.RankMode, _handle.AltBuffers, _handle.Handle):
    """One ``gs_sort16`` handle + lazily sized alt buffers (pairs and argsort; keys only needs none)."""

    _PREFIX, _KEY_TYPES, _ALT_DTYPE = "gs_sort16_", KEY16_TYPES, "int16"
    _KEYS_WANTED = "Sort16 takes 16-bit key types only"

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys = int(max_keys)
        self._pairs_mode(order, mode, value_bytes)
        self._create(device, self.max_keys, mode, self.value_bytes)

    def sort(self, keys, values=None, n: int | None = None, stream=None) -> None:
        """Sort ``keys[:n]`` (2-byte elements; and carry ``values[:n]``) in place on the current stream."""
        _require_cuda(keys, "keys")
        if keys.element_size() != 2:
            raise ValueError("keys must be 2 bytes wide")
        if (values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("values must be given exactly when the sorter was built with MODE_PAIRS")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        _require_room(values, n, "values")
        s = _stream_ptr(stream)
        if values is None:
            return self._call("sort_keys", keys.data_ptr(), n, self.key_type, self.order, s)
        if values.element_size() != self.value_bytes:
            raise ValueError(f"values must be {self.value_bytes} bytes wide for this sorter")
        alt_k, alt_v = self._alt(n)
        self._call("sort_pairs", keys.data_ptr(), values.data_ptr(), alt_k, alt_v, n, self.key_type, self.order, s)

    def argsort(self, keys, positions, n: int | None = None, stream=None) -> None:
        """Sort ``keys[:n]`` in place and write the input positions of the sorted order to ``positions[:n]`` (4-byte elements, output
        only: never read).  Needs a handle with 4-byte values."""
        _require_cuda(keys, "keys")
        if keys.element_size() != 2 or positions.element_size() != 4:
            raise ValueError("keys must be 2 and positions 4 bytes wide")
        if self.mode != MODE_PAIRS or self.value_bytes != 4:
            raise ValueError("argsort needs a sorter built with MODE_PAIRS and 4-byte values")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        _require_room(positions, n, "positions")
        alt_k, alt_v = self._alt(n)
        self._call("argsort", keys.data_ptr(), positions.data_ptr(), alt_k, alt_v, n, self.key_type, self.order, _stream_ptr(stream))

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, ranges, elements per range, tile, the kernel forms it launched."""
        return self._report("last", _lib.GS_SORT16_REPORT_WORDS, _REPORT, stream)
