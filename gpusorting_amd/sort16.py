"""Sort of 16-bit keys over the C-ABI (``gs_sort16_*`` in include/gpusort.h): float16, bfloat16, int16 and uint16 keys sorted at
their own width — keys only (a counting sort, in place), pairs with 4- or 8-byte values, and argsort (two stable 8-bit passes).

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.
``sort16_reference`` is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch and no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .segsort import KEY16_TYPES, sortable_bits

MODE_KEYS_ONLY, MODE_PAIRS = 0, 1
ORDER_ASCENDING, ORDER_DESCENDING = 0, 1
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


class Sort16:
    """One ``gs_sort16`` handle + lazily sized alt buffers (pairs and argsort; keys only needs none)."""

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, mode: int = MODE_KEYS_ONLY,
                 value_bytes: int = 0, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type not in KEY16_TYPES:
            raise ValueError("Sort16 takes 16-bit key types only")
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys = int(max_keys)
        self.order, self.key_type, self.mode = order, key_type, mode
        self.value_bytes = (value_bytes or 4) if mode == MODE_PAIRS else 0
        h = C.c_void_p()
        check(self._lib.gs_sort16_create(C.byref(h), self.max_keys, mode, self.value_bytes), "gs_sort16_create")
        self._h = h
        self._alt_keys = self._alt_vals = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gs_sort16_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rank_mode(self) -> int:
        return int(self._lib.gs_sort16_get_rank_mode(self._h))

    def set_rank_mode(self, mode: int) -> None:
        check(self._lib.gs_sort16_set_rank_mode(self._h, int(mode)), "gs_sort16_set_rank_mode")

    def _alt(self, n: int):
        import torch
        if self._alt_keys is None or self._alt_keys.numel() < n:
            self._alt_keys = torch.empty(max(n, 1), dtype=torch.int16, device=self.device)
        if self._alt_vals is None or self._alt_vals.numel() < n:
            self._alt_vals = torch.empty(max(n, 1), dtype=torch.int32 if self.value_bytes == 4 else torch.int64, device=self.device)
        return self._alt_keys.data_ptr(), self._alt_vals.data_ptr()

    def sort(self, keys, values=None, n: int | None = None, stream=None) -> None:
        """Sort ``keys[:n]`` (2-byte elements; and carry ``values[:n]``) in place on the current stream."""
        from .onesweep import _require_cuda, _require_room, _stream_ptr
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
            check(self._lib.gs_sort16_sort_keys(self._h, keys.data_ptr(), n, self.key_type, self.order, s), "gs_sort16_sort_keys")
            return
        if values.element_size() != self.value_bytes:
            raise ValueError(f"values must be {self.value_bytes} bytes wide for this sorter")
        alt_k, alt_v = self._alt(n)
        check(self._lib.gs_sort16_sort_pairs(self._h, keys.data_ptr(), values.data_ptr(), alt_k, alt_v, n, self.key_type, self.order, s),
              "gs_sort16_sort_pairs")

    def argsort(self, keys, positions, n: int | None = None, stream=None) -> None:
        """Sort ``keys[:n]`` in place and write the input positions of the sorted order to ``positions[:n]`` (4-byte elements, output
        only: never read).  Needs a handle with 4-byte values."""
        from .onesweep import _require_cuda, _require_room, _stream_ptr
        _require_cuda(keys, "keys")
        if keys.element_size() != 2 or positions.element_size() != 4:
            raise ValueError("keys must be 2 and positions 4 bytes wide")
        if self.mode != MODE_PAIRS or self.value_bytes != 4:
            raise ValueError("argsort needs a sorter built with MODE_PAIRS and 4-byte values")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        _require_room(positions, n, "positions")
        alt_k, alt_v = self._alt(n)
        check(self._lib.gs_sort16_argsort(self._h, keys.data_ptr(), positions.data_ptr(), alt_k, alt_v, n, self.key_type, self.order,
                                          _stream_ptr(stream)), "gs_sort16_argsort")

    def status(self, stream=None) -> int:
        """``gs_sort16_check`` as a status code (synchronises)."""
        from .onesweep import _stream_ptr
        return int(self._lib.gs_sort16_check(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), "gs_sort16_check")

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, ranges, elements per range, tile, the kernel forms it launched."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_SORT16_REPORT_WORDS)()
        check(self._lib.gs_sort16_last(self._h, buf, _lib.GS_SORT16_REPORT_WORDS, _stream_ptr(stream)), "gs_sort16_last")
        r = [int(x) for x in buf]
        return {"route": r[_lib.GS_SORT16_R_ROUTE], "ranges": r[_lib.GS_SORT16_R_RANGES], "per_range": r[_lib.GS_SORT16_R_PER_RANGE],
                "tile": r[_lib.GS_SORT16_R_TILE], "forms": r[_lib.GS_SORT16_R_FORMS], "status": r[_lib.GS_SORT16_R_STATUS],
                "n": r[_lib.GS_SORT16_R_N], "rank_mode": r[_lib.GS_SORT16_R_RANK]}
