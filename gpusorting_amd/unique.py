"""Unique / run-length encode of 32-bit keys over the C-ABI (``gs_unique_*`` in include/gpusort.h): the distinct keys of an array in
sorted order, how often each occurs, the lowest input position of each, and the inverse map — the library's sort followed by one
streaming run-length stage, or that stage alone on the input as it lies (``unique_consecutive``).

Equality is BITWISE: ``-0.0`` and ``+0.0`` are two keys and every NaN pattern is a key of its own, unlike ``torch.unique`` /
``numpy.unique``, which compare values.  No counterpart in the reference project.  PyTorch is used only for device memory and the
current HIP stream.  The numpy statement of the semantics is ``unique_reference``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .segsort import sortable_bits
from .topk import KEY_FLOAT32, KEY_INT32, KEY_UINT32, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING  # noqa: F401

ROUTE_NONE, ROUTE_KEYS, ROUTE_POSITIONS, ROUTE_CONSECUTIVE = 0, 1, 2, 3
_REPORT = ("route", "n", "u", "ranges", "per_range", "tile", "status", "rank")
_KEY_TYPES = (KEY_UINT32, KEY_INT32, KEY_FLOAT32)


def unique_reference(keys: np.ndarray, key_type: int = KEY_UINT32, descending: bool = False, consecutive: bool = False):
    """What ``gs_unique_positions`` (or, with ``consecutive=True``, ``gs_unique_consecutive``) delivers for the 4-byte array ``keys``:
    ``(out_keys, counts, first, inverse)`` as uint32 arrays — the distinct bit patterns in the order of the library's sort (a stable
    argsort on the sortable bits, reversed for descending), their multiplicities, the lowest input position of each, and for every
    input the index of its key.  ``consecutive=True``: runs of bitwise-equal neighbours of the input as it lies (``key_type`` and
    ``descending`` are not looked at; ``first`` is where each run starts)."""
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize != 4 or k.ndim != 1:
        raise ValueError("keys must be a 1-D array of 4-byte elements")
    bits = k.view(np.uint32)
    n = bits.size
    empty = np.zeros(0, np.uint32)
    if n == 0:
        return empty, empty.copy(), empty.copy(), empty.copy()
    if consecutive:
        perm = np.arange(n, dtype=np.int64)
    else:
        if key_type not in _KEY_TYPES:
            raise ValueError("unique takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)")
        perm = np.argsort(sortable_bits(bits, key_type), kind="stable")
        if descending:
            perm = perm[::-1]
    s = bits[perm]
    head = np.ones(n, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    starts = np.flatnonzero(head)
    rank = np.cumsum(head) - 1  # the run of every sorted element
    counts = np.diff(np.append(starts, n))
    first = np.minimum.reduceat(perm, starts)  # ascending: the run's head; descending: its tail
    inverse = np.empty(n, dtype=np.int64)
    inverse[perm] = rank
    return s[starts].copy(), counts.astype(np.uint32), first.astype(np.uint32), inverse.astype(np.uint32)


def temp_bytes(max_keys: int, mode: int = MODE_KEYS_ONLY, value_bytes: int = 0) -> int:
    """``gs_unique_temp_bytes`` (host only); 0 for invalid sizes, mode or value width."""
    return int(_lib.load().gs_unique_temp_bytes(max_keys, mode, value_bytes))


def unique_plan(n: int) -> tuple:
    """``gs_unique_plan`` (host only): ``(ranges, per_range, tile)`` of the run-length stage for ``n`` elements."""
    plan = (C.c_uint32 * 3)()
    check(_lib.load().gs_unique_plan(int(n), plan), "gs_unique_plan")
    return int(plan[0]), int(plan[1]), int(plan[2])


class Unique:
    """One ``gs_unique`` handle: an embedded sorter of capacity ``max_keys`` and the buffers it sorts in.

    ``positions=False`` makes a handle for keys and counts; ``positions=True`` one that also delivers first positions and the inverse
    (its sorter sorts (key, position) pairs).  Every call returns full-capacity tensors (``n`` elements; only the first ``u`` of keys,
    counts and first are written) plus the one-element count tensor ``num`` on the device, and does not wait on the host."""

    # the family of entries behind the class, its key width and key types (unique64.Unique64 states its own)
    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_unique_", 4, _KEY_TYPES
    _KEYS_WANTED = "Unique takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)"

    def _entry(self, name: str):
        return getattr(self._lib, self._PREFIX + name)

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int | None = None, positions: bool = False, device: int | None = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gpusorting_amd needs a GPU: the product path has no CPU fallback")
        if key_type is None:
            key_type = self._KEY_TYPES[0]
        if key_type not in self._KEY_TYPES:
            raise ValueError(self._KEYS_WANTED)
        self._lib = _lib.load()
        if device is not None:
            torch.cuda.set_device(device)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_keys = int(max_keys)
        self.order, self.key_type = order, key_type
        self.mode, self.value_bytes = (MODE_PAIRS, 4) if positions else (MODE_KEYS_ONLY, 0)
        h = C.c_void_p()
        check(self._entry("create")(C.byref(h), self.max_keys, self.mode, self.value_bytes), self._PREFIX + "create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._entry("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_keys, self.mode, self.value_bytes))

    def _keys(self, keys, n):
        from .onesweep import _require_room
        if keys.element_size() != self._KEY_BYTES:
            raise ValueError("keys must be %d-bit" % (8 * self._KEY_BYTES))
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        return n

    def _out(self, keys, n, want: bool, dtype=None):
        import torch
        return torch.empty(n, dtype=dtype or torch.int32, device=keys.device) if want else None

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def unique(self, keys, n: int | None = None, counts: bool = True, stream=None):
        """``gs_unique_keys``: ``(out_keys, out_counts | None, num)``.  ``keys`` is not written."""
        from .onesweep import _stream_ptr
        n = self._keys(keys, n)
        out_k = self._out(keys, n, True, keys.dtype)
        out_c = self._out(keys, n, counts)
        num = self._out(keys, 1, True)
        check(self._entry("keys")(self._h, keys.data_ptr(), n, out_k.data_ptr(), self._ptr(out_c), num.data_ptr(), self.key_type, self.order,
                                       _stream_ptr(stream)), self._PREFIX + "keys")
        return out_k, out_c, num

    def unique_positions(self, keys, n: int | None = None, counts: bool = True, first: bool = True, inverse: bool = True, stream=None):
        """``gs_unique_positions`` (a handle with ``positions=True``): ``(out_keys, out_counts | None, out_first | None, out_inverse | None,
        num)``; positions and the inverse are int32 tensors holding uint32 values."""
        from .onesweep import _stream_ptr
        n = self._keys(keys, n)
        out_k = self._out(keys, n, True, keys.dtype)
        out_c, out_f, out_i = self._out(keys, n, counts), self._out(keys, n, first), self._out(keys, n, inverse)
        num = self._out(keys, 1, True)
        check(self._entry("positions")(self._h, keys.data_ptr(), n, out_k.data_ptr(), self._ptr(out_c), self._ptr(out_f), self._ptr(out_i),
                                            num.data_ptr(), self.key_type, self.order, _stream_ptr(stream)), self._PREFIX + "positions")
        return out_k, out_c, out_f, out_i, num

    def unique_consecutive(self, keys, n: int | None = None, counts: bool = True, inverse: bool = True, stream=None):
        """``gs_unique_consecutive``: the run-length encode of ``keys`` as it lies: ``(out_keys, out_counts | None, out_inverse | None,
        num)``."""
        from .onesweep import _stream_ptr
        n = self._keys(keys, n)
        out_k = self._out(keys, n, True, keys.dtype)
        out_c, out_i = self._out(keys, n, counts), self._out(keys, n, inverse)
        num = self._out(keys, 1, True)
        check(self._entry("consecutive")(self._h, keys.data_ptr(), n, out_k.data_ptr(), self._ptr(out_c), self._ptr(out_i), num.data_ptr(),
                                              _stream_ptr(stream)), self._PREFIX + "consecutive")
        return out_k, out_c, out_i, num

    def status(self, stream=None) -> int:
        """``gs_unique_check`` as a status code (synchronises)."""
        from .onesweep import _stream_ptr
        return int(self._entry("check")(self._h, _stream_ptr(stream)))

    def check(self, stream=None) -> None:
        """Raises ``GpuSortError`` unless the last call went through (synchronises)."""
        check(self.status(stream), self._PREFIX + "check")

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, n, u, ranges, per_range, tile, status, rank (the sorter's rank mode)."""
        from .onesweep import _stream_ptr
        buf = (C.c_uint32 * _lib.GS_UNIQUE_REPORT_WORDS)()
        check(self._entry("last")(self._h, buf, _lib.GS_UNIQUE_REPORT_WORDS, _stream_ptr(stream)), self._PREFIX + "last")
        return {name: int(buf[i]) for i, name in enumerate(_REPORT)}
