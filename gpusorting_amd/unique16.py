"""Unique / run-length encode of 16-bit keys over the C-ABI (``gs_unique16_*`` in include/gpusort.h): the distinct keys of an array of
float16, bfloat16, int16 or uint16 keys in sorted order, how often each occurs, the lowest input position of each, and the inverse
map — from ONE 65 536-bin histogram, without a sort and without scratch that grows with the array — or the run-length encode of the
input as it lies (``unique_consecutive``).

Equality is BITWISE: ``-0.0`` and ``+0.0`` are two keys and every NaN pattern is a key of its own, unlike ``torch.unique`` /
``numpy.unique``, which compare values.  No counterpart in the reference project.  PyTorch is used only for device memory and the
current HIP stream.  The numpy statement of the semantics is ``unique16_reference``.
"""
from __future__ import annotations

import numpy as np

from . import _handle, _lib
from ._handle import _ptr, _require_cuda, _require_room, _stream_ptr
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, check  # noqa: F401
from .segsort import sortable_bits
from .topk import ORDER_ASCENDING, ORDER_DESCENDING  # noqa: F401
from .unique import _out, _runs

ROUTE_NONE, ROUTE_HISTOGRAM, ROUTE_CONSECUTIVE = 0, 1, 2
RAN_FIRST, RAN_INVERSE_LDS, RAN_INVERSE_GATHER = _lib.GS_UNIQUE16_K_FIRST, _lib.GS_UNIQUE16_K_INVERSE_LDS, _lib.GS_UNIQUE16_K_INVERSE_GATHER
INVERSE_AUTO, INVERSE_LDS, INVERSE_GATHER = 0, 1, 2  # the inverse lookup's form (gs_unique16_set_inverse_form)
INVERSE_LDS_MIN = _lib.GS_UNIQUE16_INVERSE_LDS_MIN
BINS = 1 << 16  # a call of ``unique`` never delivers more distinct keys
_REPORT = ("route", "n", "u", "status", "ran", "ranges", "per_range", "tile", "first_ranges", "inverse_ranges")
_KEY_TYPES = _handle.KEY16_TYPES


def unique16_reference(keys: np.ndarray, key_type: int = KEY_UINT16, descending: bool = False, consecutive: bool = False):
    """What ``gs_unique16_unique`` (or, with ``consecutive=True``, ``gs_unique16_consecutive``) delivers for the 2-byte array ``keys``
    (bfloat16 as its uint16 bit patterns): ``(out_keys, counts, first, inverse)`` — the distinct bit patterns as uint16 in the order of
    the library's 16-bit sort (a stable argsort on the sortable bits, reversed for descending), and as uint32 arrays their
    multiplicities, the lowest input position of each, and for every input the index of its key.  ``consecutive=True``: runs of
    bitwise-equal neighbours of the input as it lies (``key_type`` and ``descending`` are not looked at; ``first`` is where each run
    starts)."""
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize != 2 or k.ndim != 1:
        raise ValueError("keys must be a 1-D array of 2-byte elements")
    bits = k.view(np.uint16)
    n = bits.size
    empty = np.zeros(0, np.uint32)
    if n == 0:
        return np.zeros(0, np.uint16), empty, empty.copy(), empty.copy()
    if consecutive:
        perm = np.arange(n, dtype=np.int64)
    else:
        if key_type not in _KEY_TYPES:
            raise ValueError("unique16 takes 16-bit keys (KEY_UINT16, KEY_INT16, KEY_FLOAT16, KEY_BFLOAT16)")
        perm = np.argsort(sortable_bits(bits, key_type), kind="stable")
        if descending:
            perm = perm[::-1]
    return _runs(bits, perm)


def temp_bytes(max_keys: int) -> int:
    """``gs_unique16_temp_bytes`` (host only): independent of ``max_keys``; 0 for an invalid size."""
    return int(_lib.load().gs_unique16_temp_bytes(int(max_keys)))


class Unique16(_handle.Checked, _handle.Handle):
    """One ``gs_unique16`` handle: the histogram, the first-position and rank tables and the run-length stage's per-range words.

    ``unique`` returns tensors of ``min(n, 65 536)`` elements for keys, counts and first (only the first ``u`` are written) and ``n``
    for the inverse, ``unique_consecutive`` ``n`` elements each, plus the one-element count tensor ``num`` on the device; neither waits
    on the host.  Counts, positions and the inverse are int32 tensors holding uint32 values."""

    _PREFIX, _KEY_TYPES = "gs_unique16_", _KEY_TYPES
    _KEYS_WANTED = "Unique16 takes 16-bit keys (KEY_UINT16 .. KEY_BFLOAT16); 32-bit keys go to Unique"

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.order = int(max_keys), order
        self._create(device, self.max_keys)

    @property
    def temp_bytes(self) -> int:
        return temp_bytes(self.max_keys)

    def _keys(self, keys, n):
        _require_cuda(keys, "keys")
        if keys.element_size() != 2:
            raise ValueError("keys must be 16-bit")
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        return n

    def unique(self, keys, n: int | None = None, counts: bool = True, first: bool = True, inverse: bool = True, stream=None):
        """``gs_unique16_unique``: ``(out_keys, out_counts | None, out_first | None, out_inverse | None, num)``.  ``keys`` is not
        written."""
        n = self._keys(keys, n)
        cap = min(n, BINS)
        out_k = _out(keys, cap, dtype=keys.dtype)
        out_c, out_f, out_i, num = _out(keys, cap, counts), _out(keys, cap, first), _out(keys, n, inverse), _out(keys, 1)
        self._call("unique", keys.data_ptr(), n, out_k.data_ptr(), _ptr(out_c), _ptr(out_f), _ptr(out_i), num.data_ptr(), self.key_type,
                   self.order, _stream_ptr(stream))
        return out_k, out_c, out_f, out_i, num

    def unique_consecutive(self, keys, n: int | None = None, counts: bool = True, inverse: bool = True, stream=None):
        """``gs_unique16_consecutive``: the run-length encode of ``keys`` as it lies: ``(out_keys, out_counts | None, out_inverse | None,
        num)``."""
        n = self._keys(keys, n)
        out_k, out_c, out_i, num = _out(keys, n, dtype=keys.dtype), _out(keys, n, counts), _out(keys, n, inverse), _out(keys, 1)
        self._call("consecutive", keys.data_ptr(), n, out_k.data_ptr(), _ptr(out_c), _ptr(out_i), num.data_ptr(), _stream_ptr(stream))
        return out_k, out_c, out_i, num

    def set_inverse_form(self, which: int) -> None:
        """Which form of the inverse lookup ``unique`` runs from the next call on: ``INVERSE_AUTO`` (by n, the default), ``INVERSE_LDS``
        or ``INVERSE_GATHER``; the result is the same bit for bit."""
        self._call("set_inverse_form", which)

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, n, u, status, ran (``RAN_*`` bits: the optional kernels launched), ranges,
        per_range, tile, first_ranges and inverse_ranges (the workgroups of the first-position and the inverse kernel)."""
        return self._report("last", _lib.GS_UNIQUE16_REPORT_WORDS, _handle._indexed(_REPORT), stream)
