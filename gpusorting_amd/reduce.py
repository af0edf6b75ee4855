"""Reduce by key over the C-ABI (``gs_reduce_*`` in include/gpusort.h): one sum, minimum or maximum per distinct 32-bit key — the
library's stable sort of (key, value) pairs followed by one segmented reduction, or that stage alone on runs of equal neighbouring
keys of the input as it lies (``reduce_by_key_consecutive``, thrust's ``reduce_by_key``).  It is what ``unique(return_inverse=True)``
plus ``index_add_`` / ``scatter_reduce`` computes, without the inverse, without a gather and without atomics on the values.

Key equality is BITWISE, as in ``unique``.  Integer sums wrap.  MIN / MAX on floats use this library's TOTAL ORDER of floats
(``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN``) and return one of the inputs bit for bit: this DIFFERS from ``torch.amin`` /
``amax`` (which propagate NaNs) and from ``fmin`` / ``fmax`` (which drop them).  A float sum is combined in a tree fixed by n and the
run's place in the sorted array: two calls give bitwise identical output, but it is not the left-to-right sequential sum, and
ascending and descending may differ in the last bits.  No counterpart in the reference project.  PyTorch is used only for device
memory and the current HIP stream.  The numpy statement of the semantics is ``reduce_by_key_reference``.
"""
from __future__ import annotations

import numpy as np

from . import _handle, _lib
from ._handle import _ptr, _require_room, _stream_ptr
from ._lib import check  # noqa: F401
from .segsort import sortable_bits
from .topk import KEY_FLOAT32, KEY_INT32, KEY_UINT32, ORDER_ASCENDING, ORDER_DESCENDING  # noqa: F401

VALUE_INT32, VALUE_UINT32, VALUE_FLOAT32, VALUE_INT64, VALUE_UINT64, VALUE_FLOAT64 = range(6)
OP_SUM, OP_MIN, OP_MAX = range(3)
OPS = {"sum": OP_SUM, "min": OP_MIN, "max": OP_MAX}
ROUTE_NONE, ROUTE_SORTED, ROUTE_CONSECUTIVE = 0, 1, 2
_REPORT = ("route", "n", "u", "ranges", "per_range", "tile", "status", "rank", "value_type", "op")
_KEY_TYPES = _handle.KEY32_TYPES
VALUE_DTYPES = {VALUE_INT32: np.int32, VALUE_UINT32: np.uint32, VALUE_FLOAT32: np.float32, VALUE_INT64: np.int64, VALUE_UINT64: np.uint64,
                VALUE_FLOAT64: np.float64}


def value_bytes_of(value_type: int) -> int:
    return np.dtype(VALUE_DTYPES[value_type]).itemsize


def value_order_bits(values: np.ndarray, value_type: int) -> np.ndarray:
    """The unsigned pattern (uint32 / uint64) whose order is the order MIN / MAX use: signed integers flip the sign bit, floats flip
    all bits of negatives too (the sortable bits of the float keys, on the value's width)."""
    u = np.dtype("u%d" % value_bytes_of(value_type))
    b = np.ascontiguousarray(values).view(u)
    top = u.type(1) << u.type(8 * u.itemsize - 1)
    if value_type in (VALUE_UINT32, VALUE_UINT64):
        return b
    if value_type in (VALUE_INT32, VALUE_INT64):
        return b ^ top
    return b ^ np.where(b & top != 0, u.type(~u.type(0)), top).astype(u)


def value_from_order_bits(bits: np.ndarray, value_type: int) -> np.ndarray:
    """The inverse of ``value_order_bits``, as the value's dtype."""
    u = bits.dtype
    top = u.type(1) << u.type(8 * u.itemsize - 1)
    if value_type in (VALUE_UINT32, VALUE_UINT64):
        b = bits
    elif value_type in (VALUE_INT32, VALUE_INT64):
        b = bits ^ top
    else:
        b = bits ^ np.where(bits & top != 0, top, u.type(~u.type(0))).astype(u)
    return np.ascontiguousarray(b).view(VALUE_DTYPES[value_type])


def _reference_values(k: np.ndarray, values: np.ndarray, value_type: int, op: int) -> np.ndarray:
    """The references' check of their values: one per key of ``k``, of ``value_type``'s width; returned in that type's dtype."""
    if value_type not in VALUE_DTYPES or op not in (OP_SUM, OP_MIN, OP_MAX):
        raise ValueError("value_type is one of VALUE_* and op one of OP_SUM, OP_MIN, OP_MAX")
    dtype = np.dtype(VALUE_DTYPES[value_type])
    v = np.ascontiguousarray(values)
    if v.ndim != 1 or v.dtype.itemsize != dtype.itemsize or v.size != k.size:
        raise ValueError("values must be a 1-D array of the value type's width, one per key")
    return v.view(dtype)


def _reference_runs(bits: np.ndarray, v: np.ndarray, perm: np.ndarray, value_type: int, op: int):
    """The references' reduction of every run of ``bits[perm]`` (at least one element): ``(out_keys, out_values, counts)``."""
    n, dtype, is_float = bits.size, v.dtype, value_type in (VALUE_FLOAT32, VALUE_FLOAT64)
    s, sv = bits[perm], v[perm]
    head = np.ones(n, dtype=bool)
    head[1:] = s[1:] != s[:-1]
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, n)).astype(np.uint32)
    if op == OP_SUM:
        if is_float:
            out = np.add.reduceat(sv.astype(np.float64), starts)
        else:
            u = np.dtype("u%d" % dtype.itemsize)
            out = np.add.reduceat(sv.view(u), starts).astype(u).view(dtype)  # modulo 2^32 / 2^64
    else:
        ob = value_order_bits(sv, value_type)
        out = value_from_order_bits((np.minimum if op == OP_MIN else np.maximum).reduceat(ob, starts), value_type)
    return s[starts].copy(), out, counts


def reduce_by_key_reference(keys: np.ndarray, values: np.ndarray, key_type: int = KEY_UINT32, descending: bool = False,
                            value_type: int = VALUE_INT32, op: int = OP_SUM, consecutive: bool = False):
    """What ``gs_reduce_by_key`` (or, with ``consecutive=True``, ``gs_reduce_by_key_consecutive``) delivers for the 4-byte array ``keys``
    and the array ``values`` of ``value_type``'s width: ``(out_keys, out_values, counts)`` — the distinct key bit patterns in the order
    of the library's sort (uint32), the reduction of each key's values, the multiplicities (uint32).  Integer sums wrap and come in the
    value's dtype; FLOAT SUMS ARE SUMMED IN float64 and returned as float64 for the comparison (the device's order of combination is
    its own); MIN / MAX go through ``value_order_bits`` and return one of the inputs bit for bit, in the value's dtype."""
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize != 4 or k.ndim != 1:
        raise ValueError("keys must be a 1-D array of 4-byte elements")
    v = _reference_values(k, values, value_type, op)
    dtype = v.dtype
    bits = k.view(np.uint32)
    n = bits.size
    is_float = value_type in (VALUE_FLOAT32, VALUE_FLOAT64)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float64 if is_float and op == OP_SUM else dtype), np.zeros(0, np.uint32)
    if consecutive:
        perm = np.arange(n, dtype=np.int64)
    else:
        if key_type not in _KEY_TYPES:
            raise ValueError("reduce_by_key takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)")
        perm = np.argsort(sortable_bits(bits, key_type), kind="stable")
        if descending:
            perm = perm[::-1]
    return _reference_runs(bits, v, perm, value_type, op)


def temp_bytes(max_keys: int, value_bytes: int = 4) -> int:
    """``gs_reduce_temp_bytes`` (host only); 0 for invalid sizes or value width."""
    return int(_lib.load().gs_reduce_temp_bytes(max_keys, value_bytes))


def _torch_value_types():
    import torch
    m = {torch.int32: VALUE_INT32, torch.float32: VALUE_FLOAT32, torch.int64: VALUE_INT64, torch.float64: VALUE_FLOAT64}
    if hasattr(torch, "uint32"):
        m[torch.uint32] = VALUE_UINT32
    if hasattr(torch, "uint64"):
        m[torch.uint64] = VALUE_UINT64
    return m


class ReduceByKey(_handle.Checked, _handle.Handle):
    """One ``gs_reduce`` handle: an embedded pairs sorter of capacity ``max_keys`` for values of ``value_bytes`` (4 or 8) and the
    buffers it sorts in.

    Every call returns full-capacity tensors (``n`` elements; only the first ``u`` of keys, values and counts are written) plus the
    one-element count tensor ``num`` on the device, and does not wait on the host.  ``op`` is ``OP_SUM`` / ``OP_MIN`` / ``OP_MAX`` or
    "sum" / "min" / "max"; ``value_type`` defaults to the one of the values' dtype (pass ``VALUE_UINT32`` / ``VALUE_UINT64`` for unsigned
    values in int32 / int64 storage)."""

    # the family of entries behind the class, its key width and key types (reduce64.ReduceByKey64 states its own)
    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_reduce_", 4, _KEY_TYPES
    _KEYS_WANTED = "ReduceByKey takes 32-bit keys (KEY_UINT32, KEY_INT32, KEY_FLOAT32)"

    def __init__(self, max_keys: int, order: int = ORDER_ASCENDING, key_type: int | None = None, value_bytes: int = 4, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.order, self.value_bytes = int(max_keys), order, int(value_bytes)
        self._create(device, self.max_keys, self.value_bytes)

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_keys, self.value_bytes))

    def _reduce(self, entry: str, sorted_by: tuple, keys, values, op, value_type, n, counts, stream):
        """One call of ``by_key`` (``sorted_by``: the key type and the order it takes) or ``by_key_consecutive`` (which takes neither)."""
        import torch
        if keys.element_size() != self._KEY_BYTES:
            raise ValueError("keys must be %d-bit" % (8 * self._KEY_BYTES))
        if value_type is None:
            value_type = _torch_value_types().get(values.dtype)
        if value_type not in VALUE_DTYPES:
            raise ValueError("values must be int32, uint32, float32, int64, uint64 or float64")
        if values.element_size() != value_bytes_of(value_type):
            raise ValueError("the value type does not have the width of the values")
        op = OPS.get(op, op) if isinstance(op, str) else op
        if op not in (OP_SUM, OP_MIN, OP_MAX):
            raise ValueError('op is "sum", "min" or "max"')
        n = keys.numel() if n is None else int(n)
        _require_room(keys, n, "keys")
        _require_room(values, n, "values")
        out_k = torch.empty(n, dtype=keys.dtype, device=keys.device)
        out_v = torch.empty(n, dtype=values.dtype, device=keys.device)
        out_c = torch.empty(n, dtype=torch.int32, device=keys.device) if counts else None
        num = torch.empty(1, dtype=torch.int32, device=keys.device)
        self._call(entry, keys.data_ptr(), values.data_ptr(), n, out_k.data_ptr(), out_v.data_ptr(), _ptr(out_c), num.data_ptr(),
                   *sorted_by, value_type, op, _stream_ptr(stream))
        return out_k, out_v, out_c, num

    def reduce_by_key(self, keys, values, op=OP_SUM, value_type: int | None = None, n: int | None = None, counts: bool = True, stream=None):
        """``gs_reduce_by_key``: ``(out_keys, out_values, out_counts | None, num)``.  ``keys`` and ``values`` are not written."""
        return self._reduce("by_key", (self.key_type, self.order), keys, values, op, value_type, n, counts, stream)

    def reduce_by_key_consecutive(self, keys, values, op=OP_SUM, value_type: int | None = None, n: int | None = None, counts: bool = True,
                                  stream=None):
        """``gs_reduce_by_key_consecutive``: the reduction of every run of bitwise-equal neighbouring keys of the input as it lies:
        ``(out_keys, out_values, out_counts | None, num)``."""
        return self._reduce("by_key_consecutive", (), keys, values, op, value_type, n, counts, stream)

    def last(self, stream=None) -> dict:
        """Diagnostics of the last call (synchronises): route, n, u, ranges, per_range, tile, status, rank (the sorter's rank mode),
        value_type, op."""
        return self._report("last", _lib.GS_REDUCE_REPORT_WORDS, _handle._indexed(_REPORT), stream)
