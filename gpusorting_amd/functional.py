"""Tensor-in / tensor-out convenience on top of ``OneSweep`` (PyTorch-ROCm plumbing only: dtype -> key type,
handle cache, buffers).  The reference has no such layer; it is what a torch user types:

    sorted_keys = gpusorting_amd.sort(keys)                                  # int32 / uint32-as-int32 / float32,
                                                                             # float16 / bfloat16 / int16 / uint16 (Sort16)
    sorted_keys, sorted_vals = gpusorting_amd.sort(keys, values, descending=True)
    gpusorting_amd.sort_(keys, values)                                       # in place
    sorted_rows = gpusorting_amd.sort(matrix)                                # 2-D: every row on its own, torch.sort(x, dim=-1) (RowSort)
    sorted_rows = gpusorting_amd.sort_rows(half_matrix, descending=True)     # 2-D, 16- and 32-bit keys (RowSort16 / RowSort)
    positions = gpusorting_amd.argsort_rows(half_matrix)                     # int32 positions within the row
    distinct, inverse, counts = gpusorting_amd.unique(keys, return_inverse=True, return_counts=True)   # torch.unique (Unique)
    runs, counts = gpusorting_amd.unique_consecutive(keys, return_counts=True)                         # torch.unique_consecutive
    distinct, sums = gpusorting_amd.reduce_by_key(keys, values, op="sum")   # unique + index_add_ in one call, no atomics (ReduceByKey)
    distinct, index = gpusorting_amd.unique16(half_keys, return_index=True)  # float16 / bfloat16 / int16 / uint16: one histogram (Unique16)
    positions = gpusorting_amd.searchsorted(sorted_keys, queries, right=True, descending=True)  # in THIS library's order (SortedSearch)

Semantics are the library's: stable LSD radix sort; descending = exact reverse of the stable ascending result;
float keys ordered by the order-preserving bit flip (-0 < +0, NaNs by bit pattern); values bit-copied.
"""
from __future__ import annotations

import torch

from . import _lib
from .segsort import SegmentedSort, segmented_sort_reference  # noqa: F401
from .segsort16 import SegmentedSort16, segmented_sort16_reference  # noqa: F401
from .rowsort import RowSort, sort_rows_reference  # noqa: F401
from .rowsort16 import RowSort16, sort_rows16_reference  # noqa: F401
from .segtopk import SegmentedTopK, segmented_topk_reference  # noqa: F401
from .segtopk16 import SegmentedTopK16  # noqa: F401
from .sort16 import Sort16, sort16_reference  # noqa: F401
from .topk import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, TopK, rows_max_k, topk_reference, topk_rows_reference  # noqa: F401
from .topk16 import TopK16  # noqa: F401
from .reduce import OPS as _REDUCE_OPS, ReduceByKey, _torch_value_types, reduce_by_key_reference  # noqa: F401
from .unique import Unique, unique_reference  # noqa: F401
from .unique16 import Unique16, unique16_reference  # noqa: F401
from .unique64 import Unique64, unique64_reference  # noqa: F401
from .reduce64 import ReduceByKey64, reduce_by_key64_reference  # noqa: F401
from .search import ROUTE_SORT as _SEARCH_ROUTE_SORT, SortedSearch, search_plan, searchsorted_reference  # noqa: F401
from .onesweep import (KEY_FLOAT32, KEY_FLOAT64, KEY_INT32, KEY_INT64, KEY_UINT32, KEY_UINT64, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING,
                       ORDER_DESCENDING, OneSweep)

_KEY_TYPE = {torch.int32: KEY_INT32, torch.float32: KEY_FLOAT32, torch.uint32: KEY_UINT32}
# 2-byte keys: sort / sort_ / argsort (Sort16) and the row-wise top-k (torch.uint16 where this torch has it)
_KEY16_TYPE = {torch.float16: KEY_FLOAT16, torch.bfloat16: KEY_BFLOAT16, torch.int16: KEY_INT16}
if hasattr(torch, "uint16"):
    _KEY16_TYPE[torch.uint16] = KEY_UINT16
_KEY64_TYPE = {torch.int64: KEY_INT64, torch.float64: KEY_FLOAT64}
if hasattr(torch, "uint64"):
    _KEY64_TYPE[torch.uint64] = KEY_UINT64
_UNSIGNED = {torch.int16: KEY_UINT16, torch.int32: KEY_UINT32, torch.int64: KEY_UINT64}  # what ``unsigned=True`` makes of signed storage


def _key_type(keys: torch.Tensor, unsigned: bool, table: dict) -> int:
    return _UNSIGNED[keys.dtype] if (unsigned and keys.dtype in _UNSIGNED) else table[keys.dtype]


def _order(descending: bool) -> int:
    return ORDER_DESCENDING if descending else ORDER_ASCENDING


def _mode(value_bytes: int) -> int:
    return MODE_PAIRS if value_bytes else MODE_KEYS_ONLY


# ---- the handle caches: one rule -------------------------------------------------------------------------------------------------
def _cap(x: int, floor_bits: int = 16) -> int:
    """The next power of two (few re-creations while sizes wander), at least ``2^floor_bits``, at most the library's 2^30 - 1."""
    return min(1 << max(int(x - 1).bit_length(), floor_bits), (1 << 30) - 1)


def _on(device: torch.device) -> tuple:
    """(device, stream): the head of every cache key."""
    return device.index, int(torch.cuda.current_stream(device).cuda_stream)


def _cached(cache: dict, key: tuple, asked: dict, factory):
    """The cache rule of every family: the handle under ``key``, closed and re-created by ``factory(**asked)`` when one of the sizes
    ``asked`` (``max_*`` attribute -> what the call needs) outgrows it.  The factory rounds the sizes up (``_cap``)."""
    s = cache.get(key)
    if s is None or any(getattr(s, name) < size for name, size in asked.items()):
        if s is not None:
            s.close()
        s = cache[key] = factory(**asked)
    return s


_cache: dict = {}


def _flat_sorter(cls, tag: tuple, device: torch.device, n: int, key_type: int, order: int, value_bytes: int):
    return _cached(_cache, tag + _on(device) + (key_type, order, value_bytes), {"max_keys": n},
                   lambda max_keys: cls(_cap(max_keys), order, key_type, _mode(value_bytes), value_bytes, device=device.index))


def _sorter(device: torch.device, n: int, key_type: int, order: int, value_bytes: int) -> OneSweep:
    """One cached handle per (device, stream, type, order, value width); re-created when the size outgrows it."""
    return _flat_sorter(OneSweep, (), device, n, key_type, order, value_bytes)


def _sorter16(device: torch.device, n: int, key_type: int, order: int, value_bytes: int) -> Sort16:
    """The same cache rule for 16-bit keys: one ``Sort16`` handle per (device, stream, type, order, value width)."""
    return _flat_sorter(Sort16, (16,), device, n, key_type, order, value_bytes)


def _row_sorter(device: torch.device, n: int, key_type: int, order: int, value_bytes: int) -> RowSort:
    """The same cache rule for the row-wise sort: one ``RowSort`` handle per (device, stream, type, order, value width)."""
    return _flat_sorter(RowSort, ("rows",), device, n, key_type, order, value_bytes)


def _row_sorter16(device: torch.device, n: int, key_type: int, order: int, value_bytes: int) -> RowSort16:
    """The same cache rule for the row-wise sort of 16-bit keys: one ``RowSort16`` handle per (device, stream, type, order, value width)."""
    return _flat_sorter(RowSort16, ("rows16",), device, n, key_type, order, value_bytes)


def _values_width(keys: torch.Tensor, values: torch.Tensor | None) -> int:
    if values is None:
        return 0
    if values.shape != keys.shape or not values.is_contiguous() or values.device != keys.device:
        raise ValueError("values must match keys in shape and device and be contiguous")
    if values.element_size() not in (4, 8):
        raise TypeError("values must be 4 or 8 bytes wide")
    return values.element_size()


def _sort16_(keys: torch.Tensor, values: torch.Tensor | None, descending: bool, unsigned: bool, positions: torch.Tensor | None = None) -> None:
    """``sort_`` / ``argsort`` on 2-byte keys: one ``gs_sort16_*`` call (``positions``: argsort's output, made by the kernels)."""
    kt = _key_type(keys, unsigned, _KEY16_TYPE)
    vb = 4 if positions is not None else _values_width(keys, values)
    n = keys.numel()
    if n == 0:
        return
    with torch.cuda.device(keys.device):
        s = _sorter16(keys.device, n, kt, _order(descending), vb)
        if positions is not None:
            s.argsort(keys, positions, n=n)
        else:
            s.sort(keys, values, n=n)


class RowKeyTypeError(TypeError, ValueError):
    """A 2-D tensor whose dtype the row-wise sort does not take.  A TypeError like every unsupported dtype; also a ValueError,
    which is what a 2-D tensor of 16-bit keys raised while ``sort_`` took 1-D tensors only."""


def _sort_rows_(keys: torch.Tensor, values: torch.Tensor | None, descending: bool, unsigned: bool) -> None:
    """``sort_`` on a 2-D tensor: every row sorted along the last dimension by one ``gs_sort_rows_*`` call."""
    if not keys.is_contiguous() or keys.device.type != "cuda":
        raise ValueError("keys must be a contiguous 2-D device tensor")
    if keys.dtype not in _KEY_TYPE:
        raise RowKeyTypeError(f"unsupported key dtype {keys.dtype} for a 2-D tensor: rows are sorted on 32-bit keys only (int32, uint32, float32); "
                              "sort_rows / argsort_rows take 16-bit keys")
    kt = _key_type(keys, unsigned, _KEY_TYPE)
    vb = _values_width(keys, values)
    if keys.numel() == 0:
        return
    with torch.cuda.device(keys.device):
        s = _row_sorter(keys.device, keys.numel(), kt, _order(descending), vb)
        s.sort(keys.view(torch.int32) if keys.dtype != torch.int32 else keys, values)


def _require_1d_keys(keys: torch.Tensor) -> None:
    if keys.dim() != 1 or not keys.is_contiguous() or keys.device.type != "cuda":
        raise ValueError("keys must be a contiguous 1-D device tensor")


def sort_(keys: torch.Tensor, values: torch.Tensor | None = None, descending: bool = False, unsigned: bool = False) -> None:
    """Sort ``keys`` (and carry ``values``) in place on the current stream.  ``unsigned=True`` treats int32 storage
    as uint32 keys (torch has little uint32 support), and int16 storage as uint16 keys.  16-bit keys (float16, bfloat16, int16, uint16)
    are sorted at their own width (``Sort16``).  A contiguous 2-D tensor of 32-bit keys is sorted along its last dimension, every row
    on its own (``RowSort``; ``values`` of the same shape move with their keys)."""
    if keys.dim() == 2:
        return _sort_rows_(keys, values, descending, unsigned)
    _require_1d_keys(keys)
    if keys.dtype in _KEY16_TYPE:
        return _sort16_(keys, values, descending, unsigned)
    if keys.dtype not in _KEY_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: 32-bit keys (int32, uint32, float32) and 16-bit keys "
                        "(float16, bfloat16, int16, uint16)")
    kt = _key_type(keys, unsigned, _KEY_TYPE)
    vb = _values_width(keys, values)
    n = keys.numel()
    if n <= 1:
        return
    with torch.cuda.device(keys.device):
        s = _sorter(keys.device, n, kt, _order(descending), vb)
        s.sort(keys.view(torch.int32) if keys.dtype != torch.int32 else keys, values, n=n)


def sort(keys: torch.Tensor, values: torch.Tensor | None = None, descending: bool = False, unsigned: bool = False):
    """Out-of-place: returns ``sorted_keys`` or ``(sorted_keys, sorted_values)``."""
    k = keys.clone()
    v = None if values is None else values.clone()
    sort_(k, v, descending, unsigned)
    return k if v is None else (k, v)


def argsort(keys: torch.Tensor, descending: bool = False, unsigned: bool = False) -> torch.Tensor:
    """Stable permutation that sorts ``keys`` (int32 indices; n < 2^30).  16-bit keys: the kernels make the positions themselves.
    2-D tensors of 32-bit keys: int32 positions within the row, ``[rows, row_len]``."""
    if keys.dim() == 2:
        rows, row_len = keys.shape
        idx = torch.arange(row_len, dtype=torch.int32, device=keys.device).repeat(rows, 1)
        _sort_rows_(keys.clone(), idx, descending, unsigned)
        return idx
    if keys.dtype in _KEY16_TYPE:
        _require_1d_keys(keys)
        idx = torch.empty(keys.numel(), dtype=torch.int32, device=keys.device)
        _sort16_(keys.clone(), None, descending, unsigned, positions=idx)
        return idx
    idx = torch.arange(keys.numel(), dtype=torch.int32, device=keys.device)
    k = keys.clone()
    sort_(k, idx, descending, unsigned)
    return idx


# ---- row-wise sort of 16- and 32-bit keys -----------------------------------------------------------------------------------
def _require_rows(keys: torch.Tensor) -> None:
    if keys.dim() != 2 or not keys.is_contiguous() or keys.device.type != "cuda":
        raise ValueError("keys must be a contiguous 2-D device tensor")
    if keys.dtype not in _KEY16_TYPE and keys.dtype not in _KEY_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: rows are sorted on 16-bit keys (float16, bfloat16, int16, uint16) and "
                        "32-bit keys (int32, uint32, float32)")


def sort_rows_(keys: torch.Tensor, values: torch.Tensor | None = None, descending: bool = False, unsigned: bool = False) -> None:
    """Sort every row of the contiguous 2-D device tensor ``keys`` along its last dimension (and carry ``values``, same shape, 4 or 8
    bytes wide) in place on the current stream.  16-bit keys (float16, bfloat16, int16, uint16) are sorted at their own width
    (``RowSort16``), 32-bit keys go to ``RowSort``.  ``unsigned=True`` treats int16 storage as uint16 keys and int32 storage as uint32."""
    _require_rows(keys)
    if keys.dtype in _KEY_TYPE:
        return _sort_rows_(keys, values, descending, unsigned)
    kt = _key_type(keys, unsigned, _KEY16_TYPE)
    vb = _values_width(keys, values)
    if keys.numel() == 0:
        return
    with torch.cuda.device(keys.device):
        _row_sorter16(keys.device, keys.numel(), kt, _order(descending), vb).sort(keys, values)


def sort_rows(keys: torch.Tensor, values: torch.Tensor | None = None, descending: bool = False, unsigned: bool = False):
    """Out-of-place ``sort_rows_``: returns ``sorted_keys`` or ``(sorted_keys, sorted_values)``; the inputs are not written."""
    k = keys.clone()
    v = None if values is None else values.clone()
    sort_rows_(k, v, descending, unsigned)
    return k if v is None else (k, v)


def argsort_rows(keys: torch.Tensor, descending: bool = False, unsigned: bool = False) -> torch.Tensor:
    """The stable permutation that sorts every row of ``keys``: int32 positions within the row, ``[rows, row_len]``.  For 16-bit keys the
    kernels make the positions themselves; 32-bit keys forward to ``argsort``.  ``keys`` is not written."""
    _require_rows(keys)
    if keys.dtype in _KEY_TYPE:
        return argsort(keys, descending, unsigned)
    idx = torch.empty(keys.shape, dtype=torch.int32, device=keys.device)
    if keys.numel() == 0:
        return idx
    kt = _key_type(keys, unsigned, _KEY16_TYPE)
    with torch.cuda.device(keys.device):
        _row_sorter16(keys.device, keys.numel(), kt, _order(descending), 4).argsort(keys.clone(), idx)
    return idx


# ---- segmented sort ---------------------------------------------------------------------------------------------------------
_seg_cache: dict = {}


def _seg_sorter(device: torch.device, n: int, num_segments: int, key_type: int, order: int, value_bytes: int,
                long_route: str = "host") -> SegmentedSort:
    """One cached handle per (device, stream, type, order, value width, long route); re-created when keys or segments outgrow it."""
    return _cached(_seg_cache, _on(device) + (key_type, order, value_bytes, long_route), {"max_keys": n, "max_segments": num_segments},
                   lambda max_keys, max_segments: SegmentedSort(_cap(max_keys), _cap(max_segments), order, key_type, _mode(value_bytes),
                                                                value_bytes, device=device.index, long_route=long_route))


def _seg_sorter16(device: torch.device, n: int, num_segments: int, key_type: int, order: int, value_bytes: int) -> SegmentedSort16:
    """The same cache rule for 16-bit keys: one ``SegmentedSort16`` handle per (device, stream, type, order, value width)."""
    return _cached(_seg_cache, (16,) + _on(device) + (key_type, order, value_bytes), {"max_keys": n, "max_segments": num_segments},
                   lambda max_keys, max_segments: SegmentedSort16(_cap(max_keys), _cap(max_segments), order, key_type, _mode(value_bytes),
                                                                  value_bytes, device=device.index))


def _require_offsets(keys: torch.Tensor, offsets: torch.Tensor) -> None:
    if offsets.dim() != 1 or offsets.numel() < 2 or offsets.dtype not in (torch.int32, torch.uint32) or offsets.device != keys.device \
            or not offsets.is_contiguous():
        raise ValueError("offsets must be a contiguous 1-D int32 tensor of num_segments + 1 on the keys' device")


def _segmented_sort16_(keys: torch.Tensor, offsets: torch.Tensor, values: torch.Tensor | None, descending: bool, unsigned: bool,
                       max_segment_len: int, positions: torch.Tensor | None = None) -> None:
    """``segmented_sort_`` / ``segmented_argsort`` on 2-byte keys: one ``gs_segsort16_*`` call (``positions``: the argsort's output, made
    by the kernels inside the segments)."""
    _require_offsets(keys, offsets)
    kt = _key_type(keys, unsigned, _KEY16_TYPE)
    vb = 4 if positions is not None else _values_width(keys, values)
    n = keys.numel()
    if n == 0:
        return
    with torch.cuda.device(keys.device):
        s = _seg_sorter16(keys.device, n, offsets.numel() - 1, kt, _order(descending), vb)
        if positions is not None:
            s.argsort(keys, offsets, positions, n=n, max_segment_len=max_segment_len)
        else:
            s.sort(keys, offsets, values, n=n, max_segment_len=max_segment_len)


def segmented_sort_(keys: torch.Tensor, offsets: torch.Tensor, values: torch.Tensor | None = None, descending: bool = False,
                    unsigned: bool = False, max_segment_len: int = 0, long_route: str = "host") -> None:
    """Sort every segment ``keys[offsets[s]:offsets[s + 1]]`` (and carry ``values``) in place on the current stream.  ``offsets``:
    int32 tensor of ``num_segments + 1`` on the device (CSR).  ``max_segment_len``: upper bound on the segment length if the caller
    knows one (a bound that fits the LDS classes keeps the call free of host waits); 0 = unknown.  ``long_route``: how 32-bit
    segments longer than LDS holds are sorted: ``"host"`` (the default) waits on the host once for their list and sorts them one by
    one, ``"device"`` sorts all of them at once in four passes and never waits on the host, with the same result.  16-bit keys
    (float16, bfloat16, int16, uint16; ``unsigned=True`` on int16 storage selects uint16 keys) are sorted at their own width
    (``SegmentedSort16``); that call never waits on the host anyway and ignores ``long_route``."""
    if long_route not in ("host", "device"):
        raise ValueError('long_route must be "host" or "device"')
    _require_1d_keys(keys)
    if keys.dtype in _KEY16_TYPE:
        return _segmented_sort16_(keys, offsets, values, descending, unsigned, max_segment_len)
    if keys.dtype not in _KEY_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: 32-bit keys (int32, uint32, float32) and 16-bit keys "
                        "(float16, bfloat16, int16, uint16)")
    _require_offsets(keys, offsets)
    kt = _key_type(keys, unsigned, _KEY_TYPE)
    vb = _values_width(keys, values)
    n = keys.numel()
    if n == 0:
        return
    with torch.cuda.device(keys.device):
        s = _seg_sorter(keys.device, n, offsets.numel() - 1, kt, _order(descending), vb, long_route)
        s.sort(keys.view(torch.int32) if keys.dtype != torch.int32 else keys, offsets, values, n=n, max_segment_len=max_segment_len)


def segmented_sort(keys: torch.Tensor, offsets: torch.Tensor, values: torch.Tensor | None = None, descending: bool = False,
                   unsigned: bool = False, max_segment_len: int = 0, long_route: str = "host"):
    """Out-of-place: returns ``sorted_keys`` or ``(sorted_keys, sorted_values)``."""
    k = keys.clone()
    v = None if values is None else values.clone()
    segmented_sort_(k, offsets, v, descending, unsigned, max_segment_len, long_route)
    return k if v is None else (k, v)


def segmented_argsort(keys: torch.Tensor, offsets: torch.Tensor, descending: bool = False, unsigned: bool = False,
                      max_segment_len: int = 0, long_route: str = "host") -> torch.Tensor:
    """Stable permutation of the WHOLE array that sorts every segment: position within the segment's slice plus its start (int32;
    identity outside the segments).  16-bit keys: the kernels make the indices inside the segments themselves.  ``long_route``: as
    ``segmented_sort_``."""
    idx = torch.arange(keys.numel(), dtype=torch.int32, device=keys.device)
    k = keys.clone()
    if keys.dtype in _KEY16_TYPE:
        _require_1d_keys(keys)
        _segmented_sort16_(k, offsets, None, descending, unsigned, max_segment_len, positions=idx)
        return idx
    segmented_sort_(k, offsets, idx, descending, unsigned, max_segment_len, long_route)
    return idx


# ---- top-k selection --------------------------------------------------------------------------------------------------------
_topk_cache: dict = {}


def _topk_of(cls, tag: tuple, device: torch.device, n: int, k: int, key_type: int, order: int, value_bytes: int):
    # (max_k is capped by the capacity: k <= n)
    return _cached(_topk_cache, tag + _on(device) + (key_type, order, value_bytes), {"max_keys": n, "max_k": k},
                   lambda max_keys, max_k: cls(_cap(max_keys), min(_cap(max_k), _cap(max_keys)), order, key_type, _mode(value_bytes),
                                               value_bytes, device=device.index))


def _topk_handle(device: torch.device, n: int, k: int, key_type: int, order: int, value_bytes: int) -> TopK:
    """One cached handle per (device, stream, type, order, value width); re-created when n or k outgrow it."""
    return _topk_of(TopK, (), device, n, k, key_type, order, value_bytes)


def _topk16_handle(device: torch.device, n: int, k: int, key_type: int, order: int, value_bytes: int) -> TopK16:
    """The cache rule of ``_topk_handle`` for the 1-D selection on 16-bit keys."""
    return _topk_of(TopK16, (16,), device, n, k, key_type, order, value_bytes)


def _topk_1d(keys: torch.Tensor, k: int, largest: bool, values: torch.Tensor | None, kt: int, handle_for):
    """``topk`` / ``topk16`` on a 1-D tensor behind their checks of the keys: ``kt`` is the key type of ``keys.dtype``."""
    n, k = keys.numel(), int(k)
    if not 1 <= k <= n:
        raise ValueError("1 <= k <= n")
    vb = _values_width(keys, values) or 4
    out_k = torch.empty(k, dtype=keys.dtype, device=keys.device)
    out_v = torch.empty(k, dtype=torch.int32 if values is None else values.dtype, device=keys.device)
    with torch.cuda.device(keys.device):
        s = handle_for(keys.device, n, k, kt, _order(largest), vb)
        s.select(keys, k, out_k, values, out_v, n=n)
    return out_k, out_v


def topk(keys: torch.Tensor, k: int, largest: bool = True, values: torch.Tensor | None = None, unsigned: bool = False):
    """The ``k`` largest (``largest=True``, as ``torch.topk``) or smallest elements of a 1-D tensor in sorted order, without sorting
    the rest: returns ``(keys_k, indices_k)`` (int32 input positions) or, with ``values``, ``(keys_k, values_k)``.  A 2-D tensor whose
    last dimension is contiguous (``stride(1) == 1``, any ``stride(0) >= row_len``, so ``x[:, :row_len]`` works) is selected row by row
    in one call, as ``torch.topk(x, k, dim=-1)``: ``[rows, k]`` keys and int32 positions within the row, or values.
    2-D tensors may also hold 16-bit keys (float16, bfloat16, int16, uint16; ``unsigned=True`` on int16 storage selects uint16 keys): the
    kernels read them at their own width.  There, a row longer than LDS holds takes ``k <= rows_max_k`` (``ValueError`` otherwise), and a
    1-D tensor is a ``TypeError``: pass ``x[None, :]``.  The result is the head of this library's sort: floats by the order-preserving bit flip (-0 < +0, NaNs by bit pattern — NOT ``torch.topk``'s "NaN is
    largest"), ties by position (smallest: lowest positions first; largest: highest positions first).  The inputs are not written."""
    if keys.dim() == 2:
        return _topk_rows(keys, int(k), largest, values, unsigned)
    _require_1d_keys(keys)
    if keys.dtype in _KEY16_TYPE:
        raise TypeError(f"a 1-D {keys.dtype} tensor is not taken: 16-bit keys are selected row-wise, pass the 2-D form x[None, :] "
                        "(or call topk16, the 1-D selection on 16-bit keys)")
    if keys.dtype not in _KEY_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: 32-bit keys only (int32, uint32, float32)")
    return _topk_1d(keys, k, largest, values, _key_type(keys, unsigned, _KEY_TYPE), _topk_handle)


def _topk_rows(keys: torch.Tensor, k: int, largest: bool, values: torch.Tensor | None, unsigned: bool):
    """``topk`` on a 2-D tensor: one ``gs_topk_select_rows_*`` call; the handle is sized by the extent ``(rows - 1) * stride + row_len``."""
    rows, row_len = keys.shape
    if keys.device.type != "cuda" or rows == 0 or row_len == 0 or keys.stride(1) != 1 or (rows > 1 and keys.stride(0) < row_len):
        raise ValueError("keys must be a non-empty 2-D device tensor with a contiguous last dimension and a row stride >= its row length")
    key16 = keys.dtype in _KEY16_TYPE
    if not key16 and keys.dtype not in _KEY_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: 32-bit keys (int32, uint32, float32) and, row-wise, 16-bit keys "
                        "(float16, bfloat16, int16, uint16)")
    if not 1 <= k <= row_len:
        raise ValueError("1 <= k <= row length")
    if keys.data_ptr() % 16:
        raise ValueError("the first row must start on a 16-byte boundary")
    stride = keys.stride(0) if rows > 1 else row_len
    kt = _key_type(keys, unsigned, _KEY16_TYPE if key16 else _KEY_TYPE)
    vb = 4
    if values is not None:
        # (the row stride of a single row is never used)
        same_rows = values.stride(1) == 1 and (rows == 1 or values.stride(0) == keys.stride(0))
        if values.shape != keys.shape or not same_rows or values.device != keys.device or values.data_ptr() % 16:
            raise ValueError("values must match keys in shape, strides and device and start on a 16-byte boundary")
        vb = values.element_size()
        if vb not in (4, 8):
            raise TypeError("values must be 4 or 8 bytes wide")
    if key16:
        # GS_ERR_SIZE of gs_topk_select_rows_* for 2-byte keys, stated here: they have no row-by-row route
        lds_rows, max_k = _lib.load().gs_segsort_max_lds_segment(MODE_PAIRS, vb), rows_max_k(MODE_PAIRS, vb)
        if row_len > lds_rows and k > max_k:
            raise ValueError(f"16-bit keys: a row longer than {lds_rows} elements (with {vb}-byte values) takes k <= {max_k}, "
                             f"got row length {row_len} and k = {k}")
    out_k = torch.empty((rows, k), dtype=keys.dtype, device=keys.device)
    out_v = torch.empty((rows, k), dtype=torch.int32 if values is None else values.dtype, device=keys.device)
    with torch.cuda.device(keys.device):
        s = _topk_handle(keys.device, (rows - 1) * stride + row_len, k, kt, _order(largest), vb)
        s.select_rows(keys, rows, row_len, stride, k, out_k, values, out_v)
    return out_k, out_v


def topk16(keys: torch.Tensor, k: int, largest: bool = True, values: torch.Tensor | None = None, unsigned: bool = False):
    """``topk`` for a 1-D contiguous tensor of 16-bit keys (float16, bfloat16, int16, uint16; ``unsigned=True`` on int16 storage selects
    uint16 keys), read at their own width by ``gs_topk16_*``: returns ``(keys_k, indices_k)`` (int32 input positions) or, with
    ``values``, ``(keys_k, values_k)``; every ``1 <= k <= n``.  The result is the head of this library's 16-bit sort: floats by the
    order-preserving bit flip (-0 < +0, NaNs by bit pattern), ties by position (smallest: lowest positions first; largest: highest
    positions first).  A 2-D tensor is forwarded to ``topk``'s row-wise call; other dtypes are a ``TypeError``: see ``topk``."""
    if keys.dim() == 2:
        return _topk_rows(keys, int(k), largest, values, unsigned)
    if keys.dtype not in _KEY16_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: topk16 takes 16-bit keys (float16, bfloat16, int16, uint16); 32-bit keys go to topk")
    _require_1d_keys(keys)
    return _topk_1d(keys, k, largest, values, _key_type(keys, unsigned, _KEY16_TYPE), _topk16_handle)


# ---- segmented top-k ----------------------------------------------------------------------------------------------------------
_segtopk_cache: dict = {}


def _segtopk_handle(device: torch.device, n: int, num_segments: int, k: int, key_type: int, order: int, value_bytes: int) -> SegmentedTopK:
    """One cached handle per (device, stream, type, order, value width); re-created when n, the segments or k outgrow it.  A 16-bit
    key type gets a ``SegmentedTopK16``."""
    cls = SegmentedTopK16 if key_type in _KEY16_TYPE.values() else SegmentedTopK
    return _cached(_segtopk_cache, _on(device) + (key_type, order, value_bytes), {"max_keys": n, "max_segments": num_segments, "max_k": k},
                   lambda max_keys, max_segments, max_k: cls(_cap(max_keys), _cap(max_segments), _cap(max_k, 6), order, key_type, MODE_PAIRS,
                                                             value_bytes, device=device.index))


def segmented_topk(keys: torch.Tensor, offsets: torch.Tensor, k: int, largest: bool = True, values: torch.Tensor | None = None,
                   unsigned: bool = False, max_segment_len: int = 0):
    """The ``k`` largest (``largest=True``) or smallest elements of every segment ``keys[offsets[s]:offsets[s + 1]]`` in sorted order,
    in one call that never waits on the host: returns ``(keys_k [S, k], indices_k [S, k], counts [S])`` (int32 positions in the whole
    array, as ``segmented_argsort``) or, with ``values``, ``(keys_k, values_k, counts)``.  ``counts[s] = min(k, length of segment s)``
    (int32): row ``s`` holds that many results; the slots behind them hold zero keys, ``-1`` positions and zero values.  ``offsets``:
    int32 tensor of ``num_segments + 1`` on the device (CSR).  ``max_segment_len``: an upper bound on the segment length if the caller
    knows one, 0 = unknown; a segment longer than LDS holds takes ``k <= rows_max_k`` (4096), so a larger ``k`` needs a bound that
    fits LDS (``ValueError`` otherwise).  The result is the head of ``segmented_sort``: floats by the order-preserving bit flip, ties
    by position (smallest: lowest positions first; largest: highest positions first).  The inputs are not written."""
    _require_1d_keys(keys)
    if keys.dtype not in _KEY_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: 32-bit keys only (int32, uint32, float32); "
                        "float16, bfloat16, int16 and uint16 keys: segmented_topk16")
    return _segmented_topk(keys, offsets, k, largest, values, _key_type(keys, unsigned, _KEY_TYPE), max_segment_len)


def segmented_topk16(keys: torch.Tensor, offsets: torch.Tensor, k: int, largest: bool = True, values: torch.Tensor | None = None,
                     unsigned: bool = False, max_segment_len: int = 0):
    """``segmented_topk`` on 2-byte keys (float16, bfloat16, int16, and uint16 where torch has it; ``unsigned=True`` treats int16
    storage as uint16), read at their own width by ``gs_segtopk16_*``: the same arguments, the same result ``(keys_k, indices_k |
    values_k, counts)``, the same filling (zero keys, ``-1`` positions, zero values) and the same rule for ``k`` above 4096.  The result
    is the head of ``segmented_sort`` on the same tensor."""
    if keys.dtype not in _KEY16_TYPE:
        raise TypeError(f"unsupported key dtype {keys.dtype}: 16-bit keys only (float16, bfloat16, int16, uint16); "
                        "int32, uint32 and float32 keys: segmented_topk")
    _require_1d_keys(keys)
    return _segmented_topk(keys, offsets, k, largest, values, _key_type(keys, unsigned, _KEY16_TYPE), max_segment_len)


def _segmented_topk(keys: torch.Tensor, offsets: torch.Tensor, k: int, largest: bool, values: torch.Tensor | None, kt: int, max_segment_len: int):
    """``segmented_topk`` / ``segmented_topk16`` behind their checks of the keys: ``kt`` is the key type of ``keys.dtype``."""
    _require_offsets(keys, offsets)
    n, k, segs = keys.numel(), int(k), offsets.numel() - 1
    if k < 1:
        raise ValueError("k >= 1")
    vb = _values_width(keys, values) or 4
    max_segment_len = int(max_segment_len)
    lds_len, max_k = _lib.load().gs_segsort_max_lds_segment(MODE_PAIRS, vb), rows_max_k(MODE_PAIRS, vb)
    if k > max_k and not 0 < max_segment_len <= lds_len:
        # GS_ERR_SIZE of gs_segtopk_select_*, stated here: lengths are known on the device only
        raise ValueError(f"k = {k} is above {max_k}: it needs max_segment_len <= {lds_len} (with {vb}-byte values), got {max_segment_len}")
    out_k = torch.zeros((segs, k), dtype=keys.dtype, device=keys.device)
    if values is None:
        out_v = torch.full((segs, k), -1, dtype=torch.int32, device=keys.device)
    else:
        out_v = torch.zeros((segs, k), dtype=values.dtype, device=keys.device)
    counts = torch.diff(offsets.view(torch.int32)).clamp(max=k)
    if n == 0:
        return out_k, out_v, counts
    with torch.cuda.device(keys.device):
        s = _segtopk_handle(keys.device, n, segs, k, kt, _order(largest), vb)
        s.select(keys, offsets, k, out_k, values, out_v, n=n, max_segment_len=max_segment_len)
    return out_k, out_v, counts


# ---- unique / run-length encode and reduce by key: 32-, 16- and 64-bit keys -------------------------------------------------------
_unique_cache: dict = {}
_unique16_cache: dict = {}
_unique64_cache: dict = {}
_reduce_cache: dict = {}
_reduce64_cache: dict = {}
_WIDE_KEYS = {"16": "16-bit keys (float16, bfloat16, int16, uint16)", "64": "64-bit keys (int64, uint64, float64)"}


def _sized_by_keys(cache: dict, cls, device: torch.device, n: int, key_type: int, order: int, *rest, **named):
    """The cache rule of ``_sorter`` for a family sized by ``max_keys`` alone: one handle per (device, stream, type, order, ``rest``
    or ``named``: the family's own argument), built as ``cls(max_keys, order, key_type, *rest, **named, device=...)``."""
    return _cached(cache, _on(device) + (key_type, order) + rest + tuple(named.values()), {"max_keys": n},
                   lambda max_keys: cls(_cap(max_keys), order, key_type, *rest, **named, device=device.index))


def _unique_handle(device: torch.device, n: int, key_type: int, order: int, positions: bool) -> Unique:
    """One ``Unique`` handle per (device, stream, type, order, with positions); re-created when the size outgrows it."""
    return _sized_by_keys(_unique_cache, Unique, device, n, key_type, order, positions=positions)


def _unique64_handle(device: torch.device, n: int, key_type: int, order: int, positions: bool) -> Unique64:
    """The cache rule of ``_unique_handle`` for the 64-bit keys."""
    return _sized_by_keys(_unique64_cache, Unique64, device, n, key_type, order, positions=positions)


def _unique16_handle(device: torch.device, n: int, key_type: int, order: int) -> Unique16:
    """The cache rule of ``_unique_handle`` for the 16-bit keys: one ``Unique16`` handle per (device, stream, type, order); re-created
    when the size outgrows it (its scratch does not grow with the size)."""
    return _sized_by_keys(_unique16_cache, Unique16, device, n, key_type, order)


def _reduce_handle(device: torch.device, n: int, key_type: int, order: int, value_bytes: int) -> ReduceByKey:
    """One ``ReduceByKey`` handle per (device, stream, type, order, value width); re-created when the size outgrows it."""
    return _sized_by_keys(_reduce_cache, ReduceByKey, device, n, key_type, order, value_bytes)


def _reduce64_handle(device: torch.device, n: int, key_type: int, order: int, value_bytes: int) -> ReduceByKey64:
    """The cache rule of ``_reduce_handle`` for the 64-bit keys."""
    return _sized_by_keys(_reduce64_cache, ReduceByKey64, device, n, key_type, order, value_bytes)


def _takes(name: str) -> str:
    """What a frontend of the 16- or 64-bit keys says it takes: ``name`` ends in the width, and without it names the 32-bit one."""
    return f"{name} takes {_WIDE_KEYS[name[-2:]]}; 32-bit keys go to {name[:-2]}"


def _require_unique_keys(keys: torch.Tensor, table: dict = _KEY_TYPE, takes: str = "unique takes 32-bit keys (int32, uint32, float32)") -> None:
    if keys.dim() != 1:
        raise ValueError("keys must be a contiguous 1-D device tensor")
    if keys.dtype not in table:
        raise TypeError(f"unsupported key dtype {keys.dtype}: {takes}")
    if not keys.is_contiguous() or keys.device.type != "cuda":
        raise ValueError("keys must be a contiguous 1-D device tensor")


def _unique_outputs(keys: torch.Tensor, run, return_inverse: bool, return_counts: bool, return_index: bool = False):
    """What every ``unique*`` frontend returns: ``run(n)`` makes ``(out_keys, out_counts, out_first, out_inverse, num)`` (None where
    not asked for) on the keys' device; the outputs are sliced to their length (the one wait on the host) and put in torch's order."""
    n = keys.numel()
    if n == 0:
        empty = lambda: torch.empty(0, dtype=torch.int32, device=keys.device)  # noqa: E731
        out = (keys.clone(),) + ((empty(),) if return_inverse else ()) + ((empty(),) if return_counts else ()) + ((empty(),) if return_index else ())
        return out[0] if len(out) == 1 else out
    with torch.cuda.device(keys.device):
        out_k, out_c, out_f, out_i, num = run(n)
    u = int(num.item())
    out = (out_k[:u],) + ((out_i,) if return_inverse else ()) + ((out_c[:u],) if return_counts else ()) + ((out_f[:u],) if return_index else ())
    return out[0] if len(out) == 1 else out


def _unique_sorted(keys: torch.Tensor, handle_for, kt: int, descending: bool, return_inverse: bool, return_counts: bool, return_index: bool):
    """``unique`` / ``unique64`` behind their checks of the keys: a handle with positions only where the inverse or the index is asked for."""
    positions = return_inverse or return_index

    def run(n):
        s = handle_for(keys.device, n, kt, _order(descending), positions)
        if positions:
            return s.unique_positions(keys, n, counts=return_counts, first=return_index, inverse=return_inverse)
        out_k, out_c, num = s.unique(keys, n, counts=return_counts)
        return out_k, out_c, None, None, num
    return _unique_outputs(keys, run, return_inverse, return_counts, return_index)


def _unique_runs(keys: torch.Tensor, handle, return_inverse: bool, return_counts: bool):
    """``unique_consecutive*`` behind their checks of the keys: ``handle(n)`` is the family's handle (key type and order play no part)."""
    def run(n):
        out_k, out_c, out_i, num = handle(n).unique_consecutive(keys, n, counts=return_counts, inverse=return_inverse)
        return out_k, out_c, None, out_i, num
    return _unique_outputs(keys, run, return_inverse, return_counts)


def unique(keys: torch.Tensor, return_inverse: bool = False, return_counts: bool = False, return_index: bool = False, descending: bool = False,
           unsigned: bool = False):
    """The distinct elements of a 1-D contiguous int32 / uint32 / float32 tensor in sorted order, as ``torch.unique(keys, sorted=True)``:
    returns ``output`` or the tuple ``(output[, inverse][, counts][, index])``.  ``inverse`` (int32) maps every input to its place in
    ``output``, ``counts`` (int32) is each element's multiplicity, ``index`` (int32) the lowest input position that holds it (numpy's
    ``return_index``).  ``descending=True`` returns the distinct elements in falling order; ``unsigned=True`` treats int32 storage as
    uint32 keys.  Equality is BITWISE and the order is this library's sort: on floats ``-0.0`` and ``+0.0`` are two elements
    (``-0.0`` first) and every NaN bit pattern is an element of its own, placed by its bits — unlike ``torch.unique``, which compares
    values.  On integers the result equals ``torch.unique``'s.  Slicing the outputs to their length is the one wait on the host, as in
    ``torch.unique``.  ``keys`` is not written."""
    _require_unique_keys(keys)
    return _unique_sorted(keys, _unique_handle, _key_type(keys, unsigned, _KEY_TYPE), descending, return_inverse, return_counts, return_index)


def unique_consecutive(keys: torch.Tensor, return_inverse: bool = False, return_counts: bool = False):
    """``torch.unique_consecutive`` on a 1-D contiguous int32 / uint32 / float32 tensor: one element per run of BITWISE-equal neighbours of
    the input as it lies (no sort): returns ``output`` or ``(output[, inverse][, counts])`` with int32 ``inverse`` (the run of every
    input) and ``counts`` (the runs' lengths).  One wait on the host, for the length.  ``keys`` is not written."""
    _require_unique_keys(keys)
    return _unique_runs(keys, lambda n: _unique_handle(keys.device, n, KEY_UINT32, ORDER_ASCENDING, False), return_inverse, return_counts)


def _require_reduce_args(keys: torch.Tensor, values: torch.Tensor, op: str, table: dict = _KEY_TYPE, name: str = "reduce_by_key",
                         takes: str = "reduce_by_key takes 32-bit keys (int32, uint32, float32)"):
    if keys.dim() != 1 or values.dim() != 1 or keys.numel() != values.numel():
        raise ValueError("keys and values must be contiguous 1-D device tensors of one length")
    if keys.dtype not in table:
        raise TypeError(f"unsupported key dtype {keys.dtype}: {takes}")
    vt = _torch_value_types().get(values.dtype)
    if vt is None:
        raise TypeError(f"unsupported value dtype {values.dtype}: {name} takes int32, uint32, float32, int64, uint64 or float64 values")
    if op not in _REDUCE_OPS:
        raise ValueError('op is "sum", "min" or "max"')
    if not keys.is_contiguous() or not values.is_contiguous() or keys.device.type != "cuda" or values.device != keys.device:
        raise ValueError("keys and values must be contiguous 1-D device tensors of one length")
    return vt, _REDUCE_OPS[op]


def _reduce_outputs(keys: torch.Tensor, values: torch.Tensor, run, return_counts: bool):
    """What every ``reduce_by_key*`` frontend returns: ``run(n)`` makes ``(out_keys, out_values, out_counts | None, num)`` on the keys'
    device; the outputs are sliced to their length (the one wait on the host)."""
    n = keys.numel()
    if n == 0:
        return (keys.clone(), values.clone()) + ((torch.empty(0, dtype=torch.int32, device=keys.device),) if return_counts else ())
    with torch.cuda.device(keys.device):
        out_k, out_v, out_c, num = run(n)
    u = int(num.item())
    return (out_k[:u], out_v[:u]) + ((out_c[:u],) if return_counts else ())


def reduce_by_key(keys: torch.Tensor, values: torch.Tensor, op: str = "sum", descending: bool = False, return_counts: bool = False,
                  unsigned: bool = False):
    """One ``op`` ("sum", "min", "max") of ``values`` per distinct element of ``keys``: returns ``(distinct, reduced[, counts])`` with
    ``distinct`` as ``unique(keys, descending=descending, unsigned=unsigned)`` delivers it, ``reduced[j]`` the reduction of all values
    whose key is ``distinct[j]`` (the values' dtype) and ``counts`` (int32) the multiplicities — ``unique(return_inverse=True)`` followed
    by ``index_add_`` / ``scatter_reduce`` in one call, with no inverse, no gather and no atomics.  1-D contiguous tensors: keys int32 /
    uint32 / float32, values int32 / float32 / int64 / float64 (uint32, uint64 where torch has them).  Key equality is BITWISE.  Integer
    sums wrap.  "min" / "max" on floats use this library's total order (``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN``) and
    return one of the inputs bit for bit — UNLIKE ``torch.amin`` / ``amax``, which propagate NaNs, and ``fmin`` / ``fmax``, which drop
    them.  A float "sum" is combined in an order fixed by the data: two calls give bitwise identical results (``index_add_`` does not),
    but not the left-to-right sum.  One wait on the host, for the length.  Neither input is written."""
    vt, opc = _require_reduce_args(keys, values, op)
    kt = _key_type(keys, unsigned, _KEY_TYPE)
    return _reduce_outputs(keys, values, lambda n: _reduce_handle(keys.device, n, kt, _order(descending), values.element_size())
                           .reduce_by_key(keys, values, opc, vt, n, counts=return_counts), return_counts)


def reduce_by_key_consecutive(keys: torch.Tensor, values: torch.Tensor, op: str = "sum", return_counts: bool = False):
    """``reduce_by_key`` on the input as it lies (no sort): one ``op`` of ``values`` per run of BITWISE-equal neighbouring keys, as thrust's
    ``reduce_by_key``: ``(runs, reduced[, counts])``.  One wait on the host, for the length.  Neither input is written."""
    vt, opc = _require_reduce_args(keys, values, op)
    return _reduce_outputs(keys, values, lambda n: _reduce_handle(keys.device, n, KEY_UINT32, ORDER_ASCENDING, values.element_size())
                           .reduce_by_key_consecutive(keys, values, opc, vt, n, counts=return_counts), return_counts)


def unique16(keys: torch.Tensor, return_inverse: bool = False, return_counts: bool = False, return_index: bool = False, descending: bool = False,
             unsigned: bool = False):
    """``unique`` for a 1-D contiguous tensor of 16-bit keys (float16, bfloat16, int16, uint16; ``unsigned=True`` on int16 storage treats
    it as uint16 keys), read at their own width by ``gs_unique16_*``: one 65 536-bin histogram, no sort.  Returns ``output`` or the tuple
    ``(output[, inverse][, counts][, index])`` with int32 ``inverse``, ``counts`` and ``index`` (the lowest input position of each
    element), as ``unique`` does.  Equality is BITWISE and the order is this library's 16-bit sort: ``-0.0`` and ``+0.0`` are two
    elements (``-0.0`` first) and every NaN bit pattern is an element of its own.  Slicing the outputs to their length is the one wait
    on the host.  ``keys`` is not written.  Other dtypes are a ``TypeError``: see ``unique``."""
    _require_unique_keys(keys, _KEY16_TYPE, _takes("unique16"))
    kt = _key_type(keys, unsigned, _KEY16_TYPE)
    return _unique_outputs(keys, lambda n: _unique16_handle(keys.device, n, kt, _order(descending))
                           .unique(keys, n, counts=return_counts, first=return_index, inverse=return_inverse),
                           return_inverse, return_counts, return_index)


def unique_consecutive16(keys: torch.Tensor, return_inverse: bool = False, return_counts: bool = False):
    """``unique_consecutive`` for a 1-D contiguous tensor of 16-bit keys: one element per run of BITWISE-equal neighbours of the input as
    it lies (no sort): returns ``output`` or ``(output[, inverse][, counts])`` with int32 ``inverse`` and ``counts``.  One wait on the
    host, for the length.  ``keys`` is not written.  Other dtypes are a ``TypeError``: see ``unique_consecutive``."""
    _require_unique_keys(keys, _KEY16_TYPE, _takes("unique_consecutive16"))
    return _unique_runs(keys, lambda n: _unique16_handle(keys.device, n, KEY_UINT16, ORDER_ASCENDING), return_inverse, return_counts)


def unique64(keys: torch.Tensor, return_inverse: bool = False, return_counts: bool = False, return_index: bool = False, descending: bool = False,
             unsigned: bool = False):
    """``unique`` for a 1-D contiguous tensor of 64-bit keys (int64, float64, uint64 where torch has it; ``unsigned=True`` reads int64
    storage as uint64 keys), as ``torch.unique(keys, sorted=True)``: returns ``output`` or the tuple
    ``(output[, inverse][, counts][, index])`` with int32 ``inverse``, ``counts`` and ``index`` (the lowest input position of each
    element), as ``unique`` does.  Equality is BITWISE on all 64 bits and the order is this library's sort: on floats ``-0.0`` and
    ``+0.0`` are two elements (``-0.0`` first) and every NaN bit pattern is an element of its own; on integers the result equals
    ``torch.unique``'s.  Keys below 2^32 (ids) cost the sort four passes, not eight.  Slicing the outputs to their length is the one wait
    on the host.  ``keys`` is not written.  Other dtypes are a ``TypeError``: see ``unique``."""
    _require_unique_keys(keys, _KEY64_TYPE, _takes("unique64"))
    return _unique_sorted(keys, _unique64_handle, _key_type(keys, unsigned, _KEY64_TYPE), descending, return_inverse, return_counts, return_index)


def unique_consecutive64(keys: torch.Tensor, return_inverse: bool = False, return_counts: bool = False):
    """``unique_consecutive`` for a 1-D contiguous tensor of 64-bit keys: one element per run of BITWISE-equal neighbours of the input as
    it lies (no sort): returns ``output`` or ``(output[, inverse][, counts])`` with int32 ``inverse`` and ``counts``.  One wait on the
    host, for the length.  ``keys`` is not written.  Other dtypes are a ``TypeError``: see ``unique_consecutive``."""
    _require_unique_keys(keys, _KEY64_TYPE, _takes("unique_consecutive64"))
    return _unique_runs(keys, lambda n: _unique64_handle(keys.device, n, KEY_UINT64, ORDER_ASCENDING, False), return_inverse, return_counts)


def reduce_by_key64(keys: torch.Tensor, values: torch.Tensor, op: str = "sum", descending: bool = False, return_counts: bool = False,
                    unsigned: bool = False):
    """``reduce_by_key`` for 64-bit keys (int64, float64, uint64 where torch has it; ``unsigned=True`` reads int64 storage as uint64
    keys): one ``op`` ("sum", "min", "max") of ``values`` per distinct element of ``keys``: ``(distinct, reduced[, counts])`` with
    ``distinct`` as ``unique64(keys, descending=descending, unsigned=unsigned)`` delivers it, ``reduced`` in the values' dtype and
    int32 ``counts``: ``unique(return_inverse=True)`` followed by ``index_add_`` / ``scatter_reduce`` in one call, with no inverse, no
    gather and no atomics.  The operations are ``reduce_by_key``'s: integer sums wrap, "min" / "max" on floats use this library's total
    order (UNLIKE ``torch.amin`` / ``amax`` and ``fmin`` / ``fmax``), a float "sum" is reproducible bit for bit but not the
    left-to-right sum.  One wait on the host, for the length.  Neither input is written."""
    vt, opc = _require_reduce_args(keys, values, op, _KEY64_TYPE, "reduce_by_key64", _takes("reduce_by_key64"))
    kt = _key_type(keys, unsigned, _KEY64_TYPE)
    return _reduce_outputs(keys, values, lambda n: _reduce64_handle(keys.device, n, kt, _order(descending), values.element_size())
                           .reduce_by_key(keys, values, opc, vt, n, counts=return_counts), return_counts)


def reduce_by_key_consecutive64(keys: torch.Tensor, values: torch.Tensor, op: str = "sum", return_counts: bool = False):
    """``reduce_by_key_consecutive`` for 64-bit keys: one ``op`` of ``values`` per run of BITWISE-equal neighbouring keys of the input as
    it lies (no sort): ``(runs, reduced[, counts])``.  One wait on the host, for the length.  Neither input is written."""
    vt, opc = _require_reduce_args(keys, values, op, _KEY64_TYPE, "reduce_by_key_consecutive64", _takes("reduce_by_key_consecutive64"))
    return _reduce_outputs(keys, values, lambda n: _reduce64_handle(keys.device, n, KEY_UINT64, ORDER_ASCENDING, values.element_size())
                           .reduce_by_key_consecutive(keys, values, opc, vt, n, counts=return_counts), return_counts)


# ---- sorted search: the lower / upper bound of many queries ------------------------------------------------------------------------
_search_cache: dict = {}


def _search_handle(device: torch.device, n: int, m: int, key_type: int, order: int, sort_queries: bool) -> SortedSearch:
    """One ``SortedSearch`` handle per (device, stream, type, order, with the query sorter); re-created when a size outgrows it, and
    then at no less than it had: a call with many keys and few queries and one the other way round share a handle."""
    key = _on(device) + (key_type, order, sort_queries)
    old = _search_cache.get(key)
    if old is not None:
        n, m = max(n, old.max_keys), max(m, old.max_queries)
    return _cached(_search_cache, key, {"max_keys": n, "max_queries": m},
                   lambda max_keys, max_queries: SortedSearch(_cap(max_keys), _cap(max_queries), key_type, order, sort_queries=sort_queries,
                                                              device=device.index))


def searchsorted(sorted_keys: torch.Tensor, queries: torch.Tensor, right: bool = False, descending: bool = False, queries_sorted: bool = False,
                 unsigned: bool = False) -> torch.Tensor:
    """``torch.searchsorted`` in THIS library's order: for every element of ``queries`` (any shape; contiguous) its insertion position in
    the 1-D contiguous ``sorted_keys``, as int32 in the shape of ``queries``: the number of keys strictly in front of the query
    (``right=False``) or in front of or equal to it (``right=True``).  ``sorted_keys`` is what this library's sort delivers, ascending
    or ``descending``: int32, float32, int64, float64 (uint32 / uint64 where torch has them; ``unsigned=True`` reads signed storage as
    unsigned keys); floats are ordered ``-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN`` and compared BITWISE (``-0.0`` and ``+0.0``
    are two keys, every NaN pattern is its own), which is where the result differs from ``torch.searchsorted``; on integers, ascending,
    it is the same.  The order of ``sorted_keys`` is not checked (unsorted: unspecified positions within ``[0, n]``).
    ``queries_sorted=True`` declares the queries sorted in the same order and takes the fastest route.  No wait on the host.  16-bit
    dtypes are a ``TypeError``."""
    if sorted_keys.dim() != 1:
        raise ValueError("sorted_keys must be a contiguous 1-D device tensor")
    if sorted_keys.dtype != queries.dtype:
        raise TypeError(f"queries are {queries.dtype}, sorted_keys {sorted_keys.dtype}: one dtype for both")
    dt = sorted_keys.dtype
    if dt not in _KEY_TYPE and dt not in _KEY64_TYPE:
        raise TypeError(f"unsupported key dtype {dt}: searchsorted takes 32- and 64-bit keys (int32, uint32, float32, int64, uint64, float64)")
    kt = _key_type(sorted_keys, unsigned, _KEY_TYPE if dt in _KEY_TYPE else _KEY64_TYPE)
    if not sorted_keys.is_contiguous() or not queries.is_contiguous() or sorted_keys.device.type != "cuda" or queries.device != sorted_keys.device:
        raise ValueError("sorted_keys and queries must be contiguous tensors on one GPU")
    n, m = sorted_keys.numel(), queries.numel()
    if m == 0 or n == 0:  # nothing in front of anything
        return torch.zeros(queries.shape, dtype=torch.int32, device=queries.device)
    with torch.cuda.device(sorted_keys.device):
        wants_sort = not queries_sorted and search_plan(n, m, sorted_keys.element_size())["route_unsorted"] == _SEARCH_ROUTE_SORT
        s = _search_handle(sorted_keys.device, n, m, kt, _order(descending), wants_sort)
        out = s.search(sorted_keys, queries.reshape(-1), n, m, right=right, queries_sorted=queries_sorted)
    return out.reshape(queries.shape)


def bucketize(input: torch.Tensor, boundaries: torch.Tensor, right: bool = False) -> torch.Tensor:  # noqa: A002
    """``torch.bucketize`` in this library's order: ``searchsorted(boundaries, input, right=right)`` under torch's argument order
    (ascending boundaries; int32 result).  Narrower than torch's: ``boundaries`` must be 1-D and contiguous, ``input`` contiguous, both
    on one GPU and of ONE dtype (a mixed pair is a ``TypeError``: convert first; torch promotes), and there is no ``out_int32`` or
    ``out`` argument."""
    return searchsorted(boundaries, input, right=right)
