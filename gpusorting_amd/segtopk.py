"""Segmented top-k over the C-ABI (``gs_segtopk_*`` in include/gpusort.h): the first k of every segment of one array, the segments
given by CSR offsets, into a dense ``[num_segments, k]`` output, in one call that never waits on the host.

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.
``segmented_topk_reference`` is the pure-numpy statement of the semantics (tests and tools compare against it); it needs no torch
and no GPU.
"""
from __future__ import annotations

import numpy as np

from . import _handle, _lib
from ._handle import (KEY_FLOAT32, KEY_INT32, KEY_UINT32, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING,  # noqa: F401
                      _ptr, _require_cuda, _require_room, _stream_ptr)
from ._lib import check  # noqa: F401
from .topk import topk_reference

_SCALARS = ("longest", "status", "reads", "forms", "rank", "k", "packed")  # GS_SEGTOPK_R_LONGEST ..


def segmented_topk_reference(keys: np.ndarray, offsets: np.ndarray, k: int, values: np.ndarray | None = None, descending: bool = False,
                             key_type: int = KEY_UINT32, fill_key=0, fill_value=0):
    """``topk_reference`` on every segment ``keys[offsets[s]:offsets[s + 1]]`` with ``m_s = min(k, length)``: returns
    ``(keys[S, k], values[S, k], counts[S])``.  Row ``s`` holds the first ``m_s`` of the segment's sorted order in its first ``m_s``
    slots; the other slots, which the device does not write, hold ``fill_key`` / ``fill_value``.  ``values=None`` returns the
    positions in the whole array (``offsets[s]`` plus the position in the segment) as uint32.  ``counts`` is ``m_s`` (int64)."""
    keys = np.ascontiguousarray(keys)
    offsets = np.asarray(offsets).astype(np.int64)
    k = int(k)
    if keys.ndim != 1 or k < 1:
        raise ValueError("keys must be 1-D and k >= 1")
    if offsets.ndim != 1 or offsets.size < 2 or np.any(np.diff(offsets) < 0) or offsets[0] < 0 or offsets[-1] > keys.size:
        raise ValueError("offsets must be num_segments + 1 non-decreasing values that end within the keys")
    if values is not None:
        values = np.ascontiguousarray(values)
        if values.shape != keys.shape:
            raise ValueError("values must match keys in shape")
    segs = offsets.size - 1
    out_k = np.full((segs, k), fill_key, dtype=keys.dtype)
    out_v = np.full((segs, k), fill_value, dtype=np.uint32 if values is None else values.dtype)
    counts = np.minimum(np.diff(offsets), k)
    for s in range(segs):
        a, m = int(offsets[s]), int(counts[s])
        if m == 0:
            continue
        b = int(offsets[s + 1])
        hk, hv = topk_reference(keys[a:b], m, None if values is None else values[a:b], key_type, descending)
        out_k[s, :m] = hk
        out_v[s, :m] = hv + np.uint32(a) if values is None else hv
    return out_k, out_v, counts


def forms_tile(cls: int, rank: int) -> int:
    """``GS_SEGTOPK_F_TILE(cls, rank)``: the bit of a tile-class kernel in the report's forms word."""
    return _lib.GS_SEGTOPK_F_TILE(cls, rank)


_REPORT = tuple((name, _lib.GS_SEGTOPK_R_LONGEST + i) for i, name in enumerate(_SCALARS))


class SegmentedTopK(_handle.Checked, _handle.RankMode, _handle.Handle):
    """One ``gs_segtopk`` handle: the control block and the class lists (``temp_bytes``; nothing sized by ``max_keys``).

    ``value_bytes`` 0 selects keys only; 4 or 8 carries values; on a 4-byte handle ``select(keys, offsets, k, out_keys, None,
    out_values)`` delivers the positions in the whole array as values."""

    # what the key width decides (SegmentedTopK16, segtopk16.py, states its own)
    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_segtopk_", 4, _handle.KEY32_TYPES
    _KEYS_WANTED = "SegmentedTopK takes 32-bit keys only"

    def __init__(self, max_keys: int, max_segments: int, max_k: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT32,
                 mode: int = MODE_KEYS_ONLY, value_bytes: int = 0, device: int | None = None):
        self.key_type = self._check_key_type(key_type)
        self.max_keys, self.max_segments, self.max_k = int(max_keys), int(max_segments), int(max_k)
        self._pairs_mode(order, mode, value_bytes)
        self._create(device, self.max_keys, self.max_segments, self.max_k, mode, self.value_bytes)

    @property
    def temp_bytes(self) -> int:
        return int(self._entry("temp_bytes")(self.max_segments))

    @property
    def max_lds_segment(self) -> int:
        """Longest segment selected in LDS; longer ones take ``k <= rows_max_k``."""
        return int(self._lib.gs_segsort_max_lds_segment(self.mode, self.value_bytes))

    def class_of(self, length: int) -> int:
        return int(self._lib.gs_segsort_class_of(int(length), self.mode, self.value_bytes))

    def select(self, keys, offsets, k: int, out_keys, values=None, out_values=None, n: int | None = None, max_segment_len: int = 0,
               stream=None) -> None:
        """The first ``k`` of every segment ``keys[offsets[s]:offsets[s + 1]]`` of ``keys[:n]`` into ``out_keys[s * k : s * k + m_s]``
        (and ``out_values``), ``m_s = min(k, length)``, on the current stream; the other slots are not written.  ``offsets``: int32
        device tensor of ``num_segments + 1`` CSR offsets.  ``values=None`` with ``out_values`` given (4-byte handle): the values are
        the positions in the whole array.  ``max_segment_len``: a promise (0 = unknown); ``k`` above ``rows_max_k`` needs one that
        fits LDS.  The call never waits on the host; the inputs are not written."""
        _require_cuda(keys, "keys")
        _require_cuda(offsets, "offsets")
        _require_cuda(out_keys, "out_keys")
        kb = self._KEY_BYTES
        if keys.element_size() != kb or out_keys.element_size() != kb or offsets.element_size() != 4 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError(f"keys must be {8 * kb}-bit and offsets a 1-D tensor of num_segments + 1 32-bit words")
        if (out_values is not None) != (self.mode == MODE_PAIRS):
            raise ValueError("out_values must be given exactly when the handle was built with MODE_PAIRS")
        n = keys.numel() if n is None else int(n)
        k = int(k)
        num_segments = offsets.numel() - 1
        _require_room(keys, n, "keys")
        _require_room(values, n, "values")
        _require_room(out_keys, num_segments * k, "out_keys")
        _require_room(out_values, num_segments * k, "out_values")
        for t, name in ((values, "values"), (out_values, "out_values")):
            if t is not None:
                _require_cuda(t, name)
                if t.element_size() != self.value_bytes:
                    raise ValueError(f"{name} must be {self.value_bytes} bytes wide for this handle")
        s = _stream_ptr(stream)
        if out_values is None:
            self._call("select_keys", keys.data_ptr(), n, offsets.data_ptr(), num_segments, k, int(max_segment_len), out_keys.data_ptr(),
                       self.key_type, self.order, s, where="select")
        else:
            self._call("select_pairs", keys.data_ptr(), _ptr(values), n, offsets.data_ptr(), num_segments, k, int(max_segment_len),
                       out_keys.data_ptr(), out_values.data_ptr(), self.key_type, self.order, s, where="select")

    def last(self, stream=None) -> dict:
        """``gs_segtopk_last`` (synchronises): ``counts`` (segments per class of ``class_of``), ``longest``, ``status``, ``reads`` (the
        most reads of its segment any long segment took), ``forms`` (``GS_SEGTOPK_F_*``), ``rank``, ``k``, ``packed`` (segments the
        packed kernel emitted: length 1 .. 32)."""
        w = self._words("last", _lib.GS_SEGTOPK_REPORT_WORDS, stream)
        return {"counts": w[_lib.GS_SEGTOPK_R_CLASSES:_lib.GS_SEGTOPK_R_CLASSES + _lib.GS_SEGSORT_CLASSES], **{name: w[i] for name, i in _REPORT}}
