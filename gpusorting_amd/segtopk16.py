"""Segmented top-k on 16-bit keys over the C-ABI (``gs_segtopk16_*`` in include/gpusort.h): the first k of every segment of one array
of float16, bfloat16, int16 or uint16 keys, the segments given by CSR offsets, into a dense ``[num_segments, k]`` output, in one call
that never waits on the host and reads the keys at their own width.

No counterpart in the reference project.  PyTorch is used only for device memory and the current HIP stream.  The numpy statement of
the semantics is ``segmented_topk_reference`` (segtopk.py) on ``uint16`` bit patterns with a 16-bit key type.
"""
from __future__ import annotations

from ._handle import KEY16_TYPES as _KEY16_TYPES
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16  # noqa: F401
from .segtopk import MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING, SegmentedTopK, forms_tile, segmented_topk_reference  # noqa: F401


class SegmentedTopK16(SegmentedTopK):
    """One ``gs_segtopk16`` handle: ``SegmentedTopK`` (``select``, ``status``, ``check``, ``last``, ``rank_mode``, ``class_of``,
    ``max_lds_segment``, ``temp_bytes``) on 2-byte key tensors.  The report of ``last`` has the 32-bit call's layout; ``reads`` is 2 or
    3 here."""

    _PREFIX, _KEY_BYTES, _KEY_TYPES = "gs_segtopk16_", 2, _KEY16_TYPES
    _KEYS_WANTED = "SegmentedTopK16 takes 16-bit keys only"

    def __init__(self, max_keys: int, max_segments: int, max_k: int, order: int = ORDER_ASCENDING, key_type: int = KEY_UINT16,
                 mode: int = MODE_KEYS_ONLY, value_bytes: int = 0, device: int | None = None):
        super().__init__(max_keys, max_segments, max_k, order, key_type, mode, value_bytes, device)
