"""gpusorting_amd — MI355X-native OneSweep radix sort behind the reference's
GPUSortBase / OneSweep / OneSweepDispatcher dispatch surface.

Only the hot path of b0nes164/GPUSorting named by BASELINE.json is here:
  csrc/      hand-written gfx950 HIP kernels + the C-ABI (include/gpusort.h)
  onesweep   host-side mirror of the reference interface (ctypes over the C-ABI)
  sharded    one-process-per-GPU MSD split + RCCL all-to-all-v + local OneSweep
  segsort    segmented sort (CSR offsets) over gs_segsort_*, and its numpy reference
  segsort16  segmented sort of 16-bit keys at their own width over gs_segsort16_*, and its numpy reference
  rowsort    row-wise sort of a [rows, row_len] matrix of 32-bit keys over gs_sort_rows_*, and its numpy reference
  rowsort16  row-wise sort of a [rows, row_len] matrix of 16-bit keys at their own width over gs_sort_rows16_*, and its numpy reference
  sort16     sort of 16-bit keys (float16, bfloat16, int16, uint16) at their own width over gs_sort16_*, and its numpy reference
  topk       top-k selection (the head of the sort without the sort) over gs_topk_*, and its numpy reference
  segtopk    segmented top-k (the first k of every CSR segment) over gs_segtopk_*, and its numpy reference
  segtopk16  segmented top-k of 16-bit keys at their own width over gs_segtopk16_*
  topk16     1-D top-k of 16-bit keys at their own width over gs_topk16_*
  unique     distinct keys, counts, first positions and the inverse map (the sort plus a run-length stage, or that stage alone) over
             gs_unique_*, and its numpy reference
  unique16   the same on 16-bit keys at their own width, from one 65 536-bin histogram, over gs_unique16_*, and its numpy reference
  reduce     reduce by key: one sum, minimum or maximum per distinct key (the pairs sort plus one segmented reduction, or that stage alone
             on runs of equal neighbours) over gs_reduce_*, and its numpy reference
  unique64   unique on 64-bit keys (uint64, int64, float64) over gs_unique64_*, and its numpy reference
  reduce64   reduce by key on 64-bit keys over gs_reduce64_*, and its numpy reference
  search     sorted search: the lower / upper bound of many queries in a sorted array, in the library's own order (both orders, floats
             by the bit flip), over gs_search_*, and its numpy reference
  functional sort / sort_ / argsort / sort_rows / argsort_rows / segmented_sort / topk / topk16 / segmented_topk / segmented_topk16 /
             unique / unique_consecutive / unique16 / unique_consecutive16 / reduce_by_key / reduce_by_key_consecutive / unique64 /
             unique_consecutive64 / reduce_by_key64 / reduce_by_key_consecutive64 / searchsorted / bucketize on torch tensors (plumbing
             over OneSweep / RowSort / RowSort16 / SegmentedSort / SegmentedSort16 / TopK / SegmentedTopK / SegmentedTopK16 / TopK16 /
             Unique / Unique16 / ReduceByKey / Unique64 / ReduceByKey64 / SortedSearch)
"""
from .onesweep import (  # noqa: F401
    ENTROPY_PRESET_1, ENTROPY_PRESET_2, ENTROPY_PRESET_3, ENTROPY_PRESET_4, ENTROPY_PRESET_5,
    KEY_FLOAT32, KEY_FLOAT64, KEY_INT32, KEY_INT64, KEY_UINT32, KEY_UINT64, MODE_KEYS_ONLY, MODE_PAIRS, ORDER_ASCENDING, ORDER_DESCENDING,
    GPUSortingConfig, OneSweep, OneSweepDispatcher, init_random, validate,
)
from ._lib import KEY_BFLOAT16, KEY_FLOAT16, KEY_INT16, KEY_UINT16, GpuSortError  # noqa: F401
from .functional import (  # noqa: F401
    argsort, argsort_rows, reduce_by_key, reduce_by_key_consecutive, segmented_argsort, segmented_sort, segmented_sort_, segmented_topk, segmented_topk16, sort, sort_, sort_rows, sort_rows_, topk,
    topk16, unique, unique16, unique_consecutive, unique_consecutive16,
    reduce_by_key64, reduce_by_key_consecutive64, unique64, unique_consecutive64,
    bucketize, searchsorted,
)
from .reduce import ReduceByKey, reduce_by_key_reference  # noqa: F401
from .reduce64 import ReduceByKey64, reduce_by_key64_reference  # noqa: F401
from .rowsort import RowSort, sort_rows_plan, sort_rows_reference  # noqa: F401
from .rowsort16 import SORT_ROWS16_FORMS, RowSort16, sort_rows16_plan, sort_rows16_reference  # noqa: F401
from .search import SortedSearch, search_plan, search_plan_reference, searchsorted_reference  # noqa: F401
from .segsort import SegmentedSort, segmented_sort_reference, segsort_long_units  # noqa: F401
from .segsort16 import SEGSORT16_FORMS, SegmentedSort16, segmented_sort16_reference, segsort16_units  # noqa: F401
from .segtopk import SegmentedTopK, segmented_topk_reference  # noqa: F401
from .segtopk16 import SegmentedTopK16  # noqa: F401
from .sort16 import Sort16, sort16_plan, sort16_reference  # noqa: F401
from .topk import TopK, topk_reference, topk_rows_reference  # noqa: F401
from .topk16 import TopK16  # noqa: F401
from .unique import Unique, unique_plan, unique_reference  # noqa: F401
from .unique16 import Unique16, unique16_reference  # noqa: F401
from .unique64 import Unique64, unique64_reference  # noqa: F401
