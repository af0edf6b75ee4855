// gpusort_capi.hip — host side of libgpusort.so: the C-ABI of include/gpusort.h
// over the gfx950 kernels of onesweep_kernels.hpp.
//
// Replaces the dispatch half of the reference's OneSweepDispatcher
// (GPUSortingCUDA/Sort/OneSweepDispatcher.cuh:301-391): state clear, the
// 1 + 1 + 4 launch sequence, validation read-back.  Differences by design:
//   - no clear launch at all (the reference: 6 cudaMemset, :301-309): the scan state is ONE contiguous slab that
//     the GlobalHistogram kernel zeroes while it reads the keys; no host sync inside the sort (:318);
//   - the pass plan (identity passes dropped, input buffer of each pass, skew handling, position chains) is made by
//     the Scan kernel on the device;
//   - descriptor rows = tiles + 1, so the last tile's publish to row tile+1
//     stays in bounds (the reference overruns by 256 words when size==maxSize);
//   - everything is enqueued on the caller's stream.
#include "../../include/gpusort.h"
#include "onesweep_kernels.hpp"
#include "mid_kernels.hpp"
#include "hybrid_kernels.hpp"
#include "segsort_kernels.hpp"
#include "topk_kernels.hpp"
#include "topk_rows_kernels.hpp"
#include "topk_rows16_kernels.hpp"
#include "topk_seg_kernels.hpp"
#include "topk_seg16_kernels.hpp"
#include "sort16_kernels.hpp"
#include "topk16_kernels.hpp"
#include "unique_kernels.hpp"
#include "unique16_kernels.hpp"
#include "reduce_kernels.hpp"
#include "search_kernels.hpp"
#include "merge_kernels.hpp"
#include "sortrows_kernels.hpp"
#include "sortrows16_kernels.hpp"
#include "segsort16_kernels.hpp"
#include "segsort_long_kernels.hpp"

// One translation unit; one host file per concern, in this order (each may use what stands above it):
#include "host_common.hpp"      // GS_HIP, argument predicates, div_up, cu_count, DeviceScratch
#include "kernel_registry.hpp"  // launcher templates, which kernels a build flavour compiles
#include "handle_core.hpp"      // what the handles below share: layout arena, workspace + control read-back, create/destroy frame, rank mode,
                                // alternate-buffer predicates, pass ping-pong, the head of a segmented call (gs_onesweep and gs_mgpu do not use it)
#include "onesweep_host.hpp"    // gs_onesweep: slab sizing, prologue, routing, sort_impl; every gs_onesweep_* / gs_selftest_* / gs_debug_* entry
#include "segsort_host.hpp"     // gs_segsort
#include "topk_host.hpp"        // gs_topk: the 1-D selection and the row-wise one
#include "sort16_host.hpp"      // gs_sort16: the sort of 16-bit keys
#include "topk16_host.hpp"      // gs_topk16: the 1-D selection on 16-bit keys
#include "unique_host.hpp"      // gs_unique: distinct keys, counts, first positions, inverse (behind onesweep_host and sort16_host)
#include "unique16_host.hpp"    // gs_unique16: the same on 16-bit keys, from one histogram (behind sort16_host and unique_host)
#include "reduce_host.hpp"      // gs_reduce: one sum, minimum or maximum per distinct key (behind onesweep_host and unique_host)
#include "unique64_host.hpp"    // gs_unique64: gs_unique on 8-byte keys (behind unique_host)
#include "reduce64_host.hpp"    // gs_reduce64: gs_reduce on 8-byte keys (behind reduce_host)
#include "search_host.hpp"      // gs_search: lower / upper bound of many queries in a sorted array (behind onesweep_host and unique_host)
#include "merge_host.hpp"       // gs_merge: two sorted arrays into one: keys, pairs or positions (behind search_kernels.hpp: its word and staging helpers)
#include "sortrows_host.hpp"    // gs_sort_rows: every row of a matrix sorted in one call
#include "sortrows16_host.hpp"  // gs_sort_rows16: the same on 16-bit keys
#include "segsort16_host.hpp"   // gs_segsort16: the segmented sort on 16-bit keys
#include "topk_seg_host.hpp"    // gs_segtopk: the first k of every segment
#include "topk_seg16_host.hpp"  // gs_segtopk16: the same on 16-bit keys
#include "gpusort_mgpu.hpp"     // gs_mgpu, gs_onesweep_sort_sharded
