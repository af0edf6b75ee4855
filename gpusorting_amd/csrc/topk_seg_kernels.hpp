// topk_seg_kernels.hpp — segmented top-k for gs_segtopk_* (include/gpusort.h): the first k of every segment of one array, the
// segments given by CSR offsets, into a dense [num_segments, k] output, one call for all segments.  No counterpart in the reference
// project.
//
// The composition of two things the tree has: the device-side offset validation and class lists of the segmented sort
// (segsort_kernels.hpp: seg_reset_kernel, seg_classify_kernel, seg_fill_kernel, launched unchanged) and the per-row bodies of the
// row-wise top-k (topk_rows_kernels.hpp: tkr_wave_row and tkr_tile_row on TkrKey32, tkr_stream_row), called here on segment s of a class
// list: base = off[s], len = off[s + 1] - base, output row s, pos0 = off[s].  Launch sequence of one call:
//   seg_reset_kernel, seg_classify_kernel, seg_fill_kernel
//   tks_packed_kernel   length 1 .. 32: 64 consecutive segments per wave, back to back in LDS, a counting rank inside the segment; an
//                       element whose place in the output order is < k is written.  Walks all segments and filters by length (no list).
//                       Length 1 belongs here: the sort's class 0 has nothing to do for it, a top-k must emit it.
//   tks_wave_kernel     33 .. 256: TKR_WAVE_ROWS list entries per workgroup, one per wave (tkr_wave_row)
//   tks_tile_kernel     classes 3 .. 7: one list entry per workgroup on the single-tile shape of the class (tkr_tile_row)
//   tks_stream_kernel   longer than LDS holds: one list entry per workgroup, the radix select (tkr_stream_row); k <= TKR_STAGE < len
// The list kernels run on fixed grids and claim list entries by grid stride (the 1024 x 32 tile shape excepted: one workgroup per
// slot its class can have, as seg_wg_kernel): the host never learns the counts.  Every kernel reads the status word first and leaves
// if the offsets were bad; a segment longer than a non-zero promise is in no list (seg_work_class) and gets no output row.  Slots
// min(k, len) .. k of an output row are not written.  The position mode (VM 1) delivers off[s] + the position in the segment.  No
// kernel waits on another workgroup.  Registers, LDS and scratch per kernel: DESIGN.md 3.17.
#pragma once
#include "topk_rows_kernels.hpp"

namespace gs {

// words of the segmented sort's control block (cleared by seg_reset_kernel) that this handle uses beside SEGC_*
constexpr uint32_t TKSC_TKR = 48;     // where the row bodies' control words lie: TKSC_TKR + TKC_STATUS, TKSC_TKR + TKR_CTL_READS
constexpr uint32_t TKSC_PACKED = 50;  // segments the packed kernel emitted (length 1 .. 32)
static_assert(TKSC_TKR > SEGC_CURSOR + SEG_CLASSES && TKSC_PACKED < SEGC_WORDS && TKC_STATUS < 2 && TKR_CTL_READS < 2, "inside the block, beside the rest");

struct TksArgs {
    const uint32_t* keys;
    const void* vals;
    uint32_t* out_keys;
    void* out_vals;
    const uint32_t* off;
    const uint32_t* list;
    uint32_t* ctl;
    uint32_t num_segments, k, kt, descending, max_len;
};

// the row bodies' view of a call: rows = segments, the row geometry is not read (the bodies take the resolved row)
__device__ __forceinline__ TkrArgs tks_row_args(const TksArgs& a) {
    return TkrArgs{a.keys, a.vals, a.out_keys, a.out_vals, a.num_segments, 0u, 0u, a.k, a.kt, a.descending, a.ctl + TKSC_TKR};
}

// ---- packed class: 1 .. SEG_PACK_MAX elements, 64 consecutive segments per wave ------------------------------------------------
// seg_packed_kernel's layout and counting rank; the keys only go through LDS: a value is fetched by the element's place in the array
// when the element is written, and at most min(k, len) elements of a segment are.
template <int VM>
__global__ __launch_bounds__(64) void tks_packed_kernel(const TksArgs a) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t CAP = 64u * SEG_PACK_MAX;
    __shared__ uint32_t s_key[CAP];
    __shared__ uint32_t s_start[64], s_scan[65];
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const uint32_t lane = threadIdx.x, s = blockIdx.x * 64u + lane;
    uint32_t st = 0, len = 0;
    if (s < a.num_segments) {
        st = a.off[s];
        const uint32_t l = a.off[s + 1u] - st;
        if (l >= 1u && l <= SEG_PACK_MAX && (a.max_len == 0u || l <= a.max_len)) len = l;
    }
    const uint32_t incl = wave_inclusive_scan(len, lane);
    const uint32_t E = __shfl(incl, 63, 64);  // <= CAP
    if (E == 0u) return;
    const unsigned long long mine = __builtin_amdgcn_ballot_w64(len != 0u);
    if (lane == 0) atomicAdd(&a.ctl[TKSC_PACKED], (uint32_t)__popcll(mine));
    s_start[lane] = st;
    s_scan[lane] = incl - len;
    if (lane == 63u) s_scan[64] = E;
    __syncthreads();
    // the segment of layout element e: the last j with scan[j] <= e (empty slots share their successor's scan value)
    auto find = [&](uint32_t e) {
        uint32_t j = 0;
#pragma unroll
        for (uint32_t step = 32; step != 0u; step >>= 1)
            if (s_scan[j + step] <= e) j += step;
        return j;
    };
    for (uint32_t e0 = 0; e0 < E; e0 += 256u) {
        uint32_t kk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // unconditional loads on a clamped element, masked afterwards
            const uint32_t e = e0 + u * 64u + lane, ec = e < E ? e : E - 1u;
            const uint32_t j = find(ec);
            kk[u] = a.keys[s_start[j] + (ec - s_scan[j])];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = e0 + u * 64u + lane;
            if (e < E) s_key[e] = seg_to_bits(kk[u], a.kt);
        }
    }
    __syncthreads();
    for (uint32_t e = lane; e < E; e += 64u) {
        const uint32_t j = find(e);
        const uint32_t lo = s_scan[j], hi = s_scan[j + 1u];
        const uint32_t key = s_key[e];
        uint32_t rank = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t x = s_key[i];
            rank += (x < key || (x == key && i < e)) ? 1u : 0u;
        }
        const uint32_t o = a.descending ? hi - lo - 1u - rank : rank;
        const uint32_t seg = blockIdx.x * 64u + j;  // (j's segment is not empty: seg < num_segments)
        if (o < a.k && seg < a.num_segments) {
            const size_t dst = (size_t)seg * a.k + o;
            const uint32_t g = s_start[j] + (e - lo);
            a.out_keys[dst] = seg_from_bits(key, a.kt);
            if constexpr (VM == 1) static_cast<V*>(a.out_vals)[dst] = g;
            else if constexpr (VM != 0) static_cast<V*>(a.out_vals)[dst] = static_cast<const V*>(a.vals)[g];
        }
    }
}

// entry `it` of class cls's list -> segment, start and length; false where the entry is not a segment of [1, max_len] elements
// (the list holds segments of its class only; the checks keep a broken invariant in bounds)
__device__ __forceinline__ bool tks_resolve(const TksArgs& a, uint32_t list_base, uint32_t it, uint32_t max_len, uint32_t& s, uint32_t& st, uint32_t& len) {
    s = st = len = 0;
    if (list_base + it >= a.num_segments) return false;
    s = a.list[list_base + it];
    if (s >= a.num_segments) return false;
    st = a.off[s];
    len = a.off[s + 1u] - st;
    return len != 0u && len <= max_len;
}

// ---- wave class: one list entry per wave ------------------------------------------------------------------------------------------
// The trip count is the workgroup's (the passes' barriers are workgroup barriers); a wave without an entry runs them on no rows of slots.
template <int VM>
__global__ __launch_bounds__(64 * TKR_WAVE_ROWS) void tks_wave_kernel(const TksArgs a) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t count = a.ctl[SEGC_COUNT + 2], base = seg_list_base(a.ctl, 2);
    for (uint32_t it0 = blockIdx.x * TKR_WAVE_ROWS; it0 < count; it0 += gridDim.x * TKR_WAVE_ROWS) {  // (uniform over the workgroup)
        uint32_t s = 0, st = 0, len = 0;
        const bool live = it0 + wave < count && tks_resolve(a, base, it0 + wave, SEG_WAVE_MAX, s, st, len);
        tkr_wave_row<TkrKey32, VM>(t, s, live ? st : 0u, live ? len : 0u, st);
    }
}

// ---- tile classes: one list entry per workgroup ---------------------------------------------------------------------------------
// LOOP: as seg_wg_kernel (the 1024 x 32 shape sits at its register limit and takes one workgroup per slot its class can have).
template <int THREADS, int KPT, int VM, int RANK, bool LOOP>
__global__ __launch_bounds__(THREADS) void tks_tile_kernel(const TksArgs a, const uint32_t cls) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t count = a.ctl[SEGC_COUNT + cls], base = seg_list_base(a.ctl, cls);
    if constexpr (LOOP) {
        for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
            uint32_t s, st, len;
            if (tks_resolve(a, base, it, (uint32_t)(THREADS * KPT), s, st, len)) tkr_tile_row<TkrKey32, THREADS, KPT, VM, RANK>(t, s, st, len, st);
            __syncthreads();
        }
    } else {
        uint32_t s, st, len;
        if (blockIdx.x < count && tks_resolve(a, base, blockIdx.x, (uint32_t)(THREADS * KPT), s, st, len))
            tkr_tile_row<TkrKey32, THREADS, KPT, VM, RANK>(t, s, st, len, st);
    }
}

// ---- long class: one list entry per workgroup, the radix select -----------------------------------------------------------------
template <int VM, int RANK>
__global__ __launch_bounds__(TKR_THREADS) void tks_stream_kernel(const TksArgs a) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    if (a.k == 0u || a.k > TKR_STAGE) return;  // (uniform; the host's checks)
    const TkrArgs t = tks_row_args(a);
    const uint32_t count = a.ctl[SEGC_COUNT + SEG_CLASS_LONG], base = seg_list_base(a.ctl, SEG_CLASS_LONG);
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
        uint32_t s, st, len;
        if (tks_resolve(a, base, it, 0xffffffffu, s, st, len) && len >= a.k) tkr_stream_row<VM, RANK>(t, s, st, len, st);
        __syncthreads();
    }
}

}  // namespace gs
