// topk_rows_kernels.hpp — row-wise top-k for gs_topk_select_rows_* (include/gpusort.h): the first k of every row of a
// [rows, row_len] matrix (row stride in elements, any value >= row_len), one launch for all rows.  The row is the unit of
// parallelism.  No counterpart in the reference project.
//
// Everything runs in the selection space of topk_kernels.hpp: sel = to_bits(key) ^ (descending ? ~0 : 0), both orders look for the
// k smallest sel, ties by position (ascending: lowest positions first; descending: the exact reverse of the stable ascending
// order).  Rows start at 4-byte alignment only (odd strides); only the base pointers are 16-byte aligned.  Three kernels by row
// length, VM as in tk_scatter_kernel (0 keys only, 1 the value is the position in the row, 4 / 8 value bytes).  Each is a wrapper that
// finds its row in the matrix and calls the one body of its shape, tkr_wave_row / tkr_tile_row / tkr_stream_row: functions of a
// resolved row (output row, element offset, length, the position its first element counts as), which the segmented top-k
// (topk_seg_kernels.hpp) calls on its segments.  The wave and the tile body are also functions of the key width (TkrKey32 here,
// TkrKey16 in topk_rows16_kernels.hpp) and serve the 16-bit kernels; the 16-bit stream kernel has a body of its own (said there):
//   tkr_wave_kernel    row_len <= 256: one wave per row, TKR_WAVE_ROWS rows per workgroup, the wave class's four ranking passes
//                      (seg_wave_sort_passes) on the row in registers; the head is written.
//   tkr_tile_kernel    row_len <= seg_max_lds(value bytes): one workgroup per row on the single-tile shape of the length's class
//                      (g_small_class), the row read once into registers, the single-tile sort's passes, the head written.
//   tkr_stream_kernel  longer rows, k <= TKR_STAGE: one workgroup of 1024 threads per row, a radix select on 32-bit LDS counters:
//                      up to three levels of 12 + 12 + 8 bits, each one read of the row (16-byte loads behind a scalar peel) into
//                      a 4096-bin histogram and a workgroup scan for the bin P that holds the k-th element.  Narrowing stops as soon
//                      as the elements in front of P and those in P together fit the LDS staging (TKR_STAGE elements) — or at the
//                      third level, where P is the exact 32-bit pattern T.  One more read gathers them into the staging, in input
//                      order: everything in front, and of those equal everything, or, at the exact level when they do not all fit,
//                      the wanted share by position rank (the first `take` ascending, the last `take` descending).  The staged
//                      elements (sel, position) are sorted stably in LDS (the single-tile passes, 1024 x 4) and the first k written;
//                      values are fetched by position.
//                      Result: 2 reads of the row for keys that spread over their top 12 bits, 3 where the top 24 are needed,
//                      <= 3 reads of the row, 1 write of k, for every row in which at most TKR_STAGE elements share T's top 24
//                      bits; a row with more of them (long runs of one value) takes a 4th read.  Re-reads of a row of a few MiB
//                      come from L2 / MALL.  ctl[TKR_CTL_READS] records the most reads any row took.
// Every LDS and global store index is checked against its buffer's length; a count that does not add up sets TK_ST_INTERNAL and
// leaves that row's output unwritten.  No kernel waits on another workgroup.  Registers, LDS and scratch per kernel: DESIGN.md 3.10
// (none uses scratch but the 1024 x 32 tile shape in its ballot form, exactly as the single-tile sort of that shape does).
#pragma once
#include "segsort_kernels.hpp"
#include "topk_kernels.hpp"

namespace gs {

constexpr uint32_t TKR_CTL_READS = 1;        // control word beside TKC_STATUS: most reads of a row (stream kernel)
constexpr uint32_t TKR_CTL_ACC = TKC_WORDS;  // behind the words tk_init_kernel clears: the status gathered over the rows of a LOOP call
constexpr uint32_t TKR_CTL_WORDS = TKC_WORDS + 1;
constexpr uint32_t TKR_WAVE_ROWS = 4;        // rows (waves) per workgroup of the wave kernel
constexpr int TKR_THREADS = 1024;
constexpr uint32_t TKR_CHUNK = 4 * TKR_THREADS;
constexpr uint32_t TKR_UNROLL = 4;
constexpr uint32_t TKR_TILE = TKR_UNROLL * TKR_CHUNK;
constexpr uint32_t TKR_BINS = 4096;          // 12 bits per level on 32-bit counters (16 KiB)
constexpr int TKR_SORT_KPT = 4;
constexpr uint32_t TKR_STAGE = TKR_THREADS * TKR_SORT_KPT;  // staged (sel, position) pairs: the largest k of the stream kernel

struct TkrArgs {
    const uint32_t* keys;  // (the 16-bit key types, topk_rows16_kernels.hpp: 2-byte elements behind keys and out_keys)
    const void* vals;
    uint32_t* out_keys;
    void* out_vals;
    uint32_t rows, row_len, row_stride, k, kt, descending;
    uint32_t* ctl;
};

template <int VM>
struct TkrVal {
    static constexpr int VB = VM == 0 ? 0 : VM == 8 ? 8 : 4;  // what the sort carries
    using type = typename ValT<VB>::type;
};

// a call starts from a clean control block (a kernel: an ordinary node of a captured graph)
__global__ __launch_bounds__(64) void tkr_reset_kernel(uint32_t* __restrict__ ctl) {
    static_assert(TKR_CTL_WORDS <= 64, "one wave clears the block; the handle's control block is 256 bytes");
    if (threadIdx.x < TKR_CTL_WORDS) ctl[threadIdx.x] = 0u;
}

// LOOP route, behind every row's 1-D call (whose tk_init_kernel clears TKC_STATUS): the row's status joins those of the rows before
// it, and the sum is what TKC_STATUS holds when the call ends, so gs_topk_check and gs_topk_rows_last speak for every row
__global__ __launch_bounds__(64) void tkr_status_kernel(uint32_t* __restrict__ ctl) {
    if (threadIdx.x == 0) {
        const uint32_t st = ctl[TKR_CTL_ACC] | ctl[TKC_STATUS];
        ctl[TKR_CTL_ACC] = st;
        ctl[TKC_STATUS] = st;
    }
}

// ---- what the key width decides ------------------------------------------------------------------------------------------------
// The wave and the tile body take one of these (the 2-byte one: TkrKey16, topk_rows16_kernels.hpp).  A key travels through the passes
// as a 32-bit word whose low RANKED_BITS hold its sortable bits and whose other bits are 0.
struct TkrKey32 {
    using elem = uint32_t;                        // what keys and out_keys point at
    static constexpr uint32_t RANKED_BITS = 32u;  // the bits seg_wave_sort_passes / tkr_tile_sort_passes rank
    static __device__ __forceinline__ uint32_t to_bits(uint32_t u, uint32_t kt) { return seg_to_bits(u, kt); }
    static __device__ __forceinline__ uint32_t from_bits(uint32_t u, uint32_t kt) { return seg_from_bits(u, kt); }
};

// element `o` of row r's head (o < k is the caller's check); bits: the low RANKED_BITS count
template <class K, int VM>
__device__ __forceinline__ void tkr_emit(const TkrArgs& a, uint32_t r, uint32_t o, uint32_t bits, typename TkrVal<VM>::type val) {
    using V = typename TkrVal<VM>::type;
    using E = typename K::elem;
    const size_t dst = (size_t)r * a.k + o;
    reinterpret_cast<E*>(a.out_keys)[dst] = (E)K::from_bits(bits, a.kt);  // (a 2-byte store keeps the low half)
    if constexpr (VM != 0) static_cast<V*>(a.out_vals)[dst] = val;
}

// ---- the row bodies ---------------------------------------------------------------------------------------------------------------
// Each works on a resolved row: keys[base .. base + len), its head to output row r, pos0 what the row's first element counts as in
// the position mode (VM 1).  The row-wise kernels below and in topk_rows16_kernels.hpp find the row as r * row_stride with pos0 = 0,
// the segmented ones (topk_seg_kernels.hpp) take it from a class list with pos0 = the segment's start.  The LDS is each body's own.

// One row on the calling wave, len <= SEG_WAVE_MAX: sorted by the wave class's ranking passes in registers, the head written.  The
// tables are the calling wave's own; the passes' barriers are the workgroup's: every wave of the workgroup calls this, and equally
// often.  A wave without a row passes len 0: the passes run on no rows of slots and nothing is written, but the clamped loads still
// read keys[base] (and vals[base], VM 4 / 8), so such a caller passes a readable base (both callers pass 0).
template <class K, int VM>
__device__ __forceinline__ void tkr_wave_row(const TkrArgs& a, uint32_t r, size_t base, uint32_t len, uint32_t pos0) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB, KPT = SEG_WAVE_MAX / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TKR_WAVE_ROWS][RADIX];
    __shared__ uint32_t s_stage[TKR_WAVE_ROWS][SEG_WAVE_MAX];
    __shared__ V s_vstage[VB != 0 ? TKR_WAVE_ROWS : 1][VB != 0 ? SEG_WAVE_MAX : 1];
    const typename K::elem* keys = reinterpret_cast<const typename K::elem*>(a.keys);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t key[KPT];
    V val[VB != 0 ? KPT : 1];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = lane + i * 64u, ci = idx < len ? idx : (len ? len - 1u : 0u);
        key[i] = keys[base + ci];
        if constexpr (VM == 1) val[i] = pos0 + ci;
        else if constexpr (VM != 0) val[i] = static_cast<const V*>(a.vals)[base + ci];
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) key[i] = lane + i * 64u < len ? K::to_bits(key[i], a.kt) : 0xffffffffu;
    seg_wave_sort_passes<VB, K::RANKED_BITS>(key, val, (len + 63u) >> 6, lane, s_hist[wave], s_stage[wave], s_vstage[VB != 0 ? wave : 0]);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = lane + i * 64u;
        if (idx < len) {
            const uint32_t o = a.descending ? len - 1u - idx : idx;
            if (o < a.k) tkr_emit<K, VM>(a, r, o, key[i], val[VB != 0 ? i : 0]);
        }
    }
}

// ---- the passes of the single-tile sort (tile_sort_body, onesweep_kernels.hpp) on 32-bit keys that are already in registers --------
// Slot my_base + i * 64 of the tile (my_base = wave * 64 * KPT + lane) holds key[i] as sortable bits and val[i]; slots >= n hold all-one
// dummies; on return the same slots hold the sorted order.  The pass loop is tile_sort_body's for one key word, restated here because
// tile_sort_body loads from and stores to the array it sorts and a row must not be written: calling one shared function from both changed
// the register allocation of the existing single-tile and segmented-sort kernels (4 to 17 more VGPRs, SGPR spills in the RANK 1 forms),
// and those kernels stay as they are (tile_sort_body carries a note that points here: a fix to the passes belongs in both copies).
// The LDS is this function's own.  BITS: the key bits that are ranked, from bit 0 up (16: the two passes of topk_rows16_kernels.hpp).
template <int SMALL_THREADS, int SMALL_KPT, int VB, int RANK, uint32_t BITS = 32u>
__device__ __forceinline__ void tkr_tile_sort_passes(uint32_t (&key)[SMALL_KPT], typename ValT<VB>::type (&val)[VB != 0 ? SMALL_KPT : 1], uint32_t n) {
    using V = typename ValT<VB>::type;
    constexpr int KPT = SMALL_KPT, WAVES = SMALL_THREADS / 64;
    constexpr uint32_t SMALL_TILE = SMALL_THREADS * SMALL_KPT;
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[SMALL_TILE];
    __shared__ __attribute__((aligned(16))) V s_vstage[VB != 0 ? SMALL_TILE : 1];
    __shared__ uint32_t s_whist[WAVES * RADIX];
    __shared__ uint32_t s_wtot[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t my_base = wave * (64u * KPT) + lane;
    uint32_t* whist = s_whist + wave * RADIX;
#pragma unroll 1
    for (uint32_t shift_full = 0; shift_full < BITS; shift_full += 8) {
        const uint32_t shift = shift_full;
        auto dword = [&](int i) { return key[i]; };
        for (uint32_t i = tid; i < WAVES * RADIX; i += SMALL_THREADS) s_whist[i] = 0;
        __syncthreads();
        uint32_t off[KPT];
        if constexpr (RANK == 0) {
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const uint32_t w = dword(i);
                const uint32_t d = (w >> shift) & 255u;
                uint32_t acc_lo = 0, acc_hi = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t B = (uint32_t)__builtin_amdgcn_sbfe((int32_t)w, shift + k, 1);
                    const unsigned long long b = __builtin_amdgcn_ballot_w64(B != 0u);
                    acc_lo = __builtin_amdgcn_bitop3_b32(acc_lo, (uint32_t)b, B, 0xF6);
                    acc_hi = __builtin_amdgcn_bitop3_b32(acc_hi, (uint32_t)(b >> 32), B, 0xF6);
                }
                const uint32_t plo = ~acc_lo, phi = ~acc_hi;
                const uint32_t below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
                const uint32_t total = __popc(plo) + __popc(phi);
                const uint32_t pre = whist[d];
                if (below == total - 1u) whist[d] = pre + total;
                asm volatile("" ::: "memory");
                off[i] = pre + below;
            }
        } else {
            // slots >= n take no part (the dummies would all meet on the counter of digit 255, 64 lanes deep,
            // in every pass); they stay behind the n real keys, so validity is a property of the slot
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const uint32_t d = (dword(i) >> shift) & 255u;
                off[i] = 0;
                if (my_base + i * 64u < n)
                    off[i] = __hip_atomic_fetch_add(&whist[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        uint32_t run = 0, scan_incl = 0;
        if (tid < RADIX) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const uint32_t c = s_whist[w * RADIX + tid];
                s_whist[w * RADIX + tid] = run;
                run += c;
            }
            scan_incl = wave_inclusive_scan(run, lane);
            if (lane == 63) s_wtot[wave] = scan_incl;
        }
        __syncthreads();
        if (tid < RADIX) {
            uint32_t wbase = 0;
            for (uint32_t w = 0; w < wave; ++w) wbase += s_wtot[w];
            const uint32_t dpre = wbase + scan_incl - run;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s_whist[w * RADIX + tid] += dpre;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t lpos = off[i] + s_whist[wave * RADIX + ((dword(i) >> shift) & 255u)];
            if (RANK == 0 || my_base + i * 64u < n) {
                s_stage[lpos] = key[i];
                if constexpr (VB != 0) s_vstage[lpos] = val[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            key[i] = s_stage[my_base + i * 64u];
            if constexpr (VB != 0) val[i] = s_vstage[my_base + i * 64u];
        }
        // the next pass starts with a barrier (after zeroing whist) before anything writes the stage
    }
}

// One row on the calling workgroup of THREADS threads, 1 <= n <= THREADS * KPT (the caller's check): read once into registers, the
// single-tile sort's passes, the head written.  Called or not is uniform over the workgroup; a caller that goes on to another row
// puts a barrier in between (the passes' LDS is read after their last barrier).
template <class K, int THREADS, int KPT, int VM, int RANK>
__device__ __forceinline__ void tkr_tile_row(const TkrArgs& a, uint32_t r, size_t base, uint32_t n, uint32_t pos0) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB;
    const typename K::elem* keys = reinterpret_cast<const typename K::elem*>(a.keys);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t my_base = wave * (64u * KPT) + lane;
    uint32_t key[KPT];
    V val[VB != 0 ? KPT : 1];
    // unconditional loads on a clamped index, masked afterwards (as tile_sort_body)
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = my_base + i * 64u, ci = idx < n ? idx : n - 1u;
        key[i] = keys[base + ci];
        if constexpr (VM == 1) val[i] = pos0 + ci;
        else if constexpr (VM != 0) val[i] = static_cast<const V*>(a.vals)[base + ci];
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) key[i] = my_base + i * 64u < n ? K::to_bits(key[i], a.kt) : 0xffffffffu;
    tkr_tile_sort_passes<THREADS, KPT, VB, RANK, K::RANKED_BITS>(key, val, n);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = my_base + i * 64u;
        if (idx < n) {
            const uint32_t o = a.descending ? n - 1u - idx : idx;
            if (o < a.k) tkr_emit<K, VM>(a, r, o, key[i], val[VB != 0 ? i : 0]);
        }
    }
}

// The row as the index range [lo, hi) of the 16-byte aligned pointer q (lo <= 3: the peel).  Four elements of thread `tid` in the
// chunk at c; mask: which of them lie in the row.  A chunk inside the row is one 16-byte load per thread, the first and the last
// chunk are loaded element by element.
__device__ __forceinline__ uint4 tkr_load_chunk(const uint32_t* q, uint32_t c, uint32_t lo, uint32_t hi, uint32_t tid, uint32_t& mask) {
    const uint32_t i = c + tid * 4u;
    if (GS_LIKELY(c >= lo && c + TKR_CHUNK <= hi)) {  // (uniform)
        mask = 15u;
        return *reinterpret_cast<const uint4*>(q + i);
    }
    uint32_t e[4] = {0u, 0u, 0u, 0u};
    mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (i + j >= lo && i + j < hi) {
            e[j] = q[i + j];
            mask |= 1u << j;
        }
    }
    return uint4{e[0], e[1], e[2], e[3]};
}

// One row on the calling workgroup of TKR_THREADS threads, 32-bit keys, k <= TKR_STAGE and k <= row_len (the caller's checks): the
// radix select of the header, the first k to output row r.  Every return is uniform over the workgroup; a caller that goes on to
// another row puts a barrier in between.  (tkr16_stream_kernel, topk_rows16_kernels.hpp, has its own body; its header says why.)
template <int VM, int RANK>
__device__ __forceinline__ void tkr_stream_row(const TkrArgs& a, const uint32_t r, const size_t row_base, const uint32_t row_len, const uint32_t pos0) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t T = TKR_THREADS, W = T / 64, SLOTS = TKR_UNROLL * W;
    static_assert(SLOTS == 64, "the tile's wave totals are scanned by one wave");
    static_assert(TKR_BINS == 4u * T, "four bins per thread in the scan");
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TKR_BINS];
    __shared__ uint32_t s_skey[TKR_STAGE], s_spos[TKR_STAGE];
    __shared__ uint32_t s_w[2][SLOTS + 1];  // packed: front | equal << 16 (a tile holds 16 384 elements)
    __shared__ uint32_t s_ws[W], s_bc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = a.k, kt = a.kt, flip = a.descending ? 0xffffffffu : 0u;
    const uint32_t* p = a.keys + row_base;
    const uint32_t lo = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u), hi = lo + row_len;
    const uint32_t* q = p - lo;  // (the base pointer is 16-byte aligned: q never lies in front of it)
    auto fail = [&]() { if (tid == 0) atomicOr(&a.ctl[TKC_STATUS], TK_ST_INTERNAL); };

    // ---- narrow: pfx = the bits of P found so far, front = elements in front of it, equal = elements in it
    uint32_t pfx = 0, front = 0, equal = row_len, level = 0, sh = 0;
    for (;; ++level) {
        sh = level == 0u ? 20u : level == 1u ? 8u : 0u;
        const uint32_t nbits = level == 2u ? 8u : 12u, above = sh + nbits;
        reinterpret_cast<uint4*>(s_hist)[tid] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
        auto process = [&](const uint4 t, const uint32_t mask) {
            const uint32_t k4[4] = {t.x, t.y, t.z, t.w};
            uint32_t d[4], m = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t sel = seg_to_bits(k4[j], kt) ^ flip;
                d[j] = (sel >> sh) & (TKR_BINS - 1u) & ((1u << nbits) - 1u);
                if (((mask >> j) & 1u) && (level == 0u || (sel >> above) == pfx)) m |= 1u << j;
            }
            // a whole wave under one bin (sorted or constant rows): one add
            const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
            if (__builtin_amdgcn_ballot_w64(m == 15u && d[0] == f && d[1] == f && d[2] == f && d[3] == f) == ~0ull) {
                if (lane == 0) atomicAdd(&s_hist[f], 256u);
                return;
            }
            if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) return;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if ((m >> j) & 1u) atomicAdd(&s_hist[d[j]], 1u);
        };
        for (uint32_t c0 = 0; c0 < hi; c0 += TKR_TILE) {
            uint4 t[TKR_UNROLL];
            uint32_t mask[TKR_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
                const uint32_t c = c0 + u * TKR_CHUNK;
                mask[u] = 0u;
                t[u] = uint4{0u, 0u, 0u, 0u};
                if (c < hi) t[u] = tkr_load_chunk(q, c, lo, hi, tid, mask[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u)
                if (c0 + u * TKR_CHUNK < hi) process(t[u], mask[u]);  // (uniform)
        }
        __syncthreads();
        // the bin with in_front < wanted <= in_front + count
        const uint32_t wanted = k - front;
        const uint4 c = reinterpret_cast<const uint4*>(s_hist)[tid];
        const uint32_t mine = c.x + c.y + c.z + c.w;
        const uint32_t incl = wave_inclusive_scan(mine, lane);
        if (lane == 63) s_ws[wave] = incl;
        if (tid == 0) s_bc[0] = TK_NO_BIN;
        __syncthreads();
        uint32_t fr = incl - mine, total = 0;
        for (uint32_t x = 0; x < W; ++x) {
            if (x < wave) fr += s_ws[x];
            total += s_ws[x];
        }
        if (fr < wanted && wanted <= fr + mine) {  // exactly one thread
            const uint32_t cc[4] = {c.x, c.y, c.z, c.w};
            uint32_t b = 0, eq = cc[0];
#pragma unroll
            for (uint32_t i = 0; i < 3; ++i)
                if (b == i && fr + cc[i] < wanted) { fr += cc[i]; b = i + 1u; eq = cc[i + 1u]; }
            s_bc[0] = tid * 4u + b;
            s_bc[1] = fr;
            s_bc[2] = eq;
        }
        __syncthreads();
        const uint32_t bin = s_bc[0];
        if (total != equal || bin == TK_NO_BIN) { fail(); return; }  // (uniform)
        front += s_bc[1];
        equal = s_bc[2];
        pfx = (pfx << nbits) | bin;
        if (front + equal <= TKR_STAGE || level == 2u) break;
    }
    // ---- gather, in input order: [0, front) the elements in front of P, [front, front + take) those in P (by position rank)
    const uint32_t take = front + equal <= TKR_STAGE ? equal : k - front;
    const uint32_t eq_lo = (take < equal && flip) ? equal - take : 0u;
    const uint32_t G = front + take;
    if (front >= k || take == 0u || take > equal || G > TKR_STAGE) { fail(); return; }  // (uniform)
    auto stage = [&](uint32_t dst, uint32_t sel, uint32_t pos) {
        if (dst >= G) { atomicOr(&a.ctl[TKC_STATUS], TK_ST_INTERNAL); return; }  // (G <= TKR_STAGE; whichever thread meets it reports it)
        s_skey[dst] = sel;
        s_spos[dst] = pos;
    };
    uint32_t base_lt = 0, base_eq = 0, par = 0;
    for (uint32_t c0 = 0; c0 < hi; c0 += TKR_TILE, par ^= 1u) {
        uint4 t[TKR_UNROLL];
        uint32_t mask[TKR_UNROLL], fl[TKR_UNROLL], excl[TKR_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
            const uint32_t c = c0 + u * TKR_CHUNK;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (c < hi) t[u] = tkr_load_chunk(q, c, lo, hi, tid, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
            const uint32_t k4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            uint32_t f = 0, cnt = 0;  // f: bit j = in front, bit 4 + j = equal
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t h = (seg_to_bits(k4[j], kt) ^ flip) >> sh;
                const bool v = (mask[u] >> j) & 1u;
                if (v && h < pfx) { f |= 1u << j; cnt += 1u; }
                if (v && h == pfx) { f |= 16u << j; cnt += 1u << 16; }
            }
            fl[u] = f;
            const uint32_t incl = wave_inclusive_scan(cnt, lane);
            if (lane == 63) s_w[par][u * W + wave] = incl;
            excl[u] = incl - cnt;
        }
        __syncthreads();
        if (wave == 0) {  // the tile's 64 wave totals: exclusive scan, total behind them
            const uint32_t v = s_w[par][lane];
            const uint32_t in = wave_inclusive_scan(v, lane);
            s_w[par][lane] = in - v;
            if (lane == 63) s_w[par][SLOTS] = in;
        }
        __syncthreads();
        const uint32_t tot = s_w[par][SLOTS];
        if (tot != 0u) {
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
                if (fl[u] == 0u) continue;
                const uint32_t off = s_w[par][u * W + wave] + excl[u];
                uint32_t r_lt = base_lt + (off & 0xffffu), r_eq = base_eq + (off >> 16);
                const uint32_t k4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
                const uint32_t i0 = c0 + u * TKR_CHUNK + tid * 4u - lo;  // position in the row (elements in the row only)
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t sel = seg_to_bits(k4[j], kt) ^ flip;
                    if (fl[u] & (1u << j)) { stage(r_lt, sel, i0 + j); ++r_lt; }
                    else if (fl[u] & (16u << j)) {
                        if (r_eq >= eq_lo && r_eq - eq_lo < take) stage(front + (r_eq - eq_lo), sel, i0 + j);
                        ++r_eq;
                    }
                }
            }
            base_lt += tot & 0xffffu;
            base_eq += tot >> 16;
        }
    }
    if (base_lt != front || base_eq != equal) fail();  // (the stores stayed inside the staging; the row is written as staged)
    if (tid == 0) atomicMax(&a.ctl[TKR_CTL_READS], level + 2u);
    __syncthreads();
    // ---- the staged elements, sorted stably: descending loads them in reverse so that equal keys come out by falling position
    const uint32_t my_base = wave * (64u * TKR_SORT_KPT) + lane;
    uint32_t key[TKR_SORT_KPT], pos[TKR_SORT_KPT];
#pragma unroll
    for (int i = 0; i < TKR_SORT_KPT; ++i) {
        const uint32_t idx = my_base + i * 64u;
        const uint32_t j = idx < G ? (flip ? G - 1u - idx : idx) : 0u;
        key[i] = idx < G ? s_skey[j] : 0xffffffffu;
        pos[i] = s_spos[j];
    }
    tkr_tile_sort_passes<TKR_THREADS, TKR_SORT_KPT, 4, RANK>(key, pos, G);
#pragma unroll
    for (int i = 0; i < TKR_SORT_KPT; ++i) {
        const uint32_t idx = my_base + i * 64u;
        if (idx < k && pos[i] < row_len) {  // (idx < k <= G)
            if constexpr (VM == 0 || VM == 1) tkr_emit<TkrKey32, VM>(a, r, idx, key[i] ^ flip, pos0 + pos[i]);
            else tkr_emit<TkrKey32, VM>(a, r, idx, key[i] ^ flip, static_cast<const V*>(a.vals)[row_base + pos[i]]);
        }
    }
}

// ---- the row-wise kernels: the row is r * row_stride of a [rows, row_len] matrix ----------------------------------------------------
// (the wave and the tile one as functions of the key traits: topk_rows16_kernels.hpp wraps the same two on TkrKey16)

// row_len <= SEG_WAVE_MAX: one wave per row.  Waves beyond the last row run the passes on no rows of slots.
template <class K, int VM>
__device__ __forceinline__ void tkr_matrix_wave(const TkrArgs& a) {
    const uint32_t r = blockIdx.x * TKR_WAVE_ROWS + (threadIdx.x >> 6);
    const bool live = r < a.rows && a.row_len <= SEG_WAVE_MAX;
    tkr_wave_row<K, VM>(a, r, live ? (size_t)r * a.row_stride : 0, live ? a.row_len : 0u, 0u);
}
// row_len <= THREADS * KPT, the single-tile shape of the length's class: one workgroup per row
template <class K, int THREADS, int KPT, int VM, int RANK>
__device__ __forceinline__ void tkr_matrix_tile(const TkrArgs& a) {
    const uint32_t r = blockIdx.x, n = a.row_len;
    if (r >= a.rows || n == 0u || n > (uint32_t)(THREADS * KPT)) return;  // (uniform)
    tkr_tile_row<K, THREADS, KPT, VM, RANK>(a, r, (size_t)r * a.row_stride, n, 0u);
}

template <int VM>
__global__ __launch_bounds__(64 * TKR_WAVE_ROWS) void tkr_wave_kernel(const TkrArgs a) { tkr_matrix_wave<TkrKey32, VM>(a); }
template <int THREADS, int KPT, int VM, int RANK>
__global__ __launch_bounds__(THREADS) void tkr_tile_kernel(const TkrArgs a) { tkr_matrix_tile<TkrKey32, THREADS, KPT, VM, RANK>(a); }
// longer rows: one workgroup of TKR_THREADS per row
template <int VM, int RANK>
__global__ __launch_bounds__(TKR_THREADS) void tkr_stream_kernel(const TkrArgs a) {
    const uint32_t r = blockIdx.x;
    if (r >= a.rows || a.k == 0u || a.k > TKR_STAGE || a.k > a.row_len) return;  // (uniform; the host's checks)
    tkr_stream_row<VM, RANK>(a, r, (size_t)r * a.row_stride, a.row_len, 0u);
}

}  // namespace gs
