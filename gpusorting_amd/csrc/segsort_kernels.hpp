// segsort_kernels.hpp — gfx950 (wave64) device code of the segmented sort: many independent segments of one array, given by
// CSR offsets, each sorted on its own, in place (gs_segsort_* in include/gpusort.h).
//
// Behavioural spec (what, not how): reference b0nes164/GPUSorting, GPUSortingCUDA/SegSort/SplitSort/SplitSort.cuh:674-709
// (SplitSortAllocateTempMemory / SplitSortPairs: segments are binned by length on the device, every bin has its own kernel).
//
// Launch sequence of one call (all on the caller's stream, no host round trip unless long segments are allowed):
//   seg_reset_kernel      zeroes the control block (status, class counts, cursors)
//   seg_classify_kernel   validates the offsets (non-decreasing, last <= n), counts the segments per length class, records
//                         the longest segment and the status word.  NOTHING is loaded through the offsets before it has run:
//                         every later kernel reads the status word first and leaves if the offsets were bad.
//   seg_fill_kernel       one list of segment numbers per class, all in ONE array of num_segments words (class bases = prefix
//                         of the counts; slots by one atomic per workgroup and class)
//   seg_packed_kernel     class 1, 2 .. 32 elements: 64 consecutive segments per wave, counting rank inside the segment
//   seg_wave_kernel       class 2, 33 .. 256: one segment per wave, four 8-bit ranking passes in LDS
//   seg_wg_kernel         classes 3 .. 7, up to 1024 / 2048 / 8192 / 16 384 / 32 768: one segment per workgroup, the single-tile
//                         sort of onesweep_kernels.hpp (tile_sort_body) on the shape of that size
//   class 8 (longer than LDS holds) is the host's: gpusort_capi.hip reads the list back and runs the OneSweep engine per segment;
//   seg_merge_head_kernel puts the up to three leading elements the engine's 16-byte alignment leaves out back in.
// Classes 2 .. 8 claim their work from the class list with a fixed grid (grid stride): the host never learns the counts.
// No kernel here waits for another workgroup.
#pragma once
#include "onesweep_kernels.hpp"

namespace gs {

constexpr uint32_t SEG_CLASSES = 9;
constexpr uint32_t SEG_PACK_MAX = 32;    // longest segment of the packed class
constexpr uint32_t SEG_WAVE_MAX = 256;   // longest segment of the wave class (64 lanes x 4 keys)
constexpr uint32_t SEG_CLASS_LONG = 8;
// upper length bound of classes 0 .. 7 (class 6 takes no 8-byte values, class 7 keys only: seg_class_of)
constexpr uint32_t SEG_CLASS_MAX[8] = {1, SEG_PACK_MAX, SEG_WAVE_MAX, 1024, 2048, 8192, 16384, 32768};

// control block (uint32 words), zeroed by seg_reset_kernel at the start of every call
constexpr uint32_t SEGC_STATUS = 0;   // SEG_ST_* bits
constexpr uint32_t SEGC_MAXLEN = 1;   // longest segment seen
constexpr uint32_t SEGC_COUNT = 8;    // [SEG_CLASSES] segments per class
constexpr uint32_t SEGC_CURSOR = 24;  // [SEG_CLASSES] slots handed out by seg_fill_kernel
constexpr uint32_t SEGC_WORDS = 64;
constexpr uint32_t SEG_ST_ARG = 1;    // offsets decrease somewhere or end beyond n: nothing is sorted
constexpr uint32_t SEG_ST_SIZE = 2;   // a segment is longer than the caller promised: that segment is left as it is

__host__ __device__ constexpr uint32_t seg_max_lds(uint32_t vb) { return vb == 0 ? 32768u : vb == 4 ? 16384u : 8192u; }
__host__ __device__ constexpr uint32_t seg_class_of(uint32_t len, uint32_t vb) {
    return len <= 1 ? 0u : len <= SEG_PACK_MAX ? 1u : len <= SEG_WAVE_MAX ? 2u : len <= 1024 ? 3u : len <= 2048 ? 4u : len <= 8192 ? 5u
           : len > seg_max_lds(vb) ? SEG_CLASS_LONG : len <= 16384 ? 6u : 7u;
}
// first entry of class c's list: the long class first (the host reads it from a fixed place), then classes 2 .. 7
__device__ __forceinline__ uint32_t seg_list_base(const uint32_t* __restrict__ ctl, uint32_t c) {
    if (c == SEG_CLASS_LONG) return 0;
    uint32_t b = ctl[SEGC_COUNT + SEG_CLASS_LONG];
    for (uint32_t k = 2; k < c; ++k) b += ctl[SEGC_COUNT + k];
    return b;
}
// the class a segment is SORTED in: a segment longer than promised (max_len != 0) is counted in class 0 and left alone
__device__ __forceinline__ uint32_t seg_work_class(uint32_t len, uint32_t vb, uint32_t max_len) {
    return (max_len != 0u && len > max_len) ? 0u : seg_class_of(len, vb);
}
__device__ __forceinline__ uint32_t seg_to_bits(uint32_t u, uint32_t kt) {
    return kt == KEY_I32 ? to_bits<KEY_I32>(u) : kt == KEY_F32 ? to_bits<KEY_F32>(u) : u;
}
__device__ __forceinline__ uint32_t seg_from_bits(uint32_t u, uint32_t kt) {
    return kt == KEY_I32 ? from_bits<KEY_I32>(u) : kt == KEY_F32 ? from_bits<KEY_F32>(u) : u;
}

// ---- reset: every call starts from a clean control block (a kernel, so that it is an ordinary node of a captured graph) ----
__global__ __launch_bounds__(64) void seg_reset_kernel(uint32_t* __restrict__ ctl) {
    static_assert(SEGC_WORDS == 64, "one word per thread");
    ctl[threadIdx.x] = 0;
}

// ---- classify: validate + count -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_classify_kernel(const uint32_t* __restrict__ off, uint32_t num_segments, uint32_t n, uint32_t vb,
                                                           uint32_t max_len, uint32_t* __restrict__ ctl) {
    __shared__ uint32_t s_cnt[SEG_CLASSES], s_max, s_status;
    const uint32_t tid = threadIdx.x, s = blockIdx.x * 256u + tid;
    if (tid < SEG_CLASSES) s_cnt[tid] = 0;
    if (tid == 0) { s_max = 0; s_status = 0; }
    __syncthreads();
    if (s < num_segments) {
        const uint32_t a = off[s], b = off[s + 1u];
        if (b < a || (s == num_segments - 1u && b > n)) {
            atomicOr(&s_status, SEG_ST_ARG);
        } else {
            const uint32_t len = b - a;
            if (max_len != 0u && len > max_len) atomicOr(&s_status, SEG_ST_SIZE);
            atomicAdd(&s_cnt[seg_work_class(len, vb, max_len)], 1u);
            atomicMax(&s_max, len);
        }
    }
    __syncthreads();
    if (tid < SEG_CLASSES && s_cnt[tid] != 0u) atomicAdd(&ctl[SEGC_COUNT + tid], s_cnt[tid]);
    if (tid == 0) {
        if (s_max != 0u) atomicMax(&ctl[SEGC_MAXLEN], s_max);
        if (s_status != 0u) atomicOr(&ctl[SEGC_STATUS], s_status);
    }
}

// ---- fill: the class lists ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_fill_kernel(const uint32_t* __restrict__ off, uint32_t num_segments, uint32_t vb, uint32_t max_len,
                                                       uint32_t* __restrict__ ctl, uint32_t* __restrict__ list) {
    __shared__ uint32_t s_cnt[SEG_CLASSES], s_base[SEG_CLASSES];
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;  // (uniform) bad offsets: no list, no sort
    const uint32_t tid = threadIdx.x, s = blockIdx.x * 256u + tid;
    if (tid < SEG_CLASSES) s_cnt[tid] = 0;
    __syncthreads();
    uint32_t cls = 0, rank = 0;
    if (s < num_segments) {
        cls = seg_work_class(off[s + 1u] - off[s], vb, max_len);
        if (cls >= 2u) rank = atomicAdd(&s_cnt[cls], 1u);
    }
    __syncthreads();
    if (tid >= 2u && tid < SEG_CLASSES && s_cnt[tid] != 0u)
        s_base[tid] = seg_list_base(ctl, tid) + atomicAdd(&ctl[SEGC_CURSOR + tid], s_cnt[tid]);
    __syncthreads();
    // the counts are those of the same classification, so base + slot < num_segments; the guard only keeps a broken invariant in bounds
    if (cls >= 2u && s_base[cls] + rank < num_segments) list[s_base[cls] + rank] = s;
}

// ---- packed class: 2 .. SEG_PACK_MAX elements, 64 consecutive segments per wave ------------------------------------------
// One wave per workgroup.  Lane l takes segment 64 w + l; the packed segments of the wave are laid out back to back in LDS (wave
// scan of their lengths), loaded in rounds of 4 x 64 elements (segments that follow one another in memory give coalesced loads:
// element e of the layout is found by a binary search over the 64 scan values), then every element counts the elements of its
// segment that go in front of it — smaller key, or equal key and earlier — and is written straight to that place.  No ranking
// passes, no digit tables: up to 32 LDS reads per element, and a wave is busy with 64 segments instead of one.
template <int VB>
__global__ __launch_bounds__(64) void seg_packed_kernel(uint32_t* __restrict__ keys, void* __restrict__ vals_, const uint32_t* __restrict__ off,
                                                        uint32_t num_segments, uint32_t max_len, uint32_t kt, uint32_t descending,
                                                        const uint32_t* __restrict__ ctl) {
    using V = typename ValT<VB>::type;
    constexpr uint32_t CAP = 64u * SEG_PACK_MAX;
    __shared__ uint32_t s_key[CAP];
    __shared__ V s_val[VB != 0 ? CAP : 1];
    __shared__ uint32_t s_start[64], s_scan[65];
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    V* vals = static_cast<V*>(vals_);
    const uint32_t lane = threadIdx.x, s = blockIdx.x * 64u + lane;
    uint32_t a = 0, len = 0;
    if (s < num_segments) {
        a = off[s];
        const uint32_t l = off[s + 1u] - a;
        if (l >= 2u && l <= SEG_PACK_MAX && (max_len == 0u || l <= max_len)) len = l;
    }
    const uint32_t incl = wave_inclusive_scan(len, lane);
    const uint32_t E = __shfl(incl, 63, 64);  // <= CAP
    if (E == 0u) return;
    s_start[lane] = a;
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
        uint32_t k[4];
        V v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // unconditional loads on a clamped element, masked afterwards
            const uint32_t e = e0 + u * 64u + lane, ec = e < E ? e : E - 1u;
            const uint32_t j = find(ec);
            const uint32_t g = s_start[j] + (ec - s_scan[j]);
            k[u] = keys[g];
            if constexpr (VB != 0) v[u] = vals[g];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = e0 + u * 64u + lane;
            if (e < E) {
                s_key[e] = seg_to_bits(k[u], kt);
                if constexpr (VB != 0) s_val[e] = v[u];
            }
        }
    }
    __syncthreads();  // every element of the wave's segments is in LDS: from here on the segments are overwritten
    for (uint32_t e = lane; e < E; e += 64u) {
        const uint32_t j = find(e);
        const uint32_t lo = s_scan[j], hi = s_scan[j + 1u];
        const uint32_t key = s_key[e];
        uint32_t rank = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t x = s_key[i];
            rank += (x < key || (x == key && i < e)) ? 1u : 0u;
        }
        const uint32_t o = s_start[j] + (descending ? hi - lo - 1u - rank : rank);
        keys[o] = seg_from_bits(key, kt);
        if constexpr (VB != 0) vals[o] = s_val[e];
    }
}

// ---- the four ranking passes of the wave class (below) and of the row-wise top-k's wave route (topk_rows_kernels.hpp) -----------
// BITS: the key bits that are ranked, from bit 0 up (16: the two passes of the 16-bit row-wise top-k, topk_rows16_kernels.hpp).
// On keys in registers: slot lane + r * 64 holds key[r] as sortable bits (and val[r]); rows: how many rows of 64 slots are in use; slots behind the end hold all-one dummies.  The tables are the calling wave's own.  Its
// barriers are workgroup barriers: every wave of a workgroup that calls it must call it, and equally often.
template <int VB, uint32_t BITS = 32u>
__device__ __forceinline__ void seg_wave_sort_passes(uint32_t (&key)[SEG_WAVE_MAX / 64], typename ValT<VB>::type (&val)[VB != 0 ? SEG_WAVE_MAX / 64 : 1],
                                                     uint32_t rows, uint32_t lane, uint32_t* s_hist, uint32_t* s_stage,
                                                     typename ValT<VB>::type* s_vstage) {
    constexpr int KPT = SEG_WAVE_MAX / 64;
#pragma unroll 1
    for (uint32_t shift = 0; shift < BITS; shift += 8u) {
        reinterpret_cast<uint4*>(s_hist)[lane] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
        uint32_t offp[KPT];
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            offp[r] = 0;
            if ((uint32_t)r < rows) {  // (uniform)
                const uint32_t w = key[r];
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
                const uint32_t pre = s_hist[d];
                if (below == total - 1u) s_hist[d] = pre + total;
                asm volatile("" ::: "memory");
                offp[r] = pre + below;
            }
        }
        __syncthreads();
        {
            const uint4 c = reinterpret_cast<const uint4*>(s_hist)[lane];
            const uint32_t sum = c.x + c.y + c.z + c.w;
            const uint32_t ex = wave_inclusive_scan(sum, lane) - sum;
            reinterpret_cast<uint4*>(s_hist)[lane] = uint4{ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z};
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            if ((uint32_t)r < rows) {
                const uint32_t pos = offp[r] + s_hist[(key[r] >> shift) & 255u];
                s_stage[pos] = key[r];
                if constexpr (VB != 0) s_vstage[pos] = val[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            if ((uint32_t)r < rows) {
                key[r] = s_stage[lane + r * 64u];
                if constexpr (VB != 0) val[r] = s_vstage[lane + r * 64u];
            }
        }
        __syncthreads();
    }
}

// ---- wave class: SEG_PACK_MAX < length <= SEG_WAVE_MAX, one segment per wave ----------------------------------------------
// One wave per workgroup (its barriers are wave barriers), up to four keys per lane in wave-striped order; four stable 8-bit passes,
// each: 64-lane ballot multi-split on a 256-counter table, exclusive scan of the table (four counters per lane), staged by digit,
// read back in array order.  Rows of 64 slots the segment does not reach are skipped; slots behind the segment's end hold all-one
// dummies that stay behind every real key.
template <int VB>
__global__ __launch_bounds__(64) void seg_wave_kernel(uint32_t* __restrict__ keys, void* __restrict__ vals_, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ list, const uint32_t* __restrict__ ctl, uint32_t num_segments,
                                                      uint32_t kt, uint32_t descending) {
    using V = typename ValT<VB>::type;
    constexpr int KPT = SEG_WAVE_MAX / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[RADIX];
    __shared__ uint32_t s_stage[SEG_WAVE_MAX];
    __shared__ V s_vstage[VB != 0 ? SEG_WAVE_MAX : 1];
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    V* vals = static_cast<V*>(vals_);
    const uint32_t lane = threadIdx.x;
    const uint32_t count = ctl[SEGC_COUNT + 2], base = seg_list_base(ctl, 2);
    for (uint32_t it = blockIdx.x; it < count && base + it < num_segments; it += gridDim.x) {
        // (the list holds segments of this class only; the checks keep a broken invariant in bounds)
        const uint32_t s = list[base + it];
        if (s >= num_segments) continue;
        const uint32_t a = off[s], len = off[s + 1u] - a;
        if (len == 0u || len > SEG_WAVE_MAX) continue;
        const uint32_t rows = (len + 63u) >> 6;
        uint32_t key[KPT];
        V val[VB != 0 ? KPT : 1];
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const uint32_t idx = lane + r * 64u, ci = idx < len ? idx : len - 1u;
            key[r] = keys[a + ci];
            if constexpr (VB != 0) val[r] = vals[a + ci];
        }
#pragma unroll
        for (int r = 0; r < KPT; ++r) key[r] = lane + r * 64u < len ? seg_to_bits(key[r], kt) : 0xffffffffu;
        seg_wave_sort_passes<VB>(key, val, rows, lane, s_hist, s_stage, s_vstage);
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const uint32_t idx = lane + r * 64u;
            if (idx < len) {
                const uint32_t o = descending ? len - 1u - idx : idx;
                keys[a + o] = seg_from_bits(key[r], kt);
                if constexpr (VB != 0) vals[a + o] = val[r];
            }
        }
    }
}

// ---- workgroup classes: one segment per workgroup, the single-tile sort on the shape of the class ----------------------------
// LOOP: a fixed grid claims the class list by grid stride; !LOOP: one workgroup per list slot the class can have at most (the
// 1024 x 32 shape sits at its register limit: the loop around it spilled 33 dwords per lane in the build that uses LDS atomics)
template <int THREADS, int KPT, int VB, int KT, int RANK, bool LOOP>
__global__ __launch_bounds__(THREADS) void seg_wg_kernel(uint32_t* keys, void* vals_, const uint32_t* __restrict__ off,
                                                         const uint32_t* __restrict__ list, const uint32_t* __restrict__ ctl, uint32_t num_segments,
                                                         uint32_t cls, uint32_t descending) {
    using V = typename ValT<VB>::type;
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const uint32_t count = ctl[SEGC_COUNT + cls], base = seg_list_base(ctl, cls);
    auto sort_one = [&](uint32_t it) {
        // (the list holds segments of this class only; the checks keep a broken invariant in bounds)
        if (base + it >= num_segments) return;
        const uint32_t s = list[base + it];
        if (s >= num_segments) return;
        const uint32_t a = off[s], len = off[s + 1u] - a;
        if (len == 0u || len > (uint32_t)(THREADS * KPT)) return;
        tile_sort_body<THREADS, KPT, VB, KT, RANK, false>(keys + a, VB != 0 ? static_cast<void*>(static_cast<V*>(vals_) + a) : nullptr, len,
                                                          descending, nullptr);
    };
    if constexpr (LOOP) {
        for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
            sort_one(it);
            __syncthreads();
        }
    } else {
        if (blockIdx.x < count) sort_one(blockIdx.x);
    }
}

// ---- long segments: the leading elements the engine's alignment left out --------------------------------------------------
// The OneSweep engine wants 16-byte aligned buffers, a segment starts anywhere: the host sorts [start + head, end) (head <= 3
// elements up to the next multiple of four) with the engine and this kernel merges the head in.  Reads the sorted tail and the
// head from keys / vals, writes the merged segment [start, end) to alt_keys / alt_vals; the host copies it back.  A head element
// came first in the segment, so it goes in front of every tail element with an equal key (ascending) — behind them in the
// descending order, which is the exact reverse of the stable ascending one.
template <int VB>
__global__ __launch_bounds__(256) void seg_merge_head_kernel(const uint32_t* __restrict__ keys, const void* __restrict__ vals_,
                                                             uint32_t* __restrict__ alt_keys, void* __restrict__ alt_vals_, uint32_t start,
                                                             uint32_t head, uint32_t len, uint32_t kt, uint32_t descending) {
    using V = typename ValT<VB>::type;
    const V* vals = static_cast<const V*>(vals_);
    V* alt_vals = static_cast<V*>(alt_vals_);
    const uint32_t tail = len - head;
    const uint32_t* t = keys + start + head;
    // position of every head element in the merged segment (each thread computes all of them: head <= 3)
    uint32_t hpos[3] = {0, 0, 0};
    for (uint32_t x = 0; x < head; ++x) {
        const uint32_t kx = seg_to_bits(keys[start + x], kt);
        uint32_t lo = 0, hi = tail;  // ascending: tail elements < kx; descending: tail elements >= kx
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1, km = seg_to_bits(t[mid], kt);
            if (descending ? km >= kx : km < kx) lo = mid + 1u;
            else hi = mid;
        }
        uint32_t among = 0;  // head elements in front of x in the result
        for (uint32_t y = 0; y < head; ++y) {
            const uint32_t ky = seg_to_bits(keys[start + y], kt);
            const bool before = ky < kx || (ky == kx && y < x);
            among += (y != x && (descending ? !before : before)) ? 1u : 0u;
        }
        hpos[x] = lo + among;
    }
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < len; i += gridDim.x * 256u) {
        if (i < head) {
            alt_keys[start + hpos[i]] = keys[start + i];
            if constexpr (VB != 0) alt_vals[start + hpos[i]] = vals[start + i];
        } else {
            const uint32_t j = i - head;  // its place among the tail; head element x lies in front of it iff hpos[x] - (heads in front of x) <= j
            uint32_t shift = 0;
            for (uint32_t x = 0; x < head; ++x) {
                uint32_t among = 0;
                for (uint32_t y = 0; y < head; ++y) among += (y != x && hpos[y] < hpos[x]) ? 1u : 0u;
                shift += (hpos[x] - among <= j) ? 1u : 0u;
            }
            alt_keys[start + j + shift] = keys[start + i];
            if constexpr (VB != 0) alt_vals[start + j + shift] = vals[start + i];
        }
    }
}

}  // namespace gs
