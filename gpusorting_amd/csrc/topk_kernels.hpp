// topk_kernels.hpp — radix select for gs_topk_* (include/gpusort.h): the first k of the sorted order without the sort.
// No counterpart in the reference project.
//
// Selection runs in "selection space": sel = to_bits(key) ^ (descending ? ~0 : 0), so that both orders look for the k SMALLEST
// sel; the tie rule alone differs (ascending takes the lowest positions among the elements equal to the threshold, descending
// the highest).  Two levels of 16 bits, each the same five kernels over a source array cut into at most TK_MAX_RANGES
// contiguous ranges, one workgroup per range:
//   tk_hist_kernel      one read: the range's 65 536-bin histogram of the level's 16 bits in a packed 2 x 16-bit LDS table -> its slice
//   tk_reduce_kernel    sum of the slices -> sums[65 536]
//   tk_threshold_kernel one workgroup: the bin P with  in_front < wanted <= in_front + sums[P]
//   tk_rangecount_kernel per range, FROM ITS SLICE (no read of the keys): elements in front of P, elements in P
//   tk_scatter_kernel   second read: every range walks its tiles in order with a running base (no workgroup waits for another):
//                       elements in front of P -> the output, in input order; elements in P -> the candidate buffer (level 1) or,
//                       by position rank, the output (level 2), in input order
// Level 1 reads the caller's keys (top 16 bits), level 2 the candidates (low 16 bits); its element count is a device word, so its
// launches are enqueued up front and workgroups beyond the ranges in use exit at once.  The k elements in the output are then
// sorted by the handle's embedded engine (host side).
//
// Exactness of the packed table: a wrapping 16-bit counter only ever LOSES from the table's sum (see hy_histogram_kernel), so
// "decoded sum + hot count == keys of the range" proves that none wrapped.  Long runs are kept out of the table: one "hot" bin per
// range, voted from 1024 samples, is counted in registers.  A range that still wraps recounts itself in two half passes on 32-bit
// LDS counters into the level's `extra` histogram (global atomics, one per non-empty bin) and hands on an empty slice marked
// TKS_OVF; tk_rangecount_kernel then counts that range from the keys.  Nothing waits on another workgroup anywhere.
#pragma once
#include "onesweep_kernels.hpp"

namespace gs {

constexpr uint32_t TK_BINS = 65536;
constexpr uint32_t TK_TABLE_WORDS = TK_BINS / 2;           // two 16-bit counters per word
constexpr uint32_t TK_SLICE_WORDS = TK_TABLE_WORDS + 4;    // + TKS_*
constexpr uint32_t TKS_HOT_BIN = 0, TKS_HOT_COUNT = 1, TKS_OVF = 2;  // behind the table
constexpr int TK_THREADS = 1024;
constexpr uint32_t TK_CHUNK = 4 * TK_THREADS;              // keys per 16-byte load of the workgroup
constexpr uint32_t TK_UNROLL = 4;                          // chunks in flight
constexpr uint32_t TK_TILE = TK_UNROLL * TK_CHUNK;
constexpr uint32_t TK_MAX_RANGES = 256;                    // one histogram workgroup (128 KiB of LDS) per CU
constexpr uint32_t TK_MIN_RANGE = TK_TILE;                 // a range is a multiple of TK_CHUNK and at least one tile
constexpr uint32_t TK_HOT_VOTES = 32;                      // of 1024 samples: from 1/32 of a range a bin is counted in registers
constexpr uint32_t TK_NO_BIN = 0xffffffffu;

// control block (device words)
constexpr uint32_t TKC_STATUS = 0;   // TK_ST_* bits
constexpr uint32_t TKC_LEVEL = 8;    // two blocks of TKL_WORDS
constexpr uint32_t TKL_NSRC = 0;     // elements of the level's source
constexpr uint32_t TKL_RANGES = 1;   // ranges in use (<= TK_MAX_RANGES)
constexpr uint32_t TKL_PER = 2;      // elements per range
constexpr uint32_t TKL_WANTED = 3;   // how many of the source's elements are wanted
constexpr uint32_t TKL_BIN = 4;      // P
constexpr uint32_t TKL_FRONT = 5;    // elements in front of P
constexpr uint32_t TKL_EQUAL = 6;    // elements in P
constexpr uint32_t TKL_TAKE = 7;     // wanted - front: how many of P's elements are wanted
constexpr uint32_t TKL_WORDS = 8;
constexpr uint32_t TKC_WORDS = TKC_LEVEL + 2 * TKL_WORDS;
constexpr uint32_t TK_ST_INTERNAL = 1u;  // a count did not add up (cannot happen); nothing is written out of bounds

__device__ __forceinline__ uint32_t tk_sel(uint32_t key, uint32_t kt, uint32_t flip) {
    const uint32_t m = kt == 0u ? 0u : (kt == 1u || !(key >> 31)) ? 0x80000000u : 0xffffffffu;
    return key ^ m ^ flip;
}
__device__ __forceinline__ uint32_t tk_digit(uint32_t sel, uint32_t level) { return level == 0u ? sel >> 16 : sel & 0xffffu; }

// ranges of a source of nsrc elements
__device__ __forceinline__ void tk_plan_level(uint32_t* L, uint32_t nsrc, uint32_t wanted) {
    uint32_t per = ((nsrc + TK_MAX_RANGES - 1u) / TK_MAX_RANGES + TK_CHUNK - 1u) / TK_CHUNK * TK_CHUNK;
    if (per < TK_MIN_RANGE) per = TK_MIN_RANGE;
    L[TKL_NSRC] = nsrc;
    L[TKL_RANGES] = (uint32_t)(((unsigned long long)nsrc + per - 1u) / per);
    L[TKL_PER] = per;
    L[TKL_WANTED] = wanted;
}

// zeroes both levels' extra histograms and the control block, plans level 1
__global__ __launch_bounds__(256) void tk_init_kernel(uint32_t* ctl, uint32_t* extra, uint32_t n, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 2u * TK_BINS / 4u) reinterpret_cast<uint4*>(extra)[i] = uint4{0u, 0u, 0u, 0u};
    if (i == 0) {
        for (uint32_t w = 0; w < TKC_WORDS; ++w) ctl[w] = 0u;
        tk_plan_level(ctl + TKC_LEVEL, n, k);
    }
}

// four elements of thread `tid` in the chunk at c (indices stay below 2^30 + TK_TILE: no wrap); `valid`: how many lie in front of `end`
__device__ __forceinline__ uint4 tk_load_chunk(const uint32_t* src, uint32_t c, uint32_t end, uint32_t tid, uint32_t& valid) {
    const uint32_t i = c + tid * 4u;
    if (GS_LIKELY(c + TK_CHUNK <= end)) {
        valid = 4u;
        return ld_stream<true>(reinterpret_cast<const uint4*>(src + i));
    }
    valid = i >= end ? 0u : (end - i < 4u ? end - i : 4u);
    uint4 t{0u, 0u, 0u, 0u};
    if (valid > 0u) t.x = src[i];
    if (valid > 1u) t.y = src[i + 1u];
    if (valid > 2u) t.z = src[i + 2u];
    if (valid > 3u) t.w = src[i + 3u];
    return t;
}

// ---------------------------------------------------------------------------
// Histogram of one range.  LDS: the packed table (128 KiB) + the vote table.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TK_THREADS) void tk_hist_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ ctl, uint32_t level,
                                                             uint32_t kt, uint32_t flip, uint32_t* __restrict__ slices,
                                                             uint32_t* __restrict__ extra_all) {
    constexpr uint32_t T = TK_THREADS;
    __shared__ __attribute__((aligned(16))) uint32_t s_j[TK_TABLE_WORDS];
    __shared__ uint32_t s_vote[2048];
    __shared__ uint32_t s_red[4];  // 0 best vote, 1 table sum, 2 hot count
    const uint32_t* L = ctl + TKC_LEVEL + level * TKL_WORDS;
    const uint32_t g = blockIdx.x;
    if (g >= L[TKL_RANGES]) return;
    const uint32_t nsrc = L[TKL_NSRC], per = L[TKL_PER];
    const uint32_t begin = g * per, end = nsrc - begin < per ? nsrc : begin + per;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t* extra = extra_all + level * TK_BINS;
    for (uint32_t i = tid; i < TK_TABLE_WORDS / 4; i += T) reinterpret_cast<uint4*>(s_j)[i] = uint4{0u, 0u, 0u, 0u};
    for (uint32_t i = tid; i < 2048; i += T) s_vote[i] = 0u;
    if (tid < 4) s_red[tid] = 0u;
    __syncthreads();
    {  // the vote: 1024 samples spread over the range; the bin whose hash slot collects most is the candidate
        const uint32_t len = end - begin, step = len / T;
        if (step != 0u || tid < len) {
            const uint32_t d = tk_digit(tk_sel(src[begin + (step ? tid * step : tid)], kt, flip), level);
            const uint32_t old = atomicAdd(&s_vote[(d * 2654435761u) >> 21], 1u);
            atomicMax(&s_red[0], ((old + 1u) << 16) | d);
        }
    }
    __syncthreads();
    const uint32_t hot = (s_red[0] >> 16) >= TK_HOT_VOTES ? (s_red[0] & 0xffffu) : TK_NO_BIN;
    uint32_t hot_count = 0;
    auto add = [&](uint32_t d, uint32_t c) { pk16_add(s_j, d, c); };
    auto process = [&](const uint4 t, const uint32_t valid) {
        const uint32_t d[4] = {tk_digit(tk_sel(t.x, kt, flip), level), tk_digit(tk_sel(t.y, kt, flip), level),
                               tk_digit(tk_sel(t.z, kt, flip), level), tk_digit(tk_sel(t.w, kt, flip), level)};
        // a whole wave under one bin (sorted or constant input): one add
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
        if (__builtin_amdgcn_ballot_w64(valid == 4u && d[0] == f && d[1] == f && d[2] == f && d[3] == f) == ~0ull) {
            if (f == hot) hot_count += 4u;
            else if (lane == 0) add(f, 256u);
            return;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (j >= valid) break;
            if (d[j] == hot) ++hot_count;
            else add(d[j], 1u);
        }
    };
    for (uint32_t c0 = begin; c0 < end; c0 += TK_TILE) {
        uint4 t[TK_UNROLL];
        uint32_t valid[TK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u) {
            const uint32_t c = c0 + u * TK_CHUNK;
            valid[u] = 0u;
            if (c < end) t[u] = tk_load_chunk(src, c, end, tid, valid[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u)
            if (c0 + u * TK_CHUNK < end) process(t[u], valid[u]);  // uniform
    }
    __syncthreads();
    // the exact overflow test (see pk16_sum)
    uint32_t sum = 0;
    for (uint32_t i = tid; i < TK_TABLE_WORDS / 4; i += T) {
        const uint4 v = reinterpret_cast<const uint4*>(s_j)[i];
        sum += pk16_sum(v);
    }
    sum = wave_reduce_sum(sum);
    const uint32_t hsum = wave_reduce_sum(hot_count);
    if (lane == 0) {
        atomicAdd(&s_red[1], sum);
        atomicAdd(&s_red[2], hsum);
    }
    __syncthreads();
    const bool ok = s_red[1] + s_red[2] == end - begin;
    uint32_t* mine = slices + (size_t)g * TK_SLICE_WORDS;
    for (uint32_t i = tid; i < TK_TABLE_WORDS / 4; i += T)
        reinterpret_cast<uint4*>(mine)[i] = ok ? reinterpret_cast<const uint4*>(s_j)[i] : uint4{0u, 0u, 0u, 0u};
    if (tid == 0) {
        mine[TK_TABLE_WORDS + TKS_HOT_BIN] = ok ? hot : TK_NO_BIN;
        mine[TK_TABLE_WORDS + TKS_HOT_COUNT] = ok ? s_red[2] : 0u;
        mine[TK_TABLE_WORDS + TKS_OVF] = ok ? 0u : 1u;
    }
    if (GS_LIKELY(ok)) return;
    // a counter wrapped: recount on 32-bit counters, the lower half of the bins, then the upper
    for (uint32_t half = 0; half < 2; ++half) {
        __syncthreads();
        for (uint32_t i = tid; i < TK_TABLE_WORDS; i += T) s_j[i] = 0u;
        __syncthreads();
        for (uint32_t c = begin; c < end; c += TK_CHUNK) {
            uint32_t valid;
            const uint4 t = tk_load_chunk(src, c, end, tid, valid);
            const uint32_t k4[4] = {t.x, t.y, t.z, t.w};
            uint32_t run_d = TK_NO_BIN, run = 0;  // this thread's four keys: equal neighbours in one add
            for (uint32_t j = 0; j < valid; ++j) {
                const uint32_t d = tk_digit(tk_sel(k4[j], kt, flip), level);
                if (d == run_d) { ++run; continue; }
                if (run && (run_d >> 15) == half) atomicAdd(&s_j[run_d & 32767u], run);
                run_d = d;
                run = 1;
            }
            if (run && (run_d >> 15) == half) atomicAdd(&s_j[run_d & 32767u], run);
        }
        __syncthreads();
        for (uint32_t i = tid; i < TK_TABLE_WORDS; i += T)
            if (s_j[i]) atomicAdd(&extra[half * TK_TABLE_WORDS + i], s_j[i]);
    }
}

// ---------------------------------------------------------------------------
// sums[b] = the slices' counters of bin b + the hot counts + the recounts.  One thread per packed word.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tk_reduce_kernel(const uint32_t* __restrict__ slices, const uint32_t* __restrict__ ctl, uint32_t level,
                                                        const uint32_t* __restrict__ extra_all, uint32_t* __restrict__ sums) {
    const uint32_t G = ctl[TKC_LEVEL + level * TKL_WORDS + TKL_RANGES];
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    const uint32_t* extra = extra_all + level * TK_BINS;
    uint32_t lo = extra[2u * w], hi = extra[2u * w + 1u];
    constexpr uint32_t U = 8;
    for (uint32_t g0 = 0; g0 < G; g0 += U) {
        uint32_t v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = g0 + u < G ? slices[(size_t)(g0 + u) * TK_SLICE_WORDS + w] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) { lo += v[u] & 0xffffu; hi += v[u] >> 16; }
    }
    for (uint32_t g = 0; g < G; ++g) {  // (uniform addresses)
        const uint32_t hb = slices[(size_t)g * TK_SLICE_WORDS + TK_TABLE_WORDS + TKS_HOT_BIN];
        if ((hb >> 1) == w) {
            const uint32_t c = slices[(size_t)g * TK_SLICE_WORDS + TK_TABLE_WORDS + TKS_HOT_COUNT];
            if (hb & 1u) hi += c; else lo += c;
        }
    }
    sums[2u * w] = lo;
    sums[2u * w + 1u] = hi;
}

// ---------------------------------------------------------------------------
// One workgroup, 64 bins per thread: the bin P with front < wanted <= front + sums[P].  Level 1 plans level 2 (its source: P's elements).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void tk_threshold_kernel(const uint32_t* __restrict__ sums, uint32_t* ctl, uint32_t level) {
    __shared__ uint32_t s_w[16];
    uint32_t* L = ctl + TKC_LEVEL + level * TKL_WORDS;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wanted = L[TKL_WANTED];
    uint32_t c[64], mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint4 v = reinterpret_cast<const uint4*>(sums)[tid * 16u + i];
        c[4 * i] = v.x; c[4 * i + 1] = v.y; c[4 * i + 2] = v.z; c[4 * i + 3] = v.w;
        mine += v.x + v.y + v.z + v.w;
    }
    const uint32_t incl = wave_inclusive_scan(mine, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t front = incl - mine, total = 0;
    for (uint32_t x = 0; x < 16; ++x) {
        if (x < wave) front += s_w[x];
        total += s_w[x];
    }
    if (tid == 0 && (total != L[TKL_NSRC] || wanted == 0u || wanted > total)) atomicOr(&ctl[TKC_STATUS], TK_ST_INTERNAL);
    if (front < wanted && wanted <= front + mine) {  // exactly one thread
        uint32_t b = 0;
#pragma unroll
        for (uint32_t i = 0; i < 64; ++i) {
            if (front + c[i] < wanted && b == i) { front += c[i]; b = i + 1u; }
        }
        b = b < 64u ? b : 63u;
        uint32_t eq = 0;
#pragma unroll
        for (uint32_t i = 0; i < 64; ++i) eq = i == b ? c[i] : eq;
        L[TKL_BIN] = tid * 64u + b;
        L[TKL_FRONT] = front;
        L[TKL_EQUAL] = eq;
        L[TKL_TAKE] = wanted - front;
        if (level == 0u) tk_plan_level(L + TKL_WORDS, eq, wanted - front);
    }
}

// ---------------------------------------------------------------------------
// Per range: elements in front of P and in P, from the range's slice; from the keys if the slice is marked TKS_OVF.
// rc[2 * g] = front, rc[2 * g + 1] = equal.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tk_rangecount_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ slices,
                                                            const uint32_t* __restrict__ ctl, uint32_t level, uint32_t kt, uint32_t flip,
                                                            uint32_t* __restrict__ rc_all) {
    __shared__ uint32_t s_lt, s_eq;
    const uint32_t* L = ctl + TKC_LEVEL + level * TKL_WORDS;
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    if (g >= L[TKL_RANGES]) return;
    const uint32_t P = L[TKL_BIN];
    const uint32_t* mine = slices + (size_t)g * TK_SLICE_WORDS;
    uint32_t* rc = rc_all + level * 2u * TK_MAX_RANGES;
    if (tid == 0) { s_lt = 0u; s_eq = 0u; }
    __syncthreads();
    uint32_t lt = 0, eq = 0;
    if (mine[TK_TABLE_WORDS + TKS_OVF] == 0u) {
        for (uint32_t w = tid; w < (P >> 1); w += 256u) {  // whole words in front of P's word
            const uint32_t v = mine[w];
            lt += (v & 0xffffu) + (v >> 16);
        }
        if (tid == 0) {
            const uint32_t v = mine[P >> 1];
            if (P & 1u) { lt += v & 0xffffu; eq = v >> 16; } else eq = v & 0xffffu;
            const uint32_t hb = mine[TK_TABLE_WORDS + TKS_HOT_BIN], hc = mine[TK_TABLE_WORDS + TKS_HOT_COUNT];
            if (hb < P) lt += hc;
            if (hb == P) eq += hc;
        }
    } else {
        const uint32_t nsrc = L[TKL_NSRC], per = L[TKL_PER];
        const uint32_t begin = g * per, end = nsrc - begin < per ? nsrc : begin + per;
        for (uint32_t i = begin + tid; i < end; i += 256u) {
            const uint32_t d = tk_digit(tk_sel(src[i], kt, flip), level);
            lt += d < P;
            eq += d == P;
        }
    }
    lt = wave_reduce_sum(lt);
    eq = wave_reduce_sum(eq);
    if (lane == 0) { atomicAdd(&s_lt, lt); atomicAdd(&s_eq, eq); }
    __syncthreads();
    if (tid == 0) { rc[2u * g] = s_lt; rc[2u * g + 1u] = s_eq; }
}

// ---------------------------------------------------------------------------
// Ordered scatter of one range.  VM: 0 keys only, 4 / 8 value bytes, 1 the value is the element's index (level 1 of the position mode).
//   level 0: in front of P -> out[.] from 0; in P -> cand[.]
//   level 1: in front of P -> out[.] from level 0's front; in P -> by position rank r among the source's elements in P: ascending the
//            first TAKE, descending the last TAKE, behind the others
// Every destination index is checked against its buffer's length (k, cand_cap) before the store.
// ---------------------------------------------------------------------------
template <int VM>
struct TkVal { using type = uint32_t; };
template <>
struct TkVal<8> { using type = unsigned long long; };

template <int VM>
__global__ __launch_bounds__(TK_THREADS) void tk_scatter_kernel(const uint32_t* __restrict__ src, const void* __restrict__ src_vals_,
                                                                uint32_t* ctl, uint32_t level, uint32_t kt, uint32_t flip,
                                                                const uint32_t* __restrict__ rc_all, uint32_t* __restrict__ out,
                                                                void* __restrict__ out_vals_, uint32_t k, uint32_t* __restrict__ cand,
                                                                void* __restrict__ cand_vals_, uint32_t cand_cap) {
    using V = typename TkVal<VM>::type;
    constexpr uint32_t T = TK_THREADS, W = T / 64, SLOTS = TK_UNROLL * W;
    static_assert(SLOTS == 64, "the tile's wave totals are scanned by one wave");
    __shared__ uint32_t s_w[2][SLOTS + 1];  // packed: front | equal << 16 (a tile holds 16 384 elements)
    __shared__ uint32_t s_base[2];
    const uint32_t* L = ctl + TKC_LEVEL + level * TKL_WORDS;
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (g >= L[TKL_RANGES]) return;
    const uint32_t nsrc = L[TKL_NSRC], per = L[TKL_PER], P = L[TKL_BIN], take = L[TKL_TAKE], equal = L[TKL_EQUAL];
    const uint32_t begin = g * per, end = nsrc - begin < per ? nsrc : begin + per;
    const V* src_vals = static_cast<const V*>(src_vals_);
    V* out_vals = static_cast<V*>(out_vals_);
    V* cand_vals = static_cast<V*>(cand_vals_);
    const uint32_t* rc = rc_all + level * 2u * TK_MAX_RANGES;
    if (tid < 2) s_base[tid] = 0u;
    __syncthreads();
    {  // the ranges in front of this one
        uint32_t a = 0, b = 0;
        for (uint32_t j = tid; j < g; j += T) { a += rc[2u * j]; b += rc[2u * j + 1u]; }
        a = wave_reduce_sum(a);
        b = wave_reduce_sum(b);
        if (lane == 0 && (a | b)) { atomicAdd(&s_base[0], a); atomicAdd(&s_base[1], b); }
    }
    __syncthreads();
    const uint32_t out0 = level == 0u ? 0u : ctl[TKC_LEVEL + TKL_FRONT];
    uint32_t base_lt = out0 + s_base[0], base_eq = s_base[1];
    // level 1: where P's elements go by rank r: [lo, lo + take) -> out[eq0 + r - lo]
    const uint32_t eq_lo = (level == 1u && flip) ? equal - take : 0u;
    const uint32_t eq0 = out0 + L[TKL_FRONT];
    bool bad = false;
    auto emit = [&](uint32_t key, uint32_t idx, bool is_lt, uint32_t r_lt, uint32_t r_eq) {
        uint32_t* dk;
        V* dv;
        uint32_t dst;
        if (is_lt) { dk = out; dv = out_vals; dst = r_lt; if (dst >= k) { bad = true; return; } }
        else if (level == 0u) { dk = cand; dv = cand_vals; dst = r_eq; if (dst >= cand_cap) { bad = true; return; } }
        else {
            if (r_eq < eq_lo || r_eq - eq_lo >= take) return;
            dk = out; dv = out_vals; dst = eq0 + (r_eq - eq_lo);
            if (dst >= k) { bad = true; return; }
        }
        dk[dst] = key;
        if constexpr (VM == 1) dv[dst] = idx;
        else if constexpr (VM != 0) dv[dst] = src_vals[idx];
    };
    uint32_t par = 0;
    for (uint32_t c0 = begin; c0 < end; c0 += TK_TILE, par ^= 1u) {
        uint4 t[TK_UNROLL];
        uint32_t valid[TK_UNROLL], fl[TK_UNROLL], incl[TK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u) {
            const uint32_t c = c0 + u * TK_CHUNK;
            valid[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (c < end) t[u] = tk_load_chunk(src, c, end, tid, valid[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u) {
            const uint32_t k4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            uint32_t f = 0, cnt = 0;  // f: bit j = in front, bit 4 + j = equal
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t d = tk_digit(tk_sel(k4[j], kt, flip), level);
                const bool v = j < valid[u];
                if (v && d < P) { f |= 1u << j; cnt += 1u; }
                if (v && d == P) { f |= 16u << j; cnt += 1u << 16; }
            }
            fl[u] = f;
            incl[u] = wave_inclusive_scan(cnt, lane);
            if (lane == 63) s_w[par][u * W + wave] = incl[u];
            incl[u] -= cnt;  // exclusive
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
            for (uint32_t u = 0; u < TK_UNROLL; ++u) {
                if (fl[u] == 0u) continue;
                const uint32_t off = s_w[par][u * W + wave] + incl[u];
                uint32_t r_lt = base_lt + (off & 0xffffu), r_eq = base_eq + (off >> 16);
                const uint32_t k4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
                const uint32_t i0 = c0 + u * TK_CHUNK + tid * 4u;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if (fl[u] & (1u << j)) { emit(k4[j], i0 + j, true, r_lt, 0u); ++r_lt; }
                    else if (fl[u] & (16u << j)) { emit(k4[j], i0 + j, false, 0u, r_eq); ++r_eq; }
                }
            }
            base_lt += tot & 0xffffu;
            base_eq += tot >> 16;
        }
    }
    if (bad) atomicOr(&ctl[TKC_STATUS], TK_ST_INTERNAL);
}

// the single-tile route's values in the position mode: 0, 1, 2, ...
__global__ __launch_bounds__(256) void tk_iota_kernel(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) v[i] = i;
}

}  // namespace gs
