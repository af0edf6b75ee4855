// topk16_kernels.hpp — the 1-D top-k on 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16): gs_topk16_* of include/gpusort.h.
// No counterpart in the reference project.
//
// A 16-bit key is exactly one level of the two-level select of topk_kernels.hpp: one 65 536-bin histogram of bin = sortable bits ^
// flip (flip = 0xFFFF: descending) is the exact answer, so there is no second level and no candidate buffer.  The control block has
// that file's layout (TKC_*, level 0 only), so its tk_reduce_kernel and tk_threshold_kernel, and sort16_kernels.hpp's s16_clear_kernel
// and s16_scan_kernel, are launched as they are.  What is new here:
//   tk16_init_kernel        zeroes the recount histogram and the control block, plans the ranges (multiples of an 8-keys-per-thread chunk)
//   tk16_hist_kernel        one read, 16-byte non-temporal loads of 8 keys: the range's histogram in a packed 2 x 16-bit LDS table ->
//                           its slice; hot-bin vote, exact overflow test and 32-bit recount as tk_hist_kernel
//   tk16_rangecount_kernel  per range, from its slice: elements in front of P, elements in P (an overflowed slice: from the 2-byte keys)
//   tk16_scatter_kernel     second read, one workgroup per range, its tiles in order with running bases: elements in front of P ->
//                           the output in input order; of those in P the wanted share by position rank behind them
//   tk16_fill_kernel        keys only: outputs [0, k) from prefix[65 537], the keys are not read again
// tk16_hist_kernel, tk16_rangecount_kernel and tk16_scatter_kernel are copies of tk_hist_kernel, tk_rangecount_kernel and
// tk_scatter_kernel on 2-byte loads, and tk16_fill_kernel is a copy of s16_fill_kernel with the output length apart from the
// histogram's total: shared bodies would have changed the registers of the kernels they were taken from.
// No kernel waits on another workgroup.  Every LDS and global store index is checked against its buffer's length; a count that does
// not add up sets TK_ST_INTERNAL in the status word.
#pragma once
#include "sort16_kernels.hpp"
#include "topk_kernels.hpp"

namespace gs {

constexpr uint32_t TK16_CHUNK = 8 * TK_THREADS;           // keys per 16-byte load of the workgroup
constexpr uint32_t TK16_TILE = TK_UNROLL * TK16_CHUNK;    // chunks in flight
constexpr uint32_t TK16_MIN_RANGE = TK16_TILE;            // a range is a multiple of TK16_CHUNK and at least one tile
constexpr uint32_t TK16C_WORDS = 64;                      // the handle's control block: TKC_* in front, the rest zero
static_assert(TK16_TILE < 65536u, "a tile's front and equal counts are packed into 16 bits each");
static_assert(TKC_WORDS <= TK16C_WORDS && TKC_STATUS == S16C_STATUS && TK_ST_INTERNAL == S16_ST_INTERNAL && TK_BINS == S16_BINS,
              "one status word and one bin space for the kernels of both files");

#if GS_SORT16_BUILT  // (radix_pass.hpp: the product build only)

// zeroes the recount histogram and the control block, plans the one level
__global__ __launch_bounds__(256) void tk16_init_kernel(uint32_t* __restrict__ ctl, uint32_t* __restrict__ extra, uint32_t n, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < TK_BINS / 4u) reinterpret_cast<uint4*>(extra)[i] = uint4{0u, 0u, 0u, 0u};
    if (i == 0) {
        for (uint32_t w = 0; w < TK16C_WORDS; ++w) ctl[w] = 0u;
        uint32_t per = ((n + TK_MAX_RANGES - 1u) / TK_MAX_RANGES + TK16_CHUNK - 1u) / TK16_CHUNK * TK16_CHUNK;
        if (per < TK16_MIN_RANGE) per = TK16_MIN_RANGE;
        uint32_t* L = ctl + TKC_LEVEL;
        L[TKL_NSRC] = n;
        L[TKL_RANGES] = (uint32_t)(((unsigned long long)n + per - 1u) / per);
        L[TKL_PER] = per;
        L[TKL_WANTED] = k;
    }
}

// eight elements of thread `tid` in the chunk at c (a multiple of 8), two to a word, the lower index in the low half; mask: which of
// them lie in front of `end` (indices stay below 2^30 + TK16_TILE: no wrap)
__device__ __forceinline__ uint4 tk16_load_chunk(const uint16_t* src, uint32_t c, uint32_t end, uint32_t tid, uint32_t& mask) {
    const uint32_t i = c + tid * 8u;
    if (GS_LIKELY(c + TK16_CHUNK <= end)) {
        mask = 255u;
        return ld_stream<true>(reinterpret_cast<const uint4*>(src + i));
    }
    uint32_t e[4] = {0u, 0u, 0u, 0u};
    mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (i + j < end) {
            e[j >> 1] |= (uint32_t)src[i + j] << ((j & 1u) * 16u);
            mask |= 1u << j;
        }
    }
    return uint4{e[0], e[1], e[2], e[3]};
}

// ---------------------------------------------------------------------------
// Histogram of one range.  LDS: the packed table (128 KiB) + the vote table.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TK_THREADS) void tk16_hist_kernel(const uint16_t* __restrict__ src, const uint32_t* __restrict__ ctl, uint32_t kt,
                                                               uint32_t flip, uint32_t* __restrict__ slices, uint32_t* __restrict__ extra) {
    constexpr uint32_t T = TK_THREADS;
    __shared__ __attribute__((aligned(16))) uint32_t s_j[TK_TABLE_WORDS];
    __shared__ uint32_t s_vote[2048];
    __shared__ uint32_t s_red[4];  // 0 best vote, 1 table sum, 2 hot count
    const uint32_t* L = ctl + TKC_LEVEL;
    const uint32_t g = blockIdx.x;
    if (g >= L[TKL_RANGES] || g >= TK_MAX_RANGES) return;
    const uint32_t nsrc = L[TKL_NSRC], per = L[TKL_PER];
    const uint32_t begin = g * per, end = nsrc - begin < per ? nsrc : begin + per;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < TK_TABLE_WORDS / 4; i += T) reinterpret_cast<uint4*>(s_j)[i] = uint4{0u, 0u, 0u, 0u};
    for (uint32_t i = tid; i < 2048; i += T) s_vote[i] = 0u;
    if (tid < 4) s_red[tid] = 0u;
    __syncthreads();
    {  // the vote: 1024 samples spread over the range; the bin whose hash slot collects most is the candidate
        const uint32_t len = end - begin, step = len / T;
        if (step != 0u || tid < len) {
            const uint32_t d = tkr16_to_bits(src[begin + (step ? tid * step : tid)], kt) ^ flip;  // (< TK_BINS)
            const uint32_t old = atomicAdd(&s_vote[(d * 2654435761u) >> 21], 1u);
            atomicMax(&s_red[0], ((old + 1u) << 16) | d);
        }
    }
    __syncthreads();
    const uint32_t hot = (s_red[0] >> 16) >= TK_HOT_VOTES ? (s_red[0] & 0xffffu) : TK_NO_BIN;
    uint32_t hot_count = 0;
    auto add = [&](uint32_t d, uint32_t c) { atomicAdd(&s_j[(d & 0xffffu) >> 1], pk16_addend(d, c)); };  // pk16_add's add with the word index masked to the table
    auto process = [&](const uint4 t, const uint32_t mask) {
        const uint32_t w4[4] = {t.x, t.y, t.z, t.w};
        uint32_t d[8];
        bool one = mask == 255u;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            d[j] = tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip;
            one = one && d[j] == d[0];
        }
        // a whole wave under one bin (sorted or constant input): one add
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
        if (__builtin_amdgcn_ballot_w64(one && d[0] == f) == ~0ull) {
            if (f == hot) hot_count += 8u;
            else if (lane == 0) add(f, 512u);
            return;
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (!((mask >> j) & 1u)) continue;
            if (d[j] == hot) ++hot_count;
            else add(d[j], 1u);
        }
    };
    for (uint32_t c0 = begin; c0 < end; c0 += TK16_TILE) {
        uint4 t[TK_UNROLL];
        uint32_t mask[TK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u) {
            const uint32_t c = c0 + u * TK16_CHUNK;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (c < end) t[u] = tk16_load_chunk(src, c, end, tid, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u)
            if (c0 + u * TK16_CHUNK < end) process(t[u], mask[u]);  // uniform
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
        for (uint32_t c = begin; c < end; c += TK16_CHUNK) {
            uint32_t mask;
            const uint4 t = tk16_load_chunk(src, c, end, tid, mask);
            const uint32_t w4[4] = {t.x, t.y, t.z, t.w};
            uint32_t run_d = TK_NO_BIN, run = 0;  // this thread's eight keys: equal neighbours in one add
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                if (!((mask >> j) & 1u)) continue;
                const uint32_t d = tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip;
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
// Per range: elements in front of P and in P, from the range's slice; from the keys if the slice is marked TKS_OVF.
// rc[2 * g] = front, rc[2 * g + 1] = equal.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tk16_rangecount_kernel(const uint16_t* __restrict__ src, const uint32_t* __restrict__ slices,
                                                              const uint32_t* __restrict__ ctl, uint32_t kt, uint32_t flip, uint32_t* __restrict__ rc) {
    __shared__ uint32_t s_lt, s_eq;
    const uint32_t* L = ctl + TKC_LEVEL;
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    if (g >= L[TKL_RANGES] || g >= TK_MAX_RANGES) return;
    const uint32_t P = L[TKL_BIN] & 0xffffu;
    const uint32_t* mine = slices + (size_t)g * TK_SLICE_WORDS;
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
            const uint32_t d = tkr16_to_bits(src[i], kt) ^ flip;
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
// Ordered scatter of one range.  VM: 0 keys only (unused by the handle: keys only takes the fill), 1 the value is the element's
// index, 4 / 8 value bytes.  In front of P -> out[.] from 0, in input order; in P -> by position rank r among the array's elements in
// P: ascending the first TAKE, descending the last TAKE, behind the others.  Every destination index is checked against k before the store.
// ---------------------------------------------------------------------------
template <int VM>
__global__ __launch_bounds__(TK_THREADS) void tk16_scatter_kernel(const uint16_t* __restrict__ src, const void* __restrict__ src_vals_, uint32_t* ctl,
                                                                  uint32_t kt, uint32_t flip, const uint32_t* __restrict__ rc,
                                                                  uint16_t* __restrict__ out, void* __restrict__ out_vals_, uint32_t k) {
    using V = typename TkVal<VM>::type;
    constexpr uint32_t T = TK_THREADS, W = T / 64, SLOTS = TK_UNROLL * W;
    static_assert(SLOTS == 64, "the tile's wave totals are scanned by one wave");
    __shared__ uint32_t s_w[2][SLOTS + 1];  // packed: front | equal << 16 (a tile holds 32 768 elements)
    __shared__ uint32_t s_base[2];
    const uint32_t* L = ctl + TKC_LEVEL;
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (g >= L[TKL_RANGES] || g >= TK_MAX_RANGES) return;
    const uint32_t nsrc = L[TKL_NSRC], per = L[TKL_PER], P = L[TKL_BIN], take = L[TKL_TAKE], equal = L[TKL_EQUAL];
    const uint32_t begin = g * per, end = nsrc - begin < per ? nsrc : begin + per;
    const V* src_vals = static_cast<const V*>(src_vals_);
    V* out_vals = static_cast<V*>(out_vals_);
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
    uint32_t base_lt = s_base[0], base_eq = s_base[1];
    // where P's elements go by rank r: [lo, lo + take) -> out[eq0 + r - lo]
    const uint32_t eq_lo = (flip && equal >= take) ? equal - take : 0u;
    const uint32_t eq0 = L[TKL_FRONT];
    bool bad = false;
    auto emit = [&](uint32_t key, uint32_t idx, bool is_lt, uint32_t r_lt, uint32_t r_eq) {
        uint32_t dst;
        if (is_lt) dst = r_lt;
        else {
            if (r_eq < eq_lo || r_eq - eq_lo >= take) return;
            dst = eq0 + (r_eq - eq_lo);
        }
        if (dst >= k) { bad = true; return; }
        out[dst] = (uint16_t)key;
        if constexpr (VM == 1) out_vals[dst] = idx;
        else if constexpr (VM != 0) out_vals[dst] = src_vals[idx];
    };
    uint32_t par = 0;
    for (uint32_t c0 = begin; c0 < end; c0 += TK16_TILE, par ^= 1u) {
        uint4 t[TK_UNROLL];
        uint32_t mask[TK_UNROLL], fl[TK_UNROLL], incl[TK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u) {
            const uint32_t c = c0 + u * TK16_CHUNK;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (c < end) t[u] = tk16_load_chunk(src, c, end, tid, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TK_UNROLL; ++u) {
            const uint32_t w4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            uint32_t f = 0, cnt = 0;  // f: bit j = in front, bit 8 + j = equal
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t d = tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip;
                const bool v = (mask[u] >> j) & 1u;
                if (v && d < P) { f |= 1u << j; cnt += 1u; }
                if (v && d == P) { f |= 256u << j; cnt += 1u << 16; }
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
                const uint32_t w4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
                const uint32_t i0 = c0 + u * TK16_CHUNK + tid * 8u;
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) {
                    if (fl[u] & (1u << j)) { emit(tkr16_elem(w4, j), i0 + j, true, r_lt, 0u); ++r_lt; }
                    else if (fl[u] & (256u << j)) { emit(tkr16_elem(w4, j), i0 + j, false, 0u, r_eq); ++r_eq; }
                }
            }
            base_lt += tot & 0xffffu;
            base_eq += tot >> 16;
        }
    }
    if (bad) atomicOr(&ctl[TKC_STATUS], TK_ST_INTERNAL);
}

// ---------------------------------------------------------------------------
// Keys only: s16_fill_kernel with the output length k apart from the histogram's total n.  Workgroup b owns the outputs
// [b * S16_KTILE, ...) below k: first and last bin by binary search in the prefix, every non-empty bin's number dropped at the bin's
// first output inside the slice, a max-scan, the keys the numbers stand for.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(S16_KTHREADS) void tk16_fill_kernel(uint16_t* __restrict__ out, const uint32_t* __restrict__ prefix, uint32_t n, uint32_t k,
                                                                 uint32_t kt, uint32_t flip, uint32_t* __restrict__ ctl) {
    constexpr uint32_t W = S16_KTHREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_bin[S16_KTILE];
    __shared__ uint32_t s_w[W], s_fl[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t start = blockIdx.x * S16_KTILE;
    if (start >= k || k > n || prefix[S16_BINS] != n) return;  // (uniform; a histogram that does not add up was reported by the scan: nothing is written)
    const uint32_t m = k - start < S16_KTILE ? k - start : S16_KTILE;
    reinterpret_cast<uint4*>(s_bin)[tid] = uint4{0u, 0u, 0u, 0u};
    reinterpret_cast<uint4*>(s_bin)[tid + S16_KTHREADS] = uint4{0u, 0u, 0u, 0u};
    if (tid < 2) {  // the bin that holds output `target`: the last one whose prefix is <= target
        const uint32_t target = tid == 0 ? start : start + m - 1u;
        uint32_t lo = 0, hi = S16_BINS + 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (prefix[mid] <= target) lo = mid + 1u; else hi = mid;
        }
        s_fl[tid] = lo - 1u;  // (prefix[0] = 0 <= target < k <= n = prefix[65 536]: 0 <= lo - 1 <= 65 535)
    }
    __syncthreads();
    const uint32_t first = s_fl[0], last = s_fl[1];
    if (first > last || last >= S16_BINS) {  // (uniform)
        if (tid == 0) atomicOr(&ctl[TKC_STATUS], TK_ST_INTERNAL);
        return;
    }
    if (tid == 0) s_bin[0] = first;
    for (uint32_t b = first + 1u + tid; b <= last; b += S16_KTHREADS) {
        const uint32_t p = prefix[b];
        if (prefix[b + 1u] > p) {  // non-empty: it starts inside the slice, behind its first output
            const uint32_t off = p - start;
            if (off < m) s_bin[off] = b; else atomicOr(&ctl[TKC_STATUS], TK_ST_INTERNAL);
        }
    }
    __syncthreads();
    const uint4 a0 = reinterpret_cast<const uint4*>(s_bin)[2u * tid], a1 = reinterpret_cast<const uint4*>(s_bin)[2u * tid + 1u];
    uint32_t v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (uint32_t j = 1; j < 8; ++j) v[j] = v[j] > v[j - 1] ? v[j] : v[j - 1];
    const uint32_t incl = wave_inclusive_max(v[7], lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 0u;
    for (uint32_t x = 0; x < W; ++x)
        if (x < wave && s_w[x] > before) before = s_w[x];
    uint32_t w4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t bin = v[j] > before ? v[j] : before;
        w4[j >> 1] |= (tkr16_from_bits((bin ^ flip) & 0xffffu, kt) & 0xffffu) << ((j & 1u) * 16u);
    }
    const uint32_t i = tid * 8u;
    if (i + 8u <= m) {
        *reinterpret_cast<uint4*>(out + start + i) = uint4{w4[0], w4[1], w4[2], w4[3]};
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
            if (i + j < m) out[start + i + j] = (uint16_t)(w4[j >> 1] >> ((j & 1u) * 16u));
    }
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
