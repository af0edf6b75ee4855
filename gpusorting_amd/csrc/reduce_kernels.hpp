// reduce_kernels.hpp — reduce by key: one sum, minimum or maximum per distinct 32-bit key: gs_reduce_* of include/gpusort.h.  No
// counterpart in the reference project.
//
// The stage works on (key, value) pairs whose equal keys already lie side by side (the engine's stably sorted output, or the caller's
// input as it lies for gs_reduce_by_key_consecutive).  Heads, ranks and the range plan are unique_kernels.hpp's; a run carries one more
// thing across a wave, tile or range edge: the reduction of its values so far, next to the position of its head.  Three launches:
//   rd_count_kernel   one workgroup per range: heads of the range, the position of its last head, and its OPEN PARTIAL: the reduction
//                     of the values from its last head to its end, or of the whole range if it holds no head;
//   rd_scan_kernel    one workgroup, thread r for range r: heads and last head in front of every range, u, and the CARRY into every
//                     range: the open partials of the ranges in front of it, back to the nearest one that holds a head (a segmented
//                     scan over at most UQ_CAP entries, by waves and LDS);
//   rd_reduce_kernel  one workgroup per range, its tiles in order, with the running rank, last-head position and partial: a segmented
//                     scan per tile with the heads as flags.  The head of rank r writes out_keys[r] and CLOSES run r - 1: its count
//                     and its total, each exactly once; the thread that holds element n - 1 closes the last run.
//
// The order of combination.  A thread folds its eight values left to right; the threads of a wave are combined by a Hillis-Steele
// scan (distances 1, 2, .. 32), the waves of a tile left to right, the tiles of a range left to right, the ranges by the same wave
// scan and fold.  Every one of these is fixed by n and the run's place in the array, so a float sum is reproducible bit for bit; it is
// not the left-to-right sequential sum.  NO IDENTITY ELEMENT IS EVER COMBINED IN: an element that is no head has a predecessor in its
// run, so the value carried into it exists, and what lies at or behind n is never folded into anything that is read.  A run of length
// 1 therefore goes through no operation at all and comes out bit for bit.
//
// MIN / MAX run as unsigned min / max on order-preserving bits (rd_to_bits: signed integers with the sign bit flipped, floats by the
// sortable flip of the float keys) and are turned back before the store: one of the inputs, bit for bit.
//
// No kernel waits on another workgroup: no look-back, no chain, no ticket; no atomics on values.  Every global store index is checked
// against n; a count that does not add up sets UQ_ST_INTERNAL and the reduce then writes nothing.  Registers, LDS and scratch per
// kernel: DESIGN.md 3.23.
#pragma once
#include "unique_kernels.hpp"  // UQ_* constants, uq_load8, uq_left, uq_heads, uq_last_head; the wave scans behind it

namespace gs {

// how the value bits are ordered for MIN / MAX (SUM: RD_X_NONE)
constexpr uint32_t RD_X_NONE = 0, RD_X_SIGNED = 1, RD_X_FLOAT = 2;

#if GS_SORT16_BUILT  // the product build only, as the unique kernels

struct RdSumU32 { typedef uint32_t V; static __device__ __forceinline__ V op(V a, V b) { return a + b; } };
struct RdSumU64 { typedef uint64_t V; static __device__ __forceinline__ V op(V a, V b) { return a + b; } };
struct RdSumF32 { typedef float V; static __device__ __forceinline__ V op(V a, V b) { return a + b; } };
struct RdSumF64 { typedef double V; static __device__ __forceinline__ V op(V a, V b) { return a + b; } };
struct RdMinU32 { typedef uint32_t V; static __device__ __forceinline__ V op(V a, V b) { return a < b ? a : b; } };
struct RdMinU64 { typedef uint64_t V; static __device__ __forceinline__ V op(V a, V b) { return a < b ? a : b; } };
struct RdMaxU32 { typedef uint32_t V; static __device__ __forceinline__ V op(V a, V b) { return a > b ? a : b; } };
struct RdMaxU64 { typedef uint64_t V; static __device__ __forceinline__ V op(V a, V b) { return a > b ? a : b; } };

// order-preserving bits of a value and back (x uniform)
__device__ __forceinline__ uint32_t rd_to_bits(uint32_t v, uint32_t x) {
    return x == RD_X_NONE ? v : x == RD_X_SIGNED ? v ^ 0x80000000u : v ^ ((uint32_t)((int32_t)v >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint32_t rd_from_bits(uint32_t b, uint32_t x) {
    return x == RD_X_NONE ? b : x == RD_X_SIGNED ? b ^ 0x80000000u : b ^ ((uint32_t)((int32_t)~b >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint64_t rd_to_bits(uint64_t v, uint32_t x) {
    return x == RD_X_NONE ? v : x == RD_X_SIGNED ? v ^ (1ull << 63) : v ^ ((uint64_t)((int64_t)v >> 63) | (1ull << 63));
}
__device__ __forceinline__ uint64_t rd_from_bits(uint64_t b, uint32_t x) {
    return x == RD_X_NONE ? b : x == RD_X_SIGNED ? b ^ (1ull << 63) : b ^ ((uint64_t)((int64_t)~b >> 63) | (1ull << 63));
}
__device__ __forceinline__ float rd_to_bits(float v, uint32_t) { return v; }
__device__ __forceinline__ float rd_from_bits(float v, uint32_t) { return v; }
__device__ __forceinline__ double rd_to_bits(double v, uint32_t) { return v; }
__device__ __forceinline__ double rd_from_bits(double v, uint32_t) { return v; }

// eight values from index i of the 16-byte aligned array q (i a multiple of 8), as the operation sees them; what lies at or behind n
// is not loaded (and never folded: the callers test the index)
template <class V>
__device__ __forceinline__ void rd_load8(const V* __restrict__ q, uint32_t i, uint32_t n, uint32_t x, V (&v)[UQ_KPT]) {
    constexpr uint32_t PER = 16u / sizeof(V);  // values per 16-byte load
    if (GS_LIKELY(i + UQ_KPT <= n)) {
#pragma unroll
        for (uint32_t g = 0; g < UQ_KPT / PER; ++g) {
            const uint4 a = *reinterpret_cast<const uint4*>(q + i + g * PER);
            __builtin_memcpy(&v[g * PER], &a, 16);
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < UQ_KPT; ++j) v[j] = i + j < n ? q[i + j] : V(0);
    }
#pragma unroll
    for (uint32_t j = 0; j < UQ_KPT; ++j) v[j] = rd_to_bits(v[j], x);
}

// the reduction of this thread's values from its last head (or its first element) to its last element below n.  i < n.
template <class Op>
__device__ __forceinline__ typename Op::V rd_tail(const typename Op::V (&v)[UQ_KPT], uint32_t h, uint32_t i, uint32_t n) {
    typename Op::V t = v[0];
#pragma unroll
    for (uint32_t j = 1; j < UQ_KPT; ++j) {
        if ((h >> j) & 1u) t = v[j];
        else if (i + j < n) t = Op::op(t, v[j]);
    }
    return t;
}

// Segmented scan of one (flag, value) per thread over a workgroup of WAVES waves, in front of which lies `carry` (if has_carry).
// f: this thread's segment holds a head, v: its reduction from its last head (or its start) to its end.  Returns in ex the reduction
// of everything in front of this thread back to the nearest head (carry included where no head lies between), in tot the same behind
// the last thread, in any whether a thread held a head.  ex of the first thread without a carry is not meaningful (nothing lies in
// front of it), and neither is anything computed from threads that hold no element — they lie behind every thread that does.
// One barrier; s_f / s_v are WAVES entries the caller alternates between calls.
template <class Op, uint32_t WAVES>
__device__ __forceinline__ void rd_block_scan(bool f, typename Op::V v, uint32_t lane, uint32_t wave, uint32_t* s_f, typename Op::V* s_v, bool has_carry,
                                              typename Op::V carry, typename Op::V& ex, typename Op::V& tot, bool& any) {
    typedef typename Op::V V;
    uint32_t fi = f ? 1u : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t fo = __shfl_up(fi, d, 64);
        const V vo = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) {
            if (!fi) v = Op::op(vo, v);
            fi |= fo;
        }
    }
    if (lane == 63u) {
        s_f[wave] = fi;
        s_v[wave] = v;
    }
    __syncthreads();
    V run = carry, front = carry;  // run: everything up to wave x; front: in front of this wave
    bool has = has_carry, has_front = has_carry;
    any = false;
#pragma unroll
    for (uint32_t x = 0; x < WAVES; ++x) {
        if (x == wave) {
            front = run;
            has_front = has;
        }
        const bool fx = s_f[x] != 0u;
        const V vx = s_v[x];
        run = (fx || !has) ? vx : Op::op(run, vx);
        has = true;
        any = any || fx;
    }
    tot = run;
    const uint32_t ef = __shfl_up(fi, 1, 64);
    const V ev = __shfl_up(v, 1, 64);
    ex = lane == 0u ? front : ((ef != 0u || !has_front) ? ev : Op::op(front, ev));
}

// src -> keys, vals -> values (W: a value's word): the engine sorts the copies, the caller's arrays are not written
template <class K, class W>
__global__ __launch_bounds__(UQ_PREP_THREADS) void rd_prepare_kernel(const K* __restrict__ src, const W* __restrict__ vals, uint32_t n,
                                                                     K* __restrict__ keys, W* __restrict__ values) {
    const uint32_t i = (blockIdx.x * UQ_PREP_THREADS + threadIdx.x) * 4u;
    if (i >= n) return;
    if (GS_LIKELY(i + 4u <= n)) {
        constexpr uint32_t KPER = 16u / sizeof(K);  // keys per 16-byte move
#pragma unroll
        for (uint32_t g = 0; g < 4u / KPER; ++g) *reinterpret_cast<uint4*>(keys + i + g * KPER) = *reinterpret_cast<const uint4*>(src + i + g * KPER);
        constexpr uint32_t PER = 16u / sizeof(W);
#pragma unroll
        for (uint32_t g = 0; g < 4u / PER; ++g) *reinterpret_cast<uint4*>(values + i + g * PER) = *reinterpret_cast<const uint4*>(vals + i + g * PER);
        return;
    }
    for (uint32_t j = i; j < n; ++j) {
        keys[j] = src[j];
        values[j] = vals[j];
    }
}

// rc[r] = heads of range r, rl[r] = position + 1 of its last head (0: the range holds none), part[r] = its open partial (what the
// range that holds element n - 1 leaves there is read by nobody)
template <class K, class Op>
__global__ __launch_bounds__(UQ_THREADS) void rd_count_kernel(const K* __restrict__ keys, const typename Op::V* __restrict__ vals, uint32_t n,
                                                              uint32_t per_range, uint32_t xform, uint32_t* __restrict__ rc, uint32_t* __restrict__ rl,
                                                              typename Op::V* __restrict__ part) {
    typedef typename Op::V V;
    __shared__ uint32_t s_c[UQ_WAVES], s_l[UQ_WAVES], s_f[2][UQ_WAVES];
    __shared__ V s_v[2][UQ_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    uint32_t heads = 0, last = 0;  // heads: the wave's (uniform); last: this thread's (positions rise from tile to tile)
    V open = V(0);                 // the range's open partial so far (uniform)
    bool has = false;
    uint32_t par = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += UQ_TILE, par ^= 1u) {
        const uint32_t i = t0 + tid * UQ_KPT;
        K k[UQ_KPT];
        V v[UQ_KPT];
        uq_load8(keys, i, n, k);
        rd_load8(vals, i, n, xform, v);
        const uint32_t h = uq_heads(k, uq_left(keys, k, i, n, lane), i, n);
#pragma unroll
        for (uint32_t j = 0; j < UQ_KPT; ++j) heads += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(((h >> j) & 1u) != 0u));
        if (h) last = uq_last_head(h, i);
        V ex, tot;
        bool any;
        rd_block_scan<Op, UQ_WAVES>(h != 0u, rd_tail<Op>(v, h, i, n), lane, wave, s_f[par], s_v[par], has, open, ex, tot, any);
        open = tot;
        has = true;
    }
    const uint32_t wl = wave_inclusive_max(last, lane);
    if (lane == 63u) {
        s_c[wave] = heads;
        s_l[wave] = wl;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t c = 0, l = 0;
        for (uint32_t x = 0; x < UQ_WAVES; ++x) {
            c += s_c[x];
            l = s_l[x] > l ? s_l[x] : l;
        }
        rc[blockIdx.x] = c;
        rl[blockIdx.x] = l;
        part[blockIdx.x] = open;
    }
}

// One workgroup, thread r for range r: base[r] = heads in front of range r, prev[r] = position + 1 of the last head in front of it,
// carry[r] = the open partials of the ranges in front of r back to the nearest one that holds a head (range 0: nothing, not read),
// u = all heads -> the control block and, when given, out_num.  It also resets the words the reduce adds to.
template <class Op>
__global__ __launch_bounds__(UQ_CAP) void rd_scan_kernel(const uint32_t* __restrict__ rc, const uint32_t* __restrict__ rl,
                                                         const typename Op::V* __restrict__ part, uint32_t ranges, uint32_t n, uint32_t* __restrict__ base,
                                                         uint32_t* __restrict__ prev, typename Op::V* __restrict__ carry, uint32_t* __restrict__ out_num,
                                                         uint32_t* __restrict__ ctl) {
    typedef typename Op::V V;
    constexpr uint32_t W = UQ_CAP / 64u;
    __shared__ uint32_t s_s[W], s_m[W], s_f[W];
    __shared__ V s_v[W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t c = tid < ranges ? rc[tid] : 0u, l = tid < ranges ? rl[tid] : 0u;
    const V p = tid < ranges ? part[tid] : V(0);
    const uint32_t is = wave_inclusive_scan(c, lane), im = wave_inclusive_max(l, lane);
    if (lane == 63u) {
        s_s[wave] = is;
        s_m[wave] = im;
    }
    V ex, tot;
    bool any;
    rd_block_scan<Op, W>(l != 0u, p, lane, wave, s_f, s_v, false, V(0), ex, tot, any);  // (its barrier publishes s_s and s_m as well)
    uint32_t run = is - c, total = 0;
    uint32_t pm = __shfl_up(im, 1, 64);
    if (lane == 0u) pm = 0u;
    for (uint32_t x = 0; x < W; ++x) {
        if (x < wave) {
            run += s_s[x];
            pm = s_m[x] > pm ? s_m[x] : pm;
        }
        total += s_s[x];
    }
    if (tid < ranges) {
        base[tid] = run;
        prev[tid] = pm;
        carry[tid] = ex;
    }
    if (tid == 0u) {
        ctl[UQC_STATUS] = (total == 0u || total > n) ? UQ_ST_INTERNAL : 0u;  // (element 0 is a head; no more heads than elements)
        ctl[UQC_U] = total;
        ctl[UQC_WRITTEN] = 0u;
        if (out_num) *out_num = total;
    }
}

// One workgroup per range, its tiles in order.  out_counts may be null.
template <class K, class Op>
__global__ __launch_bounds__(UQ_THREADS) void rd_reduce_kernel(const K* __restrict__ keys, const typename Op::V* __restrict__ vals, uint32_t n,
                                                               uint32_t per_range, uint32_t xform, const uint32_t* __restrict__ base,
                                                               const uint32_t* __restrict__ prev, const typename Op::V* __restrict__ carry,
                                                               const uint32_t* __restrict__ rc, K* __restrict__ out_keys,
                                                               typename Op::V* __restrict__ out_values, uint32_t* __restrict__ out_counts,
                                                               uint32_t* __restrict__ ctl) {
    typedef typename Op::V V;
    __shared__ uint32_t s_c[2][UQ_WAVES], s_l[2][UQ_WAVES], s_f[2][UQ_WAVES];  // by tile parity: one barrier per tile
    __shared__ V s_v[2][UQ_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    if (lo >= n || ctl[UQC_STATUS] != 0u) return;  // (uniform; the scan reported heads that do not add up: nothing is written)
    const uint32_t run0 = base[blockIdx.x];
    uint32_t run = run0;                // heads in front of the tile
    uint32_t lastp = prev[blockIdx.x];  // position + 1 of the last head in front of the tile (0 in front of element 0 only)
    V open = carry[blockIdx.x];         // the open run's values in front of the tile (range 0: nothing, and element 0 is a head)
    bool has = blockIdx.x != 0u;
    bool bad = false;
    uint32_t par = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += UQ_TILE, par ^= 1u) {
        const uint32_t i = t0 + tid * UQ_KPT;
        K k[UQ_KPT];
        V v[UQ_KPT];
        uq_load8(keys, i, n, k);
        rd_load8(vals, i, n, xform, v);
        const uint32_t h = uq_heads(k, uq_left(keys, k, i, n, lane), i, n);
        const uint32_t c = (uint32_t)__popc(h);
        const uint32_t incl = wave_inclusive_scan(c, lane);
        const uint32_t ml = wave_inclusive_max(uq_last_head(h, i), lane);
        if (lane == 63u) {
            s_c[par][wave] = incl;
            s_l[par][wave] = ml;
        }
        V cur, tot;  // cur: the open run's values in front of this thread's eight
        bool any;
        rd_block_scan<Op, UQ_WAVES>(h != 0u, rd_tail<Op>(v, h, i, n), lane, wave, s_f[par], s_v[par], has, open, cur, tot, any);
        uint32_t r = run + incl - c;  // heads in front of this thread's eight
        uint32_t p = __shfl_up(ml, 1, 64);
        if (lane == 0u) p = 0u;
        uint32_t tile_heads = 0, tile_last = 0;
#pragma unroll
        for (uint32_t x = 0; x < UQ_WAVES; ++x) {
            const uint32_t cx = s_c[par][x], lx = s_l[par][x];
            if (x < wave) {
                r += cx;
                p = lx > p ? lx : p;
            }
            tile_heads += cx;
            tile_last = lx > tile_last ? lx : tile_last;
        }
        p = p > lastp ? p : lastp;  // position + 1 of the last head in front of this thread's eight
#pragma unroll
        for (uint32_t j = 0; j < UQ_KPT; ++j) {
            const uint32_t at = i + j;
            if ((h >> j) & 1u) {  // the head of rank r: it closes run r - 1 and opens run r
                if (r < n && (r == 0u ? at == 0u : (p != 0u && p <= at))) {
                    out_keys[r] = k[j];
                    if (r != 0u) {
                        out_values[r - 1u] = rd_from_bits(cur, xform);
                        if (out_counts) out_counts[r - 1u] = at - (p - 1u);
                    }
                } else {
                    bad = true;
                }
                p = at + 1u;
                ++r;
                cur = v[j];
            } else if (at < n) {  // (not element 0: a value lies in front of it in its run)
                cur = Op::op(cur, v[j]);
            }
        }
        if (i < n && n - i <= UQ_KPT) {  // this thread holds element n - 1: it closes the last run, whose rank is r - 1
            if (r != 0u && r <= n && p != 0u && p <= n) {
                out_values[r - 1u] = rd_from_bits(cur, xform);
                if (out_counts) out_counts[r - 1u] = n - (p - 1u);
            } else {
                bad = true;
            }
        }
        run += tile_heads;
        lastp = tile_last > lastp ? tile_last : lastp;
        open = tot;
        has = true;
    }
    if (bad) atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
    if (tid == 0u) {
        if (run - run0 != rc[blockIdx.x]) atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
        atomicAdd(&ctl[UQC_WRITTEN], run - run0);
    }
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
