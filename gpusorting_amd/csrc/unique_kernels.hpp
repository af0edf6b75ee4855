// unique_kernels.hpp — unique / run-length encode of 32-bit keys: gs_unique_* of include/gpusort.h.  No counterpart in the reference
// project.
//
// The run-length stage works on an array whose equal keys already lie side by side (the engine's sorted output, or the caller's input
// as it lies for gs_unique_consecutive).  Element i is a HEAD when i == 0 or key[i] != key[i - 1], bit for bit; the run of rank r
// starts at the r-th head.  The array is cut into at most UQ_CAP ranges of whole tiles (the plan is a function of n alone), and three
// launches follow one another on the stream:
//   uq_count_kernel    one workgroup per range: heads of the range (a ballot and a popcount per wave and key slot) and the position
//                      of its last head;
//   uq_scan_kernel     one workgroup: heads in front of every range, the last head in front of every range, and u;
//   uq_compact_kernel  the same walk with the running base: the head of rank r writes out_keys[r], CLOSES the run in front of it
//                      (out_counts[r - 1] = its position - the previous head's, and for descending out_first[r - 1] = the position
//                      stored left of it) and opens its own (ascending: out_first[r]); every element writes its rank to the inverse.
//                      The workgroup that holds element n - 1 closes the last run.  So counts are resolved inside the compact: a run
//                      that spans tiles or whole ranges is closed by the next head, wherever that lies, from the carried position
//                      of the last head; nothing intermediate goes through the caller's buffers and nothing at or behind u is written.
// uq_prepare_kernel copies the caller's keys into the workspace in front of the engine's sort and writes the positions 0 .. n - 1.
//
// No kernel waits on another workgroup: no look-back, no chain, no ticket.  A neighbour across a wave, tile or range edge is read
// from global memory.  Every global store index is checked against n; a count that does not add up sets UQ_ST_INTERNAL in the
// handle's status word and the compact then writes nothing.  Registers, LDS and scratch per kernel: DESIGN.md 3.21.
#pragma once
#include "sort16_kernels.hpp"  // GS_SORT16_BUILT (radix_pass.hpp), wave_inclusive_scan, wave_inclusive_max

namespace gs {

constexpr uint32_t UQ_THREADS = 512, UQ_KPT = 8, UQ_WAVES = UQ_THREADS / 64;
constexpr uint32_t UQ_TILE = UQ_THREADS * UQ_KPT;  // two 16-byte loads per thread
constexpr uint32_t UQ_CAP = 1024;                  // most ranges: the scan is one workgroup with one thread per range
constexpr uint32_t UQ_PREP_THREADS = 256, UQ_PREP_TILE = 4 * UQ_PREP_THREADS;
// the handle's control block
constexpr uint32_t UQC_STATUS = 0, UQC_U = 1, UQC_WRITTEN = 2, UQC_WORDS = 64;
constexpr uint32_t UQ_ST_INTERNAL = 1;
static_assert(UQ_KPT == 8 && UQ_TILE == 4096 && UQ_CAP % 64u == 0 && UQ_CAP <= 1024, "two uint4 per thread; the scan's workgroup");

#if GS_SORT16_BUILT  // the product build only, as the 16-bit sort

// The kernels below are written once over the key word K: uint32_t (gs_unique_*, gs_reduce_*) or uint64_t (gs_unique64_*,
// gs_reduce64_*: an 8-byte key is one element, compared and moved as both of its words).  Positions, counts and ranks are uint32_t.

// eight words from index i of the 16-byte aligned array q (i a multiple of 8); what lies at or behind n reads as 0 and is not loaded
__device__ __forceinline__ void uq_load8(const uint32_t* __restrict__ q, uint32_t i, uint32_t n, uint32_t (&k)[UQ_KPT]) {
    if (GS_LIKELY(i + UQ_KPT <= n)) {
        const uint4 a = *reinterpret_cast<const uint4*>(q + i), b = *reinterpret_cast<const uint4*>(q + i + 4u);
        k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
        k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < UQ_KPT; ++j) k[j] = i + j < n ? q[i + j] : 0u;
}
// the same for 8-byte keys: four 16-byte loads of two keys each
__device__ __forceinline__ void uq_load8(const uint64_t* __restrict__ q, uint32_t i, uint32_t n, uint64_t (&k)[UQ_KPT]) {
    if (GS_LIKELY(i + UQ_KPT <= n)) {
#pragma unroll
        for (uint32_t g = 0; g < UQ_KPT / 2u; ++g) {
            const uint4 a = *reinterpret_cast<const uint4*>(q + i + 2u * g);
            k[2u * g] = (uint64_t)a.x | ((uint64_t)a.y << 32);
            k[2u * g + 1u] = (uint64_t)a.z | ((uint64_t)a.w << 32);
        }
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < UQ_KPT; ++j) k[j] = i + j < n ? q[i + j] : 0ull;
}

// the word left of this thread's eight: the lane below holds it (an 8-byte key: both words); lane 0 (a wave, tile or range edge) reads
// it from global memory.  Every lane of the wave calls this.
template <class K>
__device__ __forceinline__ K uq_left(const K* __restrict__ q, const K (&k)[UQ_KPT], uint32_t i, uint32_t n, uint32_t lane) {
    K left = __shfl_up(k[UQ_KPT - 1u], 1, 64);
    if (lane == 0u && i != 0u && i < n) left = q[i - 1u];
    return left;
}

// bit j: element i + j (< n) starts a run (an 8-byte key: it differs from its left neighbour in either word)
template <class K>
__device__ __forceinline__ uint32_t uq_heads(const K (&k)[UQ_KPT], K left, uint32_t i, uint32_t n) {
    uint32_t h = 0;
#pragma unroll
    for (uint32_t j = 0; j < UQ_KPT; ++j) {
        const K before = j ? k[j ? j - 1u : 0u] : left;
        if (i + j < n && (i + j == 0u || k[j] != before)) h |= 1u << j;
    }
    return h;
}

// position + 1 of the last head among this thread's eight, 0 without one
__device__ __forceinline__ uint32_t uq_last_head(uint32_t h, uint32_t i) { return h ? i + 32u - (uint32_t)__clz((int)h) : 0u; }

// src[0 .. n) -> keys, and with POS the positions 0 .. n - 1 beside them: the engine sorts the copy, the caller's keys are not written
template <class K, bool POS>
__global__ __launch_bounds__(UQ_PREP_THREADS) void uq_prepare_kernel(const K* __restrict__ src, uint32_t n, K* __restrict__ keys,
                                                                     uint32_t* __restrict__ pos) {
    const uint32_t i = (blockIdx.x * UQ_PREP_THREADS + threadIdx.x) * 4u;
    if (i >= n) return;
    if (GS_LIKELY(i + 4u <= n)) {
        constexpr uint32_t PER = 16u / sizeof(K);  // keys per 16-byte move
#pragma unroll
        for (uint32_t g = 0; g < 4u / PER; ++g) *reinterpret_cast<uint4*>(keys + i + g * PER) = *reinterpret_cast<const uint4*>(src + i + g * PER);
        if (POS) *reinterpret_cast<uint4*>(pos + i) = uint4{i, i + 1u, i + 2u, i + 3u};
        return;
    }
    for (uint32_t j = i; j < n; ++j) {
        keys[j] = src[j];
        if (POS) pos[j] = j;
    }
}

// rc[r] = heads of range r, rl[r] = position + 1 of its last head (0: the range holds none)
template <class K>
__global__ __launch_bounds__(UQ_THREADS) void uq_count_kernel(const K* __restrict__ keys, uint32_t n, uint32_t per_range, uint32_t* __restrict__ rc,
                                                              uint32_t* __restrict__ rl) {
    __shared__ uint32_t s_c[UQ_WAVES], s_l[UQ_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    uint32_t heads = 0, last = 0;  // heads: the wave's (uniform); last: this thread's (positions rise from tile to tile)
    for (uint32_t t0 = lo; t0 < hi; t0 += UQ_TILE) {
        const uint32_t i = t0 + tid * UQ_KPT;
        K k[UQ_KPT];
        uq_load8(keys, i, n, k);
        const uint32_t h = uq_heads(k, uq_left(keys, k, i, n, lane), i, n);
#pragma unroll
        for (uint32_t j = 0; j < UQ_KPT; ++j) heads += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(((h >> j) & 1u) != 0u));
        if (h) last = uq_last_head(h, i);
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
    }
}

// One workgroup, thread r for range r: base[r] = heads in front of range r, prev[r] = position + 1 of the last head in front of it,
// u = all heads -> the control block and, when given, out_num.  It also resets the words the compact adds to.
__global__ __launch_bounds__(UQ_CAP) void uq_scan_kernel(const uint32_t* __restrict__ rc, const uint32_t* __restrict__ rl, uint32_t ranges, uint32_t n,
                                                         uint32_t* __restrict__ base, uint32_t* __restrict__ prev, uint32_t* __restrict__ out_num,
                                                         uint32_t* __restrict__ ctl) {
    constexpr uint32_t W = UQ_CAP / 64u;
    __shared__ uint32_t s_s[W], s_m[W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t c = tid < ranges ? rc[tid] : 0u, l = tid < ranges ? rl[tid] : 0u;
    const uint32_t is = wave_inclusive_scan(c, lane), im = wave_inclusive_max(l, lane);
    if (lane == 63u) {
        s_s[wave] = is;
        s_m[wave] = im;
    }
    __syncthreads();
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
    }
    if (tid == 0u) {
        ctl[UQC_STATUS] = (total == 0u || total > n) ? UQ_ST_INTERNAL : 0u;  // (element 0 is a head; no more heads than elements)
        ctl[UQC_U] = total;
        ctl[UQC_WRITTEN] = 0u;
        if (out_num) *out_num = total;
    }
}

// One workgroup per range, its tiles in order.  POS: perm[i] is the input position of element i (the engine's sorted values) and the
// inverse is scattered through it; without, the inverse is written in place (gs_unique_consecutive).  tail_first != 0 (descending):
// a run's lowest position is stored at its tail.  out_counts, out_first and out_inverse may be null.
template <class K, bool POS>
__global__ __launch_bounds__(UQ_THREADS) void uq_compact_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ perm, uint32_t n,
                                                                uint32_t per_range, uint32_t tail_first, const uint32_t* __restrict__ base,
                                                                const uint32_t* __restrict__ prev, const uint32_t* __restrict__ rc,
                                                                K* __restrict__ out_keys, uint32_t* __restrict__ out_counts,
                                                                uint32_t* __restrict__ out_first, uint32_t* __restrict__ out_inverse,
                                                                uint32_t* __restrict__ ctl) {
    __shared__ uint32_t s_c[2][UQ_WAVES], s_l[2][UQ_WAVES];  // by tile parity: one barrier per tile
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    if (lo >= n || ctl[UQC_STATUS] != 0u) return;  // (uniform; the scan reported heads that do not add up: nothing is written)
    const uint32_t run0 = base[blockIdx.x];
    uint32_t run = run0;              // heads in front of the tile
    uint32_t lastp = prev[blockIdx.x];  // position + 1 of the last head in front of the tile (0 in front of element 0 only)
    const bool first_tail = POS && out_first && tail_first != 0u, first_head = POS && out_first && tail_first == 0u;
    bool bad = false;
    uint32_t par = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += UQ_TILE, par ^= 1u) {
        const uint32_t i = t0 + tid * UQ_KPT;
        K k[UQ_KPT];
        uint32_t v[UQ_KPT];
        uq_load8(keys, i, n, k);
        const uint32_t h = uq_heads(k, uq_left(keys, k, i, n, lane), i, n);
        uint32_t vleft = 0;
        if (POS) {
            uq_load8(perm, i, n, v);
            if (first_tail) vleft = uq_left(perm, v, i, n, lane);  // (uniform)
        }
        const uint32_t c = (uint32_t)__popc(h);
        const uint32_t incl = wave_inclusive_scan(c, lane);
        const uint32_t ml = wave_inclusive_max(uq_last_head(h, i), lane);
        if (lane == 63u) {
            s_c[par][wave] = incl;
            s_l[par][wave] = ml;
        }
        __syncthreads();
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
        uint32_t inv[UQ_KPT];
#pragma unroll
        for (uint32_t j = 0; j < UQ_KPT; ++j) {
            const uint32_t at = i + j;
            if ((h >> j) & 1u) {  // the head of rank r: it closes run r - 1 and opens run r
                if (r < n && (r == 0u ? at == 0u : (p != 0u && p <= at))) {
                    out_keys[r] = k[j];
                    if (r != 0u) {
                        if (out_counts) out_counts[r - 1u] = at - (p - 1u);
                        if (first_tail) out_first[r - 1u] = j ? v[j ? j - 1u : 0u] : vleft;
                    }
                    if (first_head) out_first[r] = v[j];
                } else {
                    bad = true;
                }
                p = at + 1u;
                ++r;
            }
            inv[j] = r - 1u;  // (r >= 1 behind element 0)
        }
        if (out_inverse) {
            if (POS) {
#pragma unroll
                for (uint32_t j = 0; j < UQ_KPT; ++j) {
                    if (i + j < n) {
                        if (v[j] < n && inv[j] < n) out_inverse[v[j]] = inv[j]; else bad = true;
                    }
                }
            } else if (GS_LIKELY(i + UQ_KPT <= n)) {
                *reinterpret_cast<uint4*>(out_inverse + i) = uint4{inv[0], inv[1], inv[2], inv[3]};
                *reinterpret_cast<uint4*>(out_inverse + i + 4u) = uint4{inv[4], inv[5], inv[6], inv[7]};
            } else {
#pragma unroll
                for (uint32_t j = 0; j < UQ_KPT; ++j)
                    if (i + j < n) out_inverse[i + j] = inv[j];
            }
        }
        run += tile_heads;
        lastp = tile_last > lastp ? tile_last : lastp;
    }
    if (bad) atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
    if (tid == 0u) {
        if (run - run0 != rc[blockIdx.x]) atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
        atomicAdd(&ctl[UQC_WRITTEN], run - run0);
        if (hi == n) {  // this range holds element n - 1: close the last run, whose rank is run - 1
            if (run != 0u && run <= n && lastp != 0u && lastp <= n) {
                if (out_counts) out_counts[run - 1u] = n - (lastp - 1u);
                if (first_tail) out_first[run - 1u] = perm[n - 1u];
            } else {
                atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
            }
        }
    }
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
