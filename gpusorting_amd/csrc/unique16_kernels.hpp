// unique16_kernels.hpp — unique / run-length encode of 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16) at their own width:
// gs_unique16_* of include/gpusort.h.  No counterpart in the reference project.
//
// A 16-bit key has 65 536 patterns, so ONE HISTOGRAM of bin = sortable bits ^ flip (flip = 0xFFFF: descending, as gs_sort16) is the
// exact answer of gs_unique16_unique: the distinct keys are the non-empty bins in rising bin order, the counts are the bins, the
// inverse is a lookup in the table of the bins' ranks, the first position a minimum per bin.  No sort, nothing that grows with n:
//   s16_clear_kernel      (sort16_kernels.hpp, as it is) the control block and the histogram behind it;
//   u16_fill_kernel       the first-position table to all-ones (only when first positions are wanted);
//   s16_hist_kernel       (as it is) on gs_sort16_plan's ranges;
//   u16_first_kernel      the lowest position per bin into the global table, through the filters told at the kernel;
//   u16_rank_kernel       one workgroup: the scan of the non-empty flags, u, the rank table, out_keys / out_counts / out_first;
//   u16_inverse_kernel    out_inverse[i] = rank[bin(keys[i])], the rank table in LDS (128 KiB of 16-bit entries) or gathered from
//                         global memory.
// gs_unique16_consecutive is the run-length stage of unique_kernels.hpp on 2-byte loads: u16_count_kernel and u16_compact_kernel are
// copies of uq_count_kernel and uq_compact_kernel<false> (the head rule, the plan and the closing of a run by the next head are told
// there; a fix belongs in both files), uq_scan_kernel runs between them as it is.
//
// No kernel waits on another workgroup.  Every LDS and global store index is checked against its buffer's length; a count that does
// not add up sets UQ_ST_INTERNAL in the handle's status word and the kernels behind write nothing.  The control block has
// unique_kernels.hpp's words (UQC_*).  Registers, LDS and scratch per kernel: DESIGN.md 3.22.
#pragma once
#include "unique_kernels.hpp"  // the run-length stage's helpers and uq_scan_kernel; through it sort16_kernels.hpp

namespace gs {

constexpr uint32_t U16_THREADS = 1024, U16_TILE = 8 * U16_THREADS;  // one 16-byte load per thread
constexpr uint32_t U16_UNROLL = 4;                                  // loads in flight per thread of the inverse
constexpr uint32_t U16_FCAP = 256, U16_ICAP = 256;                  // most ranges of the first-position kernel and of the LDS inverse
constexpr uint32_t U16_FMIN_TILES = 4, U16_IMIN_TILES = 8;          // and the fewest tiles of a range: the filters and the table load pay off
constexpr uint32_t U16_SLOTS = 4096;                                // the first-position kernel's combiner: one slot per low 12 bits of the bin
constexpr uint32_t U16_NONE = 0xffffffffu;
static_assert(U16_TILE == 8192 && U16_TILE == S16_KTILE && U16_SLOTS * 16u == S16_BINS, "a slot word: 4 high bin bits above 13 bits of tile index");
static_assert(S16_BINS * 2u + 64u <= 160u * 1024u, "the rank table in LDS");

#if GS_SORT16_BUILT  // the product build only, as the 16-bit sort

// `count` 16-byte groups from p to all-ones: the first-position table in front of a call that wants first positions
__global__ __launch_bounds__(256) void u16_fill_kernel(uint4* __restrict__ p, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) p[i] = uint4{U16_NONE, U16_NONE, U16_NONE, U16_NONE};
}

// the eight 16-bit elements of a 16-byte load, one to a word
__device__ __forceinline__ void u16_split(const uint4 t, uint32_t (&k)[8]) {
    const uint32_t w4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) k[j] = tkr16_elem(w4, j);
}

// first[b] = min(first[b], position) over the elements of bin b: one workgroup per range walks its tiles in RISING position order.
// n global atomics would be ruinous on skewed inputs, so elements are dropped before they reach the table.  THE INVARIANT OF EVERY
// FILTER: an element may be dropped only if an element of the same bin at a LOWER position has been applied or is certain to be
// applied.  The filters, in the order an element meets them:
//   1. its left neighbour in the same thread has the same bin (the neighbour is lower and meets the same filters);
//   2. the bin's bit in s_seen is set.  Bits are TESTED in front of the tile's barrier and SET behind it, so a set bit seen by a test
//      was set by an element of an earlier tile of this workgroup: a lower position.  (Testing and setting in one step would let a
//      higher position in another wave set the bit first.)
//   3. the combiner: every element left min-s (bin's 4 high bits, its index in the tile) into the slot of the bin's 12 low bits.  Behind
//      the barrier an element that finds ITS bin in the slot with another index is dropped: the winner has the same bin and a lower
//      index, and goes on.  An element that finds another bin in its slot goes on as well.
//   4. a plain load of the global entry: entries only fall, so a value that is already <= the position — however stale — is one an
//      element of this bin at a lower or the same position has applied.
// What is left does atomicMin.  The three slot tables rotate: a table is cleared one tile step before it is used, behind the barrier
// that ends the step that read it last, so one barrier per tile step orders all of it.
__global__ __launch_bounds__(U16_THREADS) void u16_first_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t per_range, uint32_t kt, uint32_t flip,
                                                                uint32_t* __restrict__ first) {
    __shared__ __attribute__((aligned(16))) uint32_t s_seen[S16_BINS / 32u];
    __shared__ __attribute__((aligned(16))) uint32_t s_slot[3][U16_SLOTS];
    const uint32_t tid = threadIdx.x;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    const uint4 ones = uint4{U16_NONE, U16_NONE, U16_NONE, U16_NONE};
    if (tid < S16_BINS / 32u / 4u) reinterpret_cast<uint4*>(s_seen)[tid] = uint4{0u, 0u, 0u, 0u};
    reinterpret_cast<uint4*>(s_slot[0])[tid] = ones;  // (U16_SLOTS / 4 == U16_THREADS)
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += U16_TILE) {
        const uint32_t nxt = cur == 2u ? 0u : cur + 1u;
        reinterpret_cast<uint4*>(s_slot[nxt])[tid] = ones;  // read last two steps ago, used next behind this step's barrier
        const uint32_t at = tid * 8u, i = t0 + at;
        uint32_t mask = 0u, k[8], d[8], cand = 0u;
        uint4 t = uint4{0u, 0u, 0u, 0u};
        if (i < hi) t = s16_load8(keys, i, hi, mask);
        u16_split(t, k);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            d[j] = (tkr16_to_bits(k[j], kt) ^ flip) & 0xffffu;  // (< S16_BINS)
            const bool dup = j != 0u && d[j] == d[j ? j - 1u : 0u];  // (filter 1; element j - 1 lies below hi when j does)
            if (((mask >> j) & 1u) && !dup && ((s_seen[d[j] >> 5] >> (d[j] & 31u)) & 1u) == 0u) {  // (filter 2: the test)
                cand |= 1u << j;
                atomicMin(&s_slot[cur][d[j] & (U16_SLOTS - 1u)], ((d[j] >> 12) << 13) | (at + j));
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (((cand >> j) & 1u) == 0u) continue;
            const uint32_t v = s_slot[cur][d[j] & (U16_SLOTS - 1u)];
            if ((v >> 13) == (d[j] >> 12) && (v & (U16_TILE - 1u)) != at + j) continue;  // (filter 3)
            atomicOr(&s_seen[d[j] >> 5], 1u << (d[j] & 31u));                            // (filter 2: the set, behind the barrier)
            const uint32_t pos = i + j;
            if (__atomic_load_n(&first[d[j]], __ATOMIC_RELAXED) > pos) atomicMin(&first[d[j]], pos);  // (filter 4)
        }
        cur = nxt;
    }
}

// One workgroup, 64 bins per thread (the shape of s16_scan_kernel): rank[b] = non-empty bins below b, u = their number -> out_num and
// the control block; the non-empty bin of rank r writes out_keys[r] (a 2-byte store), out_counts[r] and out_first[r] (from the
// first-position table).  cap = min(n, 65 536) is the outputs' length.  The counts must add up to n and 1 <= u <= cap: otherwise the
// status bit is set and neither this kernel nor the inverse writes an output.  A rank is at most 65 535 and fits the table's 16
// bits; u can be 65 536 and does not: it is never stored there.
__global__ __launch_bounds__(S16_KTHREADS) void u16_rank_kernel(const uint32_t* __restrict__ ghist, const uint32_t* __restrict__ first, uint32_t n, uint32_t kt,
                                                                uint32_t flip, uint16_t* __restrict__ rank, uint16_t* __restrict__ out_keys,
                                                                uint32_t* __restrict__ out_counts, uint32_t* __restrict__ out_first,
                                                                uint32_t* __restrict__ out_num, uint32_t* __restrict__ ctl) {
    constexpr uint32_t PER = S16_BINS / S16_KTHREADS, W = S16_KTHREADS / 64;  // 64 bins per thread
    __shared__ uint32_t s_u[W], s_n[W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4* src = reinterpret_cast<const uint4*>(ghist + tid * PER);
    uint32_t mine = 0, sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER / 4u; ++i) {
        const uint4 c = src[i];
        sum += c.x + c.y + c.z + c.w;
        mine += (c.x != 0u) + (c.y != 0u) + (c.z != 0u) + (c.w != 0u);
    }
    const uint32_t incl = wave_inclusive_scan(mine, lane), isum = wave_inclusive_scan(sum, lane);
    if (lane == 63u) {
        s_u[wave] = incl;
        s_n[wave] = isum;
    }
    __syncthreads();
    uint32_t r = incl - mine, u = 0, total = 0;
    for (uint32_t x = 0; x < W; ++x) {
        if (x < wave) r += s_u[x];
        u += s_u[x];
        total += s_n[x];
    }
    const uint32_t cap = n < S16_BINS ? n : S16_BINS;
    const bool ok = total == n && u != 0u && u <= cap;  // (uniform)
    if (tid == 0u) {
        if (!ok) atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);  // (the clear in front of the call zeroed the word)
        ctl[UQC_U] = u;
        ctl[UQC_WRITTEN] = ok ? u : 0u;
        if (out_num) *out_num = u;
    }
    if (!ok) return;
    bool bad = false;
    uint4* dst = reinterpret_cast<uint4*>(rank + tid * PER);  // (tid * PER + 63 < S16_BINS)
#pragma unroll
    for (uint32_t i = 0; i < PER / 8u; ++i) {
        const uint4 a = src[2u * i], b = src[2u * i + 1u];
        const uint32_t c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t w4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            w4[j >> 1] |= (r & 0xffffu) << ((j & 1u) * 16u);  // (an empty bin's entry is never looked up)
            if (c[j] == 0u) continue;
            const uint32_t bin = tid * PER + i * 8u + j;
            if (r < cap) {
                out_keys[r] = (uint16_t)tkr16_from_bits((bin ^ flip) & 0xffffu, kt);
                if (out_counts) out_counts[r] = c[j];
                if (out_first) {
                    const uint32_t f = first[bin];
                    if (f < n) out_first[r] = f; else bad = true;
                }
            } else {
                bad = true;
            }
            ++r;
        }
        dst[i] = uint4{w4[0], w4[1], w4[2], w4[3]};
    }
    if (bad) atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
}

// out_inverse[i] = rank[bin(keys[i])]: one workgroup per range, 16-byte key loads, two 16-byte stores per thread and load.  LDS: the
// workgroup first copies the 128 KiB rank table into LDS (its fixed cost: the grid is at most U16_ICAP ranges); without, every
// lookup is a 2-byte gather from the global table (ranges of one tile).  A status word that is set (u16_rank_kernel): nothing is written.
template <bool LDS>
__global__ __launch_bounds__(U16_THREADS) void u16_inverse_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t per_range, uint32_t kt, uint32_t flip,
                                                                  const uint16_t* __restrict__ rank, uint32_t* __restrict__ out_inverse,
                                                                  const uint32_t* __restrict__ ctl) {
    __shared__ __attribute__((aligned(16))) uint16_t s_rank[LDS ? S16_BINS : 8u];
    const uint32_t tid = threadIdx.x;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    if (lo >= n || ctl[UQC_STATUS] != 0u) return;  // (uniform)
    if (LDS) {
#pragma unroll
        for (uint32_t x = 0; x < S16_BINS / 8u / U16_THREADS; ++x)
            reinterpret_cast<uint4*>(s_rank)[tid + x * U16_THREADS] = reinterpret_cast<const uint4*>(rank)[tid + x * U16_THREADS];
        __syncthreads();
    }
    for (uint32_t c0 = lo; c0 < hi; c0 += U16_UNROLL * U16_TILE) {
        uint4 t[U16_UNROLL];
        uint32_t mask[U16_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < U16_UNROLL; ++u) {
            const uint32_t i = c0 + u * U16_TILE + tid * 8u;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (i < hi) t[u] = s16_load8(keys, i, hi, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < U16_UNROLL; ++u) {
            const uint32_t i = c0 + u * U16_TILE + tid * 8u;
            if (mask[u] == 0u) continue;
            uint32_t k[8], r[8];
            u16_split(t[u], k);
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t b = (tkr16_to_bits(k[j], kt) ^ flip) & 0xffffu;  // (< S16_BINS)
                r[j] = LDS ? s_rank[b] : rank[b];
            }
            if (GS_LIKELY(mask[u] == 255u)) {  // i + 8 <= hi <= n
                *reinterpret_cast<uint4*>(out_inverse + i) = uint4{r[0], r[1], r[2], r[3]};
                *reinterpret_cast<uint4*>(out_inverse + i + 4u) = uint4{r[4], r[5], r[6], r[7]};
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j)
                    if (i + j < hi) out_inverse[i + j] = r[j];
            }
        }
    }
}

// ---- the run-length stage on 2-byte keys (gs_unique16_consecutive) -------------------------------------------------------------------
// eight elements from index i of the 16-byte aligned array q (i a multiple of 8), one to a word; what lies at or behind n reads as 0
__device__ __forceinline__ void u16_load8(const uint16_t* __restrict__ q, uint32_t i, uint32_t n, uint32_t (&k)[UQ_KPT]) {
    uint32_t mask;
    u16_split(s16_load8(q, i, n, mask), k);
}

// uq_left on 2-byte elements.  Every lane of the wave calls this.
__device__ __forceinline__ uint32_t u16_left(const uint16_t* __restrict__ q, const uint32_t (&k)[UQ_KPT], uint32_t i, uint32_t n, uint32_t lane) {
    uint32_t left = __shfl_up(k[UQ_KPT - 1u], 1, 64);
    if (lane == 0u && i != 0u && i < n) left = q[i - 1u];
    return left;
}

// uq_count_kernel on 2-byte keys: rc[r] = heads of range r, rl[r] = position + 1 of its last head (0: the range holds none)
__global__ __launch_bounds__(UQ_THREADS) void u16_count_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t per_range, uint32_t* __restrict__ rc,
                                                               uint32_t* __restrict__ rl) {
    __shared__ uint32_t s_c[UQ_WAVES], s_l[UQ_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    uint32_t heads = 0, last = 0;  // heads: the wave's (uniform); last: this thread's (positions rise from tile to tile)
    for (uint32_t t0 = lo; t0 < hi; t0 += UQ_TILE) {
        const uint32_t i = t0 + tid * UQ_KPT;
        uint32_t k[UQ_KPT];
        u16_load8(keys, i, n, k);
        const uint32_t h = uq_heads(k, u16_left(keys, k, i, n, lane), i, n);
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

// uq_compact_kernel<false> on 2-byte keys: one workgroup per range, its tiles in order; out_keys gets 2-byte stores, the inverse is
// written in place.  out_counts and out_inverse may be null.
__global__ __launch_bounds__(UQ_THREADS) void u16_compact_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t per_range,
                                                                 const uint32_t* __restrict__ base, const uint32_t* __restrict__ prev,
                                                                 const uint32_t* __restrict__ rc, uint16_t* __restrict__ out_keys,
                                                                 uint32_t* __restrict__ out_counts, uint32_t* __restrict__ out_inverse, uint32_t* __restrict__ ctl) {
    __shared__ uint32_t s_c[2][UQ_WAVES], s_l[2][UQ_WAVES];  // by tile parity: one barrier per tile
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    if (lo >= n || ctl[UQC_STATUS] != 0u) return;  // (uniform; the scan reported heads that do not add up: nothing is written)
    const uint32_t run0 = base[blockIdx.x];
    uint32_t run = run0;                // heads in front of the tile
    uint32_t lastp = prev[blockIdx.x];  // position + 1 of the last head in front of the tile (0 in front of element 0 only)
    bool bad = false;
    uint32_t par = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += UQ_TILE, par ^= 1u) {
        const uint32_t i = t0 + tid * UQ_KPT;
        uint32_t k[UQ_KPT];
        u16_load8(keys, i, n, k);
        const uint32_t h = uq_heads(k, u16_left(keys, k, i, n, lane), i, n);
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
                    out_keys[r] = (uint16_t)k[j];
                    if (r != 0u && out_counts) out_counts[r - 1u] = at - (p - 1u);
                } else {
                    bad = true;
                }
                p = at + 1u;
                ++r;
            }
            inv[j] = r - 1u;  // (r >= 1 behind element 0)
        }
        if (out_inverse) {
            if (GS_LIKELY(i + UQ_KPT <= n)) {
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
            } else {
                atomicOr(&ctl[UQC_STATUS], UQ_ST_INTERNAL);
            }
        }
    }
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
