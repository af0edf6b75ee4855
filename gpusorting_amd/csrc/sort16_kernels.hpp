// sort16_kernels.hpp — the sort of 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16) at their own width: gs_sort16_* of
// include/gpusort.h.  No counterpart in the reference project.
//
// Keys only is a counting sort: s16_hist_kernel reads the keys once per half of the bin space into the handle's exact 65 536-bin
// histogram, s16_scan_kernel turns it into prefix[65 537], and s16_fill_kernel writes the sorted array FROM THE PREFIX — the keys
// are never read again, so the sort works in place and needs no n-sized scratch.
// Pairs and argsort are two stable 8-bit passes (low byte into the alternate buffers, high byte back) of radix_pass.hpp, which
// tells the pass's structure and invariants: the whole array is the one row, cut into ranges of whole tiles; s16_count_kernel writes
// one 256-bin digit histogram per range, s16_pscan_kernel the exclusive prefix over (digit major, range minor), and
// s16_scatter_kernel — one workgroup per range — walks its tiles in order.
//
// No kernel waits on another workgroup: no look-back, no chain, no ticket.  Every LDS and global store index is checked against
// its buffer's length; a count that does not add up sets S16_ST_INTERNAL in the handle's status word.  Registers, LDS and scratch
// per kernel: DESIGN.md 3.12.
#pragma once
#include "radix_pass.hpp"  // the pass; through it tkr16_to_bits / tkr16_from_bits, KEY_U16 .. KEY_BF16 (topk_rows16_kernels.hpp)

namespace gs {

constexpr uint32_t S16_BINS = 65536, S16_HALF = S16_BINS / 2;
constexpr uint32_t S16_KTHREADS = 1024;
constexpr uint32_t S16_KTILE = 8 * S16_KTHREADS;  // keys only: one 16-byte load per thread; ranges and fill slices are multiples of it
constexpr uint32_t S16_KUNROLL = 4;               // loads in flight per thread of the histogram
constexpr uint32_t S16_KCAP = 128;                // most ranges of the histogram (two workgroups each: one per CU of a 256-CU device)
constexpr uint32_t S16_PTHREADS = PASS_THREADS, S16_PKPT = PASS_KPT, S16_PTILE = PASS_TILE;  // pairs: the pass's tile
constexpr uint32_t S16_PCAP = 512;                       // most ranges of a pass: table and bases are S16_PCAP x 256 words each
constexpr uint32_t S16C_STATUS = 0, S16C_WORDS = 64;     // the handle's control block
constexpr uint32_t S16_ST_INTERNAL = PASS_ST_INTERNAL;
static_assert(S16_PTHREADS == 512 && S16_PKPT == 8 && S16_PTILE == 4096 && S16_ST_INTERNAL == 1, "the pass's shape and status bit");
static_assert(S16_HALF * 4u <= 160u * 1024u && S16_KTILE % 8u == 0 && S16_PTILE % 8u == 0, "LDS, 16-byte loads");

#if GS_SORT16_BUILT  // (radix_pass.hpp: the product build only)

// eight elements from index i of the 16-byte aligned array q (i a multiple of 8), two to a word; mask: which lie below hi
__device__ __forceinline__ uint4 s16_load8(const uint16_t* __restrict__ q, uint32_t i, uint32_t hi, uint32_t& mask) {
    if (GS_LIKELY(i + 8u <= hi)) {
        mask = 255u;
        return *reinterpret_cast<const uint4*>(q + i);
    }
    uint32_t e[4] = {0u, 0u, 0u, 0u};
    mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (i + j < hi) {
            e[j >> 1] |= (uint32_t)q[i + j] << ((j & 1u) * 16u);
            mask |= 1u << j;
        }
    }
    return uint4{e[0], e[1], e[2], e[3]};
}

__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v = v > t ? v : t;
    }
    return v;
}

// The clear in front of a call: `count` 16-byte groups from p (the control block; keys only: the histogram behind it as well).  A
// kernel, not a memset: every node of a captured call is a kernel launch, like the rest of the library's capturable paths.
__global__ __launch_bounds__(256) void s16_clear_kernel(uint4* __restrict__ p, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) p[i] = uint4{0u, 0u, 0u, 0u};
}

// ---- keys only ----------------------------------------------------------------------------------------------------------------------
// Workgroup 2 r + h counts the keys of range r that fall into half h of the bin space, on 32 768 plain 32-bit LDS counters (nothing
// can wrap), and adds its non-zero counters to the global histogram.  bin = sortable bits ^ flip (flip = 0xFFFF: descending).  A wave
// whose 512 keys share one bin (constant or sorted input) makes one add.
__global__ __launch_bounds__(S16_KTHREADS) void s16_hist_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t per_range, uint32_t kt,
                                                                uint32_t flip, uint32_t* __restrict__ ghist) {
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[S16_HALF];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t range = blockIdx.x >> 1, half = blockIdx.x & 1u;
    for (uint32_t i = tid; i < S16_HALF / 4u; i += S16_KTHREADS) reinterpret_cast<uint4*>(s_cnt)[i] = uint4{0u, 0u, 0u, 0u};
    __syncthreads();
    const uint32_t lo = range * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    for (uint32_t c0 = lo; c0 < hi; c0 += S16_KUNROLL * S16_KTILE) {
        uint4 t[S16_KUNROLL];
        uint32_t mask[S16_KUNROLL];
#pragma unroll
        for (uint32_t u = 0; u < S16_KUNROLL; ++u) {
            const uint32_t i = c0 + u * S16_KTILE + tid * 8u;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (i < hi) t[u] = s16_load8(keys, i, hi, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < S16_KUNROLL; ++u) {
            if (c0 + u * S16_KTILE >= hi) break;  // (uniform)
            const uint32_t w4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            uint32_t d[8], m = 0;
            bool one = true;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                d[j] = tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip;  // (< S16_BINS)
                if (((mask[u] >> j) & 1u) && (d[j] >> 15) == half) m |= 1u << j;
                one = one && d[j] == d[0];
            }
            const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
            if (__builtin_amdgcn_ballot_w64(mask[u] == 255u && one && d[0] == f) == ~0ull) {
                if (lane == 0 && (f >> 15) == half) atomicAdd(&s_cnt[f & (S16_HALF - 1u)], 512u);
                continue;
            }
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                if ((m >> j) & 1u) atomicAdd(&s_cnt[d[j] & (S16_HALF - 1u)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < S16_HALF; i += S16_KTHREADS) {
        const uint32_t c = s_cnt[i];
        if (c != 0u) atomicAdd(&ghist[half * S16_HALF + i], c);
    }
}

// One workgroup: prefix[b] = keys in bins below b, prefix[65 536] = their total, which must be n.
__global__ __launch_bounds__(S16_KTHREADS) void s16_scan_kernel(const uint32_t* __restrict__ ghist, uint32_t* __restrict__ prefix, uint32_t n,
                                                                uint32_t* __restrict__ ctl) {
    constexpr uint32_t PER = S16_BINS / S16_KTHREADS, W = S16_KTHREADS / 64;  // 64 bins per thread
    __shared__ uint32_t s_w[W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4* src = reinterpret_cast<const uint4*>(ghist + tid * PER);
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER / 4u; ++i) {
        const uint4 c = src[i];
        sum += c.x + c.y + c.z + c.w;
    }
    const uint32_t incl = wave_inclusive_scan(sum, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum, total = 0;
    for (uint32_t x = 0; x < W; ++x) {
        if (x < wave) run += s_w[x];
        total += s_w[x];
    }
    uint4* dst = reinterpret_cast<uint4*>(prefix + tid * PER);
#pragma unroll
    for (uint32_t i = 0; i < PER / 4u; ++i) {
        const uint4 c = src[i];
        uint4 p;
        p.x = run;
        p.y = p.x + c.x;
        p.z = p.y + c.y;
        p.w = p.z + c.z;
        run = p.w + c.w;
        dst[i] = p;
    }
    if (tid == 0) {
        prefix[S16_BINS] = total;
        if (total != n) atomicOr(&ctl[S16C_STATUS], S16_ST_INTERNAL);
    }
}

// Workgroup b owns the outputs [b * S16_KTILE, ...): it finds its first and last bin by binary search in the prefix, drops each
// non-empty bin's number at the bin's first output inside the slice, propagates the numbers with a max-scan (bins rise with the
// position) and writes the keys the numbers stand for: O(outputs + bins it spans).
__global__ __launch_bounds__(S16_KTHREADS) void s16_fill_kernel(uint16_t* __restrict__ out, const uint32_t* __restrict__ prefix, uint32_t n, uint32_t kt,
                                                                uint32_t flip, uint32_t* __restrict__ ctl) {
    constexpr uint32_t W = S16_KTHREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_bin[S16_KTILE];
    __shared__ uint32_t s_w[W], s_fl[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t start = blockIdx.x * S16_KTILE;
    if (start >= n || prefix[S16_BINS] != n) return;  // (uniform; a histogram that does not add up was reported by the scan: nothing is written)
    const uint32_t m = n - start < S16_KTILE ? n - start : S16_KTILE;
    reinterpret_cast<uint4*>(s_bin)[tid] = uint4{0u, 0u, 0u, 0u};
    reinterpret_cast<uint4*>(s_bin)[tid + S16_KTHREADS] = uint4{0u, 0u, 0u, 0u};
    if (tid < 2) {  // the bin that holds output `target`: the last one whose prefix is <= target
        const uint32_t target = tid == 0 ? start : start + m - 1u;
        uint32_t lo = 0, hi = S16_BINS + 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (prefix[mid] <= target) lo = mid + 1u; else hi = mid;
        }
        s_fl[tid] = lo - 1u;  // (prefix[0] = 0 <= target < n = prefix[65 536]: 0 <= lo - 1 <= 65 535)
    }
    __syncthreads();
    const uint32_t first = s_fl[0], last = s_fl[1];
    if (first > last || last >= S16_BINS) {  // (uniform)
        if (tid == 0) atomicOr(&ctl[S16C_STATUS], S16_ST_INTERNAL);
        return;
    }
    if (tid == 0) s_bin[0] = first;
    for (uint32_t b = first + 1u + tid; b <= last; b += S16_KTHREADS) {
        const uint32_t p = prefix[b];
        if (prefix[b + 1u] > p) {  // non-empty: it starts inside the slice, behind its first output
            const uint32_t off = p - start;
            if (off < m) s_bin[off] = b; else atomicOr(&ctl[S16C_STATUS], S16_ST_INTERNAL);
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

// ---- pairs and argsort ----------------------------------------------------------------------------------------------------------------
// The three kernels of a pass are pass_count16_body, pass_scan_body and pass_scatter_body (radix_pass.hpp) with the whole array as
// the one row and range r = [r * per_range, ...) as its part r.

// table[r][d] = keys of range r whose byte at `shift` of the sortable bits is d.  keys is 16-byte aligned and per_range a multiple of
// the tile, so the body's peel is 0.
__global__ __launch_bounds__(S16_PTHREADS) void s16_count_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t per_range, uint32_t kt,
                                                                 uint32_t shift, uint32_t* __restrict__ table) {
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    pass_count16_body(keys + lo, hi - lo, kt, shift, table + blockIdx.x * RADIX);
}

// One workgroup: bases[r][d] = keys with a digit below d + keys of digit d in the ranges in front of r; the total must be n.
__global__ __launch_bounds__(RADIX) void s16_pscan_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ bases, uint32_t ranges, uint32_t n,
                                                          uint32_t* __restrict__ ctl) {
    pass_scan_body(table, bases, ranges, n, ctl + S16C_STATUS);
}

// One workgroup per range, its tiles in order.  VM: 1 = the value is the element's input position (argsort, first pass: made in
// registers, 4 bytes), 4 / 8 = values of that width.  reverse != 0 (descending, last pass): position p goes to n - 1 - p.  As on
// the other routes of the pass, a scatter that finds the status word set (s16_pscan_kernel: the counts did not add up) writes nothing.
template <int VM, int RANK>
__global__ __launch_bounds__(S16_PTHREADS) void s16_scatter_kernel(const uint16_t* __restrict__ kin, const void* __restrict__ vin_, uint16_t* __restrict__ kout,
                                                                   void* __restrict__ vout_, uint32_t n, uint32_t per_range, uint32_t kt, uint32_t shift,
                                                                   uint32_t reverse, const uint32_t* __restrict__ bases, uint32_t* __restrict__ ctl) {
    using V = typename S16Val<VM>::type;
    const uint32_t lo = blockIdx.x * per_range;
    const uint32_t hi = lo < n ? (n - lo < per_range ? n : lo + per_range) : lo;
    pass_scatter_body<uint16_t, VM, RANK>(kin, static_cast<const V*>(vin_), kout, static_cast<V*>(vout_), n, lo, hi, 0u, kt, shift, reverse,
                                          bases + blockIdx.x * RADIX, ctl + S16C_STATUS);
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
