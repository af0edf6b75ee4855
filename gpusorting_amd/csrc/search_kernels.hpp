// search_kernels.hpp — sorted search: the lower / upper bound of many queries in a sorted array: gs_search_* of include/gpusort.h.  No
// counterpart in the reference project.
//
// Everything runs on the order-preserving word of a key (to_bits / to_bits2 of onesweep_kernels.hpp), inverted for a descending
// haystack, so that the six key types, both orders and both sides are ONE unsigned bound: the position of query q is the number of
// haystack words h with h < q (LEFT) or h <= q (RIGHT).  The kernel bodies are written once over the key word K (uint32_t, uint64_t).
//   ss_tile_kernel          queries in order: one workgroup per tile of SS_TILE queries.  Wave 0 finds the LEFT bound of the tile's first
//                           query and wave 1 the RIGHT bound of its last one, each by a 64-way search of the whole haystack (one probe
//                           per lane and step: five dependent loads for 2^30 keys); the window [lo, hi) between them holds every
//                           answer of the tile.  A window of at most W keys is staged into LDS as words, with 16-byte loads, and
//                           every query is answered by a branch-free binary search there; a wider one (sparse queries) is searched
//                           in global memory, one thread per query, narrowed to [lo, hi].  SCATTER: the queries are the engine's
//                           sorted copy and out is stored through their positions (GS_SEARCH_ROUTE_SORT).
//   ss_sample_kernel        every S-th key of the haystack, as words, into the sample table of the workspace.
//   ss_binary_table_kernel  queries in any order: a workgroup stages the sample table once and serves queries in a grid-stride loop: the
//                           samples in LDS, then the S - 1 keys between two samples in global memory.
//   ss_binary_plain_kernel  one thread per query, every level in global memory.
//   ss_reset_kernel         zeroes the control block's counters.
//
// The haystack's order is not checked.  Whatever the keys hold: every loop is bounded by the sizes (a search interval shrinks with every
// step whatever the comparison says; the LDS search runs a number of steps fixed by the window's length), every haystack index is
// below n, every window is clamped to lo <= hi <= n, every position written is <= n, and a scattered store checks its position
// against m.  No kernel waits on another workgroup.  Registers, LDS and scratch per kernel: DESIGN.md 3.25.
#pragma once
#include "unique_kernels.hpp"  // GS_SORT16_BUILT, uq_prepare_kernel (the copy of the queries and their positions in front of the sort)

#ifndef GS_SS_TILE
#define GS_SS_TILE 2048  // queries per workgroup of the tile kernel (measured against 1024: DESIGN.md 3.25)
#endif
#ifndef GS_SS_WINDOW_BYTES
#define GS_SS_WINDOW_BYTES 32768  // the tile kernel's window in LDS: four workgroups share a CU (measured against 65536: DESIGN.md 3.25)
#endif

namespace gs {

constexpr uint32_t SS_THREADS = 512, SS_TILE = GS_SS_TILE, SS_QPT = SS_TILE / SS_THREADS;
constexpr uint32_t SS_WINDOW_BYTES = GS_SS_WINDOW_BYTES;
constexpr uint32_t SS_SAMPLE_BYTES = 65536;  // the sample table: what one workgroup of the table kernel stages
constexpr uint32_t SS_TABLE_GRID = 512;      // most workgroups of the table kernel: each stages the table once
constexpr uint32_t SS_PLAIN_THREADS = 256, SS_SAMPLE_THREADS = 256;
// the handle's control block
constexpr uint32_t SSC_LDS_TILES = 0, SSC_GLOBAL_TILES = 1, SSC_WORDS = 64;
static_assert(SS_TILE % SS_THREADS == 0 && SS_QPT >= 1 && SS_QPT <= 8, "whole rounds of the workgroup");
static_assert(SS_WINDOW_BYTES % 16u == 0 && SS_WINDOW_BYTES >= 1024 && SS_WINDOW_BYTES <= 65536, "the window is staged in 16-byte pieces");

#if GS_SORT16_BUILT  // the product build only, as the unique kernels

// the order-preserving word of a key of type kt (0 .. 2 on 4 bytes, 3 .. 5 on 8), inverted by flip = ~0 for a descending haystack
__device__ __forceinline__ uint32_t ss_word(uint32_t u, uint32_t kt, uint32_t flip) {
    return (kt == KEY_I32 ? to_bits<KEY_I32>(u) : kt == KEY_F32 ? to_bits<KEY_F32>(u) : u) ^ flip;
}
__device__ __forceinline__ uint64_t ss_word(uint64_t u, uint32_t kt, uint64_t flip) {
    uint2 k{(uint32_t)u, (uint32_t)(u >> 32)};
    k = kt == KEY_I64 ? to_bits2<KEY_I64>(k) : kt == KEY_F64 ? to_bits2<KEY_F64>(k) : k;
    return ((uint64_t)k.x | ((uint64_t)k.y << 32)) ^ flip;
}
// does haystack word h lie in front of the position of query word q
template <class K>
__device__ __forceinline__ bool ss_before(K h, K q, uint32_t right) { return right ? h <= q : h < q; }

// the 16 / sizeof(K) keys of one 16-byte piece
__device__ __forceinline__ void ss_load16(const uint32_t* p, uint32_t (&v)[4]) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void ss_load16(const uint64_t* p, uint64_t (&v)[2]) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    v[0] = (uint64_t)a.x | ((uint64_t)a.y << 32);
    v[1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
}
__device__ __forceinline__ void ss_store16(uint32_t* p, const uint32_t (&v)[4]) { *reinterpret_cast<uint4*>(p) = uint4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void ss_store16(uint64_t* p, const uint64_t (&v)[2]) {
    *reinterpret_cast<uint4*>(p) = uint4{(uint32_t)v[0], (uint32_t)(v[0] >> 32), (uint32_t)v[1], (uint32_t)(v[1] >> 32)};
}

// lo + the number of keys of hay[lo .. hi) in front of q's position; hi <= n.  All 64 lanes of a wave call this with the same
// arguments.  A step probes 64 evenly spaced keys and keeps the piece between the last probe in front and the first one behind: the
// interval shrinks from len to less than len / 64 + 1 whatever the probes say, so 2^30 keys take four steps and the last look.
template <class K>
__device__ __forceinline__ uint32_t ss_wave_bound(const K* __restrict__ hay, uint32_t lo, uint32_t hi, K q, uint32_t right, uint32_t kt, K flip,
                                                  uint32_t lane) {
    while (hi - lo > 64u) {
        const uint32_t stride = (hi - lo + 63u) / 64u;  // >= 2
        const uint32_t p = lo + lane * stride + (stride - 1u);
        const bool t = p < hi && ss_before(ss_word(p < hi ? hay[p] : (K)0, kt, flip), q, right);
        const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(t));
        uint32_t nlo = lo + c * stride;
        nlo = nlo < hi ? nlo : hi;
        hi = hi - nlo < stride - 1u ? hi : nlo + stride - 1u;
        lo = nlo;
    }
    const bool t = lo + lane < hi && ss_before(ss_word(lo + lane < hi ? hay[lo + lane] : (K)0, kt, flip), q, right);
    return lo + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(t));
}

// the same for one thread of its own: a binary search of hay[lo .. hi), lo <= hi <= n; the answer lies in [lo, hi]
template <class K>
__device__ __forceinline__ uint32_t ss_thread_bound(const K* __restrict__ hay, uint32_t lo, uint32_t hi, K q, uint32_t right, uint32_t kt, K flip) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ss_before(ss_word(hay[mid], kt, flip), q, right)) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the number of words of s[0 .. len) in front of q's position, in LDS: ceil(log2(len)) + 1 steps whatever the words hold, no branch
template <class K>
__device__ __forceinline__ uint32_t ss_lds_bound(const K* s, uint32_t len, K q, uint32_t right) {
    uint32_t base = 0;
    for (uint32_t l = len; l > 1u;) {
        const uint32_t half = l >> 1;
        base += ss_before(s[base + half - 1u], q, right) ? half : 0u;
        l -= half;
    }
    return base + ((len != 0u && ss_before(s[base], q, right)) ? 1u : 0u);
}

__global__ __launch_bounds__(64) void ss_reset_kernel(uint32_t* __restrict__ ctl) { ctl[threadIdx.x] = 0u; }
static_assert(SSC_WORDS == 64, "ss_reset_kernel: one thread per control word");

// One workgroup per tile of SS_TILE queries q[q0 .. q1), which are in order.  SCATTER: out[pos[j]], else out[j].
template <class K, bool SCATTER>
__global__ __launch_bounds__(SS_THREADS) void ss_tile_kernel(const K* __restrict__ hay, uint32_t n, const K* __restrict__ q,
                                                             const uint32_t* __restrict__ pos, uint32_t m, uint32_t* __restrict__ out, uint32_t kt,
                                                             uint32_t descending, uint32_t right, uint32_t* __restrict__ ctl) {
    constexpr uint32_t PER = 16u / sizeof(K), W = SS_WINDOW_BYTES / sizeof(K);
    __shared__ __attribute__((aligned(16))) K s_win[W + PER];  // from the 16-byte piece that holds hay[lo]
    __shared__ uint32_t s_b[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const K flip = descending ? ~(K)0 : (K)0;
    const uint32_t q0 = blockIdx.x * SS_TILE;
    if (q0 >= m) return;  // (uniform)
    const uint32_t q1 = m - q0 < SS_TILE ? m : q0 + SS_TILE;
    if (wave < 2u) {  // wave 0: LEFT of the first query; wave 1: RIGHT of the last
        const K qq = ss_word(q[wave == 0u ? q0 : q1 - 1u], kt, flip);
        const uint32_t b = ss_wave_bound(hay, 0u, n, qq, wave, kt, flip, lane);
        if (lane == 0u) s_b[wave] = b;
    }
    __syncthreads();
    const uint32_t lo = s_b[0] < n ? s_b[0] : n;
    const uint32_t hi = s_b[1] < lo ? lo : (s_b[1] < n ? s_b[1] : n);  // lo <= hi <= n, whatever the keys hold
    const bool in_lds = hi - lo <= W;                                   // (uniform)
    const uint32_t a0 = lo & ~(PER - 1u);
    if (in_lds) {
        const uint32_t pieces = (hi - a0 + PER - 1u) / PER;  // <= W / PER + 1
        for (uint32_t c = tid; c < pieces; c += SS_THREADS) {
            const uint32_t g = a0 + c * PER;
            K v[PER];
            if (GS_LIKELY(g + PER <= n)) {
                ss_load16(hay + g, v);
            } else {
#pragma unroll
                for (uint32_t x = 0; x < PER; ++x) v[x] = g + x < n ? hay[g + x] : (K)0;
            }
#pragma unroll
            for (uint32_t x = 0; x < PER; ++x) v[x] = ss_word(v[x], kt, flip);
            ss_store16(s_win + c * PER, v);
        }
        __syncthreads();
    }
    if (tid == 0u) atomicAdd(&ctl[in_lds ? SSC_LDS_TILES : SSC_GLOBAL_TILES], 1u);
    const K* win = s_win + (lo - a0);
    const uint32_t len = hi - lo;
    uint32_t j[SS_QPT], at[SS_QPT];
    K qw[SS_QPT];
#pragma unroll
    for (uint32_t u = 0; u < SS_QPT; ++u) {
        j[u] = q0 + u * SS_THREADS + tid;
        qw[u] = j[u] < q1 ? ss_word(q[j[u]], kt, flip) : (K)0;
    }
    if (in_lds) {  // the SS_QPT searches of a thread side by side
#pragma unroll
        for (uint32_t u = 0; u < SS_QPT; ++u) at[u] = 0u;
        for (uint32_t l = len; l > 1u;) {
            const uint32_t half = l >> 1;
#pragma unroll
            for (uint32_t u = 0; u < SS_QPT; ++u) at[u] += ss_before(win[at[u] + half - 1u], qw[u], right) ? half : 0u;
            l -= half;
        }
#pragma unroll
        for (uint32_t u = 0; u < SS_QPT; ++u) at[u] += (len != 0u && ss_before(win[at[u]], qw[u], right)) ? 1u : 0u;
#pragma unroll
        for (uint32_t u = 0; u < SS_QPT; ++u) at[u] += lo;
    } else {
#pragma unroll
        for (uint32_t u = 0; u < SS_QPT; ++u) at[u] = j[u] < q1 ? ss_thread_bound(hay, lo, hi, qw[u], right, kt, flip) : lo;
    }
#pragma unroll
    for (uint32_t u = 0; u < SS_QPT; ++u) {
        if (j[u] < q1) {
            if (SCATTER) {
                const uint32_t d = pos[j[u]];
                if (d < m) out[d] = at[u];
            } else {
                out[j[u]] = at[u];
            }
        }
    }
}

// samples[t] = the word of hay[(t + 1) * S - 1], t < ns = n / S
template <class K>
__global__ __launch_bounds__(SS_SAMPLE_THREADS) void ss_sample_kernel(const K* __restrict__ hay, uint32_t n, uint32_t S, uint32_t ns,
                                                                      K* __restrict__ samples, uint32_t kt, uint32_t descending) {
    const uint32_t t = blockIdx.x * SS_SAMPLE_THREADS + threadIdx.x;
    if (t >= ns) return;
    const uint32_t i = (t + 1u) * S - 1u;  // < ns * S <= n
    if (i < n) samples[t] = ss_word(hay[i], kt, descending ? ~(K)0 : (K)0);
}

// Queries in any order.  c samples lie in front of a query: so do the keys up to c * S - 1, and the key of sample c does not: the
// answer lies in [c * S, min(c * S + S - 1, n)].  S == 1: the samples are the haystack and c is the answer.
template <class K>
__global__ __launch_bounds__(SS_THREADS) void ss_binary_table_kernel(const K* __restrict__ hay, uint32_t n, const K* __restrict__ q, uint32_t m,
                                                                     uint32_t* __restrict__ out, const K* __restrict__ samples, uint32_t ns, uint32_t S,
                                                                     uint32_t kt, uint32_t descending, uint32_t right) {
    constexpr uint32_t PER = 16u / sizeof(K), CAP = SS_SAMPLE_BYTES / sizeof(K);
    __shared__ __attribute__((aligned(16))) K s_tab[CAP];
    const uint32_t tid = threadIdx.x;
    const K flip = descending ? ~(K)0 : (K)0;
    const uint32_t cnt = ns < CAP ? ns : CAP;
    for (uint32_t c = tid; c * PER < cnt; c += SS_THREADS) {  // (whole pieces: the table in the workspace has CAP words)
        K v[PER];
        ss_load16(samples + c * PER, v);
        ss_store16(s_tab + c * PER, v);
    }
    __syncthreads();
    for (uint32_t j0 = blockIdx.x * SS_THREADS; j0 < m; j0 += gridDim.x * SS_THREADS) {  // (uniform: m < 2^30)
        const uint32_t j = j0 + tid;
        const K qw = j < m ? ss_word(q[j], kt, flip) : (K)0;
        const uint32_t c = ss_lds_bound(s_tab, cnt, qw, right);
        if (j < m) {
            uint32_t lo = c * S;  // c <= ns: <= n
            lo = lo < n ? lo : n;
            const uint32_t hi = n - lo < S - 1u ? n : lo + (S - 1u);
            out[j] = ss_thread_bound(hay, lo, hi, qw, right, kt, flip);
        }
    }
}

// One thread per query, every level in global memory.
template <class K>
__global__ __launch_bounds__(SS_PLAIN_THREADS) void ss_binary_plain_kernel(const K* __restrict__ hay, uint32_t n, const K* __restrict__ q, uint32_t m,
                                                                           uint32_t* __restrict__ out, uint32_t kt, uint32_t descending,
                                                                           uint32_t right) {
    const uint32_t j = blockIdx.x * SS_PLAIN_THREADS + threadIdx.x;
    if (j >= m) return;
    const K flip = descending ? ~(K)0 : (K)0;
    out[j] = ss_thread_bound(hay, 0u, n, ss_word(q[j], kt, flip), right, kt, flip);
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
