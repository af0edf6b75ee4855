// merge_kernels.hpp — the stable merge of two sorted arrays into one: keys, pairs or positions: gs_merge_* of include/gpusort.h.  No
// counterpart in the reference project.
//
// Everything runs on the order-preserving word of a key (ss_word of search_kernels.hpp), inverted for a descending order, so that the six
// key types and both orders are ONE unsigned merge; among equal words A's elements come in front of B's.  The kernel body is written once
// over the key word K (uint32_t, uint64_t).
//   mg_tile_kernel   one workgroup per tile of T consecutive OUTPUTS [d0, d1).  Wave 0 finds the merge-path split of diagonal d0 and
//                    wave 1 that of d1, each by a 64-way search (one probe of A and one of B per lane and step); the tile then merges
//                    A[a0 .. a1) and B[b0 .. b1), (a1 - a0) + (b1 - b0) = d1 - d0.  Both pieces are staged into one LDS array as words;
//                    thread k finds the split of its own diagonal k * VT there and makes VT serial merge steps with the words and their
//                    LDS indices in registers; the words go back into LDS in output order and leave through 16-byte stores, the
//                    indices likewise: a pairs call gathers each value through its index (two ascending streams per tile), a positions
//                    call stores the index as a position in [A; B].  A tile that lies wholly in one input is a copy.
//   mg_reset_kernel  zeroes the control block: MGC_SHARDS pairs of counters, each pair on a 128-byte line of its own.  One counter that
//                    every tile adds to is the whole kernel's time at 2^28 keys (65 536 adds to one address at about 12 ns each: measured,
//                    DESIGN.md 3.27), so tile t adds to shard t % MGC_SHARDS and gs_merge_last sums the shards.
//
// The order of the inputs is not checked.  Whatever the keys hold: a diagonal's search interval shrinks with every step whatever the
// probes say, and its answer lies in [max(0, d - nb), min(d, na)]; the tile's splits are then clamped to a0 <= a1 <= na, b0 <= b1 <= nb,
// (a1 - a0) + (b1 - b0) = d1 - d0 <= T, and every later bound follows from these: the LDS search runs a number of steps fixed by the two
// lengths and answers inside its interval, every merge step is guarded by ia < ca and ib < cb and consumes exactly one of the
// (ca - ia) + (cb - ib) >= steps elements in front of it, every LDS index is below ca + cb, every input index below na or nb, every
// position below na + nb, and thread k writes the output slots [d0 + k * VT, d0 + (k + 1) * VT) below d1 and no other: every slot of
// [0, na + nb) exactly once, nothing at or behind na + nb.  No kernel waits on another workgroup; the only atomics are the counters of
// the control block.  Registers, LDS and scratch per kernel: DESIGN.md 3.27.
#pragma once
#include "search_kernels.hpp"  // GS_SORT16_BUILT, ss_word, ss_load16 / ss_store16

#ifndef GS_MG_TILE
#define GS_MG_TILE 8192  // outputs per workgroup on 4-byte keys (measured against 2048 and 4096: DESIGN.md 3.27)
#endif
#ifndef GS_MG_TILE64
#define GS_MG_TILE64 4096  // ... on 8-byte keys (measured against 2048 and 8192)
#endif

namespace gs {

constexpr uint32_t MG_THREADS = 512;
constexpr uint32_t MG_KEYS = 0, MG_PAIRS4 = 1, MG_PAIRS8 = 2, MG_POSITIONS = 3;  // the kernel forms
// the handle's control block: shard s holds its two counters at words s * MGC_STRIDE + MGC_TILES / MGC_COPY_TILES
constexpr uint32_t MGC_TILES = 0, MGC_COPY_TILES = 1, MGC_SHARDS = 32, MGC_STRIDE = 32, MGC_WORDS = MGC_SHARDS * MGC_STRIDE;
template <class K>
struct MgShape {
    static constexpr uint32_t T = sizeof(K) == 8 ? GS_MG_TILE64 : GS_MG_TILE, VT = T / MG_THREADS;
    static_assert(T % MG_THREADS == 0 && VT >= 4 && VT <= 16 && VT % 4 == 0, "whole 16-byte pieces per thread; LDS indices on 16 bits");
};
static_assert((MGC_SHARDS & (MGC_SHARDS - 1u)) == 0 && MGC_STRIDE * 4u == 128u && MGC_WORDS == 1024u, "a 128-byte line per shard; mg_reset_kernel: one thread per word");

#if GS_SORT16_BUILT  // the product build only, as the search kernels

__device__ __forceinline__ uint32_t mg_unword(uint32_t w, uint32_t kt, uint32_t flip) {
    w ^= flip;
    return kt == KEY_I32 ? from_bits<KEY_I32>(w) : kt == KEY_F32 ? from_bits<KEY_F32>(w) : w;
}
__device__ __forceinline__ uint64_t mg_unword(uint64_t w, uint32_t kt, uint64_t flip) {
    w ^= flip;
    uint2 k{(uint32_t)w, (uint32_t)(w >> 32)};
    k = kt == KEY_I64 ? from_bits2<KEY_I64>(k) : kt == KEY_F64 ? from_bits2<KEY_F64>(k) : k;
    return (uint64_t)k.x | ((uint64_t)k.y << 32);
}

__global__ __launch_bounds__(1024) void mg_reset_kernel(uint32_t* __restrict__ ctl) { ctl[threadIdx.x] = 0u; }

// The merge-path split of diagonal d <= na + nb: max(0, d - nb) + the number of a in [max(0, d - nb), min(d, na)) with
// word(A[a]) <= word(B[d - 1 - a]): on sorted inputs the smallest a for which that is false (A first on ties).  All 64 lanes of a wave
// call this with the same arguments.  Every a probed lies in [max(0, d - nb), min(d, na)): a < na and 0 <= d - 1 - a < nb.  The steps
// are ss_wave_bound's: the interval shrinks from len to less than len / 64 + 1 whatever the probes say.
template <class K>
__device__ __forceinline__ uint32_t mg_wave_split(const K* __restrict__ A, uint32_t na, const K* __restrict__ B, uint32_t nb, uint32_t d, uint32_t kt,
                                                  K flip, uint32_t lane) {
    uint32_t lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;  // lo <= hi: d <= na + nb
    while (hi - lo > 64u) {
        const uint32_t stride = (hi - lo + 63u) / 64u;  // >= 2
        const uint32_t p = lo + lane * stride + (stride - 1u);
        const bool in = p < hi;
        const K wa = ss_word(in ? A[p] : (K)0, kt, flip), wb = ss_word(in ? B[d - 1u - p] : (K)0, kt, flip);
        const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in && wa <= wb));
        uint32_t nlo = lo + c * stride;
        nlo = nlo < hi ? nlo : hi;
        hi = hi - nlo < stride - 1u ? hi : nlo + stride - 1u;
        lo = nlo;
    }
    const uint32_t p = lo + lane;
    const bool in = p < hi;
    const K wa = ss_word(in ? A[p] : (K)0, kt, flip), wb = ss_word(in ? B[d - 1u - p] : (K)0, kt, flip);
    return lo + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in && wa <= wb));
}

// The same for one thread in LDS: s[0 .. ca) holds A's words and s[ca .. ca + cb) B's; the split of diagonal d <= ca + cb in
// [max(0, d - cb), min(d, ca)].  ceil(log2(len)) + 1 steps whatever the words hold, no branch (the shape of ss_lds_bound).
template <class K>
__device__ __forceinline__ uint32_t mg_lds_split(const K* s, uint32_t ca, uint32_t cb, uint32_t d) {
    const uint32_t lo = d > cb ? d - cb : 0u, hi = d < ca ? d : ca;
    const uint32_t across = ca + d - 1u;  // s[across - a]: B's word across the diagonal from A's a-th; lo <= a < hi: ca <= across - a < ca + cb
    uint32_t base = lo;
    for (uint32_t l = hi - lo; l > 1u;) {
        const uint32_t half = l >> 1, a = base + half - 1u;  // lo <= a < hi
        base += s[a] <= s[across - a] ? half : 0u;
        l -= half;
    }
    return base + ((hi != lo && s[base] <= s[across - base]) ? 1u : 0u);  // (base < hi here)
}

// the 16-byte piece of values / positions at output j of the tile: V-byte elements, index -> element by f
template <class V, class F>
__device__ __forceinline__ void mg_store_indexed(V* __restrict__ out, uint32_t j, uint32_t cnt, F f) {
    constexpr uint32_t PERV = 16u / sizeof(V);
    if (GS_LIKELY(j + PERV <= cnt)) {
        V v[PERV];
#pragma unroll
        for (uint32_t x = 0; x < PERV; ++x) v[x] = f(j + x);
        ss_store16(out + j, v);
    } else {
        for (uint32_t x = 0; x < PERV; ++x)
            if (j + x < cnt) out[j + x] = f(j + x);
    }
}

// One workgroup per tile of T outputs out[d0 .. d1) of the merge of A[0 .. na) and B[0 .. nb).  FORM: MG_KEYS; MG_PAIRS4 / MG_PAIRS8:
// out_aux holds the values (4 / 8 bytes) of a_vals / b_vals; MG_POSITIONS: out_aux holds uint32 positions in [A; B].
template <class K, uint32_t FORM>
__global__ __launch_bounds__(MG_THREADS) void mg_tile_kernel(const K* __restrict__ A, uint32_t na, const K* __restrict__ B, uint32_t nb,
                                                             K* __restrict__ out, const void* __restrict__ a_vals, const void* __restrict__ b_vals,
                                                             void* __restrict__ out_aux, uint32_t kt, uint32_t descending, uint32_t* __restrict__ ctl) {
    constexpr uint32_t T = MgShape<K>::T, VT = MgShape<K>::VT, PER = 16u / sizeof(K);
    constexpr bool INDEXED = FORM != MG_KEYS;
    __shared__ __attribute__((aligned(16))) K s_key[T];
    __shared__ __attribute__((aligned(16))) uint16_t s_idx[INDEXED ? T : 8];  // the LDS index of every output (T <= 8192)
    __shared__ uint32_t s_split[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const K flip = descending ? ~(K)0 : (K)0;
    const uint32_t n = na + nb;  // <= GS_MAX_KEYS
    const uint32_t d0 = blockIdx.x * T;
    if (d0 >= n) return;  // (uniform)
    const uint32_t d1 = n - d0 < T ? n : d0 + T, cnt = d1 - d0;
    if (wave < 2u) {  // wave 0: the split of d0; wave 1: of d1
        const uint32_t a = mg_wave_split(A, na, B, nb, wave == 0u ? d0 : d1, kt, flip, lane);
        if (lane == 0u) s_split[wave] = a;
    }
    __syncthreads();
    // a0 in [max(0, d0 - nb), min(d0, na)] by the search; the clamp gives a0 <= a1 <= na, b0 <= b1 <= nb, ca + cb = cnt on any input
    const uint32_t a0 = s_split[0], b0 = d0 - a0;
    uint32_t a1 = s_split[1] < a0 ? a0 : s_split[1];
    a1 = a1 - a0 < cnt ? a1 : a0 + cnt;
    const uint32_t ca = a1 - a0, cb = cnt - ca;
    const bool copy = ca == 0u || cb == 0u;  // (uniform) the tile lies wholly in one input: its words are in output order as staged
    if (tid == 0u) {
        uint32_t* shard = ctl + (blockIdx.x & (MGC_SHARDS - 1u)) * MGC_STRIDE;
        atomicAdd(&shard[MGC_TILES], 1u);
        if (copy) atomicAdd(&shard[MGC_COPY_TILES], 1u);
    }
    // ---- stage A[a0 .. a1) into s_key[0 .. ca) and B[b0 .. b1) into s_key[ca .. cnt): aligned 16-byte loads, the words flipped once ----
#pragma unroll
    for (uint32_t side = 0; side < 2u; ++side) {
        const K* __restrict__ src = side == 0u ? A : B;
        const uint32_t g0 = side == 0u ? a0 : b0, len = side == 0u ? ca : cb, ns = side == 0u ? na : nb;
        K* dst = s_key + (side == 0u ? 0u : ca);
        const uint32_t first = g0 & ~(PER - 1u);                    // the piece that holds src[g0]
        const uint32_t pieces = len == 0u ? 0u : (g0 + len - first + PER - 1u) / PER;  // <= T / PER + 1
        for (uint32_t c = tid; c < pieces; c += MG_THREADS) {
            const uint32_t g = first + c * PER;
            K v[PER];
            if (GS_LIKELY(g + PER <= ns)) {
                ss_load16(src + g, v);
            } else {
#pragma unroll
                for (uint32_t x = 0; x < PER; ++x) v[x] = g + x < ns ? src[g + x] : (K)0;
            }
#pragma unroll
            for (uint32_t x = 0; x < PER; ++x) {
                const uint32_t at = g + x - g0;  // (wraps below g0: not < len)
                if (at < len) dst[at] = ss_word(v[x], kt, flip);
            }
        }
    }
    __syncthreads();
    if (!copy) {
        // ---- thread k: outputs [k * VT, (k + 1) * VT) of the tile ----
        const uint32_t diag = tid * VT < cnt ? tid * VT : cnt;
        const uint32_t steps = cnt - diag < VT ? cnt - diag : VT;
        uint32_t ia = mg_lds_split(s_key, ca, cb, diag), ib = diag - ia;  // ia <= ca, ib <= cb, (ca - ia) + (cb - ib) = cnt - diag >= steps
        K w[VT];
        uint32_t idx[VT];
        K ka = ia < ca ? s_key[ia] : (K)0, kb = ib < cb ? s_key[ca + ib] : (K)0;
#pragma unroll
        for (uint32_t i = 0; i < VT; ++i) {
            const bool has_a = ia < ca, has_b = ib < cb;
            const bool take_a = has_a && (!has_b || ka <= kb);  // one of the two is there while i < steps
            w[i] = take_a ? ka : kb;
            idx[i] = take_a ? ia : ca + ib;
            ia += take_a ? 1u : 0u;
            ib += take_a ? 0u : (has_b ? 1u : 0u);
            const uint32_t nx = take_a ? ia : ca + ib;          // the next word of the side that moved
            const bool there = take_a ? ia < ca : ib < cb;
            const K nw = there ? s_key[nx] : (K)0;
            ka = take_a ? nw : ka;
            kb = take_a ? kb : nw;
        }
        __syncthreads();  // every search and merge step has read s_key
#pragma unroll
        for (uint32_t i = 0; i < VT; i += PER) {
            if (i < steps) {  // (steps > i: the piece's first slot is below cnt; the slots behind cnt, below T, are never read)
                K v[PER];
#pragma unroll
                for (uint32_t x = 0; x < PER; ++x) v[x] = w[i + x];
                ss_store16(s_key + diag + i, v);
            }
        }
        if (INDEXED) {
#pragma unroll
            for (uint32_t i = 0; i < VT; ++i)
                if (i < steps) s_idx[diag + i] = (uint16_t)idx[i];
        }
        __syncthreads();
    }
    // ---- write: the keys un-flipped through 16-byte stores (out + d0 is 16-byte aligned: T is a multiple of 4) ----
    for (uint32_t j = tid * PER; j < cnt; j += MG_THREADS * PER) {
        K v[PER];
        ss_load16(s_key + j, v);
        if (GS_LIKELY(j + PER <= cnt)) {
#pragma unroll
            for (uint32_t x = 0; x < PER; ++x) v[x] = mg_unword(v[x], kt, flip);
            ss_store16(out + d0 + j, v);
        } else {
            for (uint32_t x = 0; x < PER; ++x)
                if (j + x < cnt) out[d0 + j + x] = mg_unword(v[x], kt, flip);
        }
    }
    if (INDEXED) {
        // the LDS index of output j: below ca it is A's element a0 + index, else B's element b0 + index - ca
        const auto index_of = [&](uint32_t j) -> uint32_t { return copy ? j : (uint32_t)s_idx[j]; };
        if (FORM == MG_POSITIONS) {
            uint32_t* __restrict__ o = static_cast<uint32_t*>(out_aux) + d0;
            for (uint32_t j = tid * 4u; j < cnt; j += MG_THREADS * 4u)
                mg_store_indexed(o, j, cnt, [&](uint32_t jj) -> uint32_t {
                    const uint32_t x = index_of(jj);
                    return x < ca ? a0 + x : na + b0 + (x - ca);
                });
        } else if (FORM == MG_PAIRS4) {
            const uint32_t *__restrict__ av = static_cast<const uint32_t*>(a_vals), *__restrict__ bv = static_cast<const uint32_t*>(b_vals);
            uint32_t* __restrict__ o = static_cast<uint32_t*>(out_aux) + d0;
            for (uint32_t j = tid * 4u; j < cnt; j += MG_THREADS * 4u)
                mg_store_indexed(o, j, cnt, [&](uint32_t jj) -> uint32_t {
                    const uint32_t x = index_of(jj);
                    return x < ca ? av[a0 + x] : bv[b0 + (x - ca)];
                });
        } else {
            const uint64_t *__restrict__ av = static_cast<const uint64_t*>(a_vals), *__restrict__ bv = static_cast<const uint64_t*>(b_vals);
            uint64_t* __restrict__ o = static_cast<uint64_t*>(out_aux) + d0;
            for (uint32_t j = tid * 2u; j < cnt; j += MG_THREADS * 2u)
                mg_store_indexed(o, j, cnt, [&](uint32_t jj) -> uint64_t {
                    const uint32_t x = index_of(jj);
                    return x < ca ? av[a0 + x] : bv[b0 + (x - ca)];
                });
        }
    }
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
