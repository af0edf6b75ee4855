// topk_rows16_kernels.hpp — the row-wise top-k of topk_rows_kernels.hpp on 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16):
// 2-byte elements in d_keys and d_out_keys, read once at their own width instead of being widened to 32 bits by the caller.  No
// counterpart in the reference project.
//
// Same selection space, same rules, same three kernels by row length as the 32-bit file.  The wave and the tile kernel are that
// file's bodies (tkr_wave_row, tkr_tile_row behind tkr_matrix_wave, tkr_matrix_tile) on the key traits TkrKey16 below; what differs:
//   - TkrArgs::keys / out_keys point at 2-byte elements (row_stride, row_len, k and positions keep counting elements; values stay
//     4 or 8 bytes under the same index).  Rows start at 2-byte alignment only; the base pointers are 16-byte aligned.
//   - the sortable 16 bits sit in the low half of the 32-bit word the passes rank, the high half is 0, and only the passes for
//     shift 0 and 8 run (TkrKey16::RANKED_BITS).
//   - tkr16_stream_kernel: 16-byte loads of eight elements behind a scalar peel of up to seven; the radix select is exact after two
//     levels (12 + 4 bits), so a row is read 2 or 3 times, never 4; a tile is 32 768 elements, and its front and equal counts, packed
//     into 16 bits each, stay below 65 536 (asserted).
// tkr16_stream_kernel keeps a body of its own: tkr_stream_row (topk_rows_kernels.hpp) with other constants (8 elements per load, the
// 12 + 4 level schedule, a 16-bit flip mask, mask bits at 8 + j, 512 in the one-add shortcut).  Written as one function of key traits
// and called from a wrapper, the select kept the 32-bit and the segmented kernels' resources but spilled one more SGPR in every
// tkr16_stream_kernel<VM, 0> (VM 0 / 1 / 4 / 8: 100 / 102 / 106 / 106 -> 101 / 103 / 107 / 107, to VGPR lanes, everything else equal),
// with the early-outs in a wrapper in front of the body in whatever form; DESIGN.md 3.17 has the table.  Resources were to stay what
// they were, so a fix to the select belongs in both: there and here — and in tks16_stream_row (topk_seg16_kernels.hpp), the copy of
// this kernel's body that the segmented top-k runs on a list entry (the same rule decided it).
// Every LDS and global store index is checked against its buffer's length; a count that does not add up sets TK_ST_INTERNAL.  No
// kernel waits on another workgroup.  Registers, LDS and scratch per kernel: DESIGN.md 3.11.
#pragma once
#include "topk_rows_kernels.hpp"

namespace gs {

enum : int { KEY_U16 = 6, KEY_I16 = 7, KEY_F16 = 8, KEY_BF16 = 9 };  // gs_key_type behind the 64-bit ones

constexpr uint32_t TKR16_CHUNK = 8 * TKR_THREADS;            // one 16-byte load per thread
constexpr uint32_t TKR16_TILE = TKR_UNROLL * TKR16_CHUNK;
static_assert(TKR16_TILE < 65536u, "a tile's front and equal counts are packed into 16 bits each");

// the 16 key bits (in the low half of u, the high half 0) <-> the pattern whose unsigned order is the key order: signed keys flip
// the sign bit, both float formats flip all bits of negatives too
__device__ __forceinline__ uint32_t tkr16_to_bits(uint32_t u, uint32_t kt) {
    return kt == KEY_U16 ? u : kt == KEY_I16 ? u ^ 0x8000u : u ^ ((u & 0x8000u) ? 0xffffu : 0x8000u);
}
__device__ __forceinline__ uint32_t tkr16_from_bits(uint32_t u, uint32_t kt) {
    return kt == KEY_U16 ? u : kt == KEY_I16 ? u ^ 0x8000u : u ^ ((u & 0x8000u) ? 0x8000u : 0xffffu);
}

// the row bodies' key traits for 2-byte keys (TkrKey32, topk_rows_kernels.hpp)
struct TkrKey16 {
    using elem = uint16_t;
    // Two passes.  The all-one dummies of the slots >= n tie with a real key 0xFFFF on those two bytes: they stay behind it only
    // because the passes are stable and the dummies start in the highest slots (in the RANK 1 form they take no part at all).
    // Whoever changes the dummies' place or the passes' stability breaks that.
    static constexpr uint32_t RANKED_BITS = 16u;
    static __device__ __forceinline__ uint32_t to_bits(uint32_t u, uint32_t kt) { return tkr16_to_bits(u, kt); }
    static __device__ __forceinline__ uint32_t from_bits(uint32_t u, uint32_t kt) { return tkr16_from_bits(u, kt); }  // (the low 16 bits count)
};

template <int VM>
__global__ __launch_bounds__(64 * TKR_WAVE_ROWS) void tkr16_wave_kernel(const TkrArgs a) { tkr_matrix_wave<TkrKey16, VM>(a); }
template <int THREADS, int KPT, int VM, int RANK>
__global__ __launch_bounds__(THREADS) void tkr16_tile_kernel(const TkrArgs a) { tkr_matrix_tile<TkrKey16, THREADS, KPT, VM, RANK>(a); }

// ---- stream kernel: its own body (the header says why) ----------------------------------------------------------------------------
// The row as the index range [lo, hi) of the 16-byte aligned pointer q (lo <= 7: the peel).  Eight elements of thread `tid` in the
// chunk at c, two to a word, the lower index in the low half; mask: which of them lie in the row.  A chunk inside the row is one
// 16-byte load per thread, the first and the last chunk are loaded element by element.
__device__ __forceinline__ uint4 tkr16_load_chunk(const uint16_t* q, uint32_t c, uint32_t lo, uint32_t hi, uint32_t tid, uint32_t& mask) {
    const uint32_t i = c + tid * 8u;
    if (GS_LIKELY(c >= lo && c + TKR16_CHUNK <= hi)) {  // (uniform)
        mask = 255u;
        return *reinterpret_cast<const uint4*>(q + i);
    }
    uint32_t e[4] = {0u, 0u, 0u, 0u};
    mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        if (i + j >= lo && i + j < hi) {
            e[j >> 1] |= (uint32_t)q[i + j] << ((j & 1u) * 16u);
            mask |= 1u << j;
        }
    }
    return uint4{e[0], e[1], e[2], e[3]};
}

// element j (0 .. 7) of a loaded chunk, in the low half of the result
__device__ __forceinline__ uint32_t tkr16_elem(const uint32_t (&w)[4], uint32_t j) { return (j & 1u) ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu; }

template <int VM, int RANK>
__global__ __launch_bounds__(TKR_THREADS) void tkr16_stream_kernel(const TkrArgs a) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t T = TKR_THREADS, W = T / 64, SLOTS = TKR_UNROLL * W;
    static_assert(SLOTS == 64, "the tile's wave totals are scanned by one wave");
    static_assert(TKR_BINS == 4u * T, "four bins per thread in the scan");
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TKR_BINS];
    __shared__ uint32_t s_skey[TKR_STAGE], s_spos[TKR_STAGE];
    __shared__ uint32_t s_w[2][SLOTS + 1];  // packed: front | equal << 16 (a tile holds TKR16_TILE < 65 536 elements)
    __shared__ uint32_t s_ws[W], s_bc[4];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = a.k, kt = a.kt, flip = a.descending ? 0xffffu : 0u;
    if (r >= a.rows || k == 0u || k > TKR_STAGE || k > a.row_len) return;  // (uniform; the host's checks)
    const size_t row_base = (size_t)r * a.row_stride;
    const uint16_t* p = reinterpret_cast<const uint16_t*>(a.keys) + row_base;
    const uint32_t lo = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 1) & 7u), hi = lo + a.row_len;
    const uint16_t* q = p - lo;  // (the base pointer is 16-byte aligned: q never lies in front of it)
    auto fail = [&]() { if (tid == 0) atomicOr(&a.ctl[TKC_STATUS], TK_ST_INTERNAL); };

    // ---- narrow: pfx = the bits of P found so far, front = elements in front of it, equal = elements in it
    uint32_t pfx = 0, front = 0, equal = a.row_len, level = 0, sh = 0;
    for (;; ++level) {
        sh = level == 0u ? 4u : 0u;
        const uint32_t nbits = level == 0u ? 12u : 4u, above = sh + nbits;
        reinterpret_cast<uint4*>(s_hist)[tid] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
        auto process = [&](const uint4 t, const uint32_t mask) {
            const uint32_t w4[4] = {t.x, t.y, t.z, t.w};
            uint32_t d[8], m = 0;
            bool one = true;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t sel = tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip;
                d[j] = (sel >> sh) & ((1u << nbits) - 1u);  // (< TKR_BINS)
                if (((mask >> j) & 1u) && (level == 0u || (sel >> above) == pfx)) m |= 1u << j;
                one = one && d[j] == d[0];
            }
            // a whole wave under one bin (sorted or constant rows): one add
            const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
            if (__builtin_amdgcn_ballot_w64(m == 255u && one && d[0] == f) == ~0ull) {
                if (lane == 0) atomicAdd(&s_hist[f], 512u);
                return;
            }
            if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) return;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                if ((m >> j) & 1u) atomicAdd(&s_hist[d[j]], 1u);
        };
        for (uint32_t c0 = 0; c0 < hi; c0 += TKR16_TILE) {
            uint4 t[TKR_UNROLL];
            uint32_t mask[TKR_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
                const uint32_t c = c0 + u * TKR16_CHUNK;
                mask[u] = 0u;
                t[u] = uint4{0u, 0u, 0u, 0u};
                if (c < hi) t[u] = tkr16_load_chunk(q, c, lo, hi, tid, mask[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u)
                if (c0 + u * TKR16_CHUNK < hi) process(t[u], mask[u]);  // (uniform)
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
        if (front + equal <= TKR_STAGE || level == 1u) break;  // (level 1: P is the exact 16-bit pattern)
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
    for (uint32_t c0 = 0; c0 < hi; c0 += TKR16_TILE, par ^= 1u) {
        uint4 t[TKR_UNROLL];
        uint32_t mask[TKR_UNROLL], fl[TKR_UNROLL], excl[TKR_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
            const uint32_t c = c0 + u * TKR16_CHUNK;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (c < hi) t[u] = tkr16_load_chunk(q, c, lo, hi, tid, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
            const uint32_t w4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            uint32_t f = 0, cnt = 0;  // f: bit j = in front, bit 8 + j = equal
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t h = (tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip) >> sh;
                const bool v = (mask[u] >> j) & 1u;
                if (v && h < pfx) { f |= 1u << j; cnt += 1u; }
                if (v && h == pfx) { f |= 256u << j; cnt += 1u << 16; }
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
                const uint32_t w4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
                const uint32_t i0 = c0 + u * TKR16_CHUNK + tid * 8u - lo;  // position in the row (elements in the row only)
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) {
                    const uint32_t sel = tkr16_to_bits(tkr16_elem(w4, j), kt) ^ flip;
                    if (fl[u] & (1u << j)) { stage(r_lt, sel, i0 + j); ++r_lt; }
                    else if (fl[u] & (256u << j)) {
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
    tkr_tile_sort_passes<TKR_THREADS, TKR_SORT_KPT, 4, RANK, 16u>(key, pos, G);
#pragma unroll
    for (int i = 0; i < TKR_SORT_KPT; ++i) {
        const uint32_t idx = my_base + i * 64u;
        if (idx < k && pos[i] < a.row_len) {  // (idx < k <= G)
            if constexpr (VM == 0 || VM == 1) tkr_emit<TkrKey16, VM>(a, r, idx, key[i] ^ flip, pos[i]);
            else tkr_emit<TkrKey16, VM>(a, r, idx, key[i] ^ flip, static_cast<const V*>(a.vals)[row_base + pos[i]]);
        }
    }
}

}  // namespace gs
