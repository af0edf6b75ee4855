// topk_seg16_kernels.hpp — the segmented top-k of topk_seg_kernels.hpp on 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16)
// for gs_segtopk16_* (include/gpusort.h): 2-byte elements in d_keys and d_out_keys, read once at their own width.  No counterpart in
// the reference project.
//
// Same launch sequence, same classes, same grids, same control words as the 32-bit file (seg_reset_kernel, seg_classify_kernel and
// seg_fill_kernel do not look at the keys and are launched unchanged); TksArgs::keys / out_keys point at 2-byte elements, offsets, k
// and positions keep counting elements, values stay 4 or 8 bytes under the same index.  Segments and output rows start at 2-byte
// alignment only; the base pointers are 16-byte aligned.
//   tks16_packed_kernel   length 1 .. 32: tks_packed_kernel's layout and counting rank on 2-byte loads and 2-byte stores
//   tks16_wave_kernel     33 .. 256: tkr_wave_row on TksKey16 (= TkrKey16), one list entry per wave
//   tks16_tile_kernel     classes 3 .. 7: tkr_tile_row on TksKey16, one list entry per workgroup
//   tks16_stream_kernel   longer than LDS holds: the 16-bit radix select (12 + 4 bits, eight elements per 16-byte load behind a peel
//                         of up to seven, tiles of 32 768 elements with 16-bit packed counts: 2 or 3 reads of the segment), one
//                         list entry per workgroup, on a grid of one workgroup per slot the class can have (no loop: inside a
//                         grid-stride loop the kernel spilled four to seven VGPRs to scratch)
// tks16_stream_row below is a COPY of tkr16_stream_kernel's body (topk_rows16_kernels.hpp).  One body for both was tried first: the
// kernel, early-outs included, as a __forceinline__ function of (row, base, length, pos0) that tkr16_stream_kernel calls with
// (blockIdx.x, r * row_stride, row_len, 0) — alone in the library or with the segmented kernel as a second caller of an instantiation
// of its own, tkr16_stream_kernel<0 / 1 / 4 / 8, 0> then compiled to 38 712 / 38 936 / 38 844 / 38 840 bytes of code where it has
// 38 360 / 38 504 / 38 712 / 38 712, and the last two to 103 spilled SGPRs where they have 106.  Resources and code of
// the kernels that exist were to stay what they are, so the select stands twice on 16-bit keys: a fix to it belongs in
// tkr16_stream_kernel AND in tks16_stream_row (and, for what the two widths share, in tkr_stream_row, topk_rows_kernels.hpp).
// The list walking is that of tks_wave_kernel, tks_tile_kernel and tks_stream_kernel, written again beside them because those
// kernels were to stay what they compile to; a fix to it belongs in both files.
// Every key store is a 2-byte store of its own slot: two output rows share a 32-bit word when k is odd, and the unwritten slots of a
// short segment's row must survive beside a written one, so nothing here widens a store or reads a word to write it back.
// Every kernel reads the status word first; every LDS and global store index is checked against its buffer; no kernel waits on
// another workgroup.  Registers, LDS and scratch per kernel: DESIGN.md 3.18.
#pragma once
#include "topk_rows16_kernels.hpp"
#include "topk_seg_kernels.hpp"

namespace gs {

// TkrKey16 under a name of this file's own: tkr_wave_row and tkr_tile_row are instantiated for the segmented kernels apart from the
// row-wise ones.  The compiler specialises a function on what all callers of one instantiation pass (the row-wise kernels: pos0 = 0,
// a length known to be >= k), so a second caller of the same instantiation changes the code of the first; with two instantiations
// of the one text tkr16_wave_kernel and tkr16_tile_kernel compile to what they were.
struct TksKey16 : TkrKey16 {};

// ---- packed class: 1 .. SEG_PACK_MAX elements, 64 consecutive segments per wave ------------------------------------------------
template <int VM>
__global__ __launch_bounds__(64) void tks16_packed_kernel(const TksArgs a) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t CAP = 64u * SEG_PACK_MAX;
    __shared__ uint32_t s_key[CAP];  // the sortable 16 bits, the high half 0
    __shared__ uint32_t s_start[64], s_scan[65];
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const uint16_t* keys = reinterpret_cast<const uint16_t*>(a.keys);
    uint16_t* out_keys = reinterpret_cast<uint16_t*>(a.out_keys);
    const uint32_t lane = threadIdx.x, s = blockIdx.x * 64u + lane;
    uint32_t st = 0, len = 0;
    if (s < a.num_segments) {
        st = a.off[s];
        const uint32_t l = a.off[s + 1u] - st;
        if (l >= 1u && l <= SEG_PACK_MAX && (a.max_len == 0u || l <= a.max_len)) len = l;
    }
    const uint32_t incl = wave_inclusive_scan(len, lane);
    const uint32_t E = __shfl(incl, 63, 64);  // <= CAP
    if (E == 0u) return;
    const unsigned long long mine = __builtin_amdgcn_ballot_w64(len != 0u);
    if (lane == 0) atomicAdd(&a.ctl[TKSC_PACKED], (uint32_t)__popcll(mine));
    s_start[lane] = st;
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
        uint32_t kk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // unconditional 2-byte loads on a clamped element, masked afterwards
            const uint32_t e = e0 + u * 64u + lane, ec = e < E ? e : E - 1u;
            const uint32_t j = find(ec);
            kk[u] = keys[s_start[j] + (ec - s_scan[j])];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = e0 + u * 64u + lane;
            if (e < E) s_key[e] = tkr16_to_bits(kk[u], a.kt);
        }
    }
    __syncthreads();
    for (uint32_t e = lane; e < E; e += 64u) {
        const uint32_t j = find(e);
        const uint32_t lo = s_scan[j], hi = s_scan[j + 1u];
        const uint32_t key = s_key[e];
        uint32_t rank = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t x = s_key[i];
            rank += (x < key || (x == key && i < e)) ? 1u : 0u;
        }
        const uint32_t o = a.descending ? hi - lo - 1u - rank : rank;
        const uint32_t seg = blockIdx.x * 64u + j;  // (j's segment is not empty: seg < num_segments)
        if (o < a.k && seg < a.num_segments) {
            const size_t dst = (size_t)seg * a.k + o;
            const uint32_t g = s_start[j] + (e - lo);
            out_keys[dst] = (uint16_t)tkr16_from_bits(key, a.kt);  // (a 2-byte store: the neighbour in the word is not touched)
            if constexpr (VM == 1) static_cast<V*>(a.out_vals)[dst] = g;
            else if constexpr (VM != 0) static_cast<V*>(a.out_vals)[dst] = static_cast<const V*>(a.vals)[g];
        }
    }
}

// ---- wave class: one list entry per wave (the loop of tks_wave_kernel) -----------------------------------------------------------
template <int VM>
__global__ __launch_bounds__(64 * TKR_WAVE_ROWS) void tks16_wave_kernel(const TksArgs a) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t count = a.ctl[SEGC_COUNT + 2], base = seg_list_base(a.ctl, 2);
    for (uint32_t it0 = blockIdx.x * TKR_WAVE_ROWS; it0 < count; it0 += gridDim.x * TKR_WAVE_ROWS) {  // (uniform over the workgroup)
        uint32_t s = 0, st = 0, len = 0;
        const bool live = it0 + wave < count && tks_resolve(a, base, it0 + wave, SEG_WAVE_MAX, s, st, len);
        tkr_wave_row<TksKey16, VM>(t, s, live ? st : 0u, live ? len : 0u, st);
    }
}

// ---- tile classes: one list entry per workgroup (the loop of tks_tile_kernel) ----------------------------------------------------
// LOOP false: one workgroup per slot the class can have; here for both shapes of 1024 threads (topk_seg16_host.hpp says why).
template <int THREADS, int KPT, int VM, int RANK, bool LOOP>
__global__ __launch_bounds__(THREADS) void tks16_tile_kernel(const TksArgs a, const uint32_t cls) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t count = a.ctl[SEGC_COUNT + cls], base = seg_list_base(a.ctl, cls);
    if constexpr (LOOP) {
        for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
            uint32_t s, st, len;
            if (tks_resolve(a, base, it, (uint32_t)(THREADS * KPT), s, st, len)) tkr_tile_row<TksKey16, THREADS, KPT, VM, RANK>(t, s, st, len, st);
            __syncthreads();
        }
    } else {
        uint32_t s, st, len;
        if (blockIdx.x < count && tks_resolve(a, base, blockIdx.x, (uint32_t)(THREADS * KPT), s, st, len))
            tkr_tile_row<TksKey16, THREADS, KPT, VM, RANK>(t, s, st, len, st);
    }
}

// ---- long class: one list entry per workgroup, the 16-bit radix select -----------------------------------------------------------
// tkr16_stream_kernel's body (topk_rows16_kernels.hpp) as a function of a resolved row: keys16[row_base .. row_base + row_len), its
// head to output row r, positions pos0 + i, values at vals[row_base + i].  A COPY, the file header says why; what differs from the
// original: r, row_base and row_len are arguments (there: blockIdx.x, r * row_stride, a.row_len) and the position mode adds pos0.
// The uniform early-outs stand where they stand there: r < a.rows, 1 <= k <= TKR_STAGE and k <= row_len, or nothing happens.
template <int VM, int RANK>
__device__ __forceinline__ void tks16_stream_row(const TkrArgs& a, const uint32_t r, const size_t row_base, const uint32_t row_len, const uint32_t pos0) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t T = TKR_THREADS, W = T / 64, SLOTS = TKR_UNROLL * W;
    static_assert(SLOTS == 64, "the tile's wave totals are scanned by one wave");
    static_assert(TKR_BINS == 4u * T, "four bins per thread in the scan");
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TKR_BINS];
    __shared__ uint32_t s_skey[TKR_STAGE], s_spos[TKR_STAGE];
    __shared__ uint32_t s_w[2][SLOTS + 1];  // packed: front | equal << 16 (a tile holds TKR16_TILE < 65 536 elements)
    __shared__ uint32_t s_ws[W], s_bc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = a.k, kt = a.kt, flip = a.descending ? 0xffffu : 0u;
    if (r >= a.rows || k == 0u || k > TKR_STAGE || k > row_len) return;  // (uniform; the host's checks)
    const uint16_t* p = reinterpret_cast<const uint16_t*>(a.keys) + row_base;
    const uint32_t lo = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 1) & 7u), hi = lo + row_len;
    const uint16_t* q = p - lo;  // (the base pointer is 16-byte aligned: q never lies in front of it)
    auto fail = [&]() { if (tid == 0) atomicOr(&a.ctl[TKC_STATUS], TK_ST_INTERNAL); };

    // ---- narrow: pfx = the bits of P found so far, front = elements in front of it, equal = elements in it
    uint32_t pfx = 0, front = 0, equal = row_len, level = 0, sh = 0;
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
        if (idx < k && pos[i] < row_len) {  // (idx < k <= G)
            if constexpr (VM == 0 || VM == 1) tkr_emit<TkrKey16, VM>(a, r, idx, key[i] ^ flip, pos0 + pos[i]);
            else tkr_emit<TkrKey16, VM>(a, r, idx, key[i] ^ flip, static_cast<const V*>(a.vals)[row_base + pos[i]]);
        }
    }
}

template <int VM, int RANK>
__global__ __launch_bounds__(TKR_THREADS) void tks16_stream_kernel(const TksArgs a) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t count = a.ctl[SEGC_COUNT + SEG_CLASS_LONG], base = seg_list_base(a.ctl, SEG_CLASS_LONG);
    uint32_t s, st, len;
    if (blockIdx.x < count && tks_resolve(a, base, blockIdx.x, 0xffffffffu, s, st, len)) tks16_stream_row<VM, RANK>(t, s, st, len, st);
}

}  // namespace gs
