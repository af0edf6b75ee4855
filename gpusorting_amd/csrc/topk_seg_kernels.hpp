// topk_seg_kernels.hpp — segmented top-k for gs_segtopk_* (include/gpusort.h): the first k of every segment of one array, the
// segments given by CSR offsets, into a dense [num_segments, k] output, one call for all segments.  No counterpart in the reference
// project.
//
// The composition of two things the tree has: the device-side offset validation and class lists of the segmented sort
// (segsort_kernels.hpp: seg_reset_kernel, seg_classify_kernel, seg_fill_kernel, launched unchanged) and the per-row bodies of the
// row-wise top-k (topk_rows_kernels.hpp), restated below on a resolved row (tks_wave_row, tks_tile_row, tks_stream_row).  Here the row is
// segment s of a class list: base = off[s], len = off[s + 1] - base, output row s.  Launch sequence of one call:
//   seg_reset_kernel, seg_classify_kernel, seg_fill_kernel
//   tks_packed_kernel   length 1 .. 32: 64 consecutive segments per wave, back to back in LDS, a counting rank inside the segment; an
//                       element whose place in the output order is < k is written.  Walks all segments and filters by length (no list).
//                       Length 1 belongs here: the sort's class 0 has nothing to do for it, a top-k must emit it.
//   tks_wave_kernel     33 .. 256: TKR_WAVE_ROWS list entries per workgroup, one per wave (tks_wave_row)
//   tks_tile_kernel     classes 3 .. 7: one list entry per workgroup on the single-tile shape of the class (tks_tile_row)
//   tks_stream_kernel   longer than LDS holds: one list entry per workgroup, the radix select (tks_stream_row); k <= TKR_STAGE < len
// The list kernels run on fixed grids and claim list entries by grid stride (the 1024 x 32 tile shape excepted: one workgroup per
// slot its class can have, as seg_wg_kernel): the host never learns the counts.  Every kernel reads the status word first and leaves
// if the offsets were bad; a segment longer than a non-zero promise is in no list (seg_work_class) and gets no output row.  Slots
// min(k, len) .. k of an output row are not written.  The position mode (VM 1) delivers off[s] + the position in the segment.  No
// kernel waits on another workgroup.  Registers, LDS and scratch per kernel: DESIGN.md 3.17.
#pragma once
#include "topk_rows_kernels.hpp"

namespace gs {

// words of the segmented sort's control block (cleared by seg_reset_kernel) that this handle uses beside SEGC_*
constexpr uint32_t TKSC_TKR = 48;     // where the row bodies' control words lie: TKSC_TKR + TKC_STATUS, TKSC_TKR + TKR_CTL_READS
constexpr uint32_t TKSC_PACKED = 50;  // segments the packed kernel emitted (length 1 .. 32)
static_assert(TKSC_TKR > SEGC_CURSOR + SEG_CLASSES && TKSC_PACKED < SEGC_WORDS && TKC_STATUS < 2 && TKR_CTL_READS < 2, "inside the block, beside the rest");

struct TksArgs {
    const uint32_t* keys;
    const void* vals;
    uint32_t* out_keys;
    void* out_vals;
    const uint32_t* off;
    const uint32_t* list;
    uint32_t* ctl;
    uint32_t num_segments, k, kt, descending, max_len;
};

// the row bodies' view of a call: rows = segments, the row geometry is not read (the bodies take the resolved row)
__device__ __forceinline__ TkrArgs tks_row_args(const TksArgs& a) {
    return TkrArgs{a.keys, a.vals, a.out_keys, a.out_vals, a.num_segments, 0u, 0u, a.k, a.kt, a.descending, a.ctl + TKSC_TKR};
}

// ---- packed class: 1 .. SEG_PACK_MAX elements, 64 consecutive segments per wave ------------------------------------------------
// seg_packed_kernel's layout and counting rank; the keys only go through LDS: a value is fetched by the element's place in the array
// when the element is written, and at most min(k, len) elements of a segment are.
template <int VM>
__global__ __launch_bounds__(64) void tks_packed_kernel(const TksArgs a) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t CAP = 64u * SEG_PACK_MAX;
    __shared__ uint32_t s_key[CAP];
    __shared__ uint32_t s_start[64], s_scan[65];
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
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
        for (int u = 0; u < 4; ++u) {  // unconditional loads on a clamped element, masked afterwards
            const uint32_t e = e0 + u * 64u + lane, ec = e < E ? e : E - 1u;
            const uint32_t j = find(ec);
            kk[u] = a.keys[s_start[j] + (ec - s_scan[j])];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = e0 + u * 64u + lane;
            if (e < E) s_key[e] = seg_to_bits(kk[u], a.kt);
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
            a.out_keys[dst] = seg_from_bits(key, a.kt);
            if constexpr (VM == 1) static_cast<V*>(a.out_vals)[dst] = g;
            else if constexpr (VM != 0) static_cast<V*>(a.out_vals)[dst] = static_cast<const V*>(a.vals)[g];
        }
    }
}

// ---- the row bodies ---------------------------------------------------------------------------------------------------------------
// tkr_wave_kernel, tkr_tile_kernel and tkr_stream_kernel (topk_rows_kernels.hpp) restated on a resolved row: they find their row as
// r * row_stride and take its length from the call, here both come from a class list.  Calling one shared function from both was
// tried: registers, LDS and scratch of every tkr_* instantiation stayed what they were, their code did not (the tile kernels 0.4 to 6.1 %
// more instruction bytes, the stream kernels 0.2 to 0.4 %), and those kernels stay as they are, as sr_count_kernel did
// when the long segments moved to the device: a fix to a body belongs in both copies.  What the bodies are made of is shared:
// seg_wave_sort_passes, tkr_tile_sort_passes, tkr_load_chunk, tkr_emit.  pos0: what the row's first element counts as in the position
// mode (the segment's start).

// One row on the calling wave: keys[base .. base + len) sorted by the wave class's passes, its head written to output row r.  The
// tables are the calling wave's own; the passes' barriers are the workgroup's: every wave of the workgroup calls this, and equally
// often (len 0: the passes run on no rows of slots).
template <int VM>
__device__ __forceinline__ void tks_wave_row(const TkrArgs& a, uint32_t r, size_t base, uint32_t len, uint32_t pos0, uint32_t lane, uint32_t* s_hist,
                                             uint32_t* s_stage, typename TkrVal<VM>::type* s_vstage) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB, KPT = SEG_WAVE_MAX / 64;
    uint32_t key[KPT];
    V val[VB != 0 ? KPT : 1];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = lane + i * 64u, ci = idx < len ? idx : (len ? len - 1u : 0u);
        key[i] = a.keys[base + ci];
        if constexpr (VM == 1) val[i] = pos0 + ci;
        else if constexpr (VM != 0) val[i] = static_cast<const V*>(a.vals)[base + ci];
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) key[i] = lane + i * 64u < len ? seg_to_bits(key[i], a.kt) : 0xffffffffu;
    seg_wave_sort_passes<VB>(key, val, (len + 63u) >> 6, lane, s_hist, s_stage, s_vstage);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = lane + i * 64u;
        if (idx < len) {
            const uint32_t o = a.descending ? len - 1u - idx : idx;
            if (o < a.k) tkr_emit<VM>(a, r, o, key[i], val[VB != 0 ? i : 0]);
        }
    }
}

// One row on the calling workgroup: keys[base .. base + n), 1 <= n <= THREADS * KPT (the caller's check), its head to output row r.
template <int THREADS, int KPT, int VM, int RANK>
__device__ __forceinline__ void tks_tile_row(const TkrArgs& a, uint32_t r, size_t base, uint32_t n, uint32_t pos0) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t my_base = wave * (64u * KPT) + lane;
    uint32_t key[KPT];
    V val[VB != 0 ? KPT : 1];
    // unconditional loads on a clamped index, masked afterwards (as tile_sort_body)
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = my_base + i * 64u, ci = idx < n ? idx : n - 1u;
        key[i] = a.keys[base + ci];
        if constexpr (VM == 1) val[i] = pos0 + ci;
        else if constexpr (VM != 0) val[i] = static_cast<const V*>(a.vals)[base + ci];
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) key[i] = my_base + i * 64u < n ? seg_to_bits(key[i], a.kt) : 0xffffffffu;
    tkr_tile_sort_passes<THREADS, KPT, VB, RANK>(key, val, n);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = my_base + i * 64u;
        if (idx < n) {
            const uint32_t o = a.descending ? n - 1u - idx : idx;
            if (o < a.k) tkr_emit<VM>(a, r, o, key[i], val[VB != 0 ? i : 0]);
        }
    }
}

// One row on the calling workgroup of TKR_THREADS threads: keys[row_base .. row_base + row_len), row_len >= k (the caller's check), the
// first k to output row r.  Every return is uniform over the workgroup; a caller that goes on to another row puts a barrier in
// between (the LDS is this function's own).
template <int VM, int RANK>
__device__ __forceinline__ void tks_stream_row(const TkrArgs& a, const uint32_t r, const size_t row_base, const uint32_t row_len, const uint32_t pos0) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t T = TKR_THREADS, W = T / 64, SLOTS = TKR_UNROLL * W;
    static_assert(SLOTS == 64, "the tile's wave totals are scanned by one wave");
    static_assert(TKR_BINS == 4u * T, "four bins per thread in the scan");
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TKR_BINS];
    __shared__ uint32_t s_skey[TKR_STAGE], s_spos[TKR_STAGE];
    __shared__ uint32_t s_w[2][SLOTS + 1];  // packed: front | equal << 16 (a tile holds 16 384 elements)
    __shared__ uint32_t s_ws[W], s_bc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = a.k, kt = a.kt, flip = a.descending ? 0xffffffffu : 0u;
    const uint32_t* p = a.keys + row_base;
    const uint32_t lo = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u), hi = lo + row_len;
    const uint32_t* q = p - lo;  // (the base pointer is 16-byte aligned: q never lies in front of it)
    auto fail = [&]() { if (tid == 0) atomicOr(&a.ctl[TKC_STATUS], TK_ST_INTERNAL); };

    // ---- narrow: pfx = the bits of P found so far, front = elements in front of it, equal = elements in it
    uint32_t pfx = 0, front = 0, equal = row_len, level = 0, sh = 0;
    for (;; ++level) {
        sh = level == 0u ? 20u : level == 1u ? 8u : 0u;
        const uint32_t nbits = level == 2u ? 8u : 12u, above = sh + nbits;
        reinterpret_cast<uint4*>(s_hist)[tid] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
        auto process = [&](const uint4 t, const uint32_t mask) {
            const uint32_t k4[4] = {t.x, t.y, t.z, t.w};
            uint32_t d[4], m = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t sel = seg_to_bits(k4[j], kt) ^ flip;
                d[j] = (sel >> sh) & (TKR_BINS - 1u) & ((1u << nbits) - 1u);
                if (((mask >> j) & 1u) && (level == 0u || (sel >> above) == pfx)) m |= 1u << j;
            }
            // a whole wave under one bin (sorted or constant rows): one add
            const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
            if (__builtin_amdgcn_ballot_w64(m == 15u && d[0] == f && d[1] == f && d[2] == f && d[3] == f) == ~0ull) {
                if (lane == 0) atomicAdd(&s_hist[f], 256u);
                return;
            }
            if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) return;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if ((m >> j) & 1u) atomicAdd(&s_hist[d[j]], 1u);
        };
        for (uint32_t c0 = 0; c0 < hi; c0 += TKR_TILE) {
            uint4 t[TKR_UNROLL];
            uint32_t mask[TKR_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
                const uint32_t c = c0 + u * TKR_CHUNK;
                mask[u] = 0u;
                t[u] = uint4{0u, 0u, 0u, 0u};
                if (c < hi) t[u] = tkr_load_chunk(q, c, lo, hi, tid, mask[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < TKR_UNROLL; ++u)
                if (c0 + u * TKR_CHUNK < hi) process(t[u], mask[u]);  // (uniform)
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
        if (front + equal <= TKR_STAGE || level == 2u) break;
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
    for (uint32_t c0 = 0; c0 < hi; c0 += TKR_TILE, par ^= 1u) {
        uint4 t[TKR_UNROLL];
        uint32_t mask[TKR_UNROLL], fl[TKR_UNROLL], excl[TKR_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
            const uint32_t c = c0 + u * TKR_CHUNK;
            mask[u] = 0u;
            t[u] = uint4{0u, 0u, 0u, 0u};
            if (c < hi) t[u] = tkr_load_chunk(q, c, lo, hi, tid, mask[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < TKR_UNROLL; ++u) {
            const uint32_t k4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            uint32_t f = 0, cnt = 0;  // f: bit j = in front, bit 4 + j = equal
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t h = (seg_to_bits(k4[j], kt) ^ flip) >> sh;
                const bool v = (mask[u] >> j) & 1u;
                if (v && h < pfx) { f |= 1u << j; cnt += 1u; }
                if (v && h == pfx) { f |= 16u << j; cnt += 1u << 16; }
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
                const uint32_t k4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
                const uint32_t i0 = c0 + u * TKR_CHUNK + tid * 4u - lo;  // position in the row (elements in the row only)
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t sel = seg_to_bits(k4[j], kt) ^ flip;
                    if (fl[u] & (1u << j)) { stage(r_lt, sel, i0 + j); ++r_lt; }
                    else if (fl[u] & (16u << j)) {
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
    tkr_tile_sort_passes<TKR_THREADS, TKR_SORT_KPT, 4, RANK>(key, pos, G);
#pragma unroll
    for (int i = 0; i < TKR_SORT_KPT; ++i) {
        const uint32_t idx = my_base + i * 64u;
        if (idx < k && pos[i] < row_len) {  // (idx < k <= G)
            if constexpr (VM == 0 || VM == 1) tkr_emit<VM>(a, r, idx, key[i] ^ flip, pos0 + pos[i]);
            else tkr_emit<VM>(a, r, idx, key[i] ^ flip, static_cast<const V*>(a.vals)[row_base + pos[i]]);
        }
    }
}


// entry `it` of class cls's list -> segment, start and length; false where the entry is not a segment of [1, max_len] elements
// (the list holds segments of its class only; the checks keep a broken invariant in bounds)
__device__ __forceinline__ bool tks_resolve(const TksArgs& a, uint32_t list_base, uint32_t it, uint32_t max_len, uint32_t& s, uint32_t& st, uint32_t& len) {
    s = st = len = 0;
    if (list_base + it >= a.num_segments) return false;
    s = a.list[list_base + it];
    if (s >= a.num_segments) return false;
    st = a.off[s];
    len = a.off[s + 1u] - st;
    return len != 0u && len <= max_len;
}

// ---- wave class: one list entry per wave ------------------------------------------------------------------------------------------
// The trip count is the workgroup's (the passes' barriers are workgroup barriers); a wave without an entry runs them on no rows of slots.
template <int VM>
__global__ __launch_bounds__(64 * TKR_WAVE_ROWS) void tks_wave_kernel(const TksArgs a) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TKR_WAVE_ROWS][RADIX];
    __shared__ uint32_t s_stage[TKR_WAVE_ROWS][SEG_WAVE_MAX];
    __shared__ V s_vstage[VB != 0 ? TKR_WAVE_ROWS : 1][VB != 0 ? SEG_WAVE_MAX : 1];
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t count = a.ctl[SEGC_COUNT + 2], base = seg_list_base(a.ctl, 2);
    for (uint32_t it0 = blockIdx.x * TKR_WAVE_ROWS; it0 < count; it0 += gridDim.x * TKR_WAVE_ROWS) {  // (uniform over the workgroup)
        uint32_t s = 0, st = 0, len = 0;
        const bool live = it0 + wave < count && tks_resolve(a, base, it0 + wave, SEG_WAVE_MAX, s, st, len);
        tks_wave_row<VM>(t, s, live ? st : 0u, live ? len : 0u, st, lane, s_hist[wave], s_stage[wave], s_vstage[VB != 0 ? wave : 0]);
    }
}

// ---- tile classes: one list entry per workgroup ---------------------------------------------------------------------------------
// LOOP: as seg_wg_kernel (the 1024 x 32 shape sits at its register limit and takes one workgroup per slot its class can have).
template <int THREADS, int KPT, int VM, int RANK, bool LOOP>
__global__ __launch_bounds__(THREADS) void tks_tile_kernel(const TksArgs a, const uint32_t cls) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const TkrArgs t = tks_row_args(a);
    const uint32_t count = a.ctl[SEGC_COUNT + cls], base = seg_list_base(a.ctl, cls);
    if constexpr (LOOP) {
        for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
            uint32_t s, st, len;
            if (tks_resolve(a, base, it, (uint32_t)(THREADS * KPT), s, st, len)) tks_tile_row<THREADS, KPT, VM, RANK>(t, s, st, len, st);
            __syncthreads();
        }
    } else {
        uint32_t s, st, len;
        if (blockIdx.x < count && tks_resolve(a, base, blockIdx.x, (uint32_t)(THREADS * KPT), s, st, len))
            tks_tile_row<THREADS, KPT, VM, RANK>(t, s, st, len, st);
    }
}

// ---- long class: one list entry per workgroup, the radix select -----------------------------------------------------------------
template <int VM, int RANK>
__global__ __launch_bounds__(TKR_THREADS) void tks_stream_kernel(const TksArgs a) {
    if (a.ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    if (a.k == 0u || a.k > TKR_STAGE) return;  // (uniform; the host's checks)
    const TkrArgs t = tks_row_args(a);
    const uint32_t count = a.ctl[SEGC_COUNT + SEG_CLASS_LONG], base = seg_list_base(a.ctl, SEG_CLASS_LONG);
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
        uint32_t s, st, len;
        if (tks_resolve(a, base, it, 0xffffffffu, s, st, len) && len >= a.k) tks_stream_row<VM, RANK>(t, s, st, len, st);
        __syncthreads();
    }
}

}  // namespace gs
