// segsort16_kernels.hpp — gfx950 (wave64) device code of the segmented sort of 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16)
// at their own width: many independent segments of one array of 2-byte elements, given by CSR offsets, each sorted on its own, in
// place (gs_segsort16_* in include/gpusort.h).  No counterpart in the reference project.
//
// Launch sequence of one call, all on the caller's stream, NO host round trip whatever the segment lengths:
//   seg_reset / seg_classify / seg_fill_kernel   as they are (segsort_kernels.hpp: they do not depend on the key width).  Nothing is
//                         loaded through the offsets before seg_classify_kernel has validated them; every later kernel reads the status
//                         word first and leaves if the offsets were bad.
//   seg16_packed_kernel   class 1, 2 .. 32 elements (1 .. 32 in the argsort form, which writes the position of a lone element):
//                         seg_packed_kernel on 2-byte loads and stores
//   seg16_wave_kernel     class 2, 33 .. 256: one segment per wave, seg_wave_sort_passes<VB, 16>: two ranking passes
//   seg16_wg_kernel       classes 3 .. 7: one segment per workgroup on the shapes of g_small_class, tkr_tile_sort_passes<.., 16>
//   class 8 (longer than LDS holds): two stable 8-bit LSD passes over ALL long segments at once, the low byte from the caller's
//   buffers into the alternates, the high byte back:
//     seg16_units_kernel  one thread per long-list entry: cuts its segment into parts of `part` elements (whole tiles), claims that
//                         many consecutive unit slots with one atomic and writes one descriptor per unit, one record per segment
//     per pass: seg16_count_kernel (one 256-bin table per unit), seg16_scan_kernel (one workgroup per long segment: the exclusive
//                         prefix over (digit major, part minor) within the segment; the counts must add up to its length),
//                         seg16_scatter_kernel (one workgroup per unit, its tiles in order with running bases)
//     count, scan and scatter run on fixed grids sized by the host's bound on units and long segments (gs_segsort16_units):
//     workgroups beyond the device's own counts leave at once.  Count, scan and scatter are the bodies of radix_pass.hpp, which tells
//     the pass's structure and invariants, with a long segment as the row and a unit descriptor as its part.
//
// In place at 2-byte boundaries: a packed, wave or workgroup segment is whole in registers (packed: in LDS) before
// its first store, and belongs to one wave or one workgroup.  Neighbouring segments, sorted by other workgroups, share dwords and
// 16-byte lines at every odd boundary, so EVERY key store here is a 2-byte store and nothing is read-modify-written.
// The all-one dummies of the slots behind a segment's end tie with a real key whose sortable bits are 0xFFFF; what keeps them behind
// it (highest slots, stable ranking) is the rule radix_pass.hpp states, and it holds for every class here.
// No kernel waits on another workgroup.  Every LDS and global store index is checked against its segment's bounds; a count that does
// not add up sets SEG16C_INTERNAL, and a scatter that finds it set writes nothing.  Registers, LDS and scratch per kernel: DESIGN.md 3.15.
#pragma once
#include "segsort_kernels.hpp"
#include "topk_rows16_kernels.hpp"  // tkr16_to_bits / tkr16_from_bits, TkrVal, tkr_tile_sort_passes
#include "sortrows16_kernels.hpp"   // SR_* constants; through it radix_pass.hpp: the three bodies of the pass

namespace gs {

// words of the segmented sort's control block (SEGC_*, zeroed by seg_reset_kernel) that only this sort uses
constexpr uint32_t SEG16C_UNITS = 40;     // (segment, part) units claimed by seg16_units_kernel
constexpr uint32_t SEG16C_INTERNAL = 41;  // SR_ST_INTERNAL: a long segment's counts did not add up, or the tables were too small
static_assert(SEG16C_INTERNAL < SEGC_WORDS && SEG16C_UNITS >= SEGC_CURSOR + SEG_CLASSES, "free words of the control block");

#if GS_SORT_ROWS_BUILT

// ---- packed class: seg_packed_kernel on 2-byte elements -----------------------------------------------------------------------------
// VM: 0 keys only, 1 = the value is the element's index in the array (argsort: made in registers, vals_ is written only, and a
// segment of ONE element is written too), 4 / 8 = values of that width.
template <int VM>
__global__ __launch_bounds__(64) void seg16_packed_kernel(uint16_t* keys, void* vals_, const uint32_t* __restrict__ off, uint32_t num_segments,
                                                          uint32_t max_len, uint32_t kt, uint32_t descending, const uint32_t* __restrict__ ctl) {
    using V = typename TkrVal<VM>::type;
    constexpr uint32_t CAP = 64u * SEG_PACK_MAX, MIN_LEN = VM == 1 ? 1u : 2u;
    __shared__ uint32_t s_key[CAP];  // sortable bits
    __shared__ V s_val[VM != 0 ? CAP : 1];
    __shared__ uint32_t s_start[64], s_scan[65];
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    V* vals = static_cast<V*>(vals_);
    const uint32_t lane = threadIdx.x, s = blockIdx.x * 64u + lane;
    uint32_t a = 0, len = 0;
    if (s < num_segments) {
        a = off[s];
        const uint32_t l = off[s + 1u] - a;
        if (l >= MIN_LEN && l <= SEG_PACK_MAX && (max_len == 0u || l <= max_len)) len = l;
    }
    const uint32_t incl = wave_inclusive_scan(len, lane);
    const uint32_t E = __shfl(incl, 63, 64);  // <= CAP
    if (E == 0u) return;
    s_start[lane] = a;
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
        uint32_t k[4];
        V v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // unconditional loads on a clamped element, masked afterwards
            const uint32_t e = e0 + u * 64u + lane, ec = e < E ? e : E - 1u;
            const uint32_t j = find(ec);
            const uint32_t g = s_start[j] + (ec - s_scan[j]);
            k[u] = keys[g];
            if constexpr (VM == 1) v[u] = g;
            else if constexpr (VM != 0) v[u] = vals[g];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = e0 + u * 64u + lane;
            if (e < E) {
                s_key[e] = tkr16_to_bits(k[u], kt);
                if constexpr (VM != 0) s_val[e] = v[u];
            }
        }
    }
    __syncthreads();  // every element of the wave's segments is in LDS: from here on the segments are overwritten
    for (uint32_t e = lane; e < E; e += 64u) {
        const uint32_t j = find(e);
        const uint32_t lo = s_scan[j], hi = s_scan[j + 1u];
        const uint32_t key = s_key[e];
        uint32_t rank = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t x = s_key[i];
            rank += (x < key || (x == key && i < e)) ? 1u : 0u;
        }
        const uint32_t o = s_start[j] + (descending ? hi - lo - 1u - rank : rank);
        keys[o] = (uint16_t)tkr16_from_bits(key, kt);
        if constexpr (VM != 0) vals[o] = s_val[e];
    }
}

// ---- wave class: seg_wave_kernel on 2-byte elements, two passes ---------------------------------------------------------------------
template <int VM>
__global__ __launch_bounds__(64) void seg16_wave_kernel(uint16_t* keys, void* vals_, const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ list, const uint32_t* __restrict__ ctl, uint32_t num_segments,
                                                        uint32_t kt, uint32_t descending) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB, KPT = SEG_WAVE_MAX / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[RADIX];
    __shared__ uint32_t s_stage[SEG_WAVE_MAX];
    __shared__ V s_vstage[VB != 0 ? SEG_WAVE_MAX : 1];
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    V* vals = static_cast<V*>(vals_);
    const uint32_t lane = threadIdx.x;
    const uint32_t count = ctl[SEGC_COUNT + 2], base = seg_list_base(ctl, 2);
    for (uint32_t it = blockIdx.x; it < count && base + it < num_segments; it += gridDim.x) {
        // (the list holds segments of this class only; the checks keep a broken invariant in bounds)
        const uint32_t s = list[base + it];
        if (s >= num_segments) continue;
        const uint32_t a = off[s], len = off[s + 1u] - a;
        if (len == 0u || len > SEG_WAVE_MAX) continue;
        const uint32_t rows = (len + 63u) >> 6;
        uint32_t key[KPT];
        V val[VB != 0 ? KPT : 1];
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const uint32_t idx = lane + r * 64u, ci = idx < len ? idx : len - 1u;
            key[r] = keys[a + ci];
            if constexpr (VM == 1) val[r] = a + ci;
            else if constexpr (VM != 0) val[r] = vals[a + ci];
        }
#pragma unroll
        for (int r = 0; r < KPT; ++r) key[r] = lane + r * 64u < len ? tkr16_to_bits(key[r], kt) : 0xffffffffu;
        seg_wave_sort_passes<VB, 16u>(key, val, rows, lane, s_hist, s_stage, s_vstage);
        // the whole segment is in registers: from here on it is overwritten
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const uint32_t idx = lane + r * 64u;
            if (idx < len) {
                const uint32_t o = descending ? len - 1u - idx : idx;
                keys[a + o] = (uint16_t)tkr16_from_bits(key[r] & 0xffffu, kt);
                if constexpr (VM != 0) vals[a + o] = val[VB != 0 ? r : 0];
            }
        }
    }
}

// ---- workgroup classes: one segment per workgroup, tkr_tile_sort_passes on the shape of the class, two passes ---------------------------
// LOOP: a fixed grid claims the class list by grid stride; !LOOP: one workgroup per list slot the class can have at most (the
// 1024 x 32 shape sits at its register limit, as in seg_wg_kernel)
template <int THREADS, int KPT, int VM, int RANK, bool LOOP>
__global__ __launch_bounds__(THREADS) void seg16_wg_kernel(uint16_t* keys, void* vals_, const uint32_t* __restrict__ off,
                                                           const uint32_t* __restrict__ list, const uint32_t* __restrict__ ctl, uint32_t num_segments,
                                                           uint32_t cls, uint32_t kt, uint32_t descending) {
    using V = typename TkrVal<VM>::type;
    constexpr int VB = TkrVal<VM>::VB;
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const uint32_t count = ctl[SEGC_COUNT + cls], base = seg_list_base(ctl, cls);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t my_base = wave * (64u * KPT) + lane;
    auto sort_one = [&](uint32_t it) {  // (everything it decides on is uniform over the workgroup)
        // (the list holds segments of this class only; the checks keep a broken invariant in bounds)
        if (base + it >= num_segments) return;
        const uint32_t s = list[base + it];
        if (s >= num_segments) return;
        const uint32_t a = off[s], n = off[s + 1u] - a;
        if (n == 0u || n > (uint32_t)(THREADS * KPT)) return;
        uint16_t* k = keys + a;
        V* v = static_cast<V*>(vals_) + (VM != 0 ? a : 0u);
        uint32_t key[KPT];
        V val[VB != 0 ? KPT : 1];
        // unconditional loads on a clamped index, masked afterwards
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = my_base + i * 64u, ci = idx < n ? idx : n - 1u;
            key[i] = k[ci];
            if constexpr (VM == 1) val[i] = a + ci;
            else if constexpr (VM != 0) val[i] = v[ci];
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) key[i] = my_base + i * 64u < n ? tkr16_to_bits(key[i], kt) : 0xffffffffu;
        tkr_tile_sort_passes<THREADS, KPT, VB, RANK, 16u>(key, val, n);
        // the whole segment is in registers: from here on it is overwritten
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = my_base + i * 64u;
            if (idx < n) {
                const uint32_t o = descending ? n - 1u - idx : idx;
                k[o] = (uint16_t)tkr16_from_bits(key[i] & 0xffffu, kt);
                if constexpr (VM != 0) v[o] = val[VB != 0 ? i : 0];
            }
        }
    };
    if constexpr (LOOP) {
        for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {  // (uniform over the workgroup)
            sort_one(it);
            __syncthreads();
        }
    } else {
        if (blockIdx.x < count) sort_one(blockIdx.x);
    }
}

// ---- long segments: the work list ------------------------------------------------------------------------------------------------------
// One thread per entry of the long list (it starts the list array).  rec[i] = (first unit, parts, segment start, segment length);
// desc[u] = (segment start, segment length, part's first element, part's end), both relative to nothing but the array / the segment.
// A segment of length L has at most L / part + 1 parts, so unit_cap = n / part + (long segments at most) units always suffice; a
// claim that does not fit is reported and the segment is left out (cannot happen).
__global__ __launch_bounds__(256) void seg16_units_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ list, uint32_t* __restrict__ ctl,
                                                          uint32_t num_segments, uint32_t part, uint32_t unit_cap, uint32_t long_cap,
                                                          uint4* __restrict__ desc, uint4* __restrict__ rec) {
    if (ctl[SEGC_STATUS] & SEG_ST_ARG) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ctl[SEGC_COUNT + SEG_CLASS_LONG] || i >= long_cap || i >= num_segments) return;
    const uint32_t s = list[i];
    uint32_t a = 0, len = 0;
    if (s < num_segments) {
        a = off[s];
        len = off[s + 1u] - a;
    }
    const uint32_t parts = (len + part - 1u) / part;
    const uint32_t first = parts != 0u ? atomicAdd(&ctl[SEG16C_UNITS], parts) : 0u;
    if (parts == 0u || first > unit_cap || parts > unit_cap - first) {
        rec[i] = uint4{0u, 0u, a, len};
        atomicOr(&ctl[SEG16C_INTERNAL], SR_ST_INTERNAL);
        return;
    }
    rec[i] = uint4{first, parts, a, len};
    for (uint32_t p = 0; p < parts; ++p) {
        const uint32_t lo = p * part;
        desc[first + p] = uint4{a, len, lo, len - lo < part ? len : lo + part};
    }
}

// table[unit][d] = keys of the unit's part whose byte at `shift` of the sortable bits is d.  Workgroup = unit (fixed grid).
__global__ __launch_bounds__(SR_THREADS) void seg16_count_kernel(const uint16_t* __restrict__ keys, const uint4* __restrict__ desc,
                                                                 const uint32_t* __restrict__ ctl, uint32_t unit_cap, uint32_t kt, uint32_t shift,
                                                                 uint32_t* __restrict__ table) {
    const uint32_t u = blockIdx.x;
    // (uniform; bad offsets claim no units; a rejected claim leaves descriptors unwritten: nothing is read through them)
    if (u >= unit_cap || u >= ctl[SEG16C_UNITS] || ctl[SEG16C_INTERNAL] != 0u) return;
    const uint4 d = desc[u];
    const uint32_t len = (d.z < d.w && d.w <= d.y) ? d.w - d.z : 0u;
    pass_count16_body(keys + d.x + d.z, len, kt, shift, table + (size_t)u * RADIX);
}

// One workgroup per long segment (fixed grid), thread = digit: sr_scan_kernel over the segment's units.
__global__ __launch_bounds__(RADIX) void seg16_scan_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ bases, const uint4* __restrict__ rec,
                                                           uint32_t* __restrict__ ctl, uint32_t unit_cap, uint32_t long_cap) {
    const uint32_t i = blockIdx.x;
    if ((ctl[SEGC_STATUS] & SEG_ST_ARG) || i >= long_cap || i >= ctl[SEGC_COUNT + SEG_CLASS_LONG]) return;  // (uniform)
    const uint4 r = rec[i];  // (first unit, parts, start, length)
    if (r.y == 0u || r.x > unit_cap || r.y > unit_cap - r.x) return;
    pass_scan_body(table + (size_t)r.x * RADIX, bases + (size_t)r.x * RADIX, r.y, r.w, ctl + SEG16C_INTERNAL);
}

// One workgroup per unit (fixed grid), its tiles in order: sr16_scatter_kernel with (row, part) replaced by the unit's descriptor.
// Positions are relative to the segment; the VM 1 form (argsort, first pass) makes start + position in registers.
template <int VM, int RANK>
__global__ __launch_bounds__(SR_THREADS) void seg16_scatter_kernel(const uint16_t* __restrict__ kin, const void* __restrict__ vin_, uint16_t* __restrict__ kout,
                                                                   void* __restrict__ vout_, const uint4* __restrict__ desc, uint32_t unit_cap, uint32_t kt,
                                                                   uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases,
                                                                   uint32_t* __restrict__ ctl) {
    using V = typename S16Val<VM>::type;
    const uint32_t u = blockIdx.x;
    if (u >= unit_cap || u >= ctl[SEG16C_UNITS]) return;  // (uniform)
    const uint4 d = desc[u];  // (start, length, part's first element, part's end)
    if (d.w > d.y) return;
    pass_scatter_body<uint16_t, VM, RANK>(kin + d.x, static_cast<const V*>(vin_) + ((VM == 4 || VM == 8) ? d.x : 0u), kout + d.x,
                                          static_cast<V*>(vout_) + (VM != 0 ? d.x : 0u), d.y, d.z, d.w, d.x, kt, shift, reverse,
                                          bases + (size_t)u * RADIX, ctl + SEG16C_INTERNAL);
}

#endif  // GS_SORT_ROWS_BUILT

}  // namespace gs
