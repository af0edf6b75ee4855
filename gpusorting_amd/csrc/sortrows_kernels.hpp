// sortrows_kernels.hpp — the row-wise sort of a [rows, row_len] matrix of 32-bit keys: the pass route of gs_sort_rows_* (include/gpusort.h).
// No counterpart in the reference project.
//
// Rows that fit LDS are sorted by the segmented sort's packed / wave / workgroup kernels (segsort_kernels.hpp) on the uniform offsets
// sr_offsets_kernel writes.  Longer rows take four stable 8-bit LSD passes over ALL rows at once, the pass of radix_pass.hpp, which
// tells its structure and invariants: every row is cut into `parts` ranges of whole tiles (a tile never straddles two rows),
// sr_count_kernel writes one 256-bin digit histogram per (row, part), sr_scan_kernel — one workgroup per row — the exclusive prefix
// WITHIN the row, and sr_scatter_kernel — one workgroup per (row, part) — walks its tiles in order.  Rows start wherever they start
// (4-byte granularity): keys are read and written one dword per lane, coalesced.
// Registers, LDS and scratch per kernel: DESIGN.md 3.13.
#pragma once
#include "sort16_kernels.hpp"  // s16_clear_kernel; through it radix_pass.hpp (the pass) and segsort_kernels.hpp (the short rows' kernels)

namespace gs {

constexpr uint32_t SR_THREADS = PASS_THREADS, SR_KPT = PASS_KPT, SR_TILE = PASS_TILE;  // the pass's tile
constexpr uint32_t SR_PCAP = 1024;                 // workgroups (rows x parts) a pass aims at and, with more than one part per row, never exceeds
constexpr uint32_t SR_MIN_TILES = 2;               // tiles a part holds at least, unless the row has fewer
constexpr uint32_t SR_PASSES = 4;
constexpr uint32_t SRC_STATUS = 0, SRC_WORDS = 64;  // the handle's control block
constexpr uint32_t SR_ST_INTERNAL = PASS_ST_INTERNAL;
static_assert(SR_THREADS == 512 && SR_KPT == 8 && SR_TILE == 4096 && SR_ST_INTERNAL == 1, "the pass's shape and status bit");

#define GS_SORT_ROWS_BUILT GS_SORT16_BUILT  // the product build only, as the segmented sort it runs short rows on
#if GS_SORT_ROWS_BUILT

// off[i] = i * row_len, i <= rows: the CSR offsets of a matrix, for the segmented sort's kernels
__global__ __launch_bounds__(256) void sr_offsets_kernel(uint32_t* __restrict__ off, uint32_t rows, uint32_t row_len) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= rows) off[i] = i * row_len;
}

// table[row][part][d] = keys of the part whose byte at `shift` of the sortable bits is d.  Workgroup = row * parts + part.
__global__ __launch_bounds__(SR_THREADS) void sr_count_kernel(const uint32_t* __restrict__ keys, uint32_t row_len, uint32_t parts, uint32_t per_part,
                                                              uint32_t kt, uint32_t shift, uint32_t* __restrict__ table) {
    constexpr uint32_t W = SR_THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_h[W * RADIX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    reinterpret_cast<uint4*>(s_h)[tid] = uint4{0u, 0u, 0u, 0u};
    static_assert(W * RADIX == 4u * SR_THREADS, "one 16-byte store per thread clears the counters");
    __syncthreads();
    uint32_t* mine = s_h + wave * RADIX;
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const uint32_t* rk = keys + (size_t)row * row_len;
    const uint32_t lo = part * per_part;
    const uint32_t hi = lo < row_len ? (row_len - lo < per_part ? row_len : lo + per_part) : lo;
    for (uint32_t c = lo; c < hi; c += SR_TILE) {
        const uint32_t m = hi - c < SR_TILE ? hi - c : SR_TILE;
        uint32_t d[SR_KPT];
        // unconditional loads on a clamped index, masked afterwards
#pragma unroll
        for (uint32_t i = 0; i < SR_KPT; ++i) {
            const uint32_t idx = tid + i * SR_THREADS;
            d[i] = rk[c + (idx < m ? idx : m - 1u)];
        }
        bool one = true;
#pragma unroll
        for (uint32_t i = 0; i < SR_KPT; ++i) {
            d[i] = (seg_to_bits(d[i], kt) >> shift) & 255u;
            one = one && d[i] == d[0];
        }
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
        if (__builtin_amdgcn_ballot_w64(m == SR_TILE && one && d[0] == f) == ~0ull) {  // the wave's 512 keys share the digit: one add
            if (lane == 0) atomicAdd(&mine[f], 64u * SR_KPT);
            continue;
        }
#pragma unroll
        for (uint32_t i = 0; i < SR_KPT; ++i)
            if (tid + i * SR_THREADS < m) atomicAdd(&mine[d[i]], 1u);
    }
    __syncthreads();
    if (tid < RADIX) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; ++w) sum += s_h[w * RADIX + tid];
        table[(size_t)blockIdx.x * RADIX + tid] = sum;
    }
}

// One workgroup per row, thread = digit: bases[row][part][d] = keys of the row with a digit below d + keys of digit d in the parts in
// front; the row's total must be row_len.
__global__ __launch_bounds__(RADIX) void sr_scan_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ bases, uint32_t parts, uint32_t row_len,
                                                        uint32_t* __restrict__ ctl) {
    pass_scan_body(table + (size_t)blockIdx.x * parts * RADIX, bases + (size_t)blockIdx.x * parts * RADIX, parts, row_len, ctl + SRC_STATUS);
}

// One workgroup per (row, part), its tiles in order: pass_scatter_body on 4-byte keys.  VB: 0 keys only, 4 / 8 = values of that width.
template <int VB, int RANK>
__global__ __launch_bounds__(SR_THREADS) void sr_scatter_kernel(const uint32_t* __restrict__ kin, const void* __restrict__ vin_, uint32_t* __restrict__ kout,
                                                                void* __restrict__ vout_, uint32_t row_len, uint32_t parts, uint32_t per_part, uint32_t kt,
                                                                uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases, uint32_t* __restrict__ ctl) {
    static_assert(VB == 0 || VB == 4 || VB == 8, "no positions made in registers on this route");
    using V = typename S16Val<VB>::type;
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const size_t row_at = (size_t)row * row_len;
    const uint32_t lo = part * per_part;
    const uint32_t hi = lo < row_len ? (row_len - lo < per_part ? row_len : lo + per_part) : lo;
    pass_scatter_body<uint32_t, VB, RANK>(kin + row_at, static_cast<const V*>(vin_) + (VB != 0 ? row_at : 0), kout + row_at,
                                          static_cast<V*>(vout_) + (VB != 0 ? row_at : 0), row_len, lo, hi, 0u, kt, shift, reverse,
                                          bases + (size_t)blockIdx.x * RADIX, ctl + SRC_STATUS);
}

#endif  // GS_SORT_ROWS_BUILT

}  // namespace gs
