// sortrows16_kernels.hpp — the row-wise sort of a [rows, row_len] matrix of 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16)
// at their own width: the pass route of gs_sort_rows16_* (include/gpusort.h).  No counterpart in the reference project.
//
// Rows that fit LDS are sorted in place by the 2-byte LDS sorts of the row-wise top-k (tkr16_wave_kernel / tkr16_tile_kernel of
// topk_rows16_kernels.hpp with k = row_len and the output pointers = the input pointers; DESIGN.md 3.14 holds the argument why that is
// sound).  Longer rows take TWO stable 8-bit LSD passes over ALL rows at once (low byte into the alternate buffers, high byte back),
// the pass of radix_pass.hpp, which tells its structure and invariants, on 2-byte keys: sr16_count_kernel per (row, part),
// sr_scan_kernel — as it is, one workgroup per row — and sr16_scatter_kernel per (row, part).  The argsort's positions are made in
// registers by the first pass.  Rows start wherever r * row_len * 2 bytes falls (every second row of an odd row_len starts 2 bytes
// off a dword): the count reads 16 bytes per thread behind a peel of up to seven elements and never outside its part, the scatter
// reads and writes one 2-byte element per lane, coalesced.
// Registers, LDS and scratch per kernel: DESIGN.md 3.14.
#pragma once
#include "sortrows_kernels.hpp"  // SR_* constants, sr_scan_kernel, the control block

namespace gs {

constexpr uint32_t SR16_PASSES = 2;

#if GS_SORT_ROWS_BUILT

// table[row][part][d] = keys of the part whose byte at `shift` of the sortable bits is d.  Workgroup = row * parts + part.
__global__ __launch_bounds__(SR_THREADS) void sr16_count_kernel(const uint16_t* __restrict__ keys, uint32_t row_len, uint32_t parts, uint32_t per_part,
                                                                uint32_t kt, uint32_t shift, uint32_t* __restrict__ table) {
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const uint32_t plo = part * per_part;
    const uint32_t len = plo < row_len ? (row_len - plo < per_part ? row_len - plo : per_part) : 0u;
    pass_count16_body(keys + (size_t)row * row_len + plo, len, kt, shift, table + (size_t)blockIdx.x * RADIX);
}

// One workgroup per (row, part), its tiles in order: pass_scatter_body on 2-byte keys.  VM: 0 keys only, 1 = the value is the element's
// position within its row (argsort, first pass: made in registers, 4 bytes, vin_ is not read), 4 / 8 = values of that width.
template <int VM, int RANK>
__global__ __launch_bounds__(SR_THREADS) void sr16_scatter_kernel(const uint16_t* __restrict__ kin, const void* __restrict__ vin_, uint16_t* __restrict__ kout,
                                                                  void* __restrict__ vout_, uint32_t row_len, uint32_t parts, uint32_t per_part, uint32_t kt,
                                                                  uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases, uint32_t* __restrict__ ctl) {
    using V = typename S16Val<VM>::type;
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const size_t row_at = (size_t)row * row_len;
    const uint32_t lo = part * per_part;
    const uint32_t hi = lo < row_len ? (row_len - lo < per_part ? row_len : lo + per_part) : lo;
    pass_scatter_body<uint16_t, VM, RANK>(kin + row_at, static_cast<const V*>(vin_) + ((VM == 4 || VM == 8) ? row_at : 0), kout + row_at,
                                          static_cast<V*>(vout_) + (VM != 0 ? row_at : 0), row_len, lo, hi, 0u, kt, shift, reverse,
                                          bases + (size_t)blockIdx.x * RADIX, ctl + SRC_STATUS);
}

#endif  // GS_SORT_ROWS_BUILT

}  // namespace gs
