// sortrows16_kernels.hpp — the row-wise sort of a [rows, row_len] matrix of 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16)
// at their own width: the pass route of gs_sort_rows16_* (include/gpusort.h).  No counterpart in the reference project.
//
// Rows that fit LDS are sorted in place by the 2-byte LDS sorts of the row-wise top-k (tkr16_wave_kernel / tkr16_tile_kernel of
// topk_rows16_kernels.hpp with k = row_len and the output pointers = the input pointers; DESIGN.md 3.14 holds the argument why that is
// sound).  Longer rows take TWO stable 8-bit LSD passes over ALL rows at once (low byte into the alternate buffers, high byte back),
// each count -> scan -> scatter in the structure of sortrows_kernels.hpp on 2-byte keys: every row is cut into `parts` ranges of whole
// tiles (a tile never straddles two rows), sr16_count_kernel writes one 256-bin digit histogram per (row, part), sr_scan_kernel — as
// it is, one workgroup per row — the exclusive prefix over (digit major, part minor) WITHIN the row, and sr16_scatter_kernel — one
// workgroup per (row, part) — walks its tiles in order with running per-digit bases in LDS.  All positions are relative to the row;
// the argsort's positions are made in registers by the first pass.  Descending ranks in ascending space and lets the last pass write
// to row_len - 1 - position (the reverse-index rule of gs_onesweep_digit_pass).
//
// No kernel waits on another workgroup: no look-back, no chain, no ticket.  Every LDS and global store index is checked against its
// row's bounds; a row whose counts do not add up sets SR_ST_INTERNAL in the handle's status word, and a scatter that finds the word
// set writes nothing.  Rows start wherever r * row_len * 2 bytes falls (every second row of an odd row_len starts 2 bytes off a
// dword): the count reads 16 bytes per thread behind a peel of up to seven elements and never outside its part, the scatter reads and
// writes one 2-byte element per lane, coalesced.  The all-one dummies of a tile's slots >= m tie with a real key whose sortable bits
// are 0xFFFF on both bytes: they stay behind it only because the ranking is stable and the dummies sit in the highest slots (in the
// RANK 1 form they take no part at all).  Whoever changes the dummies' place or the ranking's stability breaks that.
// Registers, LDS and scratch per kernel: DESIGN.md 3.14.
#pragma once
#include "sortrows_kernels.hpp"  // SR_* constants, sr_scan_kernel, the control block

namespace gs {

constexpr uint32_t SR16_PASSES = 2;
static_assert(SR_TILE == 8u * SR_THREADS, "the count reads one 16-byte vector of eight keys per thread and tile");

#if GS_SORT_ROWS_BUILT

// Eight elements from index i (a multiple of 8) of the 16-byte aligned pointer q, two to a word, the lower index in the low half;
// mask: which of them lie in [lo, hi).  A vector inside the range is one 16-byte load, every other one is loaded element by element:
// nothing outside [lo, hi) is read (the pattern of tkr16_load_chunk, decided per thread).
__device__ __forceinline__ uint4 sr16_load8(const uint16_t* q, uint32_t i, uint32_t lo, uint32_t hi, uint32_t& mask) {
    if (GS_LIKELY(i >= lo && i + 8u <= hi)) {
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

// The count of one part, shared with the segmented sort's long route (seg16_count_kernel, segsort16_kernels.hpp): out[d] = keys among
// the `len` elements at p whose byte at `shift` of the sortable bits is d.  The part is the index range [lo, hi) of the 16-byte aligned
// pointer q (lo <= 7: the peel; the base pointer is 16-byte aligned, so q never lies in front of it).  Every thread of the workgroup
// calls it (its barriers are the workgroup's); the LDS is its own.
__device__ __forceinline__ void sr16_count_body(const uint16_t* __restrict__ p, uint32_t len, uint32_t kt, uint32_t shift, uint32_t* __restrict__ out) {
    constexpr uint32_t W = SR_THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_h[W * RADIX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    reinterpret_cast<uint4*>(s_h)[tid] = uint4{0u, 0u, 0u, 0u};
    static_assert(W * RADIX == 4u * SR_THREADS, "one 16-byte store per thread clears the counters");
    __syncthreads();
    uint32_t* mine = s_h + wave * RADIX;
    if (len != 0u) {  // (uniform)
        const uint32_t lo = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 1) & 7u), hi = lo + len;
        const uint16_t* q = p - lo;
        for (uint32_t c = 0; c < hi; c += SR_TILE) {
            const uint32_t i = c + tid * 8u;
            uint32_t mask = 0u;
            uint4 t = uint4{0u, 0u, 0u, 0u};
            if (i < hi) t = sr16_load8(q, i, lo, hi, mask);
            const uint32_t w4[4] = {t.x, t.y, t.z, t.w};
            uint32_t d[8];
            bool one = true;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                d[j] = (tkr16_to_bits(tkr16_elem(w4, j), kt) >> shift) & 255u;
                one = one && d[j] == d[0];
            }
            const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
            if (__builtin_amdgcn_ballot_w64(mask == 255u && one && d[0] == f) == ~0ull) {  // the wave's 512 keys, all inside the part, share the digit: one add
                if (lane == 0) atomicAdd(&mine[f], 512u);
                continue;
            }
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                if ((mask >> j) & 1u) atomicAdd(&mine[d[j]], 1u);
        }
    }
    __syncthreads();
    if (tid < RADIX) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; ++w) sum += s_h[w * RADIX + tid];
        out[tid] = sum;
    }
}

// table[row][part][d] = keys of the part whose byte at `shift` of the sortable bits is d.  Workgroup = row * parts + part.
__global__ __launch_bounds__(SR_THREADS) void sr16_count_kernel(const uint16_t* __restrict__ keys, uint32_t row_len, uint32_t parts, uint32_t per_part,
                                                                uint32_t kt, uint32_t shift, uint32_t* __restrict__ table) {
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const uint32_t plo = part * per_part;
    const uint32_t len = plo < row_len ? (row_len - plo < per_part ? row_len - plo : per_part) : 0u;
    sr16_count_body(keys + (size_t)row * row_len + plo, len, kt, shift, table + (size_t)blockIdx.x * RADIX);
}

// One workgroup per (row, part), its tiles in order: sr_scatter_kernel on 2-byte keys.  VM: 0 keys only, 1 = the value is the element's
// position within its row (argsort, first pass: made in registers, 4 bytes, vin_ is not read), 4 / 8 = values of that width.  RANK 0:
// 64-lane ballot multi-split; 1: one returning LDS atomic per key (needs the lane-order probe, as everywhere).  A tile is ranked per
// wave (element wave * 512 + i * 64 + lane: rounds and lanes in element order, so ranks are stable), the wave counters are turned into
// tile positions, keys (at their own width) and values are staged in digit order and written out run by run; the running base of a
// digit moves on by the tile's count.  reverse != 0 (descending, last pass): position p goes to row_len - 1 - p.
//
// sr16_scatter_body: the scatter of one part [lo, hi) of a row of row_len elements, shared with the segmented sort's long route (seg16_scatter_kernel,
// segsort16_kernels.hpp).  rkin / rvin / rkout / rvout: the row's first element in each buffer; bases: the part's 256 bases (positions
// relative to the row); pos_base: what the VM 1 form adds to the position within the row; status: the word a broken count sets — a
// call that finds it set writes nothing.  Every thread of the workgroup calls it; the LDS is its own.
template <int VM, int RANK>
__device__ __forceinline__ void sr16_scatter_body(const uint16_t* __restrict__ rkin, const typename S16Val<VM>::type* __restrict__ rvin,
                                                  uint16_t* __restrict__ rkout, typename S16Val<VM>::type* __restrict__ rvout, uint32_t row_len,
                                                  uint32_t lo, uint32_t hi, uint32_t pos_base, uint32_t kt, uint32_t shift, uint32_t reverse,
                                                  const uint32_t* __restrict__ bases, uint32_t* __restrict__ status) {
    using V = typename S16Val<VM>::type;
    constexpr uint32_t THREADS = SR_THREADS, KPT = SR_KPT, WAVES = THREADS / 64, TILE = SR_TILE;
    static_assert(WAVES * RADIX == 4u * THREADS, "one 16-byte store per thread clears the wave counters");
    __shared__ __attribute__((aligned(16))) uint32_t s_whist[WAVES * RADIX];
    __shared__ uint16_t s_key[TILE];  // raw keys, at their own width
    __shared__ V s_val[VM != 0 ? TILE : 1];
    __shared__ uint32_t s_base[RADIX], s_gofs[RADIX], s_wtot[RADIX / 64], s_stop;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_stop = *status;
    __syncthreads();
    if (s_stop != 0u || lo >= hi) return;  // (uniform; a count that did not add up was reported by the scan: nothing is written)
    if (tid < RADIX) s_base[tid] = bases[tid];  // (read and written by thread `tid` only)
    uint32_t* whist = s_whist + wave * RADIX;
    const uint32_t my_base = wave * (64u * KPT) + lane;
    for (uint32_t t0 = lo; t0 < hi; t0 += TILE) {
        const uint32_t m = hi - t0 < TILE ? hi - t0 : TILE;
        uint32_t key[KPT], bits[KPT], off[KPT];
        V val[VM != 0 ? KPT : 1];
        // unconditional loads on a clamped index, masked afterwards
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) {
            const uint32_t idx = my_base + i * 64u, ci = idx < m ? idx : m - 1u;
            key[i] = rkin[t0 + ci];
            if constexpr (VM == 1) val[i] = pos_base + t0 + ci;  // the position within the row (+ the row's place in the array)
            else if constexpr (VM != 0) val[i] = rvin[t0 + ci];
        }
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) bits[i] = my_base + i * 64u < m ? tkr16_to_bits(key[i], kt) : 0xffffu;  // dummies: digit 255, highest slots
        reinterpret_cast<uint4*>(s_whist)[tid] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();  // (also: the previous tile's staging has been read)
        if constexpr (RANK == 0) {
#pragma unroll
            for (uint32_t i = 0; i < KPT; ++i) {
                const uint32_t d = (bits[i] >> shift) & 255u;
                uint32_t acc_lo = 0, acc_hi = 0;
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t B = (uint32_t)__builtin_amdgcn_sbfe((int32_t)bits[i], shift + k, 1);
                    const unsigned long long b = __builtin_amdgcn_ballot_w64(B != 0u);
                    acc_lo = __builtin_amdgcn_bitop3_b32(acc_lo, (uint32_t)b, B, 0xF6);
                    acc_hi = __builtin_amdgcn_bitop3_b32(acc_hi, (uint32_t)(b >> 32), B, 0xF6);
                }
                const uint32_t plo = ~acc_lo, phi = ~acc_hi;
                const uint32_t below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
                const uint32_t total = __popc(plo) + __popc(phi);
                const uint32_t pre = whist[d];
                if (below == total - 1u) whist[d] = pre + total;
                asm volatile("" ::: "memory");
                off[i] = pre + below;
            }
        } else {
            // slots >= m take no part: validity is a property of the slot
#pragma unroll
            for (uint32_t i = 0; i < KPT; ++i) {
                const uint32_t d = (bits[i] >> shift) & 255u;
                off[i] = 0;
                if (my_base + i * 64u < m) off[i] = __hip_atomic_fetch_add(&whist[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        uint32_t run = 0, scan_incl = 0;
        if (tid < RADIX) {
#pragma unroll
            for (uint32_t w = 0; w < WAVES; ++w) {
                const uint32_t c = s_whist[w * RADIX + tid];
                s_whist[w * RADIX + tid] = run;
                run += c;
            }
            scan_incl = wave_inclusive_scan(run, lane);
            if (lane == 63) s_wtot[wave] = scan_incl;
        }
        __syncthreads();
        if (tid < RADIX) {
            uint32_t wbase = 0;
            for (uint32_t w = 0; w < wave; ++w) wbase += s_wtot[w];
            const uint32_t dpre = wbase + scan_incl - run;  // the digit's first slot in the staged tile
#pragma unroll
            for (uint32_t w = 0; w < WAVES; ++w) s_whist[w * RADIX + tid] += dpre;
            s_gofs[tid] = s_base[tid] - dpre;  // staged slot j of this digit goes to s_gofs + j (may wrap: the sum does not)
            // the digit's count among the tile's m real keys (RANK 0 ranked the TILE - m dummies under digit 255 as well)
            s_base[tid] += (RANK == 0 && tid == RADIX - 1u) ? run - (TILE - m) : run;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) {
            const uint32_t lpos = off[i] + s_whist[wave * RADIX + ((bits[i] >> shift) & 255u)];
            if (my_base + i * 64u < m) {
                if (lpos < m) {
                    s_key[lpos] = (uint16_t)key[i];
                    if constexpr (VM != 0) s_val[lpos] = val[i];
                } else {
                    atomicOr(status, SR_ST_INTERNAL);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) {
            const uint32_t j = tid + i * THREADS;
            if (j < m) {
                const uint32_t k = s_key[j];
                const uint32_t pos = s_gofs[(tkr16_to_bits(k, kt) >> shift) & 255u] + j;
                if (pos < row_len) {
                    const uint32_t o = reverse ? row_len - 1u - pos : pos;
                    rkout[o] = (uint16_t)k;
                    if constexpr (VM != 0) rvout[o] = s_val[j];
                } else {
                    atomicOr(status, SR_ST_INTERNAL);
                }
            }
        }
        // the next tile's first barrier stands between these reads and the next writes of s_gofs and the staging
    }
}


template <int VM, int RANK>
__global__ __launch_bounds__(SR_THREADS) void sr16_scatter_kernel(const uint16_t* __restrict__ kin, const void* __restrict__ vin_, uint16_t* __restrict__ kout,
                                                                  void* __restrict__ vout_, uint32_t row_len, uint32_t parts, uint32_t per_part, uint32_t kt,
                                                                  uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases, uint32_t* __restrict__ ctl) {
    using V = typename S16Val<VM>::type;
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const size_t row_at = (size_t)row * row_len;
    const uint32_t lo = part * per_part;
    const uint32_t hi = lo < row_len ? (row_len - lo < per_part ? row_len : lo + per_part) : lo;
    sr16_scatter_body<VM, RANK>(kin + row_at, static_cast<const V*>(vin_) + ((VM == 4 || VM == 8) ? row_at : 0), kout + row_at,
                                static_cast<V*>(vout_) + (VM != 0 ? row_at : 0), row_len, lo, hi, 0u, kt, shift, reverse,
                                bases + (size_t)blockIdx.x * RADIX, ctl + SRC_STATUS);
}

#endif  // GS_SORT_ROWS_BUILT

}  // namespace gs
