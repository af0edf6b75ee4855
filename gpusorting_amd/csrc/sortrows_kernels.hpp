// sortrows_kernels.hpp — the row-wise sort of a [rows, row_len] matrix of 32-bit keys: the pass route of gs_sort_rows_* (include/gpusort.h).
// No counterpart in the reference project.
//
// Rows that fit LDS are sorted by the segmented sort's packed / wave / workgroup kernels (segsort_kernels.hpp) on the uniform offsets
// sr_offsets_kernel writes.  Longer rows take four stable 8-bit LSD passes over ALL rows at once, each count -> scan -> scatter in the
// structure of the 16-bit pairs sort (sort16_kernels.hpp): every row is cut into `parts` ranges of whole tiles (a tile never straddles
// two rows), sr_count_kernel writes one 256-bin digit histogram per (row, part), sr_scan_kernel — one workgroup per row — the
// exclusive prefix over (digit major, part minor) WITHIN the row, and sr_scatter_kernel — one workgroup per (row, part) — walks its
// tiles in order with running per-digit bases in LDS.  All positions are relative to the row.  Descending ranks in ascending space
// and lets the last pass write to row_len - 1 - position (the reverse-index rule of gs_onesweep_digit_pass).
//
// No kernel waits on another workgroup: no look-back, no chain, no ticket.  Every LDS and global store index is checked against its
// row's bounds; a row whose counts do not add up sets SR_ST_INTERNAL in the handle's status word, and a scatter that finds the word
// set writes nothing.  Rows start wherever they start (4-byte granularity): keys are read and written one dword per lane, coalesced.
// Registers, LDS and scratch per kernel: DESIGN.md 3.13.
#pragma once
#include "segsort_kernels.hpp"  // seg_to_bits
#include "sort16_kernels.hpp"   // s16_clear_kernel, S16Val

namespace gs {

constexpr uint32_t SR_THREADS = 512, SR_KPT = 8;
constexpr uint32_t SR_TILE = SR_THREADS * SR_KPT;  // elements ranked and staged at a time
constexpr uint32_t SR_PCAP = 1024;                 // workgroups (rows x parts) a pass aims at and, with more than one part per row, never exceeds
constexpr uint32_t SR_MIN_TILES = 2;               // tiles a part holds at least, unless the row has fewer
constexpr uint32_t SR_PASSES = 4;
constexpr uint32_t SRC_STATUS = 0, SRC_WORDS = 64;  // the handle's control block
constexpr uint32_t SR_ST_INTERNAL = 1;

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

// Thread = digit, over the `parts` tables at t: b[part][d] = keys of the row with a digit below d + keys of digit d in the parts in
// front; the row's total must be row_len, or `status` gets SR_ST_INTERNAL.  Shared with the segmented sort of 16-bit keys
// (seg16_scan_kernel, segsort16_kernels.hpp).
__device__ __forceinline__ void sr_scan_body(const uint32_t* __restrict__ t, uint32_t* __restrict__ b, uint32_t parts, uint32_t row_len,
                                             uint32_t* __restrict__ status) {
    constexpr uint32_t W = RADIX / 64;
    __shared__ uint32_t s_w[W];
    const uint32_t d = threadIdx.x, lane = d & 63u, wave = d >> 6;
    uint32_t total = 0;
#pragma unroll 8
    for (uint32_t p = 0; p < parts; ++p) total += t[p * RADIX + d];
    const uint32_t incl = wave_inclusive_scan(total, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t run = incl - total, all = 0;
    for (uint32_t x = 0; x < W; ++x) {
        if (x < wave) run += s_w[x];
        all += s_w[x];
    }
    if (d == 0 && all != row_len) atomicOr(status, SR_ST_INTERNAL);
#pragma unroll 8
    for (uint32_t p = 0; p < parts; ++p) {
        const uint32_t c = t[p * RADIX + d];
        b[p * RADIX + d] = run;
        run += c;
    }
}

// One workgroup per row, thread = digit: bases[row][part][d] = keys of the row with a digit below d + keys of digit d in the parts in
// front; the row's total must be row_len.
__global__ __launch_bounds__(RADIX) void sr_scan_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ bases, uint32_t parts, uint32_t row_len,
                                                        uint32_t* __restrict__ ctl) {
    sr_scan_body(table + (size_t)blockIdx.x * parts * RADIX, bases + (size_t)blockIdx.x * parts * RADIX, parts, row_len, ctl + SRC_STATUS);
}

// One workgroup per (row, part), its tiles in order: s16_scatter_kernel on 4-byte keys and positions relative to the row.  VB: 0 keys
// only, 4 / 8 = values of that width.  RANK 0: 64-lane ballot multi-split; 1: one returning LDS atomic per key (needs the lane-order
// probe, as everywhere).  A tile is ranked per wave (element wave * 512 + i * 64 + lane: rounds and lanes in element order, so ranks
// are stable), the wave counters are turned into tile positions, keys and values are staged in digit order and written out run by run;
// the running base of a digit moves on by the tile's count.  reverse != 0 (descending, last pass): position p goes to row_len - 1 - p.
template <int VB, int RANK>
__global__ __launch_bounds__(SR_THREADS) void sr_scatter_kernel(const uint32_t* __restrict__ kin, const void* __restrict__ vin_, uint32_t* __restrict__ kout,
                                                                void* __restrict__ vout_, uint32_t row_len, uint32_t parts, uint32_t per_part, uint32_t kt,
                                                                uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases, uint32_t* __restrict__ ctl) {
    using V = typename S16Val<VB>::type;
    constexpr uint32_t THREADS = SR_THREADS, KPT = SR_KPT, WAVES = THREADS / 64, TILE = SR_TILE;
    static_assert(WAVES * RADIX == 4u * THREADS, "one 16-byte store per thread clears the wave counters");
    __shared__ __attribute__((aligned(16))) uint32_t s_whist[WAVES * RADIX];
    __shared__ uint32_t s_key[TILE];  // raw keys
    __shared__ V s_val[VB != 0 ? TILE : 1];
    __shared__ uint32_t s_base[RADIX], s_gofs[RADIX], s_wtot[RADIX / 64], s_stop;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row = blockIdx.x / parts, part = blockIdx.x - row * parts;
    const size_t row_at = (size_t)row * row_len;
    const uint32_t* rkin = kin + row_at;
    uint32_t* rkout = kout + row_at;
    const V* rvin = static_cast<const V*>(vin_) + (VB != 0 ? row_at : 0);
    V* rvout = static_cast<V*>(vout_) + (VB != 0 ? row_at : 0);
    const uint32_t lo = part * per_part;
    if (tid == 0) s_stop = ctl[SRC_STATUS];
    __syncthreads();
    if (s_stop != 0u || lo >= row_len) return;  // (uniform; a count that did not add up was reported by the scan: nothing is written)
    const uint32_t hi = row_len - lo < per_part ? row_len : lo + per_part;
    if (tid < RADIX) s_base[tid] = bases[(size_t)blockIdx.x * RADIX + tid];  // (read and written by thread `tid` only)
    uint32_t* whist = s_whist + wave * RADIX;
    const uint32_t my_base = wave * (64u * KPT) + lane;
    for (uint32_t t0 = lo; t0 < hi; t0 += TILE) {
        const uint32_t m = hi - t0 < TILE ? hi - t0 : TILE;
        uint32_t key[KPT], bits[KPT], off[KPT];
        V val[KPT];
        // unconditional loads on a clamped index, masked afterwards
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) {
            const uint32_t idx = my_base + i * 64u, ci = idx < m ? idx : m - 1u;
            key[i] = rkin[t0 + ci];
            if constexpr (VB != 0) val[i] = rvin[t0 + ci];
        }
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) bits[i] = my_base + i * 64u < m ? seg_to_bits(key[i], kt) : 0xffffffffu;  // dummies: digit 255, highest slots
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
                    s_key[lpos] = key[i];
                    if constexpr (VB != 0) s_val[lpos] = val[i];
                } else {
                    atomicOr(&ctl[SRC_STATUS], SR_ST_INTERNAL);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) {
            const uint32_t j = tid + i * THREADS;
            if (j < m) {
                const uint32_t k = s_key[j];
                const uint32_t pos = s_gofs[(seg_to_bits(k, kt) >> shift) & 255u] + j;
                if (pos < row_len) {
                    const uint32_t o = reverse ? row_len - 1u - pos : pos;
                    rkout[o] = k;
                    if constexpr (VB != 0) rvout[o] = s_val[j];
                } else {
                    atomicOr(&ctl[SRC_STATUS], SR_ST_INTERNAL);
                }
            }
        }
        // the next tile's first barrier stands between these reads and the next writes of s_gofs and the staging
    }
}

#endif  // GS_SORT_ROWS_BUILT

}  // namespace gs
