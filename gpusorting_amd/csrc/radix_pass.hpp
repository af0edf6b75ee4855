// radix_pass.hpp — the one stable 8-bit LSD pass above the LDS limit, count -> scan -> scatter, that the sort of 16-bit keys
// (sort16_kernels.hpp), the row-wise sorts (sortrows_kernels.hpp, sortrows16_kernels.hpp), the segmented sort of 16-bit keys
// (segsort16_kernels.hpp) and the device route of the 32-bit segmented sort's long segments (segsort_long_kernels.hpp) run.  Those
// files hold the __global__ kernels: thin wrappers that turn their own work unit (a range of the array, a (row, part), a unit
// descriptor) into the arguments of the bodies here.  No counterpart in the reference project.
//
// Structure.  A "row" is what is sorted on its own: the whole array, a matrix row, a long segment.  It is cut into parts of whole
// tiles.  pass_count16_body writes one 256-bin digit histogram per part of 2-byte keys, pass_count32_body of 4-byte keys (another
// load pattern; sr_count_kernel keeps its own copy of that loop: as a wrapper of the body it compiled to 420 instructions and 38
// VGPRs instead of 410 and 36, with 52 SGPRs, 8192 bytes of LDS and no scratch either way), pass_scan_body — one
// workgroup per row, thread = digit — the exclusive prefix over (digit major, part minor) WITHIN the row, and pass_scatter_body —
// one workgroup per part — walks the part's tiles in order with running per-digit bases in LDS.  All positions are relative to the row.  Descending ranks in ascending space and lets the last
// pass write to row_len - 1 - position (the reverse-index rule of gs_onesweep_digit_pass): the exact reverse of the stable
// ascending result.
// No body waits on another workgroup: no look-back, no chain, no ticket.
//
// Stability.  A tile is ranked per wave, element wave * 512 + i * 64 + lane: rounds and lanes in element order, so within a wave the
// ranks rise with the element index (RANK 0: 64-lane ballot multi-split; RANK 1: one returning LDS atomic per key, which needs the
// lane-order probe, as everywhere); waves, tiles and parts follow one another in element order through the prefixes.
//
// Dummies.  The slots >= m of a partial tile hold all-one bits: digit 255 on every byte.  They tie with a real key whose sortable
// bits are all ones, and stay behind it only because the ranking is stable and the dummies sit in the HIGHEST slots (in the RANK 1
// form they take no part at all).  The RANK 0 form counts them under digit 255, hence the `run - (TILE - m)` when the base moves on.
// Whoever changes the dummies' place or the ranking's stability breaks that.
//
// Stop rule.  A row whose counts do not add up to its length sets PASS_ST_INTERNAL in the caller's status word (the scan), and a
// scatter that finds the word set writes nothing.
//
// Bounds.  The count reads nothing outside its part; the scatter loads on an index clamped to the tile; every LDS staging index is
// checked against m and every global store index against row_len, and a miss sets PASS_ST_INTERNAL instead of storing.
#pragma once
#include "topk_rows16_kernels.hpp"  // tkr16_to_bits, tkr16_elem
#include "segsort_kernels.hpp"      // seg_to_bits

namespace gs {

constexpr uint32_t PASS_THREADS = 512, PASS_KPT = 8;
constexpr uint32_t PASS_TILE = PASS_THREADS * PASS_KPT;  // elements ranked and staged at a time
constexpr uint32_t PASS_ST_INTERNAL = 1;                 // the status bit: a count did not add up, or an index left its bounds
static_assert(PASS_TILE == 8u * PASS_THREADS, "the count reads one 16-byte vector of eight keys per thread and tile");

// the pass and every sort built on it are in the product build only (as the segmented sort and the selection): the tuning and
// fault-injection flavours keep the constants and answer GS_ERR_MODE
#if !defined(GS_MINIMAL) && GS_EXP == 0
#define GS_SORT16_BUILT 1
#else
#define GS_SORT16_BUILT 0
#endif
#if GS_SORT16_BUILT

// the value type of a scatter form: 8-byte values, or 4 bytes (values, positions, or nothing)
template <int VM>
struct S16Val { using type = uint32_t; };
template <>
struct S16Val<8> { using type = uint64_t; };

// what the scatter needs to know about its key type K (the element type of the buffers and of the staged keys): raw key ->
// sortable bits, and the bits of a dummy
template <class K>
struct PassKey;
template <>
struct PassKey<uint16_t> {
    static constexpr uint32_t DUMMY = 0xffffu;
    static __device__ __forceinline__ uint32_t to_bits(uint32_t u, uint32_t kt) { return tkr16_to_bits(u, kt); }
};
template <>
struct PassKey<uint32_t> {
    static constexpr uint32_t DUMMY = 0xffffffffu;
    static __device__ __forceinline__ uint32_t to_bits(uint32_t u, uint32_t kt) { return seg_to_bits(u, kt); }
};

// Eight elements from index i (a multiple of 8) of the 16-byte aligned pointer q, two to a word, the lower index in the low half;
// mask: which of them lie in [lo, hi).  A vector inside the range is one 16-byte load, every other one is loaded element by element:
// nothing outside [lo, hi) is read (the pattern of tkr16_load_chunk, decided per thread).
__device__ __forceinline__ uint4 pass_load8(const uint16_t* q, uint32_t i, uint32_t lo, uint32_t hi, uint32_t& mask) {
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

// The count of one part of 2-byte keys: out[d] = keys among the `len` elements at p whose byte at `shift` of the sortable bits is d.
// The part is the index range [lo, hi) of the 16-byte aligned pointer q (lo <= 7: the peel; the buffer itself is 16-byte aligned, so
// q never lies in front of it).  Every thread of the workgroup calls it (its barriers are the workgroup's); the LDS is its own.
__device__ __forceinline__ void pass_count16_body(const uint16_t* __restrict__ p, uint32_t len, uint32_t kt, uint32_t shift, uint32_t* __restrict__ out) {
    constexpr uint32_t W = PASS_THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_h[W * RADIX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    reinterpret_cast<uint4*>(s_h)[tid] = uint4{0u, 0u, 0u, 0u};
    static_assert(W * RADIX == 4u * PASS_THREADS, "one 16-byte store per thread clears the counters");
    __syncthreads();
    uint32_t* mine = s_h + wave * RADIX;
    if (len != 0u) {  // (uniform)
        const uint32_t lo = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 1) & 7u), hi = lo + len;
        const uint16_t* q = p - lo;
        for (uint32_t c = 0; c < hi; c += PASS_TILE) {
            const uint32_t i = c + tid * 8u;
            uint32_t mask = 0u;
            uint4 t = uint4{0u, 0u, 0u, 0u};
            if (i < hi) t = pass_load8(q, i, lo, hi, mask);
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

// The count of one part of 4-byte keys (sr_count_kernel's loop): out[d] = keys among the `len` elements at p whose byte at `shift` of
// the sortable bits is d.  p is aligned to its element only (a row or a segment starts wherever it starts): one dword per lane,
// coalesced, unconditional loads on an index clamped to the tile.  The wave-uniform-digit shortcut is taken on full tiles only.
// Every thread of the workgroup calls it (its barriers are the workgroup's); the LDS is its own.
__device__ __forceinline__ void pass_count32_body(const uint32_t* __restrict__ p, uint32_t len, uint32_t kt, uint32_t shift, uint32_t* __restrict__ out) {
    constexpr uint32_t W = PASS_THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_h[W * RADIX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    reinterpret_cast<uint4*>(s_h)[tid] = uint4{0u, 0u, 0u, 0u};
    static_assert(W * RADIX == 4u * PASS_THREADS, "one 16-byte store per thread clears the counters");
    __syncthreads();
    uint32_t* mine = s_h + wave * RADIX;
    for (uint32_t c = 0; c < len; c += PASS_TILE) {
        const uint32_t m = len - c < PASS_TILE ? len - c : PASS_TILE;
        uint32_t d[PASS_KPT];
        // unconditional loads on a clamped index, masked afterwards
#pragma unroll
        for (uint32_t i = 0; i < PASS_KPT; ++i) {
            const uint32_t idx = tid + i * PASS_THREADS;
            d[i] = p[c + (idx < m ? idx : m - 1u)];
        }
        bool one = true;
#pragma unroll
        for (uint32_t i = 0; i < PASS_KPT; ++i) {
            d[i] = (seg_to_bits(d[i], kt) >> shift) & 255u;
            one = one && d[i] == d[0];
        }
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
        if (__builtin_amdgcn_ballot_w64(m == PASS_TILE && one && d[0] == f) == ~0ull) {  // the wave's 512 keys share the digit: one add
            if (lane == 0) atomicAdd(&mine[f], 64u * PASS_KPT);
            continue;
        }
#pragma unroll
        for (uint32_t i = 0; i < PASS_KPT; ++i)
            if (tid + i * PASS_THREADS < m) atomicAdd(&mine[d[i]], 1u);
    }
    __syncthreads();
    if (tid < RADIX) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; ++w) sum += s_h[w * RADIX + tid];
        out[tid] = sum;
    }
}

// The scan of one row, by a workgroup of RADIX threads, thread = digit, over the `parts` tables at t: b[part][d] = keys of the row
// with a digit below d + keys of digit d in the parts in front; the row's total must be row_len, or `status` gets PASS_ST_INTERNAL.
__device__ __forceinline__ void pass_scan_body(const uint32_t* __restrict__ t, uint32_t* __restrict__ b, uint32_t parts, uint32_t row_len,
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
    if (d == 0 && all != row_len) atomicOr(status, PASS_ST_INTERNAL);
#pragma unroll 8
    for (uint32_t p = 0; p < parts; ++p) {
        const uint32_t c = t[p * RADIX + d];
        b[p * RADIX + d] = run;
        run += c;
    }
}

// The scatter of one part [lo, hi) of a row of row_len elements of type K, its tiles in order.  rkin / rvin / rkout / rvout: the
// row's first element in each buffer; bases: the part's 256 bases (positions relative to the row); status: the word of the stop
// rule.  VM: 0 keys only, 1 = the value is pos_base + the element's position within its row (argsort, first pass: made in
// registers, 4 bytes, rvin is not read), 4 / 8 = values of that width.  RANK: see "Stability" above.  A tile is ranked per wave, the
// wave counters are turned into tile positions, keys (at their own width) and values are staged in digit order and written out run by
// run; the running base of a digit moves on by the tile's count.  reverse != 0 (descending, last pass): position p goes to
// row_len - 1 - p.  Every thread of the workgroup calls it; the LDS is its own.
template <class K, int VM, int RANK>
__device__ __forceinline__ void pass_scatter_body(const K* __restrict__ rkin, const typename S16Val<VM>::type* __restrict__ rvin, K* __restrict__ rkout,
                                                  typename S16Val<VM>::type* __restrict__ rvout, uint32_t row_len, uint32_t lo, uint32_t hi,
                                                  uint32_t pos_base, uint32_t kt, uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases,
                                                  uint32_t* __restrict__ status) {
    using V = typename S16Val<VM>::type;
    using KT = PassKey<K>;
    constexpr uint32_t THREADS = PASS_THREADS, KPT = PASS_KPT, WAVES = THREADS / 64, TILE = PASS_TILE;
    static_assert(WAVES * RADIX == 4u * THREADS, "one 16-byte store per thread clears the wave counters");
    __shared__ __attribute__((aligned(16))) uint32_t s_whist[WAVES * RADIX];
    __shared__ K s_key[TILE];  // raw keys, at their own width
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
        for (uint32_t i = 0; i < KPT; ++i) bits[i] = my_base + i * 64u < m ? KT::to_bits(key[i], kt) : KT::DUMMY;  // dummies: digit 255, highest slots
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
                    s_key[lpos] = (K)key[i];
                    if constexpr (VM != 0) s_val[lpos] = val[i];
                } else {
                    atomicOr(status, PASS_ST_INTERNAL);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < KPT; ++i) {
            const uint32_t j = tid + i * THREADS;
            if (j < m) {
                const uint32_t k = s_key[j];
                const uint32_t pos = s_gofs[(KT::to_bits(k, kt) >> shift) & 255u] + j;
                if (pos < row_len) {
                    const uint32_t o = reverse ? row_len - 1u - pos : pos;
                    rkout[o] = (K)k;
                    if constexpr (VM != 0) rvout[o] = s_val[j];
                } else {
                    atomicOr(status, PASS_ST_INTERNAL);
                }
            }
        }
        // the next tile's first barrier stands between these reads and the next writes of s_gofs and the staging
    }
}

#endif  // GS_SORT16_BUILT

}  // namespace gs
