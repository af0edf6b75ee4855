// kernel_registry.hpp — part of the gpusort_capi.hip translation unit: the launcher templates of every kernel family and the kernel
// registry, the one place that decides which kernel instantiations a build flavour compiles.
namespace {

// ---- launchers: one per kernel family, instantiated by the kernel registry below and nowhere else ------------------
struct Shape { int threads, kpt; };  // a workgroup's threads x keys per thread

using BinLauncher = void (*)(hipStream_t, uint32_t grid, uint32_t*, uint32_t*, void*, void*,
                             uint32_t* desc, uint32_t* counters, const uint32_t* info, uint32_t* hsub, uint32_t* status,
                             uint32_t n, uint32_t shift, uint32_t mode);

// VR 2: the two-round form of the 8-byte-value pass (two workgroups per CU), launched beside the one-round form in full sorts;
// the pass's PF_SKEW flag decides on the device which of the two works
template <int THREADS, int KPT, int VB, int KT, int RANK, int VR = 1>
void launch_bin(hipStream_t s, uint32_t grid, uint32_t* ka, uint32_t* kb, void* va, void* vb, uint32_t* desc,
                uint32_t* counters, const uint32_t* info, uint32_t* hsub, uint32_t* status, uint32_t n, uint32_t shift,
                uint32_t mode) {
    hipLaunchKernelGGL((gs::digit_binning_kernel<THREADS, KPT, VB, KT, RANK, VR>), dim3(grid), dim3(THREADS), 0, s, ka, kb,
                       va, vb, desc, counters, info, hsub, status, n, shift, mode);
}

// keys-only sorts of 32-bit keys on the default tile that the Scan kernel may plan on position chains (PF_POS, skewed keys): one
// launch per pass of the dual kernel — persistent workgroups that run the plain or the position-chain form, as planned.
// tile of the counting position-chain passes, as the Scan kernel takes it (bit 31: the plan's last pass runs on it as well).
// Keys-only: the full tile, counters packed 2 x 16 bit; pairs: 512 x 24 with 32-bit counters — and for 8-byte values in the last
// pass too (its two staging rounds run 9 % faster on the smaller tile, profiles/r04_pos_packed_counters.txt)
constexpr uint32_t POS_TILE = 512 * gs::POS_KPT;
inline uint32_t pos_tile_for(uint32_t vb) {
    return vb == 0 ? POS_TILE : (512u * gs::POSV_KPT) | ((vb == 8 && gs::POSV8_LAST_SMALL) ? 0x80000000u : 0u);
}
template <int KT, bool LAST>
void launch_dual(hipStream_t s, uint32_t grid, uint32_t* ka, uint32_t* kb, void* va, void* vb, uint32_t* desc, uint32_t* counters,
                 const uint32_t* info, uint32_t* hsub, uint32_t* status, uint32_t n, uint32_t shift, uint32_t mode) {
    hipLaunchKernelGGL((gs::digit_binning_dual_kernel<KT, LAST>), dim3(grid), dim3(512), 0, s, ka, kb, va, vb, desc, counters, info,
                       hsub, status, n, shift, mode);
}
// pairs: the position-chain form of the pass, launched beside the plain form(s)
template <int VB, int KT, bool LAST>
void launch_posv(hipStream_t s, uint32_t grid, uint32_t* ka, uint32_t* kb, void* va, void* vb, uint32_t* desc, uint32_t* counters,
                 const uint32_t* info, uint32_t* hsub, uint32_t* status, uint32_t n, uint32_t shift, uint32_t mode) {
    hipLaunchKernelGGL((gs::digit_binning_posv_kernel<VB, KT, LAST>), dim3(grid), dim3(512), 0, s, ka, kb, va, vb, desc, counters, info,
                       hsub, status, n, shift, mode);
}
// pairs on the two-level plan: the plain form of the pass as persistent workgroups; rank mode 1 only
template <int T, int K, int VB, int KT>
void launch_persist(hipStream_t s, uint32_t grid, uint32_t* ka, uint32_t* kb, void* va, void* vb, uint32_t* desc, uint32_t* counters,
                    const uint32_t* info, uint32_t* hsub, uint32_t* status, uint32_t n, uint32_t shift, uint32_t mode) {
    hipLaunchKernelGGL((gs::digit_binning_persist_kernel<T, K, VB, KT, 1>), dim3(grid), dim3(T), 0, s, ka, kb, va, vb, desc, counters, info, hsub,
                       status, n, shift, mode);
}

using HistLauncher = void (*)(hipStream_t, uint32_t, const uint32_t*, uint32_t*, size_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                              uint32_t*);
template <int KT>
void launch_hist(hipStream_t s, uint32_t blocks, const uint32_t* keys, uint32_t* slab, size_t used_words, uint32_t n,
                 uint32_t seg_len0, uint32_t p0, uint32_t np, uint32_t word, uint32_t allow_pos, uint32_t* partials) {
    hipLaunchKernelGGL((gs::global_histogram_kernel<KT>), dim3(blocks), dim3(gs::GHIST_THREADS), 0, s, keys, slab,
                       used_words, n, seg_len0, p0, np, word, allow_pos, partials);
    // the workgroups' tables -> the HIST region (one thread per bin)
    hipLaunchKernelGGL(gs::hist_reduce_kernel, dim3(np * gs::NCH * gs::RADIX / 64u), dim3(256), 0, s, partials, blocks,
                       np * gs::NCH * gs::RADIX, slab + gs::SLAB_HIST);
}

// ---- two-level plan (hybrid_kernels.hpp) ----
using HyHistLauncher = void (*)(hipStream_t, uint32_t grid, const uint32_t* keys, uint32_t* slab, size_t used_words, uint32_t n, uint32_t seg_len0,
                                uint32_t per_wg, uint32_t wg_per_seg, uint32_t* slices, uint32_t cap);
template <int KT>
void launch_hy_hist(hipStream_t s, uint32_t grid, const uint32_t* keys, uint32_t* slab, size_t used_words, uint32_t n, uint32_t seg_len0,
                    uint32_t per_wg, uint32_t wg_per_seg, uint32_t* slices, uint32_t cap) {
    hipLaunchKernelGGL((gs::hy_histogram_kernel<KT>), dim3(grid), dim3(gs::HY_HIST_THREADS), 0, s, keys, slab, used_words, n, seg_len0, per_wg,
                       wg_per_seg, slices, cap);
}
using HyLocalLauncher = void (*)(hipStream_t, uint32_t grid, uint32_t* keys, const uint32_t* tab, uint32_t* slab, uint32_t n, uint32_t descending);
template <int KT, int T, int K, bool HALF>
void launch_hy_local(hipStream_t s, uint32_t grid, uint32_t* keys, const uint32_t* tab, uint32_t* slab, uint32_t n, uint32_t descending) {
    hipLaunchKernelGGL((gs::hy_local_sort_kernel<KT, T, K, HALF>), dim3(grid), dim3(T), 0, s, keys, tab, slab, n, descending);
}
using HyLocalPairsLauncher = void (*)(hipStream_t, uint32_t* keys, void* vals, const uint32_t* tab, const uint32_t* slab, uint32_t n, uint32_t descending);
template <int KT, int VB, int T, int K>
void launch_hy_local_pairs(hipStream_t s, uint32_t* keys, void* vals, const uint32_t* tab, const uint32_t* slab, uint32_t n, uint32_t descending) {
    hipLaunchKernelGGL((gs::hy_local_sort_pairs_kernel<KT, VB, T, K>), dim3(gs::HY_BINS), dim3(T), 0, s, keys, vals, tab, slab, n, descending);
}
// the local sort's workgroup by the mean bucket n / 65 536: it holds 1.5 x the mean at the top of its class (uniform keys stay within
// a few per cent of the mean; what does not fit sends the sort to the LSD passes).  Tests force a class at any n (gs_debug_set_hy_class;
// hy_class_of in onesweep_host.hpp): a bucket of exactly cap keys then takes a sort of 2^21 keys, not of 2^28
struct HyLocalClass {
    uint32_t max_n;
    int threads, kpt;
    constexpr uint32_t cap() const { return (uint32_t)threads * kpt; }
};
constexpr HyLocalClass g_hy_class[4] = {{1u << 27, 256, 12}, {1u << 28, 512, 12}, {1u << 29, 1024, 12}, {GS_MAX_KEYS, 1024, 24}};
// the keys-only kernel's own workgroup per class: the same cap on a shape of its own.  Class 1 sorts 256 x 24 on 16-bit halves (HALF of
// hy_local_sort_kernel): half the waves per bucket, 64 registers and 14 KiB of LDS, so that eight buckets are resident per CU
// instead of four (profiles/local_sort_residency_ab.txt)
struct HyKeysShape {
    int threads, kpt;
    bool half;
};
constexpr HyKeysShape g_hy_keys_shape[4] = {{256, 12, false}, {256, 24, true}, {1024, 12, false}, {1024, 24, false}};
constexpr bool hy_keys_shapes_hold_cap() {
    for (int c = 0; c < 4; ++c)
        if ((uint32_t)g_hy_keys_shape[c].threads * g_hy_keys_shape[c].kpt != g_hy_class[c].cap()) return false;
    return true;
}
static_assert(hy_keys_shapes_hold_cap(), "the histogram's cap and the plan's validity are decided on g_hy_class");
inline int hy_class(uint32_t n) { return n <= g_hy_class[0].max_n ? 0 : n <= g_hy_class[1].max_n ? 1 : n <= g_hy_class[2].max_n ? 2 : 3; }
constexpr uint32_t HY_MIN_PAIRS_DEFAULT = (1u << 25) + 1u;  // pairs: from where the position-chain plan (its fall-back) starts — at 2^25 pairs the two-level plan already wins (61.6 against 58.8, 44.6 against 40.4 GKeys/s with 4- / 8-byte values), at 2^24 it loses
constexpr uint32_t HY_MIN_KEYS_DEFAULT = 3u << 24;  // 50 M keys: measured, the LSD passes win at 2^25 (121 against 102 GKeys/s), the two-level plan at 2^26 (139 against 122): below, its 65 536 buckets are a few hundred keys each and a workgroup per bucket is mostly launch (profiles/r05_two_level_threshold.txt)

// ---- single-tile fast path: one launch, no scan state ----
using SmallLauncher = void (*)(hipStream_t, uint32_t*, void*, uint32_t, uint32_t, uint32_t*);
template <int T, int K, int VB, int KT, int RANK>
void launch_small(hipStream_t s, uint32_t* keys, void* vals, uint32_t n, uint32_t descending, uint32_t* status) {
    hipLaunchKernelGGL((gs::small_sort_kernel<T, K, VB, KT, RANK>), dim3(1), dim3(T), 0, s, keys, vals, n, descending, status);
}
// size classes by slots: 8192 slots (every mode), 16384 (keys-only and 4-byte values), 32768 (keys-only) — what fits 160 KiB of LDS;
// 64-bit keys: the classes up to 8192 slots.  The two smallest classes (256 x 4 and 256 x 8 slots) exist because a sort of 2^10 keys
// in the 8192-slot shape pays for 8192 slots in every pass: 10.5 us against 8.1 (profiles/r04_small_shapes.txt; the reference's size
// sweep starts there, GPUSortingD3D12/Tests.h:392-393,415-416)
constexpr Shape g_small_class[5] = {{256, 4}, {256, 8}, {512, 16}, {1024, 16}, {1024, 32}};
inline int small_class(uint32_t n) { return n <= 1024 ? 0 : n <= 2048 ? 1 : n <= 8192 ? 2 : n <= 16384 ? 3 : n <= 32768 ? 4 : 5; }

// ---- segmented sort (segsort_kernels.hpp): the workgroup classes run the single-tile sort on the shapes of g_small_class ----
using SegWgLauncher = void (*)(hipStream_t, uint32_t grid, uint32_t* keys, void* vals, const uint32_t* off, const uint32_t* list,
                               const uint32_t* ctl, uint32_t num_segments, uint32_t cls, uint32_t descending);
constexpr bool SEG_WG_LOOP(int threads, int kpt) { return threads * kpt < 32768; }  // the 1024 x 32 shape: one workgroup per possible segment
template <int T, int K, int VB, int KT, int RANK>
void launch_seg_wg(hipStream_t s, uint32_t grid, uint32_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
                   uint32_t num_segments, uint32_t cls, uint32_t descending) {
    hipLaunchKernelGGL((gs::seg_wg_kernel<T, K, VB, KT, RANK, SEG_WG_LOOP(T, K)>), dim3(grid), dim3(T), 0, s, keys, vals, off, list, ctl, num_segments, cls, descending);
}
// the kernels that do not depend on the key type (it is a run-time argument there): packed class, wave class, head merge
struct SegVbLaunchers {
    void (*packed)(hipStream_t, uint32_t grid, uint32_t* keys, void* vals, const uint32_t* off, uint32_t num_segments, uint32_t max_len,
                   uint32_t kt, uint32_t descending, const uint32_t* ctl);
    void (*wave)(hipStream_t, uint32_t grid, uint32_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
                 uint32_t num_segments, uint32_t kt, uint32_t descending);
    void (*merge_head)(hipStream_t, uint32_t grid, const uint32_t* keys, const void* vals, uint32_t* alt_keys, void* alt_vals, uint32_t start,
                       uint32_t head, uint32_t len, uint32_t kt, uint32_t descending);
};
template <int VB>
constexpr SegVbLaunchers seg_vb_launchers() {
    return {
        [](hipStream_t s, uint32_t grid, uint32_t* keys, void* vals, const uint32_t* off, uint32_t num_segments, uint32_t max_len, uint32_t kt,
           uint32_t descending, const uint32_t* ctl) {
            hipLaunchKernelGGL((gs::seg_packed_kernel<VB>), dim3(grid), dim3(64), 0, s, keys, vals, off, num_segments, max_len, kt, descending, ctl);
        },
        [](hipStream_t s, uint32_t grid, uint32_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
           uint32_t num_segments, uint32_t kt, uint32_t descending) {
            hipLaunchKernelGGL((gs::seg_wave_kernel<VB>), dim3(grid), dim3(64), 0, s, keys, vals, off, list, ctl, num_segments, kt, descending);
        },
        [](hipStream_t s, uint32_t grid, const uint32_t* keys, const void* vals, uint32_t* alt_keys, void* alt_vals, uint32_t start, uint32_t head,
           uint32_t len, uint32_t kt, uint32_t descending) {
            hipLaunchKernelGGL((gs::seg_merge_head_kernel<VB>), dim3(grid), dim3(256), 0, s, keys, vals, alt_keys, alt_vals, start, head, len, kt,
                               descending);
        }};
}

// ---- row-wise top-k (topk_rows_kernels.hpp, topk_rows16_kernels.hpp): VM 0 keys only, 1 positions, 4 / 8 value bytes ----
using TkrLauncher = void (*)(hipStream_t, uint32_t grid, const gs::TkrArgs& a);
// K16 1: the kernel for 2-byte keys
template <int VM, int K16>
void launch_tkr_wave(hipStream_t s, uint32_t grid, const gs::TkrArgs& a) {
    if constexpr (K16) hipLaunchKernelGGL((gs::tkr16_wave_kernel<VM>), dim3(grid), dim3(64 * gs::TKR_WAVE_ROWS), 0, s, a);
    else hipLaunchKernelGGL((gs::tkr_wave_kernel<VM>), dim3(grid), dim3(64 * gs::TKR_WAVE_ROWS), 0, s, a);
}
template <int T, int K, int VM, int RANK, int K16>
void launch_tkr_tile(hipStream_t s, uint32_t grid, const gs::TkrArgs& a) {
    if constexpr (K16) hipLaunchKernelGGL((gs::tkr16_tile_kernel<T, K, VM, RANK>), dim3(grid), dim3(T), 0, s, a);
    else hipLaunchKernelGGL((gs::tkr_tile_kernel<T, K, VM, RANK>), dim3(grid), dim3(T), 0, s, a);
}
template <int VM, int K16>
void launch_tkr_stream(hipStream_t s, uint32_t grid, const gs::TkrArgs& a) {
    if constexpr (K16) hipLaunchKernelGGL((gs::tkr16_stream_kernel<VM, 0>), dim3(grid), dim3(gs::TKR_THREADS), 0, s, a);
    else hipLaunchKernelGGL((gs::tkr_stream_kernel<VM, 0>), dim3(grid), dim3(gs::TKR_THREADS), 0, s, a);
}
constexpr int VM_OF[4] = {0, 1, 4, 8};  // value mode by vm index

// ---- mid sizes: two launches (mid_kernels.hpp) ----
using MidLauncher = void (*)(hipStream_t, uint32_t n_tiles, uint32_t* keys, uint32_t* alt, void* vals, void* valt, uint32_t* scratch,
                             uint32_t* status, uint32_t n, uint32_t descending);
template <int VB, int KT, int RANK, int T, int K, int T2, int K2>
void launch_mid(hipStream_t s, uint32_t tiles, uint32_t* keys, uint32_t* alt, void* vals, void* valt, uint32_t* scratch, uint32_t* status,
                uint32_t n, uint32_t descending) {
    hipLaunchKernelGGL((gs::mid_msd_kernel<VB, KT, RANK, T, K, T2 * K2>), dim3(tiles), dim3(T), 0, s, keys, alt, vals, valt, scratch, status,
                       n, descending);
    hipLaunchKernelGGL((gs::bucket_sort_kernel<VB, KT, RANK, T2, K2>), dim3(gs::RADIX), dim3(T2), 0, s, keys, alt, vals, valt, scratch,
                       status, n, descending);
}
// Classes by the bucket K2 can hold: 8192 keys (n <= 2^20, every value width; K1: <= 128 tiles of 8192), 16 384 (n <= 2^21, keys-only
// and 4-byte values; K1: <= 128 tiles of 16 384), 32 768 (n <= 2^22, keys-only; K1: <= 256 tiles of 16 384 — the 32 768-key tile
// spilled there and kept half the CUs idle, 44 us of a 67 us sort, profiles/r03_mid_size_timeline.txt).
// Round 5: class 3 — keys-only up to 2^23 (K1: 256 tiles of 32 768, one per CU; K2 holds 34 816 keys: 6 % above the mean bucket) — and
// class 4 — 4-byte values up to 2^22 pairs (K1: 256 tiles of 16 384; K2 holds 17 408 pairs): 74.6 -> 102 GKeys/s at 2^23 keys,
// profiles/r05_mid_classes.txt.  K1's tiles: never more than fit the chip at once (512 tiles of 16 384 keys for 2^23 keys left half of
// them to be adopted one by one — 1.7 ms).
struct MidClass {
    int threads, kpt;    // K1 (mid_msd_kernel): its tile
    int threads2, kpt2;  // K2 (bucket_sort_kernel): the bucket it holds
    uint32_t max_tiles;  // K1's tiles at most (<= MID_MAX_TILES)
    constexpr uint32_t tile() const { return (uint32_t)threads * kpt; }
};
constexpr MidClass g_mid_class[5] = {{512, 16, 512, 16, 128}, {512, 32, 512, 32, 128}, {512, 32, 1024, 32, 256}, {1024, 32, 1024, 34, 256},
                                     {512, 32, 512, 34, 256}};
static_assert(g_mid_class[3].max_tiles <= gs::MID_MAX_TILES && g_mid_class[4].max_tiles <= gs::MID_MAX_TILES, "mid-size classes");
// class of a mid-size sort, -1: the general pipeline
inline int mid_class(uint32_t n, uint32_t vb) {
    auto fits = [n](int c) { return n <= g_mid_class[c].max_tiles * g_mid_class[c].tile(); };
    if (fits(0)) return 0;
    if (fits(1) && vb != 8) return 1;
    if (fits(2) && vb == 0) return 2;
    if (fits(3) && vb == 0) return 3;
    if (fits(4) && vb == 4) return 4;
    return -1;
}

// ---- kernel registry ------------------------------------------------------------------------------------------------
// Which kernel instantiations this build compiles: one predicate per family — the only place that reads the build flavour — and
// one lookup per family, which returns the launcher for run-time parameters or nullptr if that combination is not built (left out
// of this build flavour, or not existing by design: 64-bit keys on tiles above 8192 keys, the 24 576-pair local sort with 8-byte
// values, single-tile and mid-size classes that do not fit LDS).  Nothing the predicates reject is instantiated.
//   GS_MINIMAL (experiment builds, libgpusort_tuning.so): u32 keys-only kernels, plus the histogram of every key type — a 10 s compile;
//   GS_TUNING: three more tile shapes for on-device tuning sweeps (u32 keys only).
#ifdef GS_MINIMAL
constexpr bool FULL = false;
#else
constexpr bool FULL = true;
#endif
// tile shapes of the binning passes; shape 0 is the default
constexpr Shape g_shapes[] = {
    {512, 32},   // default for keys-only and 8-byte values: 16384-key tiles, 2 workgroups per CU
    {1024, 16},  // default for 4-byte values (measured best, profiles/r01_sweep_v16_*)
    {512, 16},   // mid sizes (n <= mid_keys): 8192-key tiles, shorter per-tile latency, more workgroups;
                 // and the shape of 64-bit keys at every size (8-byte stage slots: 64 KiB per tile)
#ifdef GS_TUNING  // tuning build only (libgpusort_tuning.so)
    {256, 32}, {256, 16},
    {512, 20},  // 10 240-key tiles: 52 KiB of LDS, three workgroups per CU
#endif
};
constexpr int g_num_shapes = sizeof(g_shapes) / sizeof(g_shapes[0]);
constexpr int MID_SHAPE = 2;  // g_shapes index used for n <= mid_keys(vb) unless the caller picked a shape
constexpr int NKT = 6;               // key types: 3 x 32-bit, 3 x 64-bit
constexpr int VB_OF[3] = {0, 4, 8};  // value bytes by vb index
constexpr bool key32(int kt) { return FULL ? kt < 3 : kt == 0; }  // 32-bit key types of the keys-only kernels

// digit_binning_kernel (vr 1: every shape and rank mode; vr 2: the two-round form of 8-byte values on the default tile)
constexpr bool bin_built(int shape, int vb, int kt, int vr) {
    if (vr == 2) return FULL && shape == 0 && vb == 8 && kt < 3;
    if (!FULL) return vb == 0 && kt == 0;
    return shape == MID_SHAPE || (shape < 3 ? kt < 3 : kt == 0);  // 64-bit keys on 512 x 16 only; the tuning shapes: u32 keys
}
// the position-chain forms, last pass or not: digit_binning_dual_kernel (keys-only) and digit_binning_posv_kernel (pairs)
constexpr bool pos_built(int vb, int kt) { return vb == 0 ? key32(kt) : FULL && kt < 3; }
// digit_binning_persist_kernel (pairs on the two-level plan; 4-byte values on 1024 x 16, 8-byte values on 512 x 32);
// hy_local_sort_pairs_kernel (all four classes with 4-byte values, the first three with 8-byte values)
constexpr bool persist_built(int kt) { return FULL && kt < 3; }
constexpr bool hy_pairs_built(int vb, int cls, int kt) { return FULL && kt < 3 && !(vb == 8 && cls == 3); }
// hy_histogram_kernel and hy_local_sort_kernel: key32(kt); global_histogram_kernel: every key type
// small_sort_kernel: classes 0-2 take every value width and key type, class 3 keys-only and 4-byte values, class 4 keys-only
constexpr bool small_built(int cls, int vb, int kt) { return FULL && (cls < 3 || (kt < 3 && (cls == 3 ? vb != 8 : vb == 0))); }
// mid_msd_kernel + bucket_sort_kernel: the value widths of mid_class
constexpr bool mid_built(int cls, int vb, int kt) {
    return FULL && kt < 3 && (cls == 0 || (cls == 1 ? vb != 8 : cls == 4 ? vb == 4 : vb == 0));
}
// the segmented sort's kernels: in the product build only (the fault-injection and tuning builds answer GS_ERR_MODE); workgroup class
// c runs on g_small_class[c] and takes the value widths that shape holds: classes 0-2 all, class 3 no 8-byte values, class 4 keys only
constexpr bool SEG_BUILT = FULL && GS_EXP == 0;
constexpr bool seg_built(int cls, int vb, int kt) { return SEG_BUILT && kt < 3 && small_built(cls, vb, kt); }
// the selection's kernels (topk_kernels.hpp, topk_rows_kernels.hpp, topk_rows16_kernels.hpp): the product build only, as the segmented
// sort.  The row-wise tile kernel runs on g_small_class[c] with the value widths that shape holds (positions are 4-byte values), for
// 4-byte and for 2-byte keys alike (the row-length borders of the routes are the same)
constexpr bool TK_BUILT = SEG_BUILT;
constexpr bool tkr_tile_built(int cls, int vm) { return TK_BUILT && small_built(cls, vm == 0 ? 0 : vm == 8 ? 8 : 4, 0); }

// A launcher table over D0 x D1 x ... (row-major): entry = f(c0, c1, ...), every coordinate a std::integral_constant, so that
// f instantiates nothing but what it returns.
template <int... D>
struct Table {
    template <class F> static constexpr auto make(F f) { return make_(f, std::make_integer_sequence<int, (D * ...)>{}); }
    static constexpr int index(std::array<int, sizeof...(D)> c) {
        int i = 0, k = 0;
        for (int d : {D...}) i = i * d + c[k++];
        return i;
    }
    // for gs_debug_registry_*: the extents -> out, returns how many; the index of a caller's coordinate, -1 if it lies outside
    static int extents(int32_t* out) {
        int k = 0;
        for (int d : {D...}) out[k++] = d;
        return k;
    }
    static int checked_index(const int32_t* c) {
        int i = 0, k = 0;
        for (int d : {D...}) {
            if (c[k] < 0 || c[k] >= d) return -1;
            i = i * d + c[k++];
        }
        return i;
    }
  private:
    static constexpr int coord(int i, int k) {
        const int d[] = {D...};
        for (int j = (int)sizeof...(D) - 1; j > k; --j) i /= d[j];
        return i % d[k];
    }
    template <int I, class F, size_t... K>
    static constexpr auto entry(F f, std::index_sequence<K...>) { return f(std::integral_constant<int, coord(I, K)>{}...); }
    template <class F, int... I>
    static constexpr auto make_(F f, std::integer_sequence<int, I...>) { return std::array{entry<I>(f, std::make_index_sequence<sizeof...(D)>{})...}; }
};

using BinTable = Table<2, g_num_shapes, 2, 3, NKT>;  // [vr - 1][shape][rank mode][vb index][key type]
constexpr auto g_bin = BinTable::make([](auto vr1, auto s, auto r, auto v, auto kt) -> BinLauncher {
    if constexpr (bin_built(s, VB_OF[v], kt, vr1 + 1)) return launch_bin<g_shapes[s].threads, g_shapes[s].kpt, VB_OF[v], kt, r, vr1 + 1>;
    else return nullptr;
});
using PosTable = Table<3, 2, NKT>;  // [vb index][last pass][key type]
constexpr auto g_pos = PosTable::make([](auto v, auto last, auto kt) -> BinLauncher {
    if constexpr (!pos_built(VB_OF[v], kt)) return nullptr;
    else if constexpr (v == 0) return launch_dual<kt, last == 1>;
    else return launch_posv<VB_OF[v], kt, last == 1>;
});
using PersistTable = Table<2, NKT>;  // [8-byte values][key type]
constexpr auto g_persist = PersistTable::make([](auto v8, auto kt) -> BinLauncher {
    if constexpr (!persist_built(kt)) return nullptr;
    else if constexpr (v8 == 0) return launch_persist<1024, 16, 4, kt>;
    else return launch_persist<512, 32, 8, kt>;
});
constexpr auto g_hist = Table<NKT>::make([](auto kt) -> HistLauncher { return launch_hist<kt>; });
constexpr auto g_hy_hist = Table<NKT>::make([](auto kt) -> HyHistLauncher {
    if constexpr (key32(kt)) return launch_hy_hist<kt>;
    else return nullptr;
});
using HyTable = Table<4, NKT>;  // [class][key type]
constexpr auto g_hy_local = HyTable::make([](auto c, auto kt) -> HyLocalLauncher {
    if constexpr (key32(kt)) return launch_hy_local<kt, g_hy_keys_shape[c].threads, g_hy_keys_shape[c].kpt, g_hy_keys_shape[c].half>;
    else return nullptr;
});
using HyPairsTable = Table<2, 4, NKT>;  // [8-byte values][class][key type]
constexpr auto g_hy_local_pairs = HyPairsTable::make([](auto v8, auto c, auto kt) -> HyLocalPairsLauncher {
    if constexpr (hy_pairs_built(v8 ? 8 : 4, c, kt)) return launch_hy_local_pairs<kt, v8 ? 8 : 4, g_hy_class[c].threads, g_hy_class[c].kpt>;
    else return nullptr;
});
using SmallTable = Table<5, 2, 3, NKT>;  // [class][rank mode][vb index][key type]
constexpr auto g_small = SmallTable::make([](auto c, auto r, auto v, auto kt) -> SmallLauncher {
    if constexpr (small_built(c, VB_OF[v], kt)) return launch_small<g_small_class[c].threads, g_small_class[c].kpt, VB_OF[v], kt, r>;
    else return nullptr;
});
using MidTable = Table<5, 2, 3, NKT>;  // [class][rank mode][vb index][key type]
constexpr auto g_mid = MidTable::make([](auto c, auto r, auto v, auto kt) -> MidLauncher {
    constexpr MidClass m = g_mid_class[c];
    if constexpr (mid_built(c, VB_OF[v], kt)) return launch_mid<VB_OF[v], kt, r, m.threads, m.kpt, m.threads2, m.kpt2>;
    else return nullptr;
});
using SegWgTable = Table<5, 2, 3, 3>;  // [workgroup class][rank mode][vb index][32-bit key type]
constexpr auto g_seg_wg = SegWgTable::make([](auto c, auto r, auto v, auto kt) -> SegWgLauncher {
    if constexpr (seg_built(c, VB_OF[v], kt)) return launch_seg_wg<g_small_class[c].threads, g_small_class[c].kpt, VB_OF[v], kt, r>;
    else return nullptr;
});
constexpr auto g_seg_vb = Table<3>::make([](auto v) -> SegVbLaunchers {
    if constexpr (SEG_BUILT) return seg_vb_launchers<VB_OF[v]>();
    else return SegVbLaunchers{nullptr, nullptr, nullptr};
});

using TkrTileTable = Table<2, 5, 2, 4>;  // [2-byte keys][workgroup class][rank mode][vm index]
constexpr auto g_tkr_tile = TkrTileTable::make([](auto k16, auto c, auto r, auto v) -> TkrLauncher {
    if constexpr (tkr_tile_built(c, VM_OF[v])) return launch_tkr_tile<g_small_class[c].threads, g_small_class[c].kpt, VM_OF[v], r, k16>;
    else return nullptr;
});
struct TkrVmLaunchers { TkrLauncher wave, stream; };  // the kernels with one shape
using TkrVmTable = Table<2, 4>;  // [2-byte keys][vm index]
constexpr auto g_tkr_vm = TkrVmTable::make([](auto k16, auto v) -> TkrVmLaunchers {
    if constexpr (TK_BUILT) return TkrVmLaunchers{launch_tkr_wave<VM_OF[v], k16>, launch_tkr_stream<VM_OF[v], k16>};
    else return TkrVmLaunchers{nullptr, nullptr};
});

inline int vb_index(uint32_t vb) { return vb == 0 ? 0 : vb == 4 ? 1 : 2; }
BinLauncher bin_launcher(int shape, int rank, uint32_t vb, int kt, int vr = 1) {
    return g_bin[BinTable::index({vr - 1, shape, rank, vb_index(vb), kt})];
}
BinLauncher pos_launcher(uint32_t vb, bool last, int kt) { return g_pos[PosTable::index({vb_index(vb), last ? 1 : 0, kt})]; }
BinLauncher persist_launcher(uint32_t vb, int kt) { return g_persist[PersistTable::index({vb == 8 ? 1 : 0, kt})]; }
HistLauncher hist_launcher(int kt) { return g_hist[kt]; }
HyHistLauncher hy_hist_launcher(int kt) { return g_hy_hist[kt]; }
// (cls: the size class of the sort — hy_class_of in onesweep_host.hpp, the one place that picks it)
HyLocalLauncher hy_local_launcher(int cls, int kt) { return g_hy_local[HyTable::index({cls, kt})]; }
HyLocalPairsLauncher hy_pairs_launcher(uint32_t vb, int cls, int kt) { return g_hy_local_pairs[HyPairsTable::index({vb == 8 ? 1 : 0, cls, kt})]; }
SmallLauncher small_launcher(uint32_t n, int rank, uint32_t vb, int kt) {
    const int c = small_class(n);
    return c < 5 ? g_small[SmallTable::index({c, rank, vb_index(vb), kt})] : nullptr;  // nullptr: no single-tile kernel for this case
}
SegWgLauncher seg_wg_launcher(int wg_cls, int rank, uint32_t vb, int kt) { return g_seg_wg[SegWgTable::index({wg_cls, rank, vb_index(vb), kt})]; }
const SegVbLaunchers& seg_vb(uint32_t vb) { return g_seg_vb[vb_index(vb)]; }
inline int vm_index(uint32_t vm) { return vm == 0 ? 0 : vm == 1 ? 1 : vm == 4 ? 2 : 3; }
TkrLauncher tkr_tile_launcher(bool key16, int wg_cls, int rank, uint32_t vm) {
    return g_tkr_tile[TkrTileTable::index({key16 ? 1 : 0, wg_cls, rank, vm_index(vm)})];
}
const TkrVmLaunchers& tkr_vm(bool key16, uint32_t vm) { return g_tkr_vm[TkrVmTable::index({key16 ? 1 : 0, vm_index(vm)})]; }
MidLauncher mid_launcher(int cls, int rank, uint32_t vb, int kt) { return g_mid[MidTable::index({cls, rank, vb_index(vb), kt})]; }

// The registry as data (gs_debug_registry_dims / _cell; tests hold their case list against it): family = GS_KF_*.  dims != nullptr:
// the table's extents, returns their number; otherwise 1 / 0 = the cell at coord holds a launcher or not.  -1: no such family or cell.
template <class F> bool cell_built(F f) { return f != nullptr; }
inline bool cell_built(const SegVbLaunchers& f) { return f.packed && f.wave && f.merge_head; }
inline bool cell_built(const TkrVmLaunchers& f) { return f.wave && f.stream; }
template <class Tab, class Cells>
int registry_query(const Cells& cells, int32_t* dims, const int32_t* coord) {
    if (dims) {
        for (int k = 0; k < 5; ++k) dims[k] = 1;
        return Tab::extents(dims);
    }
    int32_t ext[5] = {1, 1, 1, 1, 1};
    for (int k = Tab::extents(ext); k < 5; ++k)
        if (coord[k] != 0) return -1;
    const int i = Tab::checked_index(coord);
    return i < 0 ? -1 : cell_built(cells[i]) ? 1 : 0;
}
int registry_lookup(uint32_t family, int32_t* dims, const int32_t* coord) {
    if (!dims && !coord) return -1;
    switch (family) {
        case GS_KF_BIN: return registry_query<BinTable>(g_bin, dims, coord);
        case GS_KF_POS: return registry_query<PosTable>(g_pos, dims, coord);
        case GS_KF_PERSIST: return registry_query<PersistTable>(g_persist, dims, coord);
        case GS_KF_SMALL: return registry_query<SmallTable>(g_small, dims, coord);
        case GS_KF_MID: return registry_query<MidTable>(g_mid, dims, coord);
        case GS_KF_SEG_WG: return registry_query<SegWgTable>(g_seg_wg, dims, coord);
        case GS_KF_SEG_VB: return registry_query<Table<3>>(g_seg_vb, dims, coord);
        case GS_KF_TKR_TILE: return registry_query<TkrTileTable>(g_tkr_tile, dims, coord);
        case GS_KF_TKR_VM: return registry_query<TkrVmTable>(g_tkr_vm, dims, coord);
        case GS_KF_HIST: return registry_query<Table<NKT>>(g_hist, dims, coord);
        case GS_KF_HY_HIST: return registry_query<Table<NKT>>(g_hy_hist, dims, coord);
        case GS_KF_HY_LOCAL: return registry_query<HyTable>(g_hy_local, dims, coord);
        case GS_KF_HY_LOCAL_PAIRS: return registry_query<HyPairsTable>(g_hy_local_pairs, dims, coord);
    }
    return -1;
}
// ---- end of the kernel registry -------------------------------------------------------------------------------------

}  // namespace
