// onesweep_host.hpp — part of the gpusort_capi.hip translation unit: the gs_onesweep handle — slab sizing, GlobalHistogram + Scan
// (prologue), routing by size (sort_route), the sort itself (sort_impl) — and every gs_onesweep_* / gs_selftest_* / gs_debug_* /
// gs_init_random / gs_validate / gs_msd_splitters* entry of include/gpusort.h.
namespace {

using gs::SLAB_COUNTERS;
using gs::SLAB_DESC;
using gs::SLAB_HIST;
using gs::SLAB_INFO;
using gs::SLAB_STATUS;

constexpr uint32_t MIN_TILE = 4096;  // smallest tile of any compiled shape (sizing of the slab)
constexpr uint32_t KEY64_TILE = 8192;  // tile of every sort of 64-bit keys (MID_SHAPE: 8-byte stage slots, 64 KiB)
// profiles/r02_shape_by_size.txt (general path, back-to-back sorts): the 8192-key tile wins up to 2^25 keys for keys-only
// sorts (180 vs 194 us at 2^24, 293 vs 302 at 2^25, loses at 2^26) and for 8-byte values (whose big tile leaves one
// workgroup per CU), up to 2^23 with 4-byte values (1024 x 16 wins from 2^24)
inline uint32_t mid_keys(uint32_t vb) { return vb == 4 ? (1u << 23) : (1u << 25); }
// index in g_shapes of a tile shape this build compiles, -1: none
inline int find_shape(uint32_t threads, uint32_t kpt) {
    for (int i = 0; i < g_num_shapes; ++i)
        if ((uint32_t)g_shapes[i].threads == threads && (uint32_t)g_shapes[i].kpt == kpt) return i;
    return -1;
}

}  // namespace

struct gs_onesweep {
    uint32_t max_keys;
    gs_mode mode;
    uint32_t value_bytes;
    int shape;
    int shape_auto = 1;  // 1 = the library picks (mid sizes use MID_SHAPE); 0 after gs_onesweep_set_shape / gs_onesweep_options::shape_*
    int small_path; // 1 = single-tile kernel for n <= SMALL_TILE (default), 0 = always the tiled path
    int mid_path;    // 1 = two-launch MSD + bucket sort for single-tile limit < n <= 2^20 (default), 0 = the six-launch path
    int skip_passes; // 1 = identity passes (one digit value for all keys) are dropped in pairs (default)
    int pos_chains;  // keys-only sorts of skewed 32-bit keys run every pass on position chains: 1 allowed (default), 0 never
    int key64_sweeps;       // 64-bit keys: 1 = one GlobalHistogram + Scan for all eight passes (default), 2 = one per word (gs_onesweep_options::key64_sweeps; A/B, tests)
    uint32_t pos_min_keys;  // ... from this many keys up (default 2^25 + 1: where the big tile shape takes over; gs_onesweep_options::position_chains_min_log2)
    int rank_mode;  // 0 ballot multi-split, 1 returning LDS atomic (needs the lane-order probe to pass)
    uint32_t* slab = nullptr;
    size_t slab_words;
    uint32_t* partials = nullptr;  // the histogram workgroups' tables: hist_blocks(max_keys) x HIST_TABLE_WORDS, summed by hist_reduce_kernel
    size_t partials_words;
    int profiling = 0;
    hipEvent_t ev[GS_PROFILE_SLOTS + 1];
    bool ev_valid = false;
    bool profile_pending = false;
    void* trace_buf = nullptr;   // experiment builds only (GS_EXP & 2): per-tile phase timestamps
    const void* msd_keys = nullptr;  // shard whose top-byte histogram + scan currently sit in the slab (msd_prepare)
    uint32_t msd_n = 0, msd_grid = 0;
    gs_key_type msd_kt = GS_KEY_UINT32;
    uint32_t* pinned = nullptr;  // 1024 + 8 words of pinned host memory for read-backs
    // geometry of the last tiled call, for gs_debug_check_state (tile 0 = the last call left no scan state)
    uint32_t last_n = 0, last_tile = 0, last_tile0 = 0, last_p0 = 0, last_np = 0, last_dyn = 0, last_desc_stride = 0, last_pos_tile = 0;
    bool hist_dirty = false;   // a call failed between the histogram launch and the kernel that hands HIST back zeroed
    uint32_t hist_blocks_opt;  // gs_onesweep_options::hist_blocks (0 = the library picks)
    int first_pass_big;        // gs_onesweep_options::first_pass_big
    uint32_t debug_flags = 0;  // gs_onesweep_options::debug_flags
    int plan;              // gs_onesweep_options::plan / gs_onesweep_set_plan: 0 the library picks, 1 LSD passes only, 2 two-level plan wherever it can run
    uint32_t hy_min_keys = HY_MIN_KEYS_DEFAULT;  // plan 0: the two-level plan from this many keys up
    uint32_t* hy_tab = nullptr;  // the two-level plan's tables (gs::HYT_WORDS), nullptr: the handle cannot run it (pairs, 64-bit keys only ...)
    uint32_t hy_grid;      // workgroups of its histogram kernel (a multiple of NCH)
    int last_hy = 0;       // the last sort was enqueued with the two-level plan's launches (whether it RAN on it is the device's decision: gs_onesweep_last_plan)
    uint32_t pos_grid_forced = 0;  // gs_debug_set_pos_grid: 0 the position-chain launches run on pos_grid() workgroups, else on this many (>= NCH)
    int hy_class_forced = -1;  // gs_debug_set_hy_class: -1 the size class of the bucket-local sort follows n (hy_class), 0 .. 3 that class whatever n is
};

namespace {

// ---- the slab's descriptor rows: the one place that says how many a pass needs and whether the slab holds them ----
// Rows of one pass's descriptor region over n keys on `tile`-key tiles: every chain's tiles (+1 partial) + row 0.  hy_chains: the
// sort may run on the two-level plan, whose second pass runs on CHMAX chains instead of MAXCH.
inline uint32_t desc_rows(uint32_t n, uint32_t tile, bool hy_chains) {
    return div_up(n, tile) + (hy_chains ? 2 * gs::CHMAX + 8 : 2 * gs::MAXCH + 2);
}
// slab words up to the end of the descriptor regions of `passes` passes
inline size_t slab_words_with(uint32_t passes, uint32_t rows) { return SLAB_DESC + (size_t)passes * rows * gs::RADIX; }
inline bool slab_fits(const gs_onesweep* h, uint32_t passes, uint32_t rows) { return slab_words_with(passes, rows) <= h->slab_words; }

// The size class of the two-level plan's bucket-local sort for a sort of n keys on this handle: by n, unless a test forced one
// (gs_debug_set_hy_class).  Everything that depends on the class asks here: the bucket limit the histogram and scan kernels judge
// the plan by, the bucket-local sort's launcher, and sort_route's question whether that launcher exists.
inline int hy_class_of(const gs_onesweep* h, uint32_t n) { return h->hy_class_forced >= 0 ? h->hy_class_forced : hy_class(n); }

size_t slab_words_for(uint32_t max_keys) {
    // descriptor rows: four passes on the smallest tile, or the eight passes of a 64-bit sort on its 8192-key tile
    // (two-level plan: its second pass has CHMAX chains — on 16 384-key tiles, from 2^20 keys up at the earliest: covered by the rows of
    //  the smallest tile as soon as max_keys / 4096 - max_keys / 16 384 >= 2 * CHMAX, i.e. from 2^12 x 171 keys)
    const size_t words4 = slab_words_with(4, desc_rows(max_keys, MIN_TILE, false));
    const size_t words8 = slab_words_with(gs::MAX_PASSES, desc_rows(max_keys, KEY64_TILE, false));
    return words4 > words8 ? words4 : words8;
}

// HIST (four joint tables + what the keys look like as a whole) is zero between calls: hist_reduce_kernel OVERWRITES only the
// tables it sums, the histogram kernel adds the HX words with atomics.  The first pass launched after the Scan hands it back zeroed
// (BM_ZERO_HIST); a call that launches none does it here.  hist_dirty records a call that failed in between: prologue zeroes it then.
gs_status hand_back_hist(gs_onesweep* h, hipStream_t s) {
    GS_HIP(hipMemsetAsync(h->slab + SLAB_HIST, 0, gs::HIST_WORDS * sizeof(uint32_t), s));
    h->hist_dirty = false;
    return GS_OK;
}

// the tile shape of a binning pass of this handle: `shape` if it has a kernel for the key type, else MID_SHAPE — 64-bit keys
// (8-byte stage slots) fit 8192-key tiles only
int bin_shape(const gs_onesweep* h, gs_key_type kt, uint32_t vb, int shape) {
    return (is_key64(kt) && !bin_launcher(shape, h->rank_mode, vb, kt)) ? MID_SHAPE : shape;
}

uint32_t hist_blocks(uint32_t n, uint32_t forced = 0) {
    // one chunk per workgroup at mid sizes (measured: 4/8/16 chunks per workgroup — fewer closing global atomics,
    // less parallelism — are slower: 11 -> 15-23 us at 2^16..2^20)
    // Above that ONE workgroup per CU (half of them up to 2^22 keys): every workgroup closes with one global atomic per
    // non-empty bin of its 4 x 4096-bin LDS histograms (~14 000 of them) — most of the kernel at mid sizes and still 6 %
    // of it at 2^28.  512 -> 256 workgroups: 30 -> 21 us at 2^21, 59 -> 51 us at 2^25, 179 -> 156 us at 2^27,
    // 300 -> 282 us at 2^28; counts that do not divide the CUs evenly (320, 384, 448) lose 10-35 %
    // (profiles/r02_hist_blocks_mid_sizes.txt).
    const uint32_t cus = cu_count();
    const uint32_t want = div_up(n, gs::HIST_CHUNK);
    const uint32_t cap = n <= (1u << 22) ? (cus + 1) / 2 : cus;
    if (forced > 0) return forced < want ? forced : want;  // gs_onesweep_options::hist_blocks (tuning aid)
    return want < 1 ? 1 : (want > cap ? cap : want);
}

// persistent workgroups of the position-chain pass: two per CU (76 KiB of LDS each)
uint32_t pos_grid() { return 2u * cu_count(); }
// ... of this handle's position-chain launches (pos_launcher): a test may have set another grid (gs_debug_set_pos_grid).  Any grid of
// NCH workgroups or more is correct: a workgroup draws tickets on chain blockIdx % NCH (group by group on a CHMAX-chain pass), then
// takes tiles of the chains that still have some, and no tile waits for a workgroup that has not started.
uint32_t pos_grid_of(const gs_onesweep* h) { return h->pos_grid_forced ? h->pos_grid_forced : pos_grid(); }

// workgroups of the two-level plan's histogram kernel: one per CU, a multiple of NCH (position segments get equal numbers of them)
uint32_t hy_grid_for_device() {
    const uint32_t cus = cu_count();
    return cus >= gs::NCH ? cus / gs::NCH * gs::NCH : gs::NCH;
}

// most workgroups the histogram kernel is ever launched with for a handle of max_keys keys (sizes its slices)
uint32_t hist_blocks_cap(uint32_t max_keys, uint32_t forced = 0) {
    uint32_t m = hist_blocks(max_keys);
    if (max_keys > (1u << 22)) { const uint32_t b = hist_blocks(1u << 22); m = b > m ? b : m; }
    if (forced > m) m = forced;
    return m;
}

// the value buffers of a pairs call: a pairs handle, both buffers, aligned
gs_status check_vals(const gs_onesweep* h, const void* a, const void* b) {
    if (h->mode != GS_MODE_PAIRS) return GS_ERR_MODE;
    return (!a || !b || misaligned(a) || misaligned(b)) ? GS_ERR_ARG : GS_OK;
}

// one launch of a binning pass with pass p's scan state (descriptor region, counters, info block) and the shared words
void launch_pass(const gs_onesweep* h, BinLauncher f, hipStream_t s, uint32_t grid, uint32_t p, uint32_t desc_stride, const void* keys_in,
                 void* keys_out, const void* vals_in, void* vals_out, uint32_t n, uint32_t shift, uint32_t mode) {
    f(s, grid, const_cast<uint32_t*>(static_cast<const uint32_t*>(keys_in)), static_cast<uint32_t*>(keys_out), const_cast<void*>(vals_in), vals_out,
      h->slab + SLAB_DESC + (size_t)p * desc_stride, h->slab + SLAB_COUNTERS + p * gs::COUNTERS_PER_PASS * gs::COUNTER_STRIDE,
      h->slab + SLAB_INFO + p * gs::INFO_STRIDE, h->slab + gs::SLAB_HSUB, h->slab + SLAB_STATUS, n, shift, mode);
}

// Clears the scan state and runs GlobalHistogram + Scan for passes p0 .. p0+np-1
// (pass p0 over position segments, later passes over digit groups of the previous digit).
struct PassPlan {
    uint32_t grid, desc_stride;
    uint32_t grid0;  // grid of the plan's first pass (shape0_index)
};
// What a prologue is asked for; a call site sets by name what differs from the defaults.
struct PrologueIn {
    uint32_t first_pass = 0, num_passes = 4;  // the passes planned: first_pass .. first_pass + num_passes - 1
    uint32_t scan_plan = 0;        // the Scan kernel's plan bits: 1 descending, 2 planned on the device, 4 may run on position chains
    int shape_index = -1;          // tile shape of the passes (g_shapes), -1: the handle's
    int shape0_index = -1;         // >= 0: the plan's first pass runs on that (larger) tile shape, the others on shape_index
    uint32_t word = 0;             // 64-bit keys sorted in two rounds: the key word of this round
    uint32_t pos_tile = POS_TILE;  // tile of the position-chain passes (pos_tile_for)
    bool hy = false;               // the sort may run on the two-level plan (hybrid_kernels.hpp): its histogram sweep replaces GlobalHistogram,
                                   // its scan runs in front of the ordinary one, and both plans' launches follow (sort_impl)
    bool pregrouped = false;       // ... and its input is already grouped by its top byte (sort_impl)
    bool keys_only = false;        // ... and it carries no values: pass B hands the bucket-local sort 16-bit halves (PF_HALF16)
};
gs_status prologue(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt, hipStream_t s, const PrologueIn& in, PassPlan* plan) {
    const uint32_t p0 = in.first_pass, np = in.num_passes, scan_plan = in.scan_plan, word = in.word, pos_tile = in.pos_tile;
    const int shape_index = in.shape_index, shape0_index = in.shape0_index;
    const bool hy = in.hy, pregrouped = in.pregrouped;
    h->msd_keys = nullptr;  // whatever an earlier gs_onesweep_msd_prepare left in the slab is overwritten now
    h->last_hy = hy ? 1 : 0;
    const Shape& sh = g_shapes[shape_index < 0 ? h->shape : shape_index];
    const uint32_t tile = (uint32_t)sh.threads * sh.kpt;
    const uint32_t tile0 = shape0_index < 0 ? tile : (uint32_t)g_shapes[shape0_index].threads * g_shapes[shape0_index].kpt;
    // rows on the smallest tile a pass may run on; bit 2 of the plan: the sort may end up on the (smaller) position-chain tiles
    const uint32_t rows = desc_rows(n, ((scan_plan & 4u) && (pos_tile & 0x7fffffffu) < tile) ? (pos_tile & 0x7fffffffu) : (tile < tile0 ? tile : tile0), hy);
    const uint32_t desc_stride = rows * gs::RADIX;
    // (hy: the descriptor regions of LSD passes 2 and 3 are zeroed by the launch of LSD pass 1 (BM_ZERO_DESC23) if — and only if — those passes run)
    const size_t used_words = SLAB_DESC + (size_t)(hy ? 2u : np) * desc_stride;
    if (!slab_fits(h, np, rows)) return GS_ERR_SIZE;  // (cannot happen with the tiles the library picks)
    // position segments of the first pass: equal, multiples of the histogram chunk — and of the first pass's tile where that is a
    // multiple of the chunk (every shape the library picks): its chains then consist of whole tiles, 16 partial tiles fewer (at
    // mid sizes one launch round fewer: 2^24 keys are 1024 tiles of 16 384, two rounds on 512 slots)
    const uint32_t seg_unit = (tile0 % gs::HIST_CHUNK == 0u) ? tile0 : gs::HIST_CHUNK;
    const uint32_t seg_len0 = div_up(div_up(n, gs::NCH), seg_unit) * seg_unit;
    // no separate clear: the histogram kernel zeroes the scan state while it reads the keys (profile slot 0 stays 0)
    // HIST must be zero here (hand_back_hist): a call that failed in between left it dirty, zero it now, once
    if (h->hist_dirty) {
        const gs_status st = hand_back_hist(h, s);
        if (st != GS_OK) return st;
    }
    // (64-bit keys: passes 4..7 — or the second round's kernels — are charged to slot 6; the events of round 0 stay where they are)
    const bool rec = h->profiling && word == 0;
    if (rec) GS_HIP(hipEventRecord(h->ev[0], s));
    if (rec) GS_HIP(hipEventRecord(h->ev[1], s));
    h->hist_dirty = true;  // until the caller has launched whatever zeroes HIST again
    if (hy) {
        // one workgroup per CU at most, NCH position segments of equal numbers of workgroups, every workgroup >= one tile of keys
        const uint32_t seg_tiles = seg_len0 / tile0;
        const uint32_t wg_per_seg = seg_tiles < h->hy_grid / gs::NCH ? (seg_tiles ? seg_tiles : 1u) : h->hy_grid / gs::NCH;
        const uint32_t G = wg_per_seg * gs::NCH;
        const uint32_t per_wg = div_up(div_up(seg_len0, wg_per_seg), gs::HIST_CHUNK) * gs::HIST_CHUNK;
        const uint32_t cap = g_hy_class[hy_class_of(h, n)].cap();  // what the bucket-local sort's workgroup holds
        hy_hist_launcher(kt)(s, G, static_cast<const uint32_t*>(d_keys), h->slab, used_words, n, seg_len0, per_wg, wg_per_seg, h->partials, cap);
        hipLaunchKernelGGL(gs::hy_reduce_kernel, dim3(gs::RADIX + gs::NCH), dim3(256), 0, s, h->partials, G, wg_per_seg, h->hy_tab, h->slab + SLAB_HIST);
        if (rec) GS_HIP(hipEventRecord(h->ev[2], s));
        hipLaunchKernelGGL(gs::hy_scan_kernel, dim3(1), dim3(1024), 0, s, h->slab, h->hy_tab, n, seg_len0, desc_stride, cap, tile, pregrouped ? 1u : 0u,
                           in.keys_only ? 1u : 0u);
    } else {
        hist_launcher(kt)(s, hist_blocks(n, h->hist_blocks_opt), static_cast<const uint32_t*>(d_keys), h->slab, used_words, n, seg_len0, p0, np, word,
                          (scan_plan & 4u) ? (h->pos_chains == 2 ? 3u : 1u) : 0u, h->partials);
    }
#if (GS_EXP & 2)
    GS_HIP(hipMemcpyAsync(h->slab + SLAB_STATUS + 8, &h->trace_buf, sizeof(void*), hipMemcpyHostToDevice, s));
#endif
    if (rec && !hy) GS_HIP(hipEventRecord(h->ev[2], s));
    if (np > 4)  // 64-bit keys: all eight passes from one sweep
        hipLaunchKernelGGL(gs::scan_kernel<8>, dim3(np), dim3(256), 0, s, h->slab + SLAB_HIST, h->slab + SLAB_DESC,
                           h->slab + SLAB_INFO, desc_stride, n, seg_len0, tile, scan_plan, pos_tile, tile0);
    else
        hipLaunchKernelGGL(gs::scan_kernel<4>, dim3(np), dim3(256), 0, s, h->slab + SLAB_HIST, h->slab + SLAB_DESC,
                           h->slab + SLAB_INFO, desc_stride, n, seg_len0, tile, scan_plan, pos_tile, tile0);
    if (rec) GS_HIP(hipEventRecord(h->ev[3], s));
    plan->grid = div_up(n, tile) + (hy ? gs::CHMAX : gs::MAXCH) + 1;  // chains end in partial tiles: at most one more tile per chain than n/tile
    plan->grid0 = div_up(n, tile0) + gs::MAXCH + 1;
    plan->desc_stride = desc_stride;
    h->last_n = n; h->last_tile = tile; h->last_tile0 = tile0; h->last_p0 = p0; h->last_np = np; h->last_dyn = (scan_plan & 2u) ? 1u : 0u; h->last_pos_tile = pos_tile;
    h->last_desc_stride = desc_stride;
    return GS_OK;
}

// ---- the structural entries (GlobalHistogram, Scan, the multi-GPU split's histograms): a histogram + scan that no pass follows ----
// their arguments: a handle, aligned keys of a 32-bit type, somewhere to put the result
gs_status check_hist_args(const gs_onesweep* h, const void* d_keys, const void* h_out, uint32_t n, gs_key_type kt) {
    if (!h || !d_keys || !h_out || misaligned(d_keys) || !is_key32_type(kt)) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys) return GS_ERR_SIZE;  // (max_keys <= GS_MAX_KEYS)
    return GS_OK;
}
// GlobalHistogram + Scan of passes p0 .. p0 + np - 1, `copy` (what the entry wants in pinned memory), HIST handed back zeroed — no pass
// follows —, the host waits.  pass_slots: a profiled call closes the pass slots (they read 0) and leaves a profile to fetch.
template <class Copy>
gs_status hist_and_wait(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt, hipStream_t s, uint32_t p0, uint32_t np, PassPlan* plan,
                        Copy copy, bool pass_slots = false) {
    PrologueIn in;
    in.first_pass = p0;
    in.num_passes = np;
    gs_status st = prologue(h, d_keys, n, kt, s, in, plan);
    if (st == GS_OK) st = copy();
    if (st == GS_OK) st = hand_back_hist(h, s);
    if (st != GS_OK) return st;
    if (pass_slots) {
        if (h->profiling)
            for (int e = 4; e <= 7; ++e) GS_HIP(hipEventRecord(h->ev[e], s));
        h->profile_pending = h->profiling != 0;
    }
    GS_HIP(hipStreamSynchronize(s));
    return GS_OK;
}
// ... with the joint tables of those passes (np x NCH x RADIX words of HIST) in h->pinned
gs_status read_hist(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt, hipStream_t s, uint32_t p0, uint32_t np, PassPlan* plan,
                    bool pass_slots = false) {
    return hist_and_wait(h, d_keys, n, kt, s, p0, np, plan, [&] {
        GS_HIP(hipMemcpyAsync(h->pinned, h->slab + SLAB_HIST, (size_t)np * gs::NCH * gs::RADIX * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return GS_OK;
    }, pass_slots);
}

gs_status check_common(gs_onesweep* h, const void* a, const void* b, uint32_t n, gs_key_type kt, gs_order order) {
    if (!h || !a || !b || misaligned(a) || misaligned(b)) return GS_ERR_ARG;
    if (!valid_key_type(kt) || !valid_order(order)) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys || n > GS_MAX_KEYS) return GS_ERR_SIZE;
    return GS_OK;
}

// Which way a sort of n elements goes — decided on the host from sizes, modes and options alone (what the KEYS look like is the
// device's business: identity passes, skew, the two-level plan's validity).  sort_impl enqueues accordingly; gs_onesweep_sort_sharded
// asks whether a bucket it is about to receive will be offered the two-level plan (`hy`) before it chooses the exchange's layout.
struct SortRoute {
    SmallLauncher small;  // != nullptr: one workgroup, one launch
    int mid_cls;          // >= 0: the two-launch mid-size route (mid_kernels.hpp), class index
    int shape, shape0;    // tile shapes of the general pipeline: passes 1.., first pass
    uint32_t dyn;         // 2: the Scan kernel plans the passes on the device (identity passes dropped, source buffers); 0: fixed ping-pong
    bool pos;             // the sort may be planned on position chains (PF_POS): every pass is launched in both chain forms
    bool hy;              // the sort is offered the two-level plan (hybrid_kernels.hpp): both plans' launches are enqueued
};
SortRoute sort_route(const gs_onesweep* h, uint32_t n, gs_key_type kt, uint32_t vb) {
    SortRoute r{};
    // routing by size: one workgroup up to 8192 keys; two launches (MSD pass + bucket sorts) up to 2^20 (2^22 pairs with 4-byte
    // values, 2^23 keys-only: mid_class); the general pipeline above.  (The 16 384- and 32 768-slot single-tile kernels serve when the mid-size route is switched off:
    // with it, 2^15 keys take 18 us instead of 34, profiles/r02_size_and_entropy_sweep.txt.)
    r.mid_cls = (h->mid_path && h->shape_auto && n > gs::SMALL_TILE && !is_key64(kt)) ? mid_class(n, vb) : -1;
    if (r.mid_cls >= 0 && !mid_launcher(r.mid_cls, h->rank_mode, vb, kt)) r.mid_cls = -1;  // (not in this build)
    r.small = (h->small_path && r.mid_cls < 0) ? small_launcher(n, h->rank_mode, vb, kt) : nullptr;
    // 64-bit keys: the mid-size shape at every size (bin_shape)
    // (a sort that may be planned on position chains — see `pos` below — runs on the default tile: the dual kernel's shapes)
    const bool pos_size = h->skip_passes && h->rank_mode == 1 && !is_key64(kt) && h->pos_chains != 0 && n >= h->pos_min_keys;
    r.shape = bin_shape(h, kt, vb, (h->shape_auto && n <= mid_keys(vb) && !pos_size) ? MID_SHAPE : h->shape);
    const Shape& sh = g_shapes[r.shape];
    // Mid sizes, keys-only (2^22 < n <= 2^25: the 8192-key tile): the FIRST pass runs on the 16 384-key tile.  Its position segments are
    // whole tiles (prologue), so 2^24 keys are exactly 1024 tiles — two launch rounds on the 512 slots of that shape instead of three
    // rounds of 8192-key tiles on 768 — and its input is cold, which the larger tile streams better; the later passes' chains are
    // digit groups with a partial tile at each end, which overflow the round.  gs_onesweep_options::first_pass_big = 0 switches it off (A/B).
    r.shape0 = (h->first_pass_big && h->shape_auto && r.shape == MID_SHAPE && vb == 0 && !is_key64(kt) && n > (1u << 22) &&
                bin_launcher(0, h->rank_mode, 0, kt) != nullptr) ? 0 : r.shape;
    // The scan kernel decides on the device which passes run and which buffer each one reads (identity passes
    // are dropped in pairs, see scan_kernel); every pass is handed (keys, alt) and the sort's order.
    r.dyn = h->skip_passes ? 2u : 0u;
    // The sort may run on position chains in every pass (PF_POS; decided on the device: the histogram kernel finds the
    // digit groups uneven, the Scan kernel plans accordingly) — every pass is then launched in both chain forms and the
    // plan says which one works.  Sorts of 32-bit keys on the big tile shape, LDS-atomic ranking; gs_onesweep_options::position_chains = 0
    // switches it off.
    r.pos = r.dyn && h->rank_mode == 1 && !is_key64(kt) && h->pos_chains != 0 && n >= h->pos_min_keys &&
            pos_launcher(vb, false, kt) != nullptr &&
            (vb == 4 ? sh.threads * sh.kpt == 16384 : (sh.threads == 512 && sh.kpt == 32));  // (the plan's last pass runs on 16 384-key tiles)
    // Two-level plan (hybrid_kernels.hpp): sorts of 32-bit keys — keys-only and pairs with 4- / 8-byte values — that may also run on
    // position chains (its fall-back when the keys turn out skewed) — the histogram sweep counts the 16-bit prefixes, and the device decides which plan runs.
    // (position_chains = 2 asks for the position-chain plan whatever the keys look like: only plan 2 overrides that)
    r.hy = r.pos && !r.small && r.mid_cls < 0 && h->hy_tab != nullptr && hy_hist_launcher(kt) != nullptr && h->plan != 1 &&
           (h->plan == 2 || (n >= (vb ? HY_MIN_PAIRS_DEFAULT : h->hy_min_keys) && h->pos_chains != 2)) &&
           (vb == 0 ? hy_local_launcher(hy_class_of(h, n), kt) != nullptr
                    : (persist_launcher(vb, kt) != nullptr && hy_pairs_launcher(vb, hy_class_of(h, n), kt) != nullptr)) &&
           slab_fits(h, 4, desc_rows(n, pos_tile_for(vb) & 0x7fffffffu, true));  // (what sort_impl's prologue will ask for)
    return r;
}

// The routes that need no scan state — the single-tile kernel and the two-launch mid-size route: wait for the values, launch, and charge
// everything to profile slot 0 (and the total).
template <class Launch>
gs_status one_launch_route(gs_onesweep* h, hipStream_t s, hipEvent_t values_ready, Launch launch) {
    if (values_ready) GS_HIP(hipStreamWaitEvent(s, values_ready, 0));
    if (h->profiling) GS_HIP(hipEventRecord(h->ev[0], s));
    launch();
    h->last_tile = 0;
    h->last_hy = 0;
    if (h->profiling)
        for (int e = 1; e <= 7; ++e) GS_HIP(hipEventRecord(h->ev[e], s));
    GS_HIP(hipGetLastError());
    h->profile_pending = h->profiling != 0;
    return GS_OK;
}

// values_ready (multi-GPU): an event behind which d_vals is complete — the keys already are, so GlobalHistogram + Scan (which read
// keys only) run before the stream waits for it; the one- and two-launch routes wait first.
gs_status sort_impl(gs_onesweep* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n,
                    gs_key_type kt, gs_order order, hipStream_t s, uint32_t vb, hipEvent_t values_ready = nullptr, bool pregrouped = false) {
    // pregrouped (multi-GPU, gs_onesweep_sort_sharded): the input lies in the ALTERNATE buffers, already grouped by its top byte in
    // ascending order — the bucket exchange landed it bin by bin — and the caller made sure (hy_offered) that the sort is offered the
    // two-level plan: its pass A (the top-byte partition) is skipped, pass B reads the alternate buffers as it always does.  If the device
    // finds the plan void, hy_void_copy_kernel moves the input to the caller's buffers and the four LSD passes run as ever.
    const SortRoute route = sort_route(h, n, kt, vb);
    if (pregrouped && !route.hy) return GS_ERR_ARG;  // (the caller asks sort_route first)
    const uint32_t descending = order == GS_ORDER_DESCENDING ? 1u : 0u;
    if (SmallLauncher small = route.small)  // (the single-tile kernel has no spin and cannot time out: it sets the status word to OK)
        return one_launch_route(h, s, values_ready, [&] { small(s, static_cast<uint32_t*>(d_keys), d_vals, n, descending, h->slab + SLAB_STATUS); });
    if (route.mid_cls >= 0)  // one MSD pass + one LDS sort per top-byte bucket (a skewed top byte: the LSD passes inside the first kernel)
        return one_launch_route(h, s, values_ready, [&] {
            mid_launcher(route.mid_cls, h->rank_mode, vb, kt)(s, div_up(n, g_mid_class[route.mid_cls].tile()), static_cast<uint32_t*>(d_keys),
                                                              static_cast<uint32_t*>(d_alt_keys), d_vals, d_alt_vals, h->slab + gs::SLAB_MID,
                                                              h->slab + SLAB_STATUS, n, descending);
        });
    const int shape = route.shape, shape0 = route.shape0;
    const Shape& sh = g_shapes[shape];
    BinLauncher fn = bin_launcher(shape, h->rank_mode, vb, kt);
    if (!fn) return GS_ERR_ARG;
    BinLauncher fn0 = bin_launcher(shape0, h->rank_mode, vb, kt);
    const uint32_t dyn = route.dyn;
    const bool pos = route.pos, hy = route.hy;
    uint32_t* k[2] = {static_cast<uint32_t*>(d_keys), static_cast<uint32_t*>(d_alt_keys)};
    void* v[2] = {d_vals, d_alt_vals};
    // 64-bit keys: ONE GlobalHistogram + Scan plans all eight passes (eight joint tables from one sweep over the keys; the
    // chains of pass 4 are the groups of byte 3's values, as inside a word) — identity passes are dropped in pairs across the
    // whole key (keys below 2^32: four passes).  key64_sweeps = 2 (A/B) or a caller-picked tile too small for the slab's
    // eight descriptor regions: two rounds of histogram + scan + 4 passes — the low word's bytes, then (stable) the high
    // word's; each round leaves its result in the caller's buffers, only the last one carries the descending reversal.
    const bool one_sweep = is_key64(kt) && h->key64_sweeps == 1 && slab_fits(h, gs::MAX_PASSES, desc_rows(n, (uint32_t)sh.threads * sh.kpt, false));
    const uint32_t rounds = (is_key64(kt) && !one_sweep) ? 2u : 1u;
    const uint32_t NP = one_sweep ? gs::MAX_PASSES : 4u;
    for (uint32_t word = 0; word < rounds; ++word) {
        const uint32_t desc_bit = (order == GS_ORDER_DESCENDING && word + 1 == rounds) ? 1u : 0u;
        PassPlan plan;
        PrologueIn in;
        in.num_passes = NP;
        in.scan_plan = desc_bit | dyn | (pos ? 4u : 0u);
        in.shape_index = shape;
        in.shape0_index = shape0;
        in.word = word;
        in.pos_tile = pos_tile_for(vb);
        in.hy = hy;
        in.pregrouped = pregrouped;
        in.keys_only = vb == 0;
        gs_status st = prologue(h, pregrouped ? d_alt_keys : d_keys, n, kt, s, in, &plan);
        if (st != GS_OK) return st;
        if (values_ready && word == 0) GS_HIP(hipStreamWaitEvent(s, values_ready, 0));  // histogram + scan ran on the keys meanwhile
        if (pregrouped) {  // the plan may turn out void: the LSD passes read the caller's buffers (exits at once otherwise)
            const size_t kw = (size_t)n;  // key words
            hipLaunchKernelGGL(gs::hy_void_copy_kernel, dim3(pos_grid()), dim3(256), 0, s, h->slab, static_cast<const uint4*>(d_alt_keys), static_cast<uint4*>(d_keys),
                               kw / 4, static_cast<const uint32_t*>(d_alt_keys) + (kw & ~(size_t)3), static_cast<uint32_t*>(d_keys) + (kw & ~(size_t)3), (uint32_t)(kw & 3));
            if (vb) {
                const size_t vw = (size_t)n * (vb / 4);
                hipLaunchKernelGGL(gs::hy_void_copy_kernel, dim3(pos_grid()), dim3(256), 0, s, h->slab, static_cast<const uint4*>(d_alt_vals), static_cast<uint4*>(d_vals),
                                   vw / 4, static_cast<const uint32_t*>(d_alt_vals) + (vw & ~(size_t)3), static_cast<uint32_t*>(d_vals) + (vw & ~(size_t)3), (uint32_t)(vw & 3));
            }
        }
        // one launch of pass p: form `f` on `grid` workgroups, reading k[a] / v[a] and writing the other pair, with pass p's scan state
        auto launch = [&](BinLauncher f, uint32_t grid, uint32_t p, uint32_t a, uint32_t shift, uint32_t mode) {
            launch_pass(h, f, s, grid, p, plan.desc_stride, k[a], k[a ^ 1u], v[a], v[a ^ 1u], n, shift, mode);
        };
        const bool skip_local = (h->debug_flags & 0x40000000u) != 0u;  // (tuning builds, tools/hy_bringup.py: pass B's output stays as it is — keys only: 16-bit halves)
        for (uint32_t p = 0; p < NP; ++p) {
            const uint32_t a = dyn ? 0u : (p & 1u);
            const uint32_t mode = (dyn ? (desc_bit | gs::BM_PLANNED) : ((desc_bit && p == NP - 1) ? gs::BM_REVERSE : 0u)) | (p == 0 ? gs::BM_ZERO_HIST : 0u);
            if (pos && vb == 0) {
                // (1) keys-only sorts that may run on position chains: ONE launch per pass serves every plan (persistent workgroups, two per
                // CU).  Offered the two-level plan, the first two launches are pass A / pass B or LSD passes 0 / 1 — digit and chain count come
                // from the info block — the bucket-local sort follows them, and LSD passes 2 and 3 exit on PF_SKIP if it ran.
                launch(pos_launcher(vb, p == 3, kt), pos_grid_of(h), p, a, p * 8,
                       mode | ((hy && p < 2) ? gs::BM_INFO_SHIFT | gs::BM_INFO_CHAINS : 0u) | ((hy && p == 1) ? gs::BM_ZERO_DESC23 : 0u));
                if (hy && p == 1) {
                    if (h->profiling) GS_HIP(hipEventRecord(h->ev[5], s));  // slot 4 = pass B; slot 5: the local sort (+ LSD pass 2's launch); slot 6: LSD pass 3's
                    if (!skip_local) hy_local_launcher(hy_class_of(h, n), kt)(s, gs::HY_BINS, k[0], h->hy_tab, h->slab, n, desc_bit);
                }
            } else if (hy) {
                // (2) pairs that are offered the two-level plan: launches 0 and 1 = its two DigitBinningPasses (the plain form as persistent
                // workgroups: digit and chain count from the info block) or, on position chains, LSD passes 0 and 1 (the position-chain
                // form, which also serves LSD passes 2 and 3); the bucket-local sort sits between them.  The non-persistent plain forms
                // are not launched at all: whichever plan the device picks, one of these two forms is the one that works.
                if (p < 2) launch(persist_launcher(vb, kt), pos_grid() / 2u, p, a, p * 8, mode | gs::BM_FORMS | gs::BM_INFO_SHIFT | gs::BM_INFO_CHAINS);
                launch(pos_launcher(vb, p == 3, kt), pos_grid_of(h), p, a, p * 8, (mode & ~gs::BM_ZERO_HIST) | gs::BM_FORMS | (p == 1 ? gs::BM_ZERO_DESC23 : 0u));
                if (p == 1) {
                    if (h->profiling) GS_HIP(hipEventRecord(h->ev[5], s));
                    if (!skip_local) hy_pairs_launcher(vb, hy_class_of(h, n), kt)(s, k[0], v[0], h->hy_tab, h->slab, n, desc_bit);
                }
            } else {
                // (3) everything else: the plain form, one tile per workgroup.  8-byte values on the big tile come in two forms and the
                // pass's skew flag picks one (BinCfg::VROUNDS); pairs that may run on position chains add that form as a launch of its own.
                const bool two_forms = dyn && vb == 8 && !is_key64(kt) && sh.threads == 512 && sh.kpt == 32;
                launch(p == 0 ? fn0 : fn, p == 0 ? plan.grid0 : plan.grid, p, a, word * 32 + p * 8,
                       mode | (two_forms ? gs::BM_IF_EVEN : 0u) | ((pos && vb != 0) ? gs::BM_FORMS : 0u));
                if (two_forms) launch(bin_launcher(shape, h->rank_mode, vb, kt, 2), plan.grid, p, a, word * 32 + p * 8, mode | gs::BM_IF_SKEW | ((pos && vb == 8) ? gs::BM_FORMS : 0u));
                if (pos && vb != 0) launch(pos_launcher(vb, p == 3, kt), pos_grid_of(h), p, a, p * 8, (mode & ~gs::BM_ZERO_HIST) | gs::BM_FORMS);
            }
            if (h->profiling && word == 0 && p < 4 && !(hy && p == 1)) GS_HIP(hipEventRecord(h->ev[4 + p], s));
        }
    }
    if (h->profiling && is_key64(kt)) GS_HIP(hipEventRecord(h->ev[7], s));  // slot 6 then holds pass 3 and everything behind it
    GS_HIP(hipGetLastError());
    h->hist_dirty = false;  // pass 0 (BM_ZERO_HIST) was launched: it zeroes HIST
    h->profile_pending = h->profiling != 0;
    return GS_OK;
}

}  // namespace

extern "C" gs_status gs_selftest_lds_atomic_order(uint32_t iters, uint32_t seed, uint64_t* h_failures, void* stream);
#ifdef GS_TUNING
extern "C" gs_status gs_debug_copy_floor(const void* d_in, void* d_out, uint32_t n, uint32_t threads, uint32_t kpt, void* stream);
#endif

namespace {
bool lds_atomic_order_ok() {
    static int cached[64];  // per device: 0 unknown, 1 ok, 2 failed
    static std::mutex guard;  // handles may be created from several host threads
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    std::lock_guard<std::mutex> lock(guard);
    if (cached[dev] == 0) {
        uint64_t fails = 1;
        const gs_status st = gs_selftest_lds_atomic_order(64, 0x9e3779b9u, &fails, nullptr);
        cached[dev] = (st == GS_OK && fails == 0) ? 1 : 2;
    }
    return cached[dev] == 1;
}
}  // namespace

extern "C" {

const char* gs_version(void) { return "gpusort-mi355x 0.1 (gfx950 OneSweep)"; }

const char* gs_status_string(gs_status s) {
    switch (s) {
        case GS_OK: return "ok";
        case GS_ERR_ARG: return "bad argument";
        case GS_ERR_SIZE: return "bad size";
        case GS_ERR_HIP: return "HIP runtime error";
        case GS_ERR_TIMEOUT: return "look-back timeout on device";
        case GS_ERR_MODE: return "mode / value width mismatch";
        case GS_ERR_NO_DEVICE: return "no GPU device";
        case GS_ERR_COMM: return "multi-GPU communication (RCCL) error";
    }
    return "unknown";
}

int gs_last_hip_error(void) { return g_last_hip_error; }

size_t gs_onesweep_temp_bytes(uint32_t max_keys) {
    // an upper bound over modes and options (default hist_blocks): slab + the histogram workgroups' slices + the two-level plan's tables
    const size_t slices = (size_t)hist_blocks_cap(max_keys) * gs::HIST_TABLE_WORDS, hy_slices = (size_t)hy_grid_for_device() * gs::HY_SLICE_WORDS;
    const bool hy = max_keys > (1u << 20);
    return (slab_words_for(max_keys) + (hy && hy_slices > slices ? hy_slices : slices) + (hy ? gs::HYT_WORDS : 0)) * sizeof(uint32_t);
}

uint32_t gs_onesweep_partition_size(gs_mode mode, uint32_t value_bytes) {
    const Shape& sh = g_shapes[(mode == GS_MODE_PAIRS && value_bytes == 4) ? 1 : 0];
    return (uint32_t)sh.threads * sh.kpt;
}

void gs_onesweep_options_default(gs_onesweep_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(*o);
    o->rank_mode = -1;
    o->small_path = 1;
    o->mid_path = 1;
    o->skip_passes = 1;
    o->position_chains = 1;
    o->position_chains_min_log2 = 25;
    o->key64_sweeps = 1;
    o->plan = 0;
    o->first_pass_big = 1;
}

gs_status gs_onesweep_create(gs_onesweep** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    return gs_onesweep_create_ex(out, max_keys, mode, value_bytes, nullptr);
}

gs_status gs_onesweep_create_ex(gs_onesweep** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes, const gs_onesweep_options* options) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    gs_onesweep_options o;
    gs_onesweep_options_default(&o);
    if (options) {
        if (options->struct_size != sizeof(gs_onesweep_options)) return GS_ERR_ARG;  // (one layout so far)
        o = *options;
    }
    const int max_plan = 2;
    if (o.rank_mode < -1 || o.rank_mode > 1 || o.position_chains < 0 || o.position_chains > 2 || o.plan < 0 || o.plan > max_plan ||
        (o.key64_sweeps != 1 && o.key64_sweeps != 2) || o.position_chains_min_log2 < 20 || o.position_chains_min_log2 > 30)
        return GS_ERR_ARG;
    int shape_pick = -1;
    if ((o.shape_threads || o.shape_keys_per_thread) && (shape_pick = find_shape(o.shape_threads, o.shape_keys_per_thread)) < 0) return GS_ERR_ARG;
    if (max_keys == 0 || max_keys > GS_MAX_KEYS) return GS_ERR_SIZE;
    if (mode == GS_MODE_KEYS_ONLY) {
        if (value_bytes != 0) return GS_ERR_MODE;
    } else if (mode == GS_MODE_PAIRS) {
        if (value_bytes != 4 && value_bytes != 8) return GS_ERR_MODE;
    } else {
        return GS_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GS_ERR_NO_DEVICE;
    gs_onesweep* h = new (std::nothrow) gs_onesweep();
    if (!h) return GS_ERR_ARG;
    h->max_keys = max_keys;
    h->mode = mode;
    h->value_bytes = value_bytes;
    h->shape = (mode == GS_MODE_PAIRS && value_bytes == 4) ? 1 : 0;
    if (shape_pick >= 0) { h->shape = shape_pick; h->shape_auto = 0; }
    h->small_path = o.small_path ? 1 : 0;
    h->pos_chains = o.position_chains;
    h->pos_min_keys = o.position_chains_min_log2 == 25 ? (1u << 25) + 1u : 1u << o.position_chains_min_log2;
    h->key64_sweeps = o.key64_sweeps;
    h->skip_passes = o.skip_passes ? 1 : 0;
    h->mid_path = o.mid_path ? 1 : 0;
    h->hist_blocks_opt = o.hist_blocks;
    h->first_pass_big = o.first_pass_big ? 1 : 0;
    // debug bits belong to tuning builds; every other build keeps 0 (bit 30 — skip the bucket-local sort,
    // tools/hy_bringup.py — would hand back keys ordered on their top 16 bits only)
#ifdef GS_TUNING
    h->debug_flags = o.debug_flags;
#endif
    h->plan = o.plan;
    h->hy_grid = hy_grid_for_device();
    h->slab_words = slab_words_for(max_keys);
    // Tile ranking: the returning-LDS-atomic path needs same-address lanes of one
    // wave-instruction served in ascending lane order.  Probe the device once per
    // process; fall back to the ballot multi-split if a single lane disagrees.
    h->rank_mode = o.rank_mode >= 0 ? o.rank_mode : (lds_atomic_order_ok() ? 1 : 0);
    hipError_t e = hipMalloc(&h->slab, h->slab_words * sizeof(uint32_t));
    // the two-level plan's tables (0.8 MiB) and its histogram slices (hy_grid x 129 KiB: 33 MiB on 256 CUs): only for handles the default
    // routing can send there — keys-only and pairs handles that hold a sort of the plan's size — or that ask for plan 2 (tests, tools:
    // wherever the position-chain plan, its fall-back, runs: from 2^20 keys); gs_onesweep_set_plan(2) allocates them on demand otherwise
    const bool hy_handle = o.plan != 1 && (o.plan == 2 ? max_keys > (1u << 20) : max_keys >= (mode == GS_MODE_PAIRS ? HY_MIN_PAIRS_DEFAULT : HY_MIN_KEYS_DEFAULT));
    h->partials_words = (size_t)hist_blocks_cap(max_keys, o.hist_blocks) * gs::HIST_TABLE_WORDS;
    if (hy_handle && (size_t)h->hy_grid * gs::HY_SLICE_WORDS > h->partials_words) h->partials_words = (size_t)h->hy_grid * gs::HY_SLICE_WORDS;
    if (e == hipSuccess) e = hipMalloc(&h->partials, h->partials_words * sizeof(uint32_t));
    if (e == hipSuccess && hy_handle) e = hipMalloc(&h->hy_tab, gs::HYT_WORDS * sizeof(uint32_t));
    // counters/status/info start defined: gs_onesweep_check() may run before any tiled sort (single-tile path)
    if (e == hipSuccess) e = hipMemset(h->slab, 0, SLAB_DESC * sizeof(uint32_t));
    if (e == hipSuccess) e = hipHostMalloc(&h->pinned, (4 * gs::NCH * gs::RADIX + 8) * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        if (h->slab) (void)hipFree(h->slab);
        if (h->partials) (void)hipFree(h->partials);
        if (h->hy_tab) (void)hipFree(h->hy_tab);
        delete h;
        return GS_ERR_HIP;
    }
    *out = h;
    return GS_OK;
}

gs_status gs_onesweep_destroy(gs_onesweep* h) {
    if (!h) return GS_ERR_ARG;
    if (h->ev_valid)
        for (auto& e : h->ev) (void)hipEventDestroy(e);
    if (h->pinned) (void)hipHostFree(h->pinned);
    if (h->slab) (void)hipFree(h->slab);
    if (h->partials) (void)hipFree(h->partials);
    if (h->hy_tab) (void)hipFree(h->hy_tab);
    delete h;
    return GS_OK;
}

gs_status gs_debug_read_slab(gs_onesweep* h, uint32_t first_word, uint32_t count, uint32_t* h_out, void* stream) {
    // bit 31 of first_word: the workgroups' table slices (hist partials) instead of the slab
    const bool part = (first_word >> 31) != 0u;
    first_word &= 0x7fffffffu;
    const size_t limit = part ? (h ? h->partials_words : 0) : (h ? h->slab_words : 0);
    if (!h || !h_out || (size_t)first_word + count > limit) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GS_HIP(hipMemcpyAsync(h_out, (part ? h->partials : h->slab) + first_word, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    return GS_OK;
}

gs_status gs_debug_sort_route(gs_onesweep* h, uint32_t n, gs_key_type kt, uint32_t report[8]) {
    if (!h || !report || !valid_key_type(kt)) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys) return GS_ERR_SIZE;
    const uint32_t vb = h->value_bytes;
    const SortRoute r = sort_route(h, n, kt, vb);
    report[GS_ROUTE_R_SMALL] = r.small ? (uint32_t)small_class(n) : GS_ROUTE_NONE;
    report[GS_ROUTE_R_MID] = (uint32_t)r.mid_cls;
    report[GS_ROUTE_R_SHAPE] = (uint32_t)r.shape;
    report[GS_ROUTE_R_SHAPE0] = (uint32_t)r.shape0;
    report[GS_ROUTE_R_DYN] = r.dyn;
    report[GS_ROUTE_R_POS] = r.pos ? pos_tile_for(vb) : 0u;
    report[GS_ROUTE_R_HY] = r.hy ? 1u : 0u;
    report[GS_ROUTE_R_RANK] = (uint32_t)h->rank_mode;
    return GS_OK;
}

static_assert(GS_PF_SKEW == gs::PF_SKEW && GS_PF_SKIP == gs::PF_SKIP && GS_PF_SRC_ALT == gs::PF_SRC_ALT && GS_PF_LAST == gs::PF_LAST &&
              GS_PF_POS == gs::PF_POS && GS_PF_HALF16 == gs::PF_HALF16, "header and kernels agree on the pass flags");
static_assert(GS_SLAB_STATUS_WORD == gs::SLAB_STATUS && GS_ST_GUARD_HANDOVERS == gs::ST_GUARD_HANDOVERS && GS_ST_STOLEN_TILES == gs::ST_STOLEN_TILES,
              "header and kernels agree on the status block");
uint32_t gs_debug_hy_half_slot(uint32_t base_p, uint32_t base_p1, uint32_t n, uint32_t descending, uint32_t rank) {
    return gs::hy_half_slot(base_p, base_p1, n, descending, rank);
}
gs_status gs_debug_pass_flags(gs_onesweep* h, uint32_t flags[8], void* stream) {
    if (!h || !flags) return GS_ERR_ARG;
    for (uint32_t q = 0; q < gs::MAX_PASSES; ++q) flags[q] = 0;
    if (h->last_tile == 0) return GS_OK;  // single-tile or mid-size route, or nothing yet: no pass plan was made
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (uint32_t q = 0; q < gs::MAX_PASSES; ++q)
        GS_HIP(hipMemcpyAsync(h->pinned + q, h->slab + SLAB_INFO + q * gs::INFO_STRIDE + gs::PASS_FLAGS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    for (uint32_t q = 0; q < h->last_np && q < gs::MAX_PASSES; ++q) flags[q] = h->pinned[q];
    return GS_OK;
}

int gs_debug_registry_dims(uint32_t family, int32_t dims[5]) { return dims ? registry_lookup(family, dims, nullptr) : -1; }
int gs_debug_registry_cell(uint32_t family, const int32_t coord[5]) { return coord ? registry_lookup(family, nullptr, coord) : -1; }

gs_status gs_onesweep_set_plan(gs_onesweep* h, int plan) {
    if (!h || plan < 0) return GS_ERR_ARG;
    if (plan > 2) return GS_ERR_ARG;
    if (plan == 2 && !h->hy_tab) {
        // the handle was created without the plan's tables (below the plan's default size, or plan 1): allocate them now.  The caller
        // must not have a sort of this handle in flight (as for every setter): the slices are re-allocated.
        if (h->max_keys <= (1u << 20)) return GS_ERR_MODE;  // (the plan's fall-back, the position-chain plan, starts above 2^20 keys)
        const size_t need = (size_t)h->hy_grid * gs::HY_SLICE_WORDS;
        if (need > h->partials_words) {
            uint32_t* p = nullptr;
            GS_HIP(hipDeviceSynchronize());
            GS_HIP(hipMalloc(&p, need * sizeof(uint32_t)));
            (void)hipFree(h->partials);
            h->partials = p;
            h->partials_words = need;
        }
        GS_HIP(hipMalloc(&h->hy_tab, gs::HYT_WORDS * sizeof(uint32_t)));
    }
    h->plan = plan;
    return GS_OK;
}

gs_status gs_debug_set_hy_class(gs_onesweep* h, int cls) {
    if (!h || cls < -1 || cls > 3) return GS_ERR_ARG;
    h->hy_class_forced = cls;
    return GS_OK;
}

gs_status gs_debug_set_pos_grid(gs_onesweep* h, uint32_t workgroups) {
    if (!h || (workgroups != 0u && (workgroups < gs::NCH || workgroups > 65535u))) return GS_ERR_ARG;
    h->pos_grid_forced = workgroups;
    return GS_OK;
}

gs_status gs_onesweep_last_plan(gs_onesweep* h, uint32_t* plan, uint32_t* largest_bucket, void* stream) {
    if (!h || !plan) return GS_ERR_ARG;
    *plan = 0;
    if (largest_bucket) *largest_bucket = 0;
    if (!h->last_hy) return GS_OK;  // the last sort was not offered the two-level plan (size, mode, options): LSD passes, or a one- / two-launch route
    hipStream_t s = static_cast<hipStream_t>(stream);
    GS_HIP(hipMemcpyAsync(h->pinned, h->slab + gs::SLAB_HY, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    *plan = h->pinned[gs::HY_VALID] ? 1u : 0u;
    if (largest_bucket) *largest_bucket = h->pinned[gs::HY_MAXBUCKET];
    return GS_OK;
}

gs_status gs_onesweep_set_shape(gs_onesweep* h, uint32_t threads, uint32_t keys_per_thread) {
    const int shape = find_shape(threads, keys_per_thread);
    if (!h || shape < 0) return GS_ERR_ARG;
    h->shape = shape;
    h->shape_auto = 0;
    return GS_OK;
}

gs_status gs_debug_set_trace(gs_onesweep* h, void* d_buf) {  // experiment builds: 4 passes x grid x 8 words
    if (!h) return GS_ERR_ARG;
    h->trace_buf = d_buf;
    return GS_OK;
}

gs_status gs_onesweep_set_small_path(gs_onesweep* h, int on) {
    if (!h) return GS_ERR_ARG;
    h->small_path = on ? 1 : 0;
    return GS_OK;
}

gs_status gs_onesweep_set_mid_path(gs_onesweep* h, int on) {
    if (!h) return GS_ERR_ARG;
    h->mid_path = on ? 1 : 0;
    return GS_OK;
}

gs_status gs_onesweep_set_skip_passes(gs_onesweep* h, int on) {
    if (!h) return GS_ERR_ARG;
    h->skip_passes = on ? 1 : 0;
    return GS_OK;
}

gs_status gs_onesweep_set_rank_mode(gs_onesweep* h, int mode) {
    if (!h || mode < 0 || mode > 1) return GS_ERR_ARG;
    h->rank_mode = mode;
    return GS_OK;
}

int gs_onesweep_get_rank_mode(gs_onesweep* h) { return h ? h->rank_mode : -1; }

gs_status gs_selftest_lds_atomic_order(uint32_t iters, uint32_t seed, uint64_t* h_failures, void* stream) {
    if (!h_failures || iters == 0) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceScratch d(sizeof(uint32_t));
    gs_status st = d.alloc_zeroed(s);
    if (st != GS_OK) return st;
    hipLaunchKernelGGL(gs::lds_atomic_order_probe, dim3(256 * 4), dim3(512), 0, s, seed, iters, d.as<uint32_t>());
    uint32_t h32 = 0;
    st = d.read_back(&h32, s);
    *h_failures = h32;
    return st;
}

gs_status gs_selftest_wave_primitives(uint32_t seed, uint32_t waves, uint32_t* d_out, void* stream) {
    if (!d_out || waves == 0 || (waves & 3u) != 0u || waves > (1u << 20)) return GS_ERR_ARG;
    hipLaunchKernelGGL(gs::wave_primitives_kernel, dim3(waves / 4u), dim3(256), 0, static_cast<hipStream_t>(stream), seed, d_out);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

#ifdef GS_TUNING
// Tuning aid: global access pattern of a DigitBinningPass without ranking or look-back (memory floor of the tile shape);
// threads == 0: plain streaming copies (kpt 0 / 1 / 2 = default / nt loads / nt loads and stores) and a read-only sweep (kpt 3).
gs_status gs_debug_copy_floor(const void* d_in, void* d_out, uint32_t n, uint32_t threads, uint32_t kpt, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t tiles = threads ? n / (threads * (kpt ? kpt : 1u)) : 1u;
    if (!tiles) return GS_ERR_SIZE;
    const uint32_t* in = static_cast<const uint32_t*>(d_in);
    uint32_t* out = static_cast<uint32_t*>(d_out);
    if (threads == 512 && kpt == 32) hipLaunchKernelGGL((gs::copy_floor_kernel<512, 32>), dim3(tiles), dim3(512), 0, s, in, out, n);
    else if (threads == 512 && kpt == 16) hipLaunchKernelGGL((gs::copy_floor_kernel<512, 16>), dim3(tiles), dim3(512), 0, s, in, out, n);
    else if (threads == 1024 && kpt == 16) hipLaunchKernelGGL((gs::copy_floor_kernel<1024, 16>), dim3(tiles), dim3(1024), 0, s, in, out, n);
    else if (threads == 256 && kpt == 32) hipLaunchKernelGGL((gs::copy_floor_kernel<256, 32>), dim3(tiles), dim3(256), 0, s, in, out, n);
    else if (threads == 0) {  // calibration copies: kpt = 0/1/2 copy policy, 3 = read-only sweep
        const uint32_t nvec = n / 4, grid = 256 * 8;
        const gs::u32x4* vi = static_cast<const gs::u32x4*>(d_in);
        gs::u32x4* vo = static_cast<gs::u32x4*>(d_out);
        if (kpt == 0) hipLaunchKernelGGL(gs::copy_x4_kernel<0>, dim3(grid), dim3(256), 0, s, vi, vo, nvec);
        else if (kpt == 1) hipLaunchKernelGGL(gs::copy_x4_kernel<1>, dim3(grid), dim3(256), 0, s, vi, vo, nvec);
        else if (kpt == 2) hipLaunchKernelGGL(gs::copy_x4_kernel<2>, dim3(grid), dim3(256), 0, s, vi, vo, nvec);
        else if (kpt == 3) hipLaunchKernelGGL(gs::read_x4_kernel, dim3(grid), dim3(256), 0, s, vi, out, nvec);
        // round 4: the best shapes tools/r04_probe.hip found — 4: read, four nt loads in flight, two workgroups per CU; 5: copy, four nt
        // loads in flight, one-shot grid of n / 8192 workgroups; 6: copy, four plain loads in flight, one workgroup per CU; 7: hipMemcpyAsync
        else if (kpt == 4) hipLaunchKernelGGL((gs::read_xu_kernel<4, true>), dim3(256 * 2), dim3(256), 0, s, vi, out, (size_t)nvec);
        else if (kpt == 5) hipLaunchKernelGGL((gs::copy_xu_kernel<4, true>), dim3(nvec / (256 * 4) / 2 ? nvec / (256 * 4) / 2 : 1), dim3(256), 0, s, vi, vo, (size_t)nvec);
        else if (kpt == 6) hipLaunchKernelGGL((gs::copy_xu_kernel<4, false>), dim3(256), dim3(256), 0, s, vi, vo, (size_t)nvec);
        else if (kpt == 7) GS_HIP(hipMemcpyAsync(d_out, d_in, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        else return GS_ERR_ARG;
    } else return GS_ERR_ARG;
    GS_HIP(hipGetLastError());
    return GS_OK;
}
#endif

uint32_t gs_onesweep_get_partition_size(gs_onesweep* h) {
    return h ? (uint32_t)g_shapes[h->shape].threads * g_shapes[h->shape].kpt : 0;
}

gs_status gs_onesweep_sort_keys(gs_onesweep* h, void* d_keys, void* d_alt, uint32_t n, gs_key_type kt, gs_order order,
                                void* stream) {
    gs_status st = check_common(h, d_keys, d_alt, n, kt, order);
    if (st != GS_OK) return st;
    return sort_impl(h, d_keys, nullptr, d_alt, nullptr, n, kt, order, static_cast<hipStream_t>(stream), 0);
}

gs_status gs_onesweep_sort_pairs(gs_onesweep* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals,
                                 uint32_t n, gs_key_type kt, gs_order order, void* stream) {
    gs_status st = check_common(h, d_keys, d_alt_keys, n, kt, order);
    if (st != GS_OK) return st;
    if ((st = check_vals(h, d_vals, d_alt_vals)) != GS_OK) return st;
    return sort_impl(h, d_keys, d_vals, d_alt_keys, d_alt_vals, n, kt, order, static_cast<hipStream_t>(stream),
                     h->value_bytes);
}

gs_status gs_onesweep_check(gs_onesweep* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GS_HIP(hipMemcpyAsync(h->pinned, h->slab + SLAB_STATUS, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    return h->pinned[0] == gs::STATUS_OK ? GS_OK : GS_ERR_TIMEOUT;
}

gs_status gs_debug_poke_status(gs_onesweep* h, uint32_t word, void* stream) {  // tests: forge the device status word
    if (!h) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    h->pinned[0] = word;
    GS_HIP(hipMemcpyAsync(h->slab + SLAB_STATUS, h->pinned, sizeof(uint32_t), hipMemcpyHostToDevice, s));
    GS_HIP(hipStreamSynchronize(s));
    return GS_OK;
}

gs_status gs_debug_check_state(gs_onesweep* h, uint64_t report[8], void* stream) {
    if (!h || !report) return GS_ERR_ARG;
    for (int i = 0; i < 8; ++i) report[i] = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h->last_tile == 0) return GS_OK;  // single-tile sort or nothing yet: there is no scan state to check
    DeviceScratch d(8 * sizeof(unsigned long long));
    const gs_status st = d.alloc_zeroed(s);
    if (st != GS_OK) return st;
    hipLaunchKernelGGL(gs::check_state_kernel, dim3(h->last_hy ? gs::CHMAX : gs::MAXCH, h->last_np), dim3(256), 0, s, h->slab, h->last_desc_stride,
                       h->last_tile, 0u, h->last_dyn, d.as<unsigned long long>(), h->last_pos_tile, h->last_tile0);
    return d.read_back(report, s);
}

gs_status gs_onesweep_global_histogram(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt, uint32_t* h_hist,
                                       void* stream) {
    PassPlan plan;
    gs_status st = check_hist_args(h, d_keys, h_hist, n, kt);
    if (st == GS_OK) st = read_hist(h, d_keys, n, kt, static_cast<hipStream_t>(stream), 0, 4, &plan);
    if (st != GS_OK) return st;
    for (uint32_t q = 0; q < 4; ++q)  // digit totals = joint histogram summed over chains
        for (uint32_t d = 0; d < gs::RADIX; ++d) {
            uint32_t g = 0;
            for (uint32_t x = 0; x < gs::NCH; ++x) g += h->pinned[gs::hist_index(q, d, x)];
            h_hist[q * gs::RADIX + d] = g;
        }
    return GS_OK;
}

gs_status gs_onesweep_scan(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt, uint32_t* h_rows, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    PassPlan plan;
    gs_status st = check_hist_args(h, d_keys, h_rows, n, kt);
    // chain 0 of every pass starts at row 0 of the pass's descriptor region: its seed row holds the digit starts themselves
    if (st == GS_OK)
        st = hist_and_wait(h, d_keys, n, kt, s, 0, 4, &plan, [&] {
            for (uint32_t q = 0; q < 4; ++q)
                GS_HIP(hipMemcpyAsync(h->pinned + q * gs::RADIX, h->slab + SLAB_DESC + (size_t)q * plan.desc_stride, gs::RADIX * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, s));
            return GS_OK;
        });
    if (st != GS_OK) return st;
    memcpy(h_rows, h->pinned, 4 * gs::RADIX * sizeof(uint32_t));
    return GS_OK;
}

gs_status gs_onesweep_digit_pass(gs_onesweep* h, const void* d_keys_in, void* d_keys_out, const void* d_vals_in,
                                 void* d_vals_out, uint32_t n, uint32_t pass, gs_key_type kt, int reverse_index,
                                 void* stream) {
    gs_status st = check_common(h, d_keys_in, d_keys_out, n, kt, GS_ORDER_ASCENDING);
    if (st != GS_OK) return st;
    if (pass > (is_key64(kt) ? 7u : 3u)) return GS_ERR_ARG;
    const bool pairs = d_vals_in || d_vals_out;
    if (pairs && (st = check_vals(h, d_vals_in, d_vals_out)) != GS_OK) return st;
    const uint32_t vb = pairs ? h->value_bytes : 0u;
    const int shape = bin_shape(h, kt, vb, h->shape);
    BinLauncher fn = bin_launcher(shape, h->rank_mode, vb, kt);
    if (!fn) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PassPlan plan;
    PrologueIn in;  // a stand-alone pass: position segments on ANY input
    in.first_pass = pass & 3u;
    in.num_passes = 1;
    in.shape_index = shape;
    in.word = pass >> 2;
    st = prologue(h, d_keys_in, n, kt, s, in, &plan);
    if (st != GS_OK) return st;
    launch_pass(h, fn, s, plan.grid, 0, plan.desc_stride, d_keys_in, d_keys_out, d_vals_in, d_vals_out, n, pass * 8,
                (reverse_index ? gs::BM_REVERSE : 0u) | gs::BM_ZERO_HIST);
    GS_HIP(hipGetLastError());
    h->hist_dirty = false;
    if (h->profiling)  // slot 3 = this pass, slots 4..6 = 0
        for (int e = 4; e <= 7; ++e) GS_HIP(hipEventRecord(h->ev[e], s));
    h->profile_pending = h->profiling != 0;
    return GS_OK;
}

// ---- multi-GPU MSD split in two steps that share ONE histogram + scan of the shard -------------
gs_status gs_onesweep_msd_prepare(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt, uint32_t* h_hist256,
                                  void* stream) {
    PassPlan plan;
    gs_status st = check_hist_args(h, d_keys, h_hist256, n, kt);
    // top byte, position chains (HIST is handed back here: msd_partition may never be called)
    if (st == GS_OK) st = read_hist(h, d_keys, n, kt, static_cast<hipStream_t>(stream), 3, 1, &plan);
    if (st != GS_OK) return st;
    for (uint32_t d = 0; d < gs::RADIX; ++d) {
        uint32_t g = 0;
        for (uint32_t x = 0; x < gs::NCH; ++x) g += h->pinned[gs::hist_index(0, d, x)];
        h_hist256[d] = g;
    }
    h->msd_keys = d_keys;
    h->msd_n = n;
    h->msd_kt = kt;
    h->msd_grid = plan.grid;
    return GS_OK;
}

gs_status gs_onesweep_msd_partition(gs_onesweep* h, const void* d_keys_in, void* d_keys_out, const void* d_vals_in,
                                    void* d_vals_out, uint32_t n, void* stream) {
    if (!h || h->msd_keys == nullptr || h->msd_keys != d_keys_in || h->msd_n != n) return GS_ERR_ARG;  // needs its prepare
    gs_status st = check_common(h, d_keys_in, d_keys_out, n, h->msd_kt, GS_ORDER_ASCENDING);
    if (st != GS_OK) return st;
    const bool pairs = d_vals_in || d_vals_out;
    if (pairs && (st = check_vals(h, d_vals_in, d_vals_out)) != GS_OK) return st;
    BinLauncher fn = bin_launcher(h->shape, h->rank_mode, pairs ? h->value_bytes : 0u, h->msd_kt);
    if (!fn) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_pass(h, fn, s, h->msd_grid, 0, 0, d_keys_in, d_keys_out, d_vals_in, d_vals_out, n, 24, gs::BM_ZERO_HIST);
    GS_HIP(hipGetLastError());
    h->msd_keys = nullptr;  // the scan state is consumed
    h->profile_pending = false;
    return GS_OK;
}

gs_status gs_onesweep_set_profiling(gs_onesweep* h, int enabled) {
    if (!h) return GS_ERR_ARG;
    if (enabled && !h->ev_valid) {
        for (auto& e : h->ev) GS_HIP(hipEventCreate(&e));
        h->ev_valid = true;
    }
    h->profiling = enabled ? 1 : 0;
    h->profile_pending = false;
    return GS_OK;
}

gs_status gs_onesweep_get_profile(gs_onesweep* h, float ms[GS_PROFILE_SLOTS]) {
    if (!h || !ms) return GS_ERR_ARG;
    if (!h->profile_pending) return GS_ERR_ARG;
    GS_HIP(hipEventSynchronize(h->ev[7]));
    for (int i = 0; i < 7; ++i) GS_HIP(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
    GS_HIP(hipEventElapsedTime(&ms[7], h->ev[0], h->ev[7]));
    return GS_OK;
}

gs_status gs_init_random(void* d_keys, void* d_vals, uint32_t value_bytes, uint32_t and_count, uint32_t seed, uint32_t n,
                         void* stream) {
    if (!d_keys || n == 0) return n == 0 ? GS_ERR_SIZE : GS_ERR_ARG;
    if (and_count > 31) return GS_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* k = static_cast<uint32_t*>(d_keys);
    if (!d_vals || value_bytes == 0)
        hipLaunchKernelGGL(gs::init_random_kernel<0>, dim3(256), dim3(256), 0, s, k, nullptr, and_count, seed, n);
    else if (value_bytes == 4)
        hipLaunchKernelGGL(gs::init_random_kernel<4>, dim3(256), dim3(256), 0, s, k, d_vals, and_count, seed, n);
    else if (value_bytes == 8)
        hipLaunchKernelGGL(gs::init_random_kernel<8>, dim3(256), dim3(256), 0, s, k, d_vals, and_count, seed, n);
    else
        return GS_ERR_MODE;
    GS_HIP(hipGetLastError());
    return GS_OK;
}

gs_status gs_validate(const void* d_keys, const void* d_vals, uint32_t value_bytes, uint32_t n, gs_key_type kt,
                      gs_order order, uint32_t* h_err_count, void* stream) {
    if (!d_keys || !h_err_count || !valid_key_type(kt)) return GS_ERR_ARG;
    if (n == 0) return GS_ERR_SIZE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceScratch scratch(sizeof(uint32_t));
    const gs_status st = scratch.alloc_zeroed(s);
    if (st != GS_OK) return st;
    uint32_t* d_err = scratch.as<uint32_t>();
    const uint32_t blocks = div_up(n, 256 * 16) < 2048 ? div_up(n, 256 * 16) : 2048;
    const uint32_t* k = static_cast<const uint32_t*>(d_keys);
    const int desc = order == GS_ORDER_DESCENDING;
    if (is_key64(kt))  // 64-bit keys: the keys' order only
        hipLaunchKernelGGL(gs::validate64_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const uint2*>(d_keys), n, (int)kt, desc, d_err);
    else if (!d_vals || value_bytes == 0)
        hipLaunchKernelGGL(gs::validate_kernel<0>, dim3(blocks), dim3(256), 0, s, k, nullptr, n, (int)kt, desc, d_err);
    else if (value_bytes == 4)
        hipLaunchKernelGGL(gs::validate_kernel<4>, dim3(blocks), dim3(256), 0, s, k, d_vals, n, (int)kt, desc, d_err);
    else if (value_bytes == 8)
        hipLaunchKernelGGL(gs::validate_kernel<8>, dim3(blocks), dim3(256), 0, s, k, d_vals, n, (int)kt, desc, d_err);
    else
        return GS_ERR_MODE;
    return scratch.read_back(h_err_count, s);
}

gs_status gs_msd_splitters_n(const uint64_t* hist, uint32_t nbins, uint32_t world, uint32_t* first_bin) {
    if (!hist || !first_bin || world == 0 || nbins == 0 || world > nbins) return GS_ERR_ARG;
    uint64_t total = 0;
    for (uint32_t b = 0; b < nbins; ++b) total += hist[b];
    // Rank r starts at the first bin whose exclusive prefix reaches ceil(r * total / world):
    // equal-count buckets at bin granularity.
    first_bin[0] = 0;
    uint64_t excl = 0;
    uint32_t b = 0;
    for (uint32_t r = 1; r < world; ++r) {
        const uint64_t target = (total * r + world - 1) / world;
        while (b < nbins && excl < target) excl += hist[b++];
        first_bin[r] = b;
    }
    first_bin[world] = nbins;
    return GS_OK;
}

gs_status gs_msd_splitters(const uint64_t hist256[256], uint32_t world, uint32_t* first_bin) {
    if (world > 256) return GS_ERR_ARG;
    return gs_msd_splitters_n(hist256, 256, world, first_bin);
}

// 12-bit prefix histogram of a shard: (top byte, top nibble of the byte below) = the joint histogram the sort's
// own GlobalHistogram kernel counts for the last pass (chain = group of the previous digit), bin = d3*16 + (d2>>4).
gs_status gs_onesweep_msd_fine_histogram(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type kt,
                                         uint32_t* h_hist4096, void* stream) {
    if (gs::NCH != 16) return GS_ERR_ARG;  // the fine MSD histogram is the 16-chain joint histogram (tuning builds with other chain counts)
    PassPlan plan;
    gs_status st = check_hist_args(h, d_keys, h_hist4096, n, kt);
    // bytes 2 and 3: row 1 = H(d3, group of d2); profiled: slots 0..2 (clear, histogram, scan) are this call's, the pass slots read 0
    if (st == GS_OK) st = read_hist(h, d_keys, n, kt, static_cast<hipStream_t>(stream), 2, 2, &plan, true);
    if (st != GS_OK) return st;
    for (uint32_t d = 0; d < gs::RADIX; ++d)
        for (uint32_t x = 0; x < gs::NCH; ++x) h_hist4096[d * gs::NCH + x] = h->pinned[gs::hist_index(1, d, x)];
    return GS_OK;
}

}  // extern "C"

namespace {
// a sort on another handle's engine (segmented sort, top-k): the public entry for the handle's mode
inline gs_status engine_sort(gs_onesweep* engine, bool pairs, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n,
                             gs_key_type kt, gs_order order, hipStream_t s) {
    return pairs ? gs_onesweep_sort_pairs(engine, d_keys, d_vals, d_alt_keys, d_alt_vals, n, kt, order, s)
                 : gs_onesweep_sort_keys(engine, d_keys, d_alt_keys, n, kt, order, s);
}
}  // namespace
