// topk_seg_host.hpp — part of the gpusort_capi.hip translation unit: the gs_segtopk handle (topk_seg_kernels.hpp) and its entries.
// The handle's own: the launchers, the per-class launches of a call and the report.  Allocation, create/destroy, the control
// read-back, the rank mode and the head of a segmented call are handle_core.hpp's.  No counterpart in the reference project.
struct gs_segtopk {
    uint32_t max_keys, max_segments, max_k;
    gs_mode mode;
    uint32_t value_bytes;
    int rank_mode;               // the ranking of the tile classes: 0 ballot multi-split, 1 returning LDS atomic (probed at create)
    Workspace ws;                // gs::SEGC_WORDS control words, then the class lists (max_segments words)
    // the last call (gs_segtopk_last)
    uint32_t last_forms = 0, last_k = 0;
};

static_assert(GS_SEGTOPK_R_CLASSES + GS_SEGSORT_CLASSES <= GS_SEGTOPK_R_LONGEST && GS_SEGTOPK_REPORT_WORDS >= 16, "the report holds every class");
namespace {
inline size_t segtopk_bytes(uint32_t max_segments) {
    Arena a;
    a.take(((size_t)gs::SEGC_WORDS + max_segments) * sizeof(uint32_t));
    return a.total();
}

// the kernels are launched directly (no registry family; gs_segtopk_last's forms word accounts for them)
using TksLauncher = void (*)(hipStream_t, uint32_t grid, const gs::TksArgs& a, uint32_t cls);
template <int VM>
void launch_tks_packed(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t) {
    hipLaunchKernelGGL((gs::tks_packed_kernel<VM>), dim3(grid), dim3(64), 0, s, a);
}
template <int VM>
void launch_tks_wave(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t) {
    hipLaunchKernelGGL((gs::tks_wave_kernel<VM>), dim3(grid), dim3(64 * gs::TKR_WAVE_ROWS), 0, s, a);
}
template <int VM>
void launch_tks_stream(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t) {
    hipLaunchKernelGGL((gs::tks_stream_kernel<VM, 0>), dim3(grid), dim3(gs::TKR_THREADS), 0, s, a);  // (RANK 0, as the row-wise stream kernel)
}
template <int T, int K, int VM, int RANK>
void launch_tks_tile(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t cls) {
    hipLaunchKernelGGL((gs::tks_tile_kernel<T, K, VM, RANK, SEG_WG_LOOP(T, K)>), dim3(grid), dim3(T), 0, s, a, cls);
}
struct TksVmLaunchers { TksLauncher packed, wave, stream; };
constexpr auto g_tks_vm = Table<4>::make([](auto v) -> TksVmLaunchers {  // [vm index]
    if constexpr (TK_BUILT) return TksVmLaunchers{launch_tks_packed<VM_OF[v]>, launch_tks_wave<VM_OF[v]>, launch_tks_stream<VM_OF[v]>};
    else return TksVmLaunchers{nullptr, nullptr, nullptr};
});
using TksTileTable = Table<5, 2, 4>;  // [workgroup class][rank mode][vm index]: the cells of the row-wise tile kernel (class 6 no 8-byte values, class 7 keys only)
constexpr auto g_tks_tile = TksTileTable::make([](auto c, auto r, auto v) -> TksLauncher {
    if constexpr (tkr_tile_built(c, VM_OF[v])) return launch_tks_tile<g_small_class[c].threads, g_small_class[c].kpt, VM_OF[v], r>;
    else return nullptr;
});

// what the key width decides in a call: the element size, the accepted key types, the kernels (topk_seg16_host.hpp has the 2-byte set)
struct TksRoutes {
    uint32_t key_bytes;
    const TksVmLaunchers* vm;  // [vm index]
    const TksLauncher* tile;   // TksTileTable
    // whether a tile shape's kernel walks its class list by grid stride on seg_grid's grid, or takes one workgroup per slot the class
    // can have; and the same for the stream kernel
    bool (*tile_loops)(int threads, int kpt);
    bool stream_loops;
};
constexpr TksRoutes g_tks_routes32{4u, g_tks_vm.data(), g_tks_tile.data(), SEG_WG_LOOP, true};

gs_status segtopk_impl(const TksRoutes& routes, gs_segtopk* h, const void* d_keys, const void* d_vals, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments, uint32_t k,
                       uint32_t max_len, void* d_out_keys, void* d_out_vals, gs_key_type kt, gs_order order, hipStream_t s, bool pairs) {
    if (!h || !d_keys || !d_out_keys || !d_offsets || misaligned(d_keys) || misaligned(d_out_keys) || (reinterpret_cast<uintptr_t>(d_offsets) & 3u) ||
        !(routes.key_bytes == 2u ? is_key16(kt) : is_key32_type(kt)) || !valid_order(order))
        return GS_ERR_ARG;  // (64-bit key types: out of scope; the 16-bit ones: gs_segtopk16_*)
    if (pairs != (h->mode == GS_MODE_PAIRS)) return GS_ERR_MODE;
    const uint32_t vb = h->value_bytes, kb = routes.key_bytes;
    const bool pos = pairs && !d_vals;  // the value is the element's position in the whole array
    if (pairs && (!d_out_vals || misaligned(d_out_vals) || (pos ? vb != 4u : misaligned(d_vals)))) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys || num_segments == 0 || num_segments > h->max_segments || k == 0 || k > h->max_k) return GS_ERR_SIZE;
    const unsigned long long out_elems = (unsigned long long)num_segments * k;
    const size_t off_bytes = ((size_t)num_segments + 1u) * 4u;
    if (buffers_overlap(d_keys, (size_t)n * kb, d_out_keys, (size_t)out_elems * kb) || buffers_overlap(d_offsets, off_bytes, d_out_keys, (size_t)out_elems * kb) ||
        (pairs && (buffers_overlap(d_offsets, off_bytes, d_out_vals, (size_t)out_elems * vb) || buffers_overlap(d_keys, (size_t)n * kb, d_out_vals, (size_t)out_elems * vb) ||
                   buffers_overlap(d_out_keys, (size_t)out_elems * kb, d_out_vals, (size_t)out_elems * vb) ||
                   (!pos && (buffers_overlap(d_vals, (size_t)n * vb, d_out_vals, (size_t)out_elems * vb) || buffers_overlap(d_vals, (size_t)n * vb, d_out_keys, (size_t)out_elems * kb))))))
        return GS_ERR_ARG;
    // lengths are known on the device only: a k the stream route does not take needs the promise that no segment goes there
    const bool allow_long = max_len == 0u || max_len > gs::seg_max_lds(vb);
    if (allow_long && k > gs::TKR_STAGE) return GS_ERR_SIZE;
    if (!TK_BUILT) return GS_ERR_MODE;  // this build flavour has no selection
    const uint32_t top = allow_long ? gs::SEG_CLASS_LONG : gs::seg_class_of(max_len, vb);  // the highest class a segment can fall in
    uint32_t* ctl = h->ws.ctl();
    const gs::TksArgs a{static_cast<const uint32_t*>(d_keys), d_vals, static_cast<uint32_t*>(d_out_keys), d_out_vals, d_offsets, ctl + gs::SEGC_WORDS, ctl,
                        num_segments, k, (uint32_t)kt, order == GS_ORDER_DESCENDING ? 1u : 0u, max_len};
    const uint32_t vm = !pairs ? 0u : pos ? 1u : vb, vi = (uint32_t)vm_index(vm), rank = h->rank_mode ? 1u : 0u;
    const TksVmLaunchers& f = routes.vm[vi];
    uint32_t forms = GS_SEGTOPK_F_VM << vi;
    h->last_k = k;
    h->last_forms = 0;
    seg_enqueue_head(ctl, d_offsets, num_segments, n, vb, max_len, top, s);
    f.packed(s, div_up(num_segments, 64), a, 0);
    forms |= GS_SEGTOPK_F_PACKED;
    const uint32_t vbs = vm == 0 ? 0u : vm == 8 ? 8u : 4u;  // the bytes a value takes in LDS: positions are 4-byte values
    if (top >= 2 && n > gs::SEG_PACK_MAX) {
        f.wave(s, seg_grid(div_up(seg_class_bound(n, num_segments, gs::SEG_PACK_MAX + 1), gs::TKR_WAVE_ROWS), gs::TKR_WAVE_ROWS,
                           (size_t)gs::TKR_WAVE_ROWS * gs::SEG_WAVE_MAX * (8 + vbs)), a, 0);
        forms |= GS_SEGTOPK_F_WAVE;
    }
    for (uint32_t c = 3; c <= 7 && c <= top; ++c) {
        const uint32_t min_len = gs::SEG_CLASS_MAX[c - 1] + 1;
        if (n < min_len || gs::SEG_CLASS_MAX[c] > gs::seg_max_lds(vb)) continue;
        const Shape sh = g_small_class[c - 3];
        const TksLauncher tile = routes.tile[TksTileTable::index({(int)c - 3, (int)rank, (int)vi})];
        if (!tile) return GS_ERR_MODE;
        const uint32_t bound = seg_class_bound(n, num_segments, min_len);
        tile(s, routes.tile_loops(sh.threads, sh.kpt) ? seg_grid(bound, (uint32_t)sh.threads / 64, seg_wg_lds_bytes(sh, vbs)) : bound, a, c);
        forms |= GS_SEGTOPK_F_TILE(c, rank);
    }
    if (allow_long && n > gs::seg_max_lds(vb)) {
        const uint32_t longs = seg_class_bound(n, num_segments, gs::seg_max_lds(vb) + 1);
        f.stream(s, routes.stream_loops ? seg_grid(longs, gs::TKR_THREADS / 64, 97u * 1024u) : longs, a, 0);  // (the histogram, the staging, the staged sort's tables: 96.6 KiB)
        forms |= GS_SEGTOPK_F_STREAM;
    }
    GS_HIP(hipGetLastError());
    h->last_forms = forms;
    return GS_OK;
}
}  // namespace

extern "C" {

size_t gs_segtopk_temp_bytes(uint32_t max_segments) { return segtopk_bytes(max_segments); }

gs_status gs_segtopk_create(gs_segtopk** out, uint32_t max_keys, uint32_t max_segments, uint32_t max_k, gs_mode mode, uint32_t value_bytes) {
    const bool sizes_ok = max_keys != 0 && max_keys <= GS_MAX_KEYS && max_segments != 0 && max_segments <= GS_MAX_KEYS && max_k != 0 && max_k <= GS_MAX_KEYS;
    return handle_create(out, sizes_ok, mode, value_bytes, [&](gs_segtopk* h) {
        h->max_keys = max_keys;
        h->max_segments = max_segments;
        h->max_k = max_k;
        return h->ws.alloc(segtopk_bytes(max_segments), 0, gs::SEGC_WORDS, gs::SEGC_WORDS);
    });
}

gs_status gs_segtopk_destroy(gs_segtopk* h) { return handle_destroy(h); }

gs_status gs_segtopk_select_keys(gs_segtopk* h, const void* d_keys, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments, uint32_t k,
                                 uint32_t max_segment_len, void* d_out_keys, gs_key_type key_type, gs_order order, void* stream) {
    return segtopk_impl(g_tks_routes32, h, d_keys, nullptr, n, d_offsets, num_segments, k, max_segment_len, d_out_keys, nullptr, key_type, order,
                        static_cast<hipStream_t>(stream), false);
}

gs_status gs_segtopk_select_pairs(gs_segtopk* h, const void* d_keys, const void* d_vals, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments,
                                  uint32_t k, uint32_t max_segment_len, void* d_out_keys, void* d_out_vals, gs_key_type key_type, gs_order order,
                                  void* stream) {
    return segtopk_impl(g_tks_routes32, h, d_keys, d_vals, n, d_offsets, num_segments, k, max_segment_len, d_out_keys, d_out_vals, key_type, order,
                        static_cast<hipStream_t>(stream), true);
}

gs_status gs_segtopk_check(gs_segtopk* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    const uint32_t st = h->ws.pinned[gs::SEGC_STATUS];
    if (st & gs::SEG_ST_ARG) return GS_ERR_ARG;
    if (h->ws.pinned[gs::TKSC_TKR + gs::TKC_STATUS] & gs::TK_ST_INTERNAL) return GS_ERR_HIP;
    if (st & gs::SEG_ST_SIZE) return GS_ERR_SIZE;
    return GS_OK;
}

gs_status gs_segtopk_last(gs_segtopk* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SEGTOPK_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SEGTOPK_REPORT_WORDS; ++i) report[i] = 0;
    for (uint32_t c = 0; c < GS_SEGSORT_CLASSES; ++c) report[GS_SEGTOPK_R_CLASSES + c] = h->ws.pinned[gs::SEGC_COUNT + c];
    report[GS_SEGTOPK_R_LONGEST] = h->ws.pinned[gs::SEGC_MAXLEN];
    report[GS_SEGTOPK_R_STATUS] = h->ws.pinned[gs::SEGC_STATUS] | ((h->ws.pinned[gs::TKSC_TKR + gs::TKC_STATUS] & gs::TK_ST_INTERNAL) ? 256u : 0u);
    report[GS_SEGTOPK_R_READS] = h->ws.pinned[gs::TKSC_TKR + gs::TKR_CTL_READS];
    report[GS_SEGTOPK_R_FORMS] = h->last_forms;
    report[GS_SEGTOPK_R_RANK] = (uint32_t)h->rank_mode;
    report[GS_SEGTOPK_R_K] = h->last_k;
    report[GS_SEGTOPK_R_PACKED] = h->ws.pinned[gs::TKSC_PACKED];
    return GS_OK;
}

gs_status gs_segtopk_set_rank_mode(gs_segtopk* h, int mode) { return handle_set_rank_mode(h, mode); }

int gs_segtopk_get_rank_mode(gs_segtopk* h) { return handle_get_rank_mode(h); }

}  // extern "C"
