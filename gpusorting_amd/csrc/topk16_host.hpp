// topk16_host.hpp — part of the gpusort_capi.hip translation unit: the gs_topk16 handle (topk16_kernels.hpp) and its entries: the
// layout, the three routes and the report.  Allocation, the create frame and the control read-back are handle_core.hpp's; the final
// sort of the SELECT route is an embedded gs_sort16 pairs handle (sort16_host.hpp).  No counterpart in the reference project.
struct gs_topk16 {
    uint32_t max_keys = 0, max_k = 0;
    gs_mode mode = GS_MODE_KEYS_ONLY;
    uint32_t value_bytes = 0;
    int rank_mode = 0;             // the TILE route's ranking on a keys-only handle; a pairs handle runs it with the sorter's
    gs_sort16* sorter = nullptr;   // pairs: the final sort of the k selected elements, capacity max_k
    Workspace ws;                  // one allocation: see topk16_layout; the control block lies at its start
    uint32_t count_hist = GS_TOPK16_HIST_AUTO;  // gs_topk16_set_count_histogram
    uint32_t last_route = GS_TOPK16_ROUTE_NONE, last_flip = 0, last_hist = 0, last_plan[4] = {0u, 0u, 0u, 0u};  // (last_plan: GS_TOPK16_HIST_GLOBAL)
    bool sort_failed = false;      // the sorter refused a call on the host side
    ~gs_topk16() {
        if (sorter) (void)gs_sort16_destroy(sorter);
    }
};

namespace {
struct Topk16Layout {
    size_t ctl, extra, sums, prefix, rc, slices, alt_keys, alt_vals, total;
};
// Nothing here grows with max_keys: the 65 536-bin histogram is the exact answer, so there is no candidate buffer.
Topk16Layout topk16_layout(uint32_t max_k, bool pairs, uint32_t vb) {
    Topk16Layout l{};
    Arena a;
    l.ctl = a.take(gs::TK16C_WORDS * 4u);
    l.extra = a.take(gs::TK_BINS * 4u);
    l.sums = a.take(gs::TK_BINS * 4u);
    l.prefix = a.take(pairs ? 0u : (gs::TK_BINS + 1u) * 4u);
    l.rc = a.take(pairs ? 2u * gs::TK_MAX_RANGES * 4u : 0u);
    l.slices = a.take((size_t)gs::TK_MAX_RANGES * gs::TK_SLICE_WORDS * 4u);
    l.alt_keys = a.take(pairs ? (size_t)max_k * 2u : 0u);
    l.alt_vals = a.take(pairs ? (size_t)max_k * vb : 0u);
    l.total = a.total();
    return l;
}
inline bool topk16_sizes_ok(uint32_t max_keys, uint32_t max_k) { return max_keys != 0 && max_keys <= GS_MAX_KEYS && max_k != 0 && max_k <= max_keys; }

#if GS_SORT16_BUILT
using Tk16Scatter = void (*)(hipStream_t, const uint16_t* src, const void* src_vals, uint32_t* ctl, uint32_t kt, uint32_t flip, const uint32_t* rc,
                             uint16_t* out, void* out_vals, uint32_t k);
template <int VM>
void launch_tk16_scatter(hipStream_t s, const uint16_t* src, const void* src_vals, uint32_t* ctl, uint32_t kt, uint32_t flip, const uint32_t* rc,
                         uint16_t* out, void* out_vals, uint32_t k) {
    hipLaunchKernelGGL((gs::tk16_scatter_kernel<VM>), dim3(gs::TK_MAX_RANGES), dim3(gs::TK_THREADS), 0, s, src, src_vals, ctl, kt, flip, rc, out,
                       out_vals, k);
}
inline Tk16Scatter tk16_scatter(uint32_t vm) { return vm == 1 ? launch_tk16_scatter<1> : vm == 4 ? launch_tk16_scatter<4> : launch_tk16_scatter<8>; }

// n <= gs_segsort_max_lds_segment: the row-wise 16-bit wave / tile kernel on the one row
gs_status topk16_run_tile(gs_topk16* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals, gs_key_type kt,
                          gs_order order, hipStream_t s, uint32_t vm) {
    uint32_t* ctl = h->ws.ctl();
    hipLaunchKernelGGL(gs::s16_clear_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<uint4*>(ctl), gs::TK16C_WORDS / 4u);
    const gs::TkrArgs a{static_cast<const uint32_t*>(d_keys), d_vals, static_cast<uint32_t*>(d_out_keys), d_out_vals, 1u, n, n, k,
                        (uint32_t)kt, order == GS_ORDER_DESCENDING ? 1u : 0u, ctl};
    if (n <= gs::SEG_WAVE_MAX) {
        tkr_vm(true, vm).wave(s, 1u, a);
    } else {
        const int rank = h->sorter ? h->sorter->rank_mode : h->rank_mode;
        const TkrLauncher f = tkr_tile_launcher(true, (int)gs::seg_class_of(n, h->value_bytes) - 3, rank, vm);
        if (!f) return GS_ERR_MODE;
        f(s, 1u, a);
    }
    GS_HIP(hipGetLastError());
    h->last_route = GS_TOPK16_ROUTE_TILE;
    return GS_OK;
}

// the launches COUNT and SELECT share: plan, per-range histograms, their sum, the threshold bin
void topk16_enqueue_histogram(const Topk16Layout& l, char* dev, const uint16_t* keys, uint32_t n, uint32_t k, uint32_t kt, uint32_t flip, hipStream_t s) {
    uint32_t* ctl = reinterpret_cast<uint32_t*>(dev + l.ctl);
    uint32_t* extra = reinterpret_cast<uint32_t*>(dev + l.extra);
    uint32_t* sums = reinterpret_cast<uint32_t*>(dev + l.sums);
    uint32_t* slices = reinterpret_cast<uint32_t*>(dev + l.slices);
    hipLaunchKernelGGL(gs::tk16_init_kernel, dim3(gs::TK_BINS / 4u / 256u), dim3(256), 0, s, ctl, extra, n, k);
    hipLaunchKernelGGL(gs::tk16_hist_kernel, dim3(gs::TK_MAX_RANGES), dim3(gs::TK_THREADS), 0, s, keys, ctl, kt, flip, slices, extra);
    hipLaunchKernelGGL(gs::tk_reduce_kernel, dim3(gs::TK_TABLE_WORDS / 256u), dim3(256), 0, s, slices, ctl, 0u, extra, sums);
    hipLaunchKernelGGL(gs::tk_threshold_kernel, dim3(1), dim3(1024), 0, s, sums, ctl, 0u);
}
#endif

gs_status topk16_impl(gs_topk16* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals, gs_key_type kt,
                      gs_order order, hipStream_t s, bool pairs) {
    if (!h) return GS_ERR_ARG;
    h->last_route = GS_TOPK16_ROUTE_NONE;  // a refused call leaves no route behind
    if (!d_keys || !d_out_keys || misaligned(d_keys) || misaligned(d_out_keys) || !is_key16(kt) || !valid_order(order)) return GS_ERR_ARG;
    if (pairs != (h->mode == GS_MODE_PAIRS)) return GS_ERR_MODE;
    const uint32_t vb = h->value_bytes;
    const bool pos = pairs && !d_vals;  // the value is the element's position
    if (pairs && (!d_out_vals || misaligned(d_out_vals) || (pos ? vb != 4u : misaligned(d_vals)))) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys || k == 0 || k > n || k > h->max_k) return GS_ERR_SIZE;
    if (buffers_overlap(d_keys, (size_t)n * 2u, d_out_keys, (size_t)k * 2u)) return GS_ERR_ARG;
    if (pairs) {  // neither output on an input, nor on the other output
        const void* p[4] = {d_out_keys, d_out_vals, d_keys, d_vals};
        const size_t b[4] = {(size_t)k * 2u, (size_t)k * vb, (size_t)n * 2u, (size_t)n * vb};
        if (any_overlap(p, b, 2) || buffers_overlap(d_out_vals, b[1], d_keys, b[2]) ||
            (!pos && (buffers_overlap(d_vals, b[3], d_out_vals, b[1]) || buffers_overlap(d_vals, b[3], d_out_keys, b[0]))))
            return GS_ERR_ARG;
    }
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no 16-bit selection
#if GS_SORT16_BUILT
    h->sort_failed = false;
    const uint32_t vm = !pairs ? 0u : pos ? 1u : vb;
    if (n <= gs::seg_max_lds(vb)) return topk16_run_tile(h, d_keys, d_vals, n, k, d_out_keys, d_out_vals, kt, order, s, vm);
    const Topk16Layout l = topk16_layout(h->max_k, pairs, vb);
    const uint16_t* keys = static_cast<const uint16_t*>(d_keys);
    uint16_t* out = static_cast<uint16_t*>(d_out_keys);
    uint32_t* ctl = h->ws.ctl();
    const uint32_t flip = order == GS_ORDER_DESCENDING ? 0xffffu : 0u, ktu = (uint32_t)kt;
    h->last_flip = flip;
    // COUNT below GS_TOPK16_COUNT_SLICES_MIN elements (measured): the slices cost a fixed 64 MiB of traffic, the 16-bit sort's
    // histogram kernel reads the keys twice and has no fixed cost; it adds into `sums` directly
    const bool global = !pairs && (h->count_hist == GS_TOPK16_HIST_GLOBAL || (h->count_hist == GS_TOPK16_HIST_AUTO && n < GS_TOPK16_COUNT_SLICES_MIN));
    h->last_hist = global ? GS_TOPK16_HIST_GLOBAL : GS_TOPK16_HIST_SLICES;
    if (global) {
        uint32_t* sums = reinterpret_cast<uint32_t*>(h->ws.dev + l.sums);
        sort16_plan(n, false, h->last_plan);
        hipLaunchKernelGGL(gs::tk16_init_kernel, dim3(gs::TK_BINS / 4u / 256u), dim3(256), 0, s, ctl, sums, n, k);  // (zeroes sums)
        hipLaunchKernelGGL(gs::s16_hist_kernel, dim3(2u * h->last_plan[0]), dim3(gs::S16_KTHREADS), 0, s, keys, n, h->last_plan[1], ktu, flip, sums);
        hipLaunchKernelGGL(gs::tk_threshold_kernel, dim3(1), dim3(1024), 0, s, sums, ctl, 0u);  // (the report's words)
    } else {
        topk16_enqueue_histogram(l, h->ws.dev, keys, n, k, ktu, flip, s);
    }
    if (!pairs) {  // COUNT: the first k of the sorted order from the prefix; the keys are not read again
        const uint32_t* sums = reinterpret_cast<const uint32_t*>(h->ws.dev + l.sums);
        uint32_t* prefix = reinterpret_cast<uint32_t*>(h->ws.dev + l.prefix);
        hipLaunchKernelGGL(gs::s16_scan_kernel, dim3(1), dim3(gs::S16_KTHREADS), 0, s, sums, prefix, n, ctl);
        hipLaunchKernelGGL(gs::tk16_fill_kernel, dim3(div_up(k, gs::S16_KTILE)), dim3(gs::S16_KTHREADS), 0, s, out, prefix, n, k, ktu, flip, ctl);
        GS_HIP(hipGetLastError());
        h->last_route = GS_TOPK16_ROUTE_COUNT;
        return GS_OK;
    }
    // SELECT: per-range counts from the slices, the ordered scatter, the sort of the k selected elements in place
    const uint32_t* slices = reinterpret_cast<const uint32_t*>(h->ws.dev + l.slices);
    uint32_t* rc = reinterpret_cast<uint32_t*>(h->ws.dev + l.rc);
    hipLaunchKernelGGL(gs::tk16_rangecount_kernel, dim3(gs::TK_MAX_RANGES), dim3(256), 0, s, keys, slices, ctl, ktu, flip, rc);
    tk16_scatter(vm)(s, keys, d_vals, ctl, ktu, flip, rc, out, d_out_vals, k);
    GS_HIP(hipGetLastError());
    h->last_route = GS_TOPK16_ROUTE_SELECT;
    const gs_status st = sort16_impl(h->sorter, out, d_out_vals, h->ws.dev + l.alt_keys, h->ws.dev + l.alt_vals, k, kt, order, s, 1);
    if (st != GS_OK) h->sort_failed = true;
    return st;
#else
    (void)s;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_topk16_temp_bytes(uint32_t max_keys, uint32_t max_k, gs_mode mode, uint32_t value_bytes) {
    if (!topk16_sizes_ok(max_keys, max_k) || !mode_value_ok(mode, value_bytes)) return 0;
    const bool pairs = mode == GS_MODE_PAIRS;
    return topk16_layout(max_k, pairs, value_bytes).total + (pairs ? gs_sort16_temp_bytes(max_k, mode, value_bytes) : 0u);
}

gs_status gs_topk16_create(gs_topk16** out, uint32_t max_keys, uint32_t max_k, gs_mode mode, uint32_t value_bytes) {
    return handle_create(out, topk16_sizes_ok(max_keys, max_k), mode, value_bytes, [&](gs_topk16* h) {
        h->max_keys = max_keys;
        h->max_k = max_k;
        const bool pairs = mode == GS_MODE_PAIRS;
        if (pairs) {
            const gs_status st = gs_sort16_create(&h->sorter, max_k, mode, value_bytes);
            if (st != GS_OK) return st;
        }
        const Topk16Layout l = topk16_layout(max_k, pairs, value_bytes);
        return h->ws.alloc(l.total, l.ctl, gs::TK16C_WORDS, gs::TK16C_WORDS);
    });
}

gs_status gs_topk16_destroy(gs_topk16* h) { return handle_destroy(h); }  // (the sorter with it: ~gs_topk16)

gs_status gs_topk16_select_keys(gs_topk16* h, const void* d_keys, uint32_t n, uint32_t k, void* d_out_keys, gs_key_type key_type, gs_order order,
                                void* stream) {
    return topk16_impl(h, d_keys, nullptr, n, k, d_out_keys, nullptr, key_type, order, static_cast<hipStream_t>(stream), false);
}

gs_status gs_topk16_select_pairs(gs_topk16* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals,
                                 gs_key_type key_type, gs_order order, void* stream) {
    return topk16_impl(h, d_keys, d_vals, n, k, d_out_keys, d_out_vals, key_type, order, static_cast<hipStream_t>(stream), true);
}

gs_status gs_topk16_check(gs_topk16* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    if (h->sort_failed || (h->ws.pinned[gs::TKC_STATUS] & gs::TK_ST_INTERNAL)) return GS_ERR_HIP;
    return h->last_route == GS_TOPK16_ROUTE_SELECT ? gs_sort16_check(h->sorter, stream) : GS_OK;  // the final sort
}

gs_status gs_topk16_last(gs_topk16* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_TOPK16_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_TOPK16_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_TOPK16_R_ROUTE] = h->last_route;
    report[GS_TOPK16_R_STATUS] = h->ws.pinned[gs::TKC_STATUS];
    if (h->last_route != GS_TOPK16_ROUTE_COUNT && h->last_route != GS_TOPK16_ROUTE_SELECT) return GS_OK;
    const uint32_t* L = h->ws.pinned + gs::TKC_LEVEL;
    report[GS_TOPK16_R_THRESHOLD] = L[gs::TKL_BIN] ^ h->last_flip;
    report[GS_TOPK16_R_IN_FRONT] = L[gs::TKL_FRONT];
    report[GS_TOPK16_R_EQUAL] = L[gs::TKL_EQUAL];
    report[GS_TOPK16_R_TAKEN] = L[gs::TKL_TAKE];
    const bool global = h->last_hist == GS_TOPK16_HIST_GLOBAL;
    report[GS_TOPK16_R_RANGES] = global ? h->last_plan[0] : L[gs::TKL_RANGES];
    report[GS_TOPK16_R_PER_RANGE] = global ? h->last_plan[1] : L[gs::TKL_PER];
    report[GS_TOPK16_R_HIST] = h->last_hist;
    return GS_OK;
}

gs_status gs_topk16_set_count_histogram(gs_topk16* h, uint32_t which) {
    if (!h || which > GS_TOPK16_HIST_GLOBAL) return GS_ERR_ARG;
    h->count_hist = which;
    return GS_OK;
}

}  // extern "C"
