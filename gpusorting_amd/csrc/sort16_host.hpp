// sort16_host.hpp — part of the gpusort_capi.hip translation unit: the gs_sort16 handle (sort16_kernels.hpp) and its entries: the
// layout, the plan, the launches of the two routes and the report.  Allocation, create/destroy, the control read-back, the rank mode
// and the buffer predicates are handle_core.hpp's.  No counterpart in the reference project.
struct gs_sort16 {
    uint32_t max_keys;
    gs_mode mode;
    uint32_t value_bytes;
    int rank_mode;               // the scatter's ranking: 0 ballot multi-split, 1 returning LDS atomic (probed at create)
    Workspace ws;                // one allocation: see sort16_layout; the control block lies at its start
    // the last call (gs_sort16_last)
    uint32_t last_route = GS_SORT16_ROUTE_NONE, last_n = 0, last_forms = 0, last_plan[4] = {0u, 0u, 0u, 0u};
};

namespace {
constexpr bool S16_BUILT = GS_SORT16_BUILT != 0;  // the product build only, as the segmented sort and the selection

struct Sort16Layout {
    size_t ctl, hist, prefix, table, bases, total;
};
// keys only: the 65 536-bin histogram and its prefix; pairs: the per-range digit table and its bases.  Independent of max_keys.
Sort16Layout sort16_layout(bool pairs) {
    Sort16Layout l{};
    Arena a;
    l.ctl = a.take(gs::S16C_WORDS * 4u);
    l.hist = a.take(pairs ? 0u : gs::S16_BINS * 4u);
    l.prefix = a.take(pairs ? 0u : (gs::S16_BINS + 1u) * 4u);
    l.table = a.take(pairs ? (size_t)gs::S16_PCAP * gs::RADIX * 4u : 0u);
    l.bases = a.take(pairs ? (size_t)gs::S16_PCAP * gs::RADIX * 4u : 0u);
    l.total = a.total();
    return l;
}

// plan[0] ranges, [1] elements per range (a multiple of the tile), [2] tile, [3] range cap.  The smallest range is one tile.
void sort16_plan(uint32_t n, bool pairs, uint32_t plan[4]) {
    const uint32_t tile = pairs ? gs::S16_PTILE : gs::S16_KTILE, cap = pairs ? gs::S16_PCAP : gs::S16_KCAP;
    const uint32_t per = div_up(div_up(n, cap), tile) * tile;
    plan[0] = div_up(n, per);
    plan[1] = per;
    plan[2] = tile;
    plan[3] = cap;
}

#if GS_SORT16_BUILT
using S16Scatter = void (*)(hipStream_t, uint32_t grid, const uint16_t*, const void*, uint16_t*, void*, uint32_t n, uint32_t per, uint32_t kt, uint32_t shift,
                            uint32_t reverse, const uint32_t* bases, uint32_t* ctl);
template <int VM, int RANK>
void launch_s16_scatter(hipStream_t s, uint32_t grid, const uint16_t* kin, const void* vin, uint16_t* kout, void* vout, uint32_t n, uint32_t per, uint32_t kt,
                        uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl) {
    hipLaunchKernelGGL((gs::s16_scatter_kernel<VM, RANK>), dim3(grid), dim3(gs::S16_PTHREADS), 0, s, kin, vin, kout, vout, n, per, kt, shift, reverse, bases, ctl);
}
// vm: 1 positions, 4, 8; the form's bit in the report: GS_SORT16_F_SCATTER << (2 x (0 / 1 / 2) + rank)
inline S16Scatter s16_scatter(uint32_t vm, int rank, uint32_t* form) {
    const uint32_t vi = vm == 1u ? 0u : vm == 4u ? 1u : 2u;
    *form = GS_SORT16_F_SCATTER << (2u * vi + (rank ? 1u : 0u));
    if (rank) return vm == 1u ? launch_s16_scatter<1, 1> : vm == 4u ? launch_s16_scatter<4, 1> : launch_s16_scatter<8, 1>;
    return vm == 1u ? launch_s16_scatter<1, 0> : vm == 4u ? launch_s16_scatter<4, 0> : launch_s16_scatter<8, 0>;
}

gs_status sort16_run_keys(gs_sort16* h, uint16_t* keys, uint32_t n, uint32_t kt, uint32_t flip, hipStream_t s) {
    const Sort16Layout l = sort16_layout(false);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    uint32_t* hist = reinterpret_cast<uint32_t*>(h->ws.dev + l.hist);
    uint32_t* prefix = reinterpret_cast<uint32_t*>(h->ws.dev + l.prefix);
    const uint32_t* plan = h->last_plan;
    // the clear: status word and histogram lie side by side (ctl, hist)
    const uint32_t groups = (uint32_t)((l.prefix - l.ctl) / 16u);
    hipLaunchKernelGGL(gs::s16_clear_kernel, dim3(div_up(groups, 256u)), dim3(256), 0, s, reinterpret_cast<uint4*>(h->ws.dev + l.ctl), groups);
    hipLaunchKernelGGL(gs::s16_hist_kernel, dim3(2u * plan[0]), dim3(gs::S16_KTHREADS), 0, s, keys, n, plan[1], kt, flip, hist);
    hipLaunchKernelGGL(gs::s16_scan_kernel, dim3(1), dim3(gs::S16_KTHREADS), 0, s, hist, prefix, n, ctl);
    hipLaunchKernelGGL(gs::s16_fill_kernel, dim3(div_up(n, gs::S16_KTILE)), dim3(gs::S16_KTHREADS), 0, s, keys, prefix, n, kt, flip, ctl);
    GS_HIP(hipGetLastError());
    h->last_forms = GS_SORT16_F_HIST | GS_SORT16_F_SCAN | GS_SORT16_F_FILL;
    return GS_OK;
}

// two passes: low byte from the caller's buffers into the alternate ones, high byte back.  positions: the first pass makes the value
gs_status sort16_run_pairs(gs_sort16* h, uint16_t* keys, void* vals, uint16_t* alt_keys, void* alt_vals, uint32_t n, uint32_t kt, bool descending,
                           bool positions, hipStream_t s) {
    const Sort16Layout l = sort16_layout(true);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    uint32_t* table = reinterpret_cast<uint32_t*>(h->ws.dev + l.table);
    uint32_t* bases = reinterpret_cast<uint32_t*>(h->ws.dev + l.bases);
    const uint32_t ranges = h->last_plan[0], per = h->last_plan[1];
    hipLaunchKernelGGL(gs::s16_clear_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<uint4*>(h->ws.dev + l.ctl), gs::S16C_WORDS / 4u);
    uint32_t forms = GS_SORT16_F_COUNT | GS_SORT16_F_PSCAN;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        const PingPong<uint16_t> b = ping_pong(pass, keys, vals, alt_keys, alt_vals);
        const uint32_t vm = (positions && pass == 0) ? 1u : h->value_bytes;
        uint32_t form = 0;
        const S16Scatter scatter = s16_scatter(vm, h->rank_mode, &form);
        hipLaunchKernelGGL(gs::s16_count_kernel, dim3(ranges), dim3(gs::S16_PTHREADS), 0, s, b.kin, n, per, kt, pass * 8u, table);
        hipLaunchKernelGGL(gs::s16_pscan_kernel, dim3(1), dim3(gs::RADIX), 0, s, table, bases, ranges, n, ctl);
        scatter(s, ranges, b.kin, b.vin, b.kout, b.vout, n, per, kt, pass * 8u, (descending && pass == 1) ? 1u : 0u, bases, ctl);
        forms |= form;
    }
    GS_HIP(hipGetLastError());
    h->last_forms = forms;
    return GS_OK;
}
#endif

// what: 0 keys, 1 pairs, 2 argsort
gs_status sort16_impl(gs_sort16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n, gs_key_type kt, gs_order order,
                      hipStream_t s, int what) {
    if (!h || !d_keys || misaligned(d_keys) || !is_key16(kt) || !valid_order(order)) return GS_ERR_ARG;
    const bool pairs = what != 0;
    if (pairs != (h->mode == GS_MODE_PAIRS) || (what == 2 && h->value_bytes != 4u)) return GS_ERR_MODE;
    if (pairs && (!d_vals || misaligned(d_vals) || !alt_buffers_present(d_alt_keys, d_alt_vals, true))) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys) return GS_ERR_SIZE;
    if (pairs && !alt_buffers_disjoint(d_keys, d_alt_keys, d_vals, d_alt_vals, n, 2u, h->value_bytes, true)) return GS_ERR_ARG;
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no 16-bit sort
#if GS_SORT16_BUILT
    h->last_route = GS_SORT16_ROUTE_NONE;
    h->last_forms = 0;
    h->last_n = n;
    sort16_plan(n, pairs, h->last_plan);
    const bool desc = order == GS_ORDER_DESCENDING;
    const gs_status st = pairs ? sort16_run_pairs(h, static_cast<uint16_t*>(d_keys), d_vals, static_cast<uint16_t*>(d_alt_keys), d_alt_vals, n, (uint32_t)kt,
                                                  desc, what == 2, s)
                               : sort16_run_keys(h, static_cast<uint16_t*>(d_keys), n, (uint32_t)kt, desc ? 0xffffu : 0u, s);
    if (st == GS_OK) h->last_route = pairs ? GS_SORT16_ROUTE_PAIRS : GS_SORT16_ROUTE_KEYS;
    return st;
#else
    (void)s; (void)d_alt_keys; (void)d_alt_vals; (void)d_vals;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_sort16_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (max_keys == 0 || max_keys > GS_MAX_KEYS || !mode_value_ok(mode, value_bytes)) return 0;
    return sort16_layout(mode == GS_MODE_PAIRS).total;
}

gs_status gs_sort16_plan(uint32_t n, gs_mode mode, uint32_t value_bytes, uint32_t plan[4]) {
    if (!plan) return GS_ERR_ARG;
    if (!mode_value_ok(mode, value_bytes)) return GS_ERR_MODE;
    if (n == 0 || n > GS_MAX_KEYS) return GS_ERR_SIZE;
    sort16_plan(n, mode == GS_MODE_PAIRS, plan);
    return GS_OK;
}

gs_status gs_sort16_create(gs_sort16** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    return handle_create(out, max_keys != 0 && max_keys <= GS_MAX_KEYS, mode, value_bytes, [&](gs_sort16* h) {
        h->max_keys = max_keys;
        const Sort16Layout l = sort16_layout(mode == GS_MODE_PAIRS);
        return h->ws.alloc(l.total, l.ctl, gs::S16C_WORDS, gs::S16C_WORDS);
    });
}

gs_status gs_sort16_destroy(gs_sort16* h) { return handle_destroy(h); }

gs_status gs_sort16_sort_keys(gs_sort16* h, void* d_keys, uint32_t n, gs_key_type key_type, gs_order order, void* stream) {
    return sort16_impl(h, d_keys, nullptr, nullptr, nullptr, n, key_type, order, static_cast<hipStream_t>(stream), 0);
}

gs_status gs_sort16_sort_pairs(gs_sort16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n, gs_key_type key_type,
                               gs_order order, void* stream) {
    return sort16_impl(h, d_keys, d_vals, d_alt_keys, d_alt_vals, n, key_type, order, static_cast<hipStream_t>(stream), 1);
}

gs_status gs_sort16_argsort(gs_sort16* h, void* d_keys, void* d_pos, void* d_alt_keys, void* d_alt_pos, uint32_t n, gs_key_type key_type,
                            gs_order order, void* stream) {
    return sort16_impl(h, d_keys, d_pos, d_alt_keys, d_alt_pos, n, key_type, order, static_cast<hipStream_t>(stream), 2);
}

gs_status gs_sort16_check(gs_sort16* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    return h->ws.pinned[gs::S16C_STATUS] != 0u ? GS_ERR_HIP : GS_OK;
}

gs_status gs_sort16_last(gs_sort16* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SORT16_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SORT16_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_SORT16_R_ROUTE] = h->last_route;
    report[GS_SORT16_R_RANGES] = h->last_plan[0];
    report[GS_SORT16_R_PER_RANGE] = h->last_plan[1];
    report[GS_SORT16_R_TILE] = h->last_plan[2];
    report[GS_SORT16_R_FORMS] = h->last_forms;
    report[GS_SORT16_R_STATUS] = h->ws.pinned[gs::S16C_STATUS];
    report[GS_SORT16_R_N] = h->last_n;
    report[GS_SORT16_R_RANK] = (uint32_t)h->rank_mode;
    return GS_OK;
}

gs_status gs_sort16_set_rank_mode(gs_sort16* h, int mode) { return handle_set_rank_mode(h, mode); }

int gs_sort16_get_rank_mode(gs_sort16* h) { return handle_get_rank_mode(h); }

}  // extern "C"
