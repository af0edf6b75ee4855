// sortrows16_host.hpp — part of the gpusort_capi.hip translation unit: the gs_sort_rows16 handle (sortrows16_kernels.hpp) and its
// entries: the layout, the plan, the launches of the two routes and the report.  Allocation, create/destroy, the control read-back, the
// rank mode, the buffer predicate and the ping-pong are handle_core.hpp's.  No counterpart in the reference project.
struct gs_sort_rows16 {
    uint32_t max_keys;
    gs_mode mode;
    uint32_t value_bytes;
    int rank_mode;               // the scatter's ranking and that of the LDS route's workgroup classes (probed at create)
    Workspace ws;                // one allocation: see sort_rows16_layout
    // the last call (gs_sort_rows16_last)
    uint32_t last_route = GS_SORT_ROWS_ROUTE_NONE, last_rows = 0, last_row_len = 0, last_forms = 0, last_parts = 0, last_per_part = 0;
};

namespace {
static_assert(GS_SORT_ROWS16_PASSES == gs::SR16_PASSES, "header and kernels agree on the plan");

// (row, part) tables of 256 words a handle of max_keys must hold: sort_rows_units for the same tile, cap and LDS limit
uint32_t sort_rows16_units(uint32_t max_keys, uint32_t vb) { return sort_rows_units(max_keys, vb); }

struct SortRows16Layout {
    size_t ctl, table, bases, total;
};
// ctl: the handle's control block; table, bases: sort_rows16_units x 256 words each
SortRows16Layout sort_rows16_layout(uint32_t max_keys, uint32_t vb) {
    SortRows16Layout l{};
    Arena a;
    const size_t units = sort_rows16_units(max_keys, vb);
    l.ctl = a.take(gs::SRC_WORDS * 4u);
    l.table = a.take(units * gs::RADIX * 4u);
    l.bases = a.take(units * gs::RADIX * 4u);
    l.total = a.total();
    return l;
}

// plan[GS_SORT_ROWS_P_*]: the route's border and the cut of sort_rows_plan (same tile, same aim, same least tiles per part), two passes
void sort_rows16_plan(uint32_t rows, uint32_t row_len, uint32_t vb, uint32_t plan[GS_SORT_ROWS_PLAN_WORDS]) {
    sort_rows_plan(rows, row_len, vb, plan);
    if (plan[GS_SORT_ROWS_P_ROUTE] == GS_SORT_ROWS_ROUTE_PASSES) plan[GS_SORT_ROWS_P_PASSES] = gs::SR16_PASSES;
}

#if GS_SORT_ROWS_BUILT
using Sr16Scatter = void (*)(hipStream_t, uint32_t grid, const uint16_t*, const void*, uint16_t*, void*, uint32_t row_len, uint32_t parts, uint32_t per,
                             uint32_t kt, uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl);
template <int VM, int RANK>
void launch_sr16_scatter(hipStream_t s, uint32_t grid, const uint16_t* kin, const void* vin, uint16_t* kout, void* vout, uint32_t row_len, uint32_t parts,
                         uint32_t per, uint32_t kt, uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl) {
    hipLaunchKernelGGL((gs::sr16_scatter_kernel<VM, RANK>), dim3(grid), dim3(gs::SR_THREADS), 0, s, kin, vin, kout, vout, row_len, parts, per, kt, shift,
                       reverse, bases, ctl);
}
// vm: 0 keys only, 1 positions, 4, 8; the form's bit in the report: GS_SORT_ROWS16_F_SCATTER << (2 x vm index + rank)
inline Sr16Scatter sr16_scatter(uint32_t vm, int rank, uint32_t* form) {
    *form = GS_SORT_ROWS16_F_SCATTER << (2u * (uint32_t)vm_index(vm) + (rank ? 1u : 0u));
    if (rank) return vm == 0u ? launch_sr16_scatter<0, 1> : vm == 1u ? launch_sr16_scatter<1, 1> : vm == 4u ? launch_sr16_scatter<4, 1> : launch_sr16_scatter<8, 1>;
    return vm == 0u ? launch_sr16_scatter<0, 0> : vm == 1u ? launch_sr16_scatter<1, 0> : vm == 4u ? launch_sr16_scatter<4, 0> : launch_sr16_scatter<8, 0>;
}

// short rows: the row-wise top-k's 2-byte LDS sorts with k = row_len, row_stride = row_len and the output = the input.  Both kernels
// hold the whole row in registers before their first store and a row belongs to one wave or one workgroup.
gs_status sort_rows16_run_lds(gs_sort_rows16* h, uint32_t* ctl, void* keys, void* vals, uint32_t rows, uint32_t row_len, uint32_t kt, bool descending,
                              uint32_t vm, hipStream_t s) {
    const gs::TkrArgs a{static_cast<const uint32_t*>(keys), vals, static_cast<uint32_t*>(keys), vals, rows, row_len, row_len, row_len,
                        kt, descending ? 1u : 0u, ctl};
    if (row_len <= gs::SEG_WAVE_MAX) {
        tkr_vm(true, vm).wave(s, div_up(rows, gs::TKR_WAVE_ROWS), a);
        h->last_forms |= GS_SORT_ROWS16_F_LDS_WAVE;
    } else {
        const TkrLauncher f = tkr_tile_launcher(true, (int)gs::seg_class_of(row_len, h->value_bytes) - 3, h->rank_mode, vm);
        if (!f) return GS_ERR_MODE;
        f(s, rows, a);
        h->last_forms |= GS_SORT_ROWS16_F_LDS_TILE;
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// two passes: the low byte from the caller's buffers into the alternate ones, the high byte back.  positions: the first pass makes the value
gs_status sort_rows16_run_passes(gs_sort_rows16* h, const SortRows16Layout& l, uint16_t* keys, void* vals, uint16_t* alt_keys, void* alt_vals, uint32_t rows,
                                 uint32_t row_len, uint32_t kt, bool descending, bool positions, hipStream_t s) {
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    uint32_t* table = reinterpret_cast<uint32_t*>(h->ws.dev + l.table);
    uint32_t* bases = reinterpret_cast<uint32_t*>(h->ws.dev + l.bases);
    const uint32_t parts = h->last_parts, per = h->last_per_part, grid = rows * parts;
    uint32_t forms = GS_SORT_ROWS16_F_COUNT | GS_SORT_ROWS16_F_SCAN;
    for (uint32_t pass = 0; pass < gs::SR16_PASSES; ++pass) {
        const bool fwd = pass == 0u;
        const PingPong<uint16_t> b = ping_pong(pass, keys, vals, alt_keys, alt_vals);
        uint32_t form = 0;
        const Sr16Scatter scatter = sr16_scatter((positions && fwd) ? 1u : h->value_bytes, h->rank_mode, &form);
        hipLaunchKernelGGL(gs::sr16_count_kernel, dim3(grid), dim3(gs::SR_THREADS), 0, s, b.kin, row_len, parts, per, kt, pass * 8u, table);
        hipLaunchKernelGGL(gs::sr_scan_kernel, dim3(rows), dim3(gs::RADIX), 0, s, table, bases, parts, row_len, ctl);
        scatter(s, grid, b.kin, b.vin, b.kout, b.vout, row_len, parts, per, kt, pass * 8u, (descending && !fwd) ? 1u : 0u, bases, ctl);
        forms |= form;
    }
    GS_HIP(hipGetLastError());
    h->last_forms |= forms;
    return GS_OK;
}
#endif

// what: 0 keys, 1 pairs, 2 argsort.  The order of the checks is sort_rows_impl's.
gs_status sort_rows16_impl(gs_sort_rows16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t rows, uint32_t row_len, gs_key_type kt,
                           gs_order order, hipStream_t s, int what) {
    if (!h || !d_keys || misaligned(d_keys) || !is_key16(kt) || !valid_order(order)) return GS_ERR_ARG;  // (32- and 64-bit key types: gs_sort_rows_*, out of scope)
    const bool pairs = what != 0;
    if (pairs != (h->mode == GS_MODE_PAIRS) || (what == 2 && h->value_bytes != 4u)) return GS_ERR_MODE;
    if (pairs && (!d_vals || misaligned(d_vals))) return GS_ERR_ARG;
    if (rows == 0 || row_len == 0 || (uint64_t)rows * row_len > h->max_keys) return GS_ERR_SIZE;
    const uint32_t n = rows * row_len, vb = h->value_bytes;
    uint32_t plan[GS_SORT_ROWS_PLAN_WORDS];
    sort_rows16_plan(rows, row_len, vb, plan);
    const bool passes = plan[GS_SORT_ROWS_P_ROUTE] == GS_SORT_ROWS_ROUTE_PASSES;
    if (passes && !alt_buffers_ok(d_keys, d_alt_keys, d_vals, d_alt_vals, n, 2u, vb, pairs)) return GS_ERR_ARG;
    if (!SR_BUILT) return GS_ERR_MODE;  // this build flavour has no row-wise sort
#if GS_SORT_ROWS_BUILT
    const SortRows16Layout l = sort_rows16_layout(h->max_keys, vb);
    if (passes && rows * plan[GS_SORT_ROWS_P_PARTS] > sort_rows16_units(h->max_keys, vb)) return GS_ERR_SIZE;  // (cannot happen: the tables are sized for it)
    h->last_route = GS_SORT_ROWS_ROUTE_NONE;
    h->last_rows = rows;
    h->last_row_len = row_len;
    h->last_parts = plan[GS_SORT_ROWS_P_PARTS];
    h->last_per_part = plan[GS_SORT_ROWS_P_PER_PART];
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    hipLaunchKernelGGL(gs::s16_clear_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<uint4*>(ctl), gs::SRC_WORDS / 4u);
    h->last_forms = GS_SORT_ROWS16_F_CLEAR;
    const bool desc = order == GS_ORDER_DESCENDING;
    const gs_status st = passes ? sort_rows16_run_passes(h, l, static_cast<uint16_t*>(d_keys), d_vals, static_cast<uint16_t*>(d_alt_keys), d_alt_vals, rows,
                                                         row_len, (uint32_t)kt, desc, what == 2, s)
                                : sort_rows16_run_lds(h, ctl, d_keys, d_vals, rows, row_len, (uint32_t)kt, desc, what == 0 ? 0u : what == 2 ? 1u : vb, s);
    if (st == GS_OK) h->last_route = plan[GS_SORT_ROWS_P_ROUTE];
    return st;
#else
    (void)s; (void)d_alt_keys; (void)d_alt_vals; (void)d_vals; (void)n;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_sort_rows16_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (max_keys == 0 || max_keys > GS_MAX_KEYS || !mode_value_ok(mode, value_bytes)) return 0;
    return sort_rows16_layout(max_keys, value_bytes).total;
}

gs_status gs_sort_rows16_plan(uint32_t rows, uint32_t row_len, gs_mode mode, uint32_t value_bytes, uint32_t* plan) {
    if (!plan) return GS_ERR_ARG;
    if (!mode_value_ok(mode, value_bytes)) return GS_ERR_MODE;
    if (rows == 0 || row_len == 0 || (uint64_t)rows * row_len > GS_MAX_KEYS) return GS_ERR_SIZE;
    sort_rows16_plan(rows, row_len, value_bytes, plan);
    return GS_OK;
}

gs_status gs_sort_rows16_create(gs_sort_rows16** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    return handle_create(out, max_keys != 0 && max_keys <= GS_MAX_KEYS, mode, value_bytes, [&](gs_sort_rows16* h) {
        h->max_keys = max_keys;
        const SortRows16Layout l = sort_rows16_layout(max_keys, value_bytes);
        return h->ws.alloc(l.total, l.ctl, gs::SRC_WORDS, gs::SRC_WORDS);
    });
}

gs_status gs_sort_rows16_destroy(gs_sort_rows16* h) { return handle_destroy(h); }

gs_status gs_sort_rows16_keys(gs_sort_rows16* h, void* d_keys, void* d_alt, uint32_t rows, uint32_t row_len, gs_key_type key_type, gs_order order,
                              void* stream) {
    return sort_rows16_impl(h, d_keys, nullptr, d_alt, nullptr, rows, row_len, key_type, order, static_cast<hipStream_t>(stream), 0);
}

gs_status gs_sort_rows16_pairs(gs_sort_rows16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t rows, uint32_t row_len,
                               gs_key_type key_type, gs_order order, void* stream) {
    return sort_rows16_impl(h, d_keys, d_vals, d_alt_keys, d_alt_vals, rows, row_len, key_type, order, static_cast<hipStream_t>(stream), 1);
}

gs_status gs_sort_rows16_argsort(gs_sort_rows16* h, void* d_keys, void* d_pos, void* d_alt_keys, void* d_alt_pos, uint32_t rows, uint32_t row_len,
                                 gs_key_type key_type, gs_order order, void* stream) {
    return sort_rows16_impl(h, d_keys, d_pos, d_alt_keys, d_alt_pos, rows, row_len, key_type, order, static_cast<hipStream_t>(stream), 2);
}

gs_status gs_sort_rows16_check(gs_sort_rows16* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    return h->ws.pinned[gs::SRC_STATUS] != 0u ? GS_ERR_HIP : GS_OK;
}

gs_status gs_sort_rows16_last(gs_sort_rows16* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SORT_ROWS_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SORT_ROWS_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_SORT_ROWS_R_ROUTE] = h->last_route;
    report[GS_SORT_ROWS_R_ROWS] = h->last_rows;
    report[GS_SORT_ROWS_R_ROW_LEN] = h->last_row_len;
    report[GS_SORT_ROWS_R_PARTS] = h->last_parts;
    report[GS_SORT_ROWS_R_FORMS] = h->last_forms;
    report[GS_SORT_ROWS_R_STATUS] = h->ws.pinned[gs::SRC_STATUS];
    report[GS_SORT_ROWS_R_RANK] = (uint32_t)h->rank_mode;
    report[GS_SORT_ROWS_R_PER_PART] = h->last_per_part;
    return GS_OK;
}

gs_status gs_sort_rows16_set_rank_mode(gs_sort_rows16* h, int mode) { return handle_set_rank_mode(h, mode); }

int gs_sort_rows16_get_rank_mode(gs_sort_rows16* h) { return handle_get_rank_mode(h); }

}  // extern "C"
