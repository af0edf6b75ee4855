// sortrows_host.hpp — part of the gpusort_capi.hip translation unit: the gs_sort_rows handle (sortrows_kernels.hpp) and its entries:
// the layout, the plan, the launches of the two routes and the report.  Allocation, create/destroy, the control read-back, the rank
// mode, the buffer predicate and the ping-pong are handle_core.hpp's.  No counterpart in the reference project.
struct gs_sort_rows {
    uint32_t max_keys;
    gs_mode mode;
    uint32_t value_bytes;
    int rank_mode;               // the scatter's ranking and that of the LDS route's workgroup classes (probed at create)
    Workspace ws;                // one allocation: see sort_rows_layout; its control block is the two control blocks, read back as one
    // the last call (gs_sort_rows_last)
    uint32_t last_route = GS_SORT_ROWS_ROUTE_NONE, last_rows = 0, last_row_len = 0, last_forms = 0, last_parts = 0, last_per_part = 0;
};

namespace {
constexpr bool SR_BUILT = GS_SORT_ROWS_BUILT != 0;  // the product build only, as the segmented sort and the selection
static_assert(GS_SORT_ROWS_TILE == gs::SR_TILE && GS_SORT_ROWS_PCAP == gs::SR_PCAP && GS_SORT_ROWS_PASSES == gs::SR_PASSES && GS_SORT_ROWS_MIN_TILES == gs::SR_MIN_TILES, "header and kernels agree on the plan");

// (row, part) tables of 256 words a handle of max_keys must hold: rows x parts <= max(rows, SR_PCAP) and <= the tiles of the
// matrix < max_keys / tile + rows, with rows <= max_keys / (shortest pass-route row)
uint32_t sort_rows_units(uint32_t max_keys, uint32_t vb) {
    const uint32_t rows = max_keys / (gs::seg_max_lds(vb) + 1u);  // most rows of a pass-route call
    if (rows == 0) return 0;
    const uint32_t a = rows > gs::SR_PCAP ? rows : gs::SR_PCAP, b = max_keys / gs::SR_TILE + rows;
    return a < b ? a : b;
}

constexpr uint32_t SR_CTL_WORDS = gs::SRC_WORDS + gs::SEGC_WORDS;  // the two control blocks, cleared and read back as one
static_assert(gs::SRC_WORDS * 4u == 256u, "the segmented sort's control block starts where the layout's 256-byte granule ends");

struct SortRowsLayout {
    size_t ctl, seg, offsets, table, bases, total;
};
// ctl: the handle's control block; seg, right behind it: the segmented sort's control block + class lists (rows longer than the
// packed class); offsets: rows + 1 words; table, bases: sort_rows_units x 256 words each
SortRowsLayout sort_rows_layout(uint32_t max_keys, uint32_t vb) {
    SortRowsLayout l{};
    Arena a;
    const size_t units = sort_rows_units(max_keys, vb);
    l.ctl = a.take(gs::SRC_WORDS * 4u);
    l.seg = a.take(((size_t)gs::SEGC_WORDS + max_keys / (gs::SEG_PACK_MAX + 1u) + 1u) * 4u);
    l.offsets = a.take(((size_t)max_keys + 1u) * 4u);
    l.table = a.take(units * gs::RADIX * 4u);
    l.bases = a.take(units * gs::RADIX * 4u);
    l.total = a.total();
    return l;
}

// plan[GS_SORT_ROWS_P_*].  Pass route: parts = what brings rows x parts to SR_PCAP workgroups, at least 1, and no more than gives every
// part SR_MIN_TILES tiles (a part's fixed cost — its 256 bases read, its table row written — is shared by them)
void sort_rows_plan(uint32_t rows, uint32_t row_len, uint32_t vb, uint32_t plan[GS_SORT_ROWS_PLAN_WORDS]) {
    for (uint32_t i = 0; i < GS_SORT_ROWS_PLAN_WORDS; ++i) plan[i] = 0;
    plan[GS_SORT_ROWS_P_CAP] = rows > gs::SR_PCAP ? rows : gs::SR_PCAP;
    if (row_len <= gs::seg_max_lds(vb)) {
        plan[GS_SORT_ROWS_P_ROUTE] = GS_SORT_ROWS_ROUTE_LDS;
        plan[GS_SORT_ROWS_P_PARTS] = 1;
        plan[GS_SORT_ROWS_P_PER_PART] = row_len;
        return;
    }
    const uint32_t tiles = div_up(row_len, gs::SR_TILE);
    uint32_t want = gs::SR_PCAP / rows;
    if (want > tiles / gs::SR_MIN_TILES) want = tiles / gs::SR_MIN_TILES;
    if (want < 1u) want = 1u;
    const uint32_t per = div_up(tiles, want) * gs::SR_TILE;
    plan[GS_SORT_ROWS_P_ROUTE] = GS_SORT_ROWS_ROUTE_PASSES;
    plan[GS_SORT_ROWS_P_PARTS] = div_up(row_len, per);
    plan[GS_SORT_ROWS_P_PER_PART] = per;
    plan[GS_SORT_ROWS_P_TILE] = gs::SR_TILE;
    plan[GS_SORT_ROWS_P_PASSES] = gs::SR_PASSES;
}

#if GS_SORT_ROWS_BUILT
using SrScatter = void (*)(hipStream_t, uint32_t grid, const uint32_t*, const void*, uint32_t*, void*, uint32_t row_len, uint32_t parts, uint32_t per, uint32_t kt,
                           uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl);
template <int VB, int RANK>
void launch_sr_scatter(hipStream_t s, uint32_t grid, const uint32_t* kin, const void* vin, uint32_t* kout, void* vout, uint32_t row_len, uint32_t parts,
                       uint32_t per, uint32_t kt, uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl) {
    hipLaunchKernelGGL((gs::sr_scatter_kernel<VB, RANK>), dim3(grid), dim3(gs::SR_THREADS), 0, s, kin, vin, kout, vout, row_len, parts, per, kt, shift, reverse,
                       bases, ctl);
}
// the form's bit in the report: GS_SORT_ROWS_F_SCATTER << (2 x (0 / 1 / 2 for 0 / 4 / 8 value bytes) + rank)
inline SrScatter sr_scatter(uint32_t vb, int rank, uint32_t* form) {
    *form = GS_SORT_ROWS_F_SCATTER << (2u * (uint32_t)vb_index(vb) + (rank ? 1u : 0u));
    if (rank) return vb == 0u ? launch_sr_scatter<0, 1> : vb == 4u ? launch_sr_scatter<4, 1> : launch_sr_scatter<8, 1>;
    return vb == 0u ? launch_sr_scatter<0, 0> : vb == 4u ? launch_sr_scatter<4, 0> : launch_sr_scatter<8, 0>;
}

// short rows: the segmented sort's LDS classes on uniform offsets, max_segment_len = row_len (its asynchronous path)
gs_status sort_rows_run_lds(gs_sort_rows* h, const SortRowsLayout& l, uint32_t* keys, void* vals, uint32_t rows, uint32_t row_len, gs_key_type kt, uint32_t desc,
                            hipStream_t s) {
    uint32_t* offsets = reinterpret_cast<uint32_t*>(h->ws.dev + l.offsets);
    hipLaunchKernelGGL(gs::sr_offsets_kernel, dim3(div_up(rows + 1u, 256u)), dim3(256), 0, s, offsets, rows, row_len);
    h->last_forms |= GS_SORT_ROWS_F_OFFSETS | GS_SORT_ROWS_F_LDS;
    return seg_enqueue_lds(reinterpret_cast<uint32_t*>(h->ws.dev + l.seg), h->rank_mode, h->value_bytes, keys, vals, rows * row_len, offsets, rows, row_len,
                           gs::seg_class_of(row_len, h->value_bytes), kt, desc, s);
}

// four passes: bytes 0 and 2 from the caller's buffers into the alternate ones, bytes 1 and 3 back
gs_status sort_rows_run_passes(gs_sort_rows* h, const SortRowsLayout& l, uint32_t* keys, void* vals, uint32_t* alt_keys, void* alt_vals, uint32_t rows,
                               uint32_t row_len, uint32_t kt, bool descending, hipStream_t s) {
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    uint32_t* table = reinterpret_cast<uint32_t*>(h->ws.dev + l.table);
    uint32_t* bases = reinterpret_cast<uint32_t*>(h->ws.dev + l.bases);
    const uint32_t parts = h->last_parts, per = h->last_per_part, grid = rows * parts;
    uint32_t form = 0;
    const SrScatter scatter = sr_scatter(h->value_bytes, h->rank_mode, &form);
    for (uint32_t pass = 0; pass < gs::SR_PASSES; ++pass) {
        const PingPong<uint32_t> b = ping_pong(pass, keys, vals, alt_keys, alt_vals);
        hipLaunchKernelGGL(gs::sr_count_kernel, dim3(grid), dim3(gs::SR_THREADS), 0, s, b.kin, row_len, parts, per, kt, pass * 8u, table);
        hipLaunchKernelGGL(gs::sr_scan_kernel, dim3(rows), dim3(gs::RADIX), 0, s, table, bases, parts, row_len, ctl);
        scatter(s, grid, b.kin, b.vin, b.kout, b.vout, row_len, parts, per, kt, pass * 8u, (descending && pass == gs::SR_PASSES - 1u) ? 1u : 0u, bases, ctl);
    }
    GS_HIP(hipGetLastError());
    h->last_forms |= GS_SORT_ROWS_F_COUNT | GS_SORT_ROWS_F_SCAN | form;
    return GS_OK;
}
#endif

gs_status sort_rows_impl(gs_sort_rows* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t rows, uint32_t row_len, gs_key_type kt,
                         gs_order order, hipStream_t s, bool pairs) {
    if (!h || !d_keys || misaligned(d_keys) || !is_key32_type(kt) || !valid_order(order)) return GS_ERR_ARG;  // (16-bit key types: gs_sort_rows16_*; 64-bit ones: out of scope)
    if (pairs != (h->mode == GS_MODE_PAIRS)) return GS_ERR_MODE;
    if (pairs && (!d_vals || misaligned(d_vals))) return GS_ERR_ARG;
    if (rows == 0 || row_len == 0 || (uint64_t)rows * row_len > h->max_keys) return GS_ERR_SIZE;
    const uint32_t n = rows * row_len, vb = h->value_bytes;
    uint32_t plan[GS_SORT_ROWS_PLAN_WORDS];
    sort_rows_plan(rows, row_len, vb, plan);
    const bool passes = plan[GS_SORT_ROWS_P_ROUTE] == GS_SORT_ROWS_ROUTE_PASSES;
    if (passes && !alt_buffers_ok(d_keys, d_alt_keys, d_vals, d_alt_vals, n, 4u, vb, pairs)) return GS_ERR_ARG;
    if (!SR_BUILT) return GS_ERR_MODE;  // this build flavour has no row-wise sort
#if GS_SORT_ROWS_BUILT
    const SortRowsLayout l = sort_rows_layout(h->max_keys, vb);
    if (passes && rows * plan[GS_SORT_ROWS_P_PARTS] > sort_rows_units(h->max_keys, vb)) return GS_ERR_SIZE;  // (cannot happen: the tables are sized for it)
    h->last_route = GS_SORT_ROWS_ROUTE_NONE;
    h->last_rows = rows;
    h->last_row_len = row_len;
    h->last_parts = plan[GS_SORT_ROWS_P_PARTS];
    h->last_per_part = plan[GS_SORT_ROWS_P_PER_PART];
    // the clear: both control blocks (they lie side by side), so that neither route reports an earlier call's status
    hipLaunchKernelGGL(gs::s16_clear_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<uint4*>(h->ws.dev + l.ctl), SR_CTL_WORDS / 4u);
    h->last_forms = GS_SORT_ROWS_F_CLEAR;
    const bool desc = order == GS_ORDER_DESCENDING;
    const gs_status st = passes ? sort_rows_run_passes(h, l, static_cast<uint32_t*>(d_keys), d_vals, static_cast<uint32_t*>(d_alt_keys), d_alt_vals, rows,
                                                       row_len, (uint32_t)kt, desc, s)
                                : sort_rows_run_lds(h, l, static_cast<uint32_t*>(d_keys), d_vals, rows, row_len, kt, desc ? 1u : 0u, s);
    if (st == GS_OK) h->last_route = plan[GS_SORT_ROWS_P_ROUTE];
    return st;
#else
    (void)s; (void)d_alt_keys; (void)d_alt_vals; (void)d_vals; (void)n;
    return GS_ERR_MODE;
#endif
}

// the status word of the report, from both control blocks in h->ws.pinned (the handle's own, then the segmented sort's): the pass
// route's bits, the LDS route's (gs::SEG_ST_*) shifted by 8
inline uint32_t sort_rows_status(const gs_sort_rows* h) { return h->ws.pinned[gs::SRC_STATUS] | (h->ws.pinned[gs::SRC_WORDS + gs::SEGC_STATUS] << 8); }
}  // namespace

extern "C" {

size_t gs_sort_rows_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (max_keys == 0 || max_keys > GS_MAX_KEYS || !mode_value_ok(mode, value_bytes)) return 0;
    return sort_rows_layout(max_keys, value_bytes).total;
}

gs_status gs_sort_rows_plan(uint32_t rows, uint32_t row_len, gs_mode mode, uint32_t value_bytes, uint32_t* plan) {
    if (!plan) return GS_ERR_ARG;
    if (!mode_value_ok(mode, value_bytes)) return GS_ERR_MODE;
    if (rows == 0 || row_len == 0 || (uint64_t)rows * row_len > GS_MAX_KEYS) return GS_ERR_SIZE;
    sort_rows_plan(rows, row_len, value_bytes, plan);
    return GS_OK;
}

gs_status gs_sort_rows_create(gs_sort_rows** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    return handle_create(out, max_keys != 0 && max_keys <= GS_MAX_KEYS, mode, value_bytes, [&](gs_sort_rows* h) {
        h->max_keys = max_keys;
        const SortRowsLayout l = sort_rows_layout(max_keys, value_bytes);
        return h->ws.alloc(l.total, l.ctl, SR_CTL_WORDS, SR_CTL_WORDS);
    });
}

gs_status gs_sort_rows_destroy(gs_sort_rows* h) { return handle_destroy(h); }

gs_status gs_sort_rows_keys(gs_sort_rows* h, void* d_keys, void* d_alt, uint32_t rows, uint32_t row_len, gs_key_type key_type, gs_order order, void* stream) {
    return sort_rows_impl(h, d_keys, nullptr, d_alt, nullptr, rows, row_len, key_type, order, static_cast<hipStream_t>(stream), false);
}

gs_status gs_sort_rows_pairs(gs_sort_rows* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t rows, uint32_t row_len,
                             gs_key_type key_type, gs_order order, void* stream) {
    return sort_rows_impl(h, d_keys, d_vals, d_alt_keys, d_alt_vals, rows, row_len, key_type, order, static_cast<hipStream_t>(stream), true);
}

gs_status gs_sort_rows_check(gs_sort_rows* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    return sort_rows_status(h) != 0u ? GS_ERR_HIP : GS_OK;
}

gs_status gs_sort_rows_last(gs_sort_rows* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SORT_ROWS_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SORT_ROWS_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_SORT_ROWS_R_ROUTE] = h->last_route;
    report[GS_SORT_ROWS_R_ROWS] = h->last_rows;
    report[GS_SORT_ROWS_R_ROW_LEN] = h->last_row_len;
    report[GS_SORT_ROWS_R_PARTS] = h->last_parts;
    report[GS_SORT_ROWS_R_FORMS] = h->last_forms;
    report[GS_SORT_ROWS_R_STATUS] = sort_rows_status(h);
    report[GS_SORT_ROWS_R_RANK] = (uint32_t)h->rank_mode;
    report[GS_SORT_ROWS_R_PER_PART] = h->last_per_part;
    return GS_OK;
}

gs_status gs_sort_rows_set_rank_mode(gs_sort_rows* h, int mode) { return handle_set_rank_mode(h, mode); }

int gs_sort_rows_get_rank_mode(gs_sort_rows* h) { return handle_get_rank_mode(h); }

}  // extern "C"
