// search_host.hpp — part of the gpusort_capi.hip translation unit: the gs_search handle (search_kernels.hpp) and its entries: the
// layout, the plan, the three routes and the report.  Allocation, the create frame and the control read-back are handle_core.hpp's; the
// sort of the queries in front of the tile kernel is an embedded gs_onesweep pairs engine with 4-byte values (the positions), as the
// POSITIONS route of gs_unique.  Only the stable pairs engine is ever used here: the keys-only sorter's caveat on skewed keys
// (gs_unique_create) does not arise.  No counterpart in the reference project.
struct gs_search {
    uint32_t max_keys = 0, max_queries = 0, key_bytes = 0;
    gs_mode mode = GS_MODE_KEYS_ONLY;  // (handle_core's frame: pairs with 4-byte values when the handle sorts queries)
    uint32_t value_bytes = 0;
    int rank_mode = 0;
    gs_onesweep* engine = nullptr;  // capacity max_queries; null without sort_queries
    Workspace ws;                   // one allocation: see search_layout; the control block lies at its start
    uint32_t forced_route = GS_SEARCH_ROUTE_AUTO, forced_table = GS_SEARCH_TABLE_AUTO;
    uint32_t last_route = GS_SEARCH_ROUTE_NONE, last_table = 0, last_n = 0, last_m = 0, last_plan[GS_SEARCH_PLAN_WORDS] = {};
    ~gs_search() {
        if (engine) (void)gs_onesweep_destroy(engine);
    }
};

namespace {
struct SearchLayout {
    size_t ctl, samples, keys, alt_keys, pos, alt_pos, total;
};
// the control block and the sample table; with sort_queries the engine's buffers: the copy of the queries, its alternate, positions twice
SearchLayout search_layout(uint32_t max_queries, uint32_t key_bytes, bool sort_queries) {
    SearchLayout l{};
    Arena a;
    l.ctl = a.take(gs::SSC_WORDS * 4u);
    l.samples = a.take(gs::SS_SAMPLE_BYTES);
    l.keys = a.take(sort_queries ? (size_t)max_queries * key_bytes : 0u);
    l.alt_keys = a.take(sort_queries ? (size_t)max_queries * key_bytes : 0u);
    l.pos = a.take(sort_queries ? (size_t)max_queries * 4u : 0u);
    l.alt_pos = a.take(sort_queries ? (size_t)max_queries * 4u : 0u);
    l.total = a.total();
    return l;
}
inline bool search_sizes_ok(uint32_t max_keys, uint32_t max_queries) {
    return max_keys != 0 && max_keys <= GS_MAX_KEYS && max_queries != 0 && max_queries <= GS_MAX_KEYS;
}

// gs_search_plan's words for n keys, m queries of key_bytes bytes (sizes checked by the caller)
void search_plan(uint32_t n, uint32_t m, uint32_t key_bytes, uint32_t plan[GS_SEARCH_PLAN_WORDS]) {
    const uint32_t cap = gs::SS_SAMPLE_BYTES / key_bytes;
    uint32_t S = 1;
    while (div_up(n, S) > cap) S <<= 1;  // the smallest power of two whose samples fit the table
    const uint32_t ns = n / S;
    const bool table = m >= GS_SEARCH_TABLE_MIN_QUERIES;
    for (uint32_t i = 0; i < GS_SEARCH_PLAN_WORDS; ++i) plan[i] = 0;
    plan[GS_SEARCH_P_TILE] = gs::SS_TILE;
    plan[GS_SEARCH_P_WINDOW] = gs::SS_WINDOW_BYTES / key_bytes;
    plan[GS_SEARCH_P_SAMPLES] = ns;
    plan[GS_SEARCH_P_STRIDE] = S;
    plan[GS_SEARCH_P_TILE_GRID] = div_up(m, gs::SS_TILE);
    plan[GS_SEARCH_P_TABLE] = table ? 1u : 0u;
    const uint32_t tg = div_up(m, gs::SS_THREADS);
    plan[GS_SEARCH_P_BINARY_GRID] = table ? (tg < gs::SS_TABLE_GRID ? tg : gs::SS_TABLE_GRID) : div_up(m, gs::SS_PLAIN_THREADS);
    plan[GS_SEARCH_P_SAMPLE_GRID] = div_up(ns, gs::SS_SAMPLE_THREADS);
    plan[GS_SEARCH_P_ROUTE_SORTED] = GS_SEARCH_ROUTE_TILE;
    // the rule of DESIGN.md 3.25 for queries in no order on a handle with the engine
    plan[GS_SEARCH_P_ROUTE_UNSORTED] = (m >= GS_SEARCH_SORT_MIN_QUERIES && n >= GS_SEARCH_SORT_MIN_KEYS) ? GS_SEARCH_ROUTE_SORT : GS_SEARCH_ROUTE_BINARY;
    plan[GS_SEARCH_P_ROUTE_NO_ENGINE] = GS_SEARCH_ROUTE_BINARY;
}

#if GS_SORT16_BUILT
template <class K>
gs_status search_enqueue(gs_search* h, const K* hay, uint32_t n, const K* q, uint32_t m, uint32_t* out, gs_key_type kt, gs_order order, uint32_t right,
                         uint32_t route, bool table, hipStream_t s) {
    const uint32_t* plan = h->last_plan;
    const uint32_t desc = order == GS_ORDER_DESCENDING ? 1u : 0u;
    uint32_t* ctl = h->ws.ctl();
    hipLaunchKernelGGL(gs::ss_reset_kernel, dim3(1), dim3(64), 0, s, ctl);
    if (route == GS_SEARCH_ROUTE_TILE) {
        hipLaunchKernelGGL((gs::ss_tile_kernel<K, false>), dim3(plan[GS_SEARCH_P_TILE_GRID]), dim3(gs::SS_THREADS), 0, s, hay, n, q,
                           static_cast<const uint32_t*>(nullptr), m, out, (uint32_t)kt, desc, right, ctl);
    } else if (route == GS_SEARCH_ROUTE_SORT) {
        const SearchLayout l = search_layout(h->max_queries, h->key_bytes, true);
        K* keys = reinterpret_cast<K*>(h->ws.dev + l.keys);
        uint32_t* pos = reinterpret_cast<uint32_t*>(h->ws.dev + l.pos);
        hipLaunchKernelGGL((gs::uq_prepare_kernel<K, true>), dim3(div_up(m, gs::UQ_PREP_TILE)), dim3(gs::UQ_PREP_THREADS), 0, s, q, m, keys, pos);
        GS_HIP(hipGetLastError());
        const gs_status st = gs_onesweep_sort_pairs(h->engine, keys, pos, h->ws.dev + l.alt_keys, h->ws.dev + l.alt_pos, m, kt, order, s);
        if (st != GS_OK) return st;
        hipLaunchKernelGGL((gs::ss_tile_kernel<K, true>), dim3(plan[GS_SEARCH_P_TILE_GRID]), dim3(gs::SS_THREADS), 0, s, hay, n, keys, pos, m, out,
                           (uint32_t)kt, desc, right, ctl);
    } else if (table) {
        K* samples = reinterpret_cast<K*>(h->ws.dev + search_layout(h->max_queries, h->key_bytes, h->engine != nullptr).samples);
        const uint32_t ns = plan[GS_SEARCH_P_SAMPLES], S = plan[GS_SEARCH_P_STRIDE];
        hipLaunchKernelGGL(gs::ss_sample_kernel<K>, dim3(plan[GS_SEARCH_P_SAMPLE_GRID]), dim3(gs::SS_SAMPLE_THREADS), 0, s, hay, n, S, ns, samples,
                           (uint32_t)kt, desc);
        const uint32_t tg = div_up(m, gs::SS_THREADS);
        hipLaunchKernelGGL(gs::ss_binary_table_kernel<K>, dim3(tg < gs::SS_TABLE_GRID ? tg : gs::SS_TABLE_GRID), dim3(gs::SS_THREADS), 0, s, hay, n, q, m,
                           out, samples, ns, S, (uint32_t)kt, desc, right);
    } else {
        hipLaunchKernelGGL(gs::ss_binary_plain_kernel<K>, dim3(div_up(m, gs::SS_PLAIN_THREADS)), dim3(gs::SS_PLAIN_THREADS), 0, s, hay, n, q, m, out,
                           (uint32_t)kt, desc, right);
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}
#endif
}  // namespace

extern "C" {

size_t gs_search_temp_bytes(uint32_t max_keys, uint32_t max_queries, uint32_t key_bytes, int sort_queries) {
    if (!search_sizes_ok(max_keys, max_queries) || (key_bytes != 4u && key_bytes != 8u) || (sort_queries != 0 && sort_queries != 1)) return 0;
    return search_layout(max_queries, key_bytes, sort_queries != 0).total + (sort_queries ? gs_onesweep_temp_bytes(max_queries) : 0u);
}

gs_status gs_search_create(gs_search** out, uint32_t max_keys, uint32_t max_queries, uint32_t key_bytes, int sort_queries) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!search_sizes_ok(max_keys, max_queries)) return GS_ERR_SIZE;
    if ((key_bytes != 4u && key_bytes != 8u) || (sort_queries != 0 && sort_queries != 1)) return GS_ERR_ARG;  // (2-byte keys: a follow-up)
    const gs_mode mode = sort_queries ? GS_MODE_PAIRS : GS_MODE_KEYS_ONLY;
    const uint32_t vb = sort_queries ? 4u : 0u;
    return handle_create(out, true, mode, vb, [&](gs_search* h) {
        h->max_keys = max_keys;
        h->max_queries = max_queries;
        h->key_bytes = key_bytes;
        if (sort_queries) {
            const gs_status st = gs_onesweep_create(&h->engine, max_queries, GS_MODE_PAIRS, 4u);
            if (st != GS_OK) return st;
        }
        const SearchLayout l = search_layout(max_queries, key_bytes, sort_queries != 0);
        return h->ws.alloc(l.total, l.ctl, gs::SSC_WORDS, gs::SSC_WORDS);
    });
}

gs_status gs_search_destroy(gs_search* h) { return handle_destroy(h); }  // (the engine with it: ~gs_search)

gs_status gs_search_plan(uint32_t n, uint32_t m, uint32_t key_bytes, uint32_t plan[GS_SEARCH_PLAN_WORDS]) {
    if (!plan) return GS_ERR_ARG;
    if (!search_sizes_ok(n, m)) return GS_ERR_SIZE;  // (sizes in front of the key width, as gs_search_create)
    if (key_bytes != 4u && key_bytes != 8u) return GS_ERR_ARG;
    search_plan(n, m, key_bytes, plan);
    return GS_OK;
}

gs_status gs_search_set_route(gs_search* h, uint32_t route) {
    if (!h || route > GS_SEARCH_ROUTE_BINARY) return GS_ERR_ARG;
    h->forced_route = route;
    return GS_OK;
}

gs_status gs_search_set_table(gs_search* h, uint32_t table) {
    if (!h || table > GS_SEARCH_TABLE_OFF) return GS_ERR_ARG;
    h->forced_table = table;
    return GS_OK;
}

gs_status gs_search_sorted(gs_search* h, const void* d_hay, uint32_t n, const void* d_queries, uint32_t m, void* d_out, gs_key_type key_type,
                           gs_order order, gs_search_side side, int queries_sorted, void* stream) {
    if (!h) return GS_ERR_ARG;
    h->last_route = GS_SEARCH_ROUTE_NONE;  // a refused call leaves no route behind
    if (!d_hay || !d_queries || !d_out || misaligned(d_hay) || misaligned(d_queries) || misaligned(d_out)) return GS_ERR_ARG;
    if (!(h->key_bytes == 8u ? is_key64_type(key_type) : is_key32_type(key_type)) || !valid_order(order) ||
        (side != GS_SEARCH_LEFT && side != GS_SEARCH_RIGHT))
        return GS_ERR_ARG;
    // the route of the call: a forced one, else queries in order go to the tile kernel and the others by the plan's rule
    const bool auto_route = h->forced_route == GS_SEARCH_ROUTE_AUTO;
    if (!auto_route && h->forced_route == GS_SEARCH_ROUTE_SORT && !h->engine) return GS_ERR_MODE;
    if (n == 0 || m == 0 || n > h->max_keys || m > h->max_queries) return GS_ERR_SIZE;
    {  // no buffer of the call on another: n keys, m queries, m positions
        const void* p[3] = {d_hay, d_queries, d_out};
        const size_t b[3] = {(size_t)n * h->key_bytes, (size_t)m * h->key_bytes, (size_t)m * 4u};
        if (any_overlap(p, b, 3)) return GS_ERR_ARG;
    }
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no search kernels
#if GS_SORT16_BUILT
    search_plan(n, m, h->key_bytes, h->last_plan);
    uint32_t route = h->forced_route;
    if (auto_route)
        route = queries_sorted ? h->last_plan[GS_SEARCH_P_ROUTE_SORTED]
                               : h->last_plan[h->engine ? GS_SEARCH_P_ROUTE_UNSORTED : GS_SEARCH_P_ROUTE_NO_ENGINE];
    const bool table = route == GS_SEARCH_ROUTE_BINARY &&
                       (h->forced_table == GS_SEARCH_TABLE_AUTO ? h->last_plan[GS_SEARCH_P_TABLE] != 0u : h->forced_table == GS_SEARCH_TABLE_ON);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t right = side == GS_SEARCH_RIGHT ? 1u : 0u;
    const gs_status st = h->key_bytes == 8u
                             ? search_enqueue<uint64_t>(h, static_cast<const uint64_t*>(d_hay), n, static_cast<const uint64_t*>(d_queries), m,
                                                        static_cast<uint32_t*>(d_out), key_type, order, right, route, table, s)
                             : search_enqueue<uint32_t>(h, static_cast<const uint32_t*>(d_hay), n, static_cast<const uint32_t*>(d_queries), m,
                                                        static_cast<uint32_t*>(d_out), key_type, order, right, route, table, s);
    if (st != GS_OK) return st;
    h->last_route = route;
    h->last_table = table ? 1u : 0u;
    h->last_n = n;
    h->last_m = m;
    return GS_OK;
#else
    (void)queries_sorted;
    (void)stream;
    return GS_ERR_MODE;
#endif
}

gs_status gs_search_last(gs_search* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SEARCH_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SEARCH_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_SEARCH_R_ROUTE] = h->last_route;
    report[GS_SEARCH_R_ENGINE] = h->engine ? 1u : 0u;
    if (h->last_route == GS_SEARCH_ROUTE_NONE) return GS_OK;
    report[GS_SEARCH_R_N] = h->last_n;
    report[GS_SEARCH_R_M] = h->last_m;
    report[GS_SEARCH_R_TABLE] = h->last_table;
    report[GS_SEARCH_R_LDS_TILES] = h->ws.pinned[gs::SSC_LDS_TILES];
    report[GS_SEARCH_R_GLOBAL_TILES] = h->ws.pinned[gs::SSC_GLOBAL_TILES];
    for (uint32_t i = 0; i < GS_SEARCH_PLAN_WORDS; ++i) report[GS_SEARCH_R_PLAN + i] = h->last_plan[i];
    return GS_OK;
}

}  // extern "C"
