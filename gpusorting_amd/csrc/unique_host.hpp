// unique_host.hpp — part of the gpusort_capi.hip translation unit: the gs_unique handle (unique_kernels.hpp) and its entries: the
// layout, the range plan, the three routes and the report.  Allocation, the create frame and the control read-back are
// handle_core.hpp's; the sort in front of the run-length stage is an embedded gs_onesweep (onesweep_host.hpp), keys only or pairs with
// 4-byte values (the positions).  No counterpart in the reference project.
// unique_layout, unique_enqueue_rle and unique_impl take the key word K (uint32_t here, uint64_t from unique64_host.hpp): the argument
// checks, their order and the launches are one text for both widths.
struct gs_unique {
    uint32_t max_keys = 0;
    gs_mode mode = GS_MODE_KEYS_ONLY;
    uint32_t value_bytes = 0;
    int rank_mode = 0;             // (handle_core's frame; the engine's own is what gs_unique_last reports)
    gs_onesweep* engine = nullptr;  // capacity max_keys
    Workspace ws;                  // one allocation: see unique_layout; the control block lies at its start
    uint32_t last_route = GS_UNIQUE_ROUTE_NONE, last_n = 0, last_plan[3] = {0u, 0u, 0u};
    bool sort_failed = false;      // the engine refused a call on the host side
    ~gs_unique() {
        if (engine) (void)gs_onesweep_destroy(engine);
    }
};

namespace {
struct UniqueLayout {
    size_t ctl, rc, rl, base, prev, keys, alt_keys, pos, alt_pos, total;
};
// the control block, four words per range, and the engine's buffers: the copy of the keys and its alternate, with positions twice more
UniqueLayout unique_layout(uint32_t max_keys, bool pairs, uint32_t key_bytes = 4u) {
    UniqueLayout l{};
    Arena a;
    l.ctl = a.take(gs::UQC_WORDS * 4u);
    l.rc = a.take(gs::UQ_CAP * 4u);
    l.rl = a.take(gs::UQ_CAP * 4u);
    l.base = a.take(gs::UQ_CAP * 4u);
    l.prev = a.take(gs::UQ_CAP * 4u);
    l.keys = a.take((size_t)max_keys * key_bytes);
    l.alt_keys = a.take((size_t)max_keys * key_bytes);
    l.pos = a.take(pairs ? (size_t)max_keys * 4u : 0u);
    l.alt_pos = a.take(pairs ? (size_t)max_keys * 4u : 0u);
    l.total = a.total();
    return l;
}
inline bool unique_sizes_ok(uint32_t max_keys) { return max_keys != 0 && max_keys <= GS_MAX_KEYS; }
// keys and counts: (keys only, 0); first and inverse as well: (pairs, 4)
inline bool unique_mode_ok(gs_mode mode, uint32_t vb) { return mode == GS_MODE_KEYS_ONLY ? vb == 0u : mode == GS_MODE_PAIRS && vb == 4u; }
// the key types an entry on key words K sorts: 0 .. 2 on 4-byte words, 3 .. 5 on 8-byte ones (host_common's is_key64 is kt >= 3: the
// engine asks it behind valid_key_type, so it lets the 16-bit types 6 .. 9 and anything above through, which these entries refuse)
inline bool is_key64_type(gs_key_type kt) { return (int)kt >= 3 && (int)kt <= 5; }
template <class K>
inline bool key_type_of_width(gs_key_type kt) { return sizeof(K) == 8u ? is_key64_type(kt) : is_key32_type(kt); }

// plan[0] ranges (<= UQ_CAP), [1] elements per range (a multiple of the tile), [2] tile.  The smallest range is one tile.
void unique_plan(uint32_t n, uint32_t plan[3]) {
    const uint32_t per = div_up(div_up(n, gs::UQ_CAP), gs::UQ_TILE) * gs::UQ_TILE;
    plan[0] = div_up(n, per);
    plan[1] = per;
    plan[2] = gs::UQ_TILE;
}

#if GS_SORT16_BUILT
// count, scan, compact over keys[0 .. n) (and perm beside them): every grid is the plan's, a function of n alone
template <class K>
void unique_enqueue_rle(gs_unique* h, const UniqueLayout& l, const K* keys, const uint32_t* perm, uint32_t n, bool tail_first, K* out_keys,
                        uint32_t* out_counts, uint32_t* out_first, uint32_t* out_inverse, uint32_t* out_num, hipStream_t s) {
    uint32_t* ctl = h->ws.ctl();
    uint32_t* rc = reinterpret_cast<uint32_t*>(h->ws.dev + l.rc);
    uint32_t* rl = reinterpret_cast<uint32_t*>(h->ws.dev + l.rl);
    uint32_t* base = reinterpret_cast<uint32_t*>(h->ws.dev + l.base);
    uint32_t* prev = reinterpret_cast<uint32_t*>(h->ws.dev + l.prev);
    unique_plan(n, h->last_plan);
    const uint32_t ranges = h->last_plan[0], per = h->last_plan[1];
    hipLaunchKernelGGL(gs::uq_count_kernel<K>, dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, n, per, rc, rl);
    hipLaunchKernelGGL(gs::uq_scan_kernel, dim3(1), dim3(gs::UQ_CAP), 0, s, rc, rl, ranges, n, base, prev, out_num, ctl);
    if (perm)
        hipLaunchKernelGGL((gs::uq_compact_kernel<K, true>), dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, perm, n, per, tail_first ? 1u : 0u, base, prev, rc,
                           out_keys, out_counts, out_first, out_inverse, ctl);
    else
        hipLaunchKernelGGL((gs::uq_compact_kernel<K, false>), dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, perm, n, per, 0u, base, prev, rc, out_keys,
                           out_counts, out_first, out_inverse, ctl);
}
#endif

// route: GS_UNIQUE_ROUTE_KEYS / _POSITIONS / _CONSECUTIVE
template <class K>
gs_status unique_impl(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first, void* d_out_inverse,
                      void* d_out_num, gs_key_type kt, gs_order order, hipStream_t s, uint32_t route) {
    if (!h) return GS_ERR_ARG;
    h->last_route = GS_UNIQUE_ROUTE_NONE;  // a refused call leaves no route behind
    const bool sorted = route != GS_UNIQUE_ROUTE_CONSECUTIVE;
    if (!d_keys || !d_out_keys || misaligned(d_keys) || misaligned(d_out_keys)) return GS_ERR_ARG;
    if (sorted && (!key_type_of_width<K>(kt) || !valid_order(order))) return GS_ERR_ARG;
    if (route == GS_UNIQUE_ROUTE_POSITIONS && h->mode != GS_MODE_PAIRS) return GS_ERR_MODE;
    if ((d_out_counts && misaligned(d_out_counts)) || (d_out_first && misaligned(d_out_first)) || (d_out_inverse && misaligned(d_out_inverse)) ||
        (reinterpret_cast<uintptr_t>(d_out_num) & 3u) != 0)
        return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys) return GS_ERR_SIZE;
    {  // no buffer of the call on another: n elements each, one word at d_out_num; a null pointer takes no room
        const void* p[6] = {d_keys, d_out_keys, d_out_counts, d_out_first, d_out_inverse, d_out_num};
        const size_t nb = (size_t)n * 4u, kb = (size_t)n * sizeof(K);
        const size_t b[6] = {kb, kb, d_out_counts ? nb : 0u, d_out_first ? nb : 0u, d_out_inverse ? nb : 0u, d_out_num ? 4u : 0u};
        for (int i = 0; i < 6; ++i)
            for (int j = i + 1; j < 6; ++j)
                if (b[i] && b[j] && buffers_overlap(p[i], b[i], p[j], b[j])) return GS_ERR_ARG;
    }
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no run-length kernels
#if GS_SORT16_BUILT
    h->sort_failed = false;
    const bool pairs = h->mode == GS_MODE_PAIRS;
    const UniqueLayout l = unique_layout(h->max_keys, pairs, (uint32_t)sizeof(K));
    K* out_keys = static_cast<K*>(d_out_keys);
    uint32_t* out_counts = static_cast<uint32_t*>(d_out_counts);
    uint32_t* out_first = static_cast<uint32_t*>(d_out_first);
    uint32_t* out_inverse = static_cast<uint32_t*>(d_out_inverse);
    uint32_t* out_num = static_cast<uint32_t*>(d_out_num);
    const K* src = static_cast<const K*>(d_keys);
    h->last_n = n;
    if (!sorted) {  // the input as it lies
        unique_enqueue_rle<K>(h, l, src, nullptr, n, false, out_keys, out_counts, nullptr, out_inverse, out_num, s);
        GS_HIP(hipGetLastError());
        h->last_route = route;
        return GS_OK;
    }
    K* keys = reinterpret_cast<K*>(h->ws.dev + l.keys);
    K* alt_keys = reinterpret_cast<K*>(h->ws.dev + l.alt_keys);
    const uint32_t prep_grid = div_up(n, gs::UQ_PREP_TILE);
    gs_status st;
    if (route == GS_UNIQUE_ROUTE_POSITIONS) {
        uint32_t* pos = reinterpret_cast<uint32_t*>(h->ws.dev + l.pos);
        uint32_t* alt_pos = reinterpret_cast<uint32_t*>(h->ws.dev + l.alt_pos);
        hipLaunchKernelGGL((gs::uq_prepare_kernel<K, true>), dim3(prep_grid), dim3(gs::UQ_PREP_THREADS), 0, s, src, n, keys, pos);
        GS_HIP(hipGetLastError());
        st = gs_onesweep_sort_pairs(h->engine, keys, pos, alt_keys, alt_pos, n, kt, order, s);
        if (st == GS_OK)
            unique_enqueue_rle<K>(h, l, keys, pos, n, order == GS_ORDER_DESCENDING, out_keys, out_counts, out_first, out_inverse, out_num, s);
    } else {  // a pairs handle sorts the keys alone with its pairs engine: positions nobody reads
        uint32_t* pos = pairs ? reinterpret_cast<uint32_t*>(h->ws.dev + l.pos) : nullptr;
        if (pairs) hipLaunchKernelGGL((gs::uq_prepare_kernel<K, true>), dim3(prep_grid), dim3(gs::UQ_PREP_THREADS), 0, s, src, n, keys, pos);
        else hipLaunchKernelGGL((gs::uq_prepare_kernel<K, false>), dim3(prep_grid), dim3(gs::UQ_PREP_THREADS), 0, s, src, n, keys, pos);
        GS_HIP(hipGetLastError());
        st = pairs ? gs_onesweep_sort_pairs(h->engine, keys, pos, alt_keys, h->ws.dev + l.alt_pos, n, kt, order, s)
                   : gs_onesweep_sort_keys(h->engine, keys, alt_keys, n, kt, order, s);
        if (st == GS_OK) unique_enqueue_rle<K>(h, l, keys, nullptr, n, false, out_keys, out_counts, nullptr, nullptr, out_num, s);
    }
    h->last_route = route;
    if (st != GS_OK) {
        h->sort_failed = true;
        return st;
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
#else
    (void)s;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_unique_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (!unique_sizes_ok(max_keys) || !unique_mode_ok(mode, value_bytes)) return 0;
    return unique_layout(max_keys, mode == GS_MODE_PAIRS).total + gs_onesweep_temp_bytes(max_keys);
}

gs_status gs_unique_create(gs_unique** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!unique_sizes_ok(max_keys)) return GS_ERR_SIZE;
    if (!unique_mode_ok(mode, value_bytes)) return GS_ERR_MODE;  // (8-byte values: before anything looks for a device)
    return handle_create(out, true, mode, value_bytes, [&](gs_unique* h) {
        h->max_keys = max_keys;
        const gs_status st = gs_onesweep_create(&h->engine, max_keys, mode, value_bytes);  // (either engine at the library's defaults)
        if (st != GS_OK) return st;
        const UniqueLayout l = unique_layout(max_keys, mode == GS_MODE_PAIRS);
        return h->ws.alloc(l.total, l.ctl, gs::UQC_WORDS, gs::UQC_WORDS);
    });
}

gs_status gs_unique_destroy(gs_unique* h) { return handle_destroy(h); }  // (the engine with it: ~gs_unique)

gs_status gs_unique_keys(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_num, gs_key_type key_type,
                         gs_order order, void* stream) {
    return unique_impl<uint32_t>(h, d_keys, n, d_out_keys, d_out_counts, nullptr, nullptr, d_out_num, key_type, order, static_cast<hipStream_t>(stream),
                       GS_UNIQUE_ROUTE_KEYS);
}

gs_status gs_unique_positions(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first, void* d_out_inverse,
                              void* d_out_num, gs_key_type key_type, gs_order order, void* stream) {
    return unique_impl<uint32_t>(h, d_keys, n, d_out_keys, d_out_counts, d_out_first, d_out_inverse, d_out_num, key_type, order, static_cast<hipStream_t>(stream),
                       GS_UNIQUE_ROUTE_POSITIONS);
}

gs_status gs_unique_consecutive(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_inverse, void* d_out_num,
                                void* stream) {
    return unique_impl<uint32_t>(h, d_keys, n, d_out_keys, d_out_counts, nullptr, d_out_inverse, d_out_num, GS_KEY_UINT32, GS_ORDER_ASCENDING,
                       static_cast<hipStream_t>(stream), GS_UNIQUE_ROUTE_CONSECUTIVE);
}

gs_status gs_unique_plan(uint32_t n, uint32_t plan[3]) {
    if (!plan) return GS_ERR_ARG;
    if (n == 0 || n > GS_MAX_KEYS) return GS_ERR_SIZE;
    unique_plan(n, plan);
    return GS_OK;
}

gs_status gs_unique_check(gs_unique* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    const uint32_t* c = h->ws.pinned;
    if (h->sort_failed || (c[gs::UQC_STATUS] & gs::UQ_ST_INTERNAL) || c[gs::UQC_U] != c[gs::UQC_WRITTEN]) return GS_ERR_HIP;
    const bool sorted = h->last_route == GS_UNIQUE_ROUTE_KEYS || h->last_route == GS_UNIQUE_ROUTE_POSITIONS;
    return sorted ? gs_onesweep_check(h->engine, stream) : GS_OK;
}

gs_status gs_unique_last(gs_unique* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_UNIQUE_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_UNIQUE_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_UNIQUE_R_ROUTE] = h->last_route;
    report[GS_UNIQUE_R_STATUS] = h->ws.pinned[gs::UQC_STATUS];
    report[GS_UNIQUE_R_RANK] = (uint32_t)gs_onesweep_get_rank_mode(h->engine);
    if (h->last_route == GS_UNIQUE_ROUTE_NONE) return GS_OK;
    report[GS_UNIQUE_R_N] = h->last_n;
    report[GS_UNIQUE_R_U] = h->ws.pinned[gs::UQC_U];
    report[GS_UNIQUE_R_RANGES] = h->last_plan[0];
    report[GS_UNIQUE_R_PER_RANGE] = h->last_plan[1];
    report[GS_UNIQUE_R_TILE] = h->last_plan[2];
    return GS_OK;
}

}  // extern "C"
