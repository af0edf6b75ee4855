// reduce_host.hpp — part of the gpusort_capi.hip translation unit: the gs_reduce handle (reduce_kernels.hpp) and its entries: the
// layout, the two routes and the report.  Allocation, the create frame and the control read-back are handle_core.hpp's; the range plan
// is unique_host.hpp's (gs_unique_plan); the sort in front of the stage is an embedded gs_onesweep (onesweep_host.hpp) on (key, value)
// pairs with the handle's value width.  No counterpart in the reference project.
// reduce_layout, reduce_enqueue and reduce_impl take the key word K (uint32_t here, uint64_t from reduce64_host.hpp): the argument
// checks, their order and the launches are one text for both widths.
struct gs_reduce {
    uint32_t max_keys = 0;
    gs_mode mode = GS_MODE_PAIRS;
    uint32_t value_bytes = 0;
    int rank_mode = 0;              // (handle_core's frame; the engine's own is what gs_reduce_last reports)
    gs_onesweep* engine = nullptr;  // capacity max_keys, pairs
    Workspace ws;                   // one allocation: see reduce_layout; the control block lies at its start
    size_t ws_bytes = 0;
    uint32_t last_route = GS_REDUCE_ROUTE_NONE, last_n = 0, last_plan[3] = {0u, 0u, 0u}, last_value_type = 0, last_op = 0;
    bool sort_failed = false;       // the engine refused a call on the host side
    ~gs_reduce() {
        if (engine) (void)gs_onesweep_destroy(engine);
    }
};

namespace {
struct ReduceLayout {
    size_t ctl, rc, rl, base, prev, part, carry, keys, alt_keys, vals, alt_vals, total;
};
// the control block, four words and two values (8 bytes each, whatever the width) per range, and the engine's buffers: the copies of
// the keys and the values and their alternates
ReduceLayout reduce_layout(uint32_t max_keys, uint32_t vb, uint32_t key_bytes = 4u) {
    ReduceLayout l{};
    Arena a;
    l.ctl = a.take(gs::UQC_WORDS * 4u);
    l.rc = a.take(gs::UQ_CAP * 4u);
    l.rl = a.take(gs::UQ_CAP * 4u);
    l.base = a.take(gs::UQ_CAP * 4u);
    l.prev = a.take(gs::UQ_CAP * 4u);
    l.part = a.take(gs::UQ_CAP * 8u);
    l.carry = a.take(gs::UQ_CAP * 8u);
    l.keys = a.take((size_t)max_keys * key_bytes);
    l.alt_keys = a.take((size_t)max_keys * key_bytes);
    l.vals = a.take((size_t)max_keys * vb);
    l.alt_vals = a.take((size_t)max_keys * vb);
    l.total = a.total();
    return l;
}
inline bool reduce_sizes_ok(uint32_t max_keys) { return max_keys != 0 && max_keys <= GS_MAX_KEYS; }
inline bool reduce_width_ok(uint32_t vb) { return vb == 4u || vb == 8u; }
inline bool valid_value_type(gs_value_type vt) { return (int)vt >= 0 && (int)vt <= 5; }
inline bool valid_reduce_op(gs_reduce_op op) { return (int)op >= 0 && (int)op <= 2; }
inline uint32_t value_type_bytes(gs_value_type vt) { return (int)vt <= (int)GS_VALUE_FLOAT32 ? 4u : 8u; }

#if GS_SORT16_BUILT
// count, scan, reduce over (keys, vals)[0 .. n): every grid is the plan's, a function of n alone
template <class K, class Op>
void reduce_enqueue_op(gs_reduce* h, const ReduceLayout& l, const K* keys, const void* vals, uint32_t n, uint32_t xform, K* out_keys,
                       void* out_values, uint32_t* out_counts, uint32_t* out_num, hipStream_t s) {
    typedef typename Op::V V;
    uint32_t* ctl = h->ws.ctl();
    uint32_t* rc = reinterpret_cast<uint32_t*>(h->ws.dev + l.rc);
    uint32_t* rl = reinterpret_cast<uint32_t*>(h->ws.dev + l.rl);
    uint32_t* base = reinterpret_cast<uint32_t*>(h->ws.dev + l.base);
    uint32_t* prev = reinterpret_cast<uint32_t*>(h->ws.dev + l.prev);
    V* part = reinterpret_cast<V*>(h->ws.dev + l.part);
    V* carry = reinterpret_cast<V*>(h->ws.dev + l.carry);
    const V* v = static_cast<const V*>(vals);
    unique_plan(n, h->last_plan);
    const uint32_t ranges = h->last_plan[0], per = h->last_plan[1];
    hipLaunchKernelGGL((gs::rd_count_kernel<K, Op>), dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, v, n, per, xform, rc, rl, part);
    hipLaunchKernelGGL(gs::rd_scan_kernel<Op>, dim3(1), dim3(gs::UQ_CAP), 0, s, rc, rl, part, ranges, n, base, prev, carry, out_num, ctl);
    hipLaunchKernelGGL((gs::rd_reduce_kernel<K, Op>), dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, v, n, per, xform, base, prev, carry, rc, out_keys,
                       static_cast<V*>(out_values), out_counts, ctl);
}
// The instantiation of (value type, op).  SUM: the integers of one width share the modular sum, the floats have their own.  MIN / MAX:
// unsigned on order-preserving bits, one instantiation per width.
template <class K>
void reduce_enqueue(gs_reduce* h, const ReduceLayout& l, const K* keys, const void* vals, uint32_t n, gs_value_type vt, gs_reduce_op op,
                    K* out_keys, void* out_values, uint32_t* out_counts, uint32_t* out_num, hipStream_t s) {
    const bool wide = value_type_bytes(vt) == 8u;
    const bool flt = vt == GS_VALUE_FLOAT32 || vt == GS_VALUE_FLOAT64, sgn = vt == GS_VALUE_INT32 || vt == GS_VALUE_INT64;
#define GS_RD(OP, X) reduce_enqueue_op<K, gs::OP>(h, l, keys, vals, n, X, out_keys, out_values, out_counts, out_num, s)
    if (op == GS_REDUCE_SUM) {
        if (flt) { if (wide) GS_RD(RdSumF64, gs::RD_X_NONE); else GS_RD(RdSumF32, gs::RD_X_NONE); }
        else { if (wide) GS_RD(RdSumU64, gs::RD_X_NONE); else GS_RD(RdSumU32, gs::RD_X_NONE); }
        return;
    }
    const uint32_t x = flt ? gs::RD_X_FLOAT : sgn ? gs::RD_X_SIGNED : gs::RD_X_NONE;
    if (op == GS_REDUCE_MIN) { if (wide) GS_RD(RdMinU64, x); else GS_RD(RdMinU32, x); }
    else { if (wide) GS_RD(RdMaxU64, x); else GS_RD(RdMaxU32, x); }
#undef GS_RD
}
#endif

// route: GS_REDUCE_ROUTE_SORTED / _CONSECUTIVE
template <class K>
gs_status reduce_impl(gs_reduce* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values, void* d_out_counts,
                      void* d_out_num, gs_key_type kt, gs_order order, gs_value_type vt, gs_reduce_op op, hipStream_t s, uint32_t route) {
    if (!h) return GS_ERR_ARG;
    h->last_route = GS_REDUCE_ROUTE_NONE;  // a refused call leaves no route behind
    const bool sorted = route == GS_REDUCE_ROUTE_SORTED;
    if (!d_keys || !d_values || !d_out_keys || !d_out_values || misaligned(d_keys) || misaligned(d_values) || misaligned(d_out_keys) ||
        misaligned(d_out_values))
        return GS_ERR_ARG;
    if (sorted && (!key_type_of_width<K>(kt) || !valid_order(order))) return GS_ERR_ARG;
    if (!valid_value_type(vt) || !valid_reduce_op(op)) return GS_ERR_ARG;
    if (value_type_bytes(vt) != h->value_bytes) return GS_ERR_MODE;
    if ((d_out_counts && misaligned(d_out_counts)) || (reinterpret_cast<uintptr_t>(d_out_num) & 3u) != 0) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys) return GS_ERR_SIZE;
    {  // no buffer of the call on another, nor on the handle's workspace: n elements each, one word at d_out_num; null takes no room
        const size_t kb = (size_t)n * sizeof(K), vb = (size_t)n * h->value_bytes, cb = (size_t)n * 4u;
        const void* p[7] = {d_keys, d_values, d_out_keys, d_out_values, d_out_counts, d_out_num, h->ws.dev};
        const size_t b[7] = {kb, vb, kb, vb, d_out_counts ? cb : 0u, d_out_num ? 4u : 0u, h->ws_bytes};
        for (int i = 0; i < 7; ++i)
            for (int j = i + 1; j < 7; ++j)
                if (b[i] && b[j] && buffers_overlap(p[i], b[i], p[j], b[j])) return GS_ERR_ARG;
    }
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no reduce kernels
#if GS_SORT16_BUILT
    h->sort_failed = false;
    const ReduceLayout l = reduce_layout(h->max_keys, h->value_bytes, (uint32_t)sizeof(K));
    K* out_keys = static_cast<K*>(d_out_keys);
    uint32_t* out_counts = static_cast<uint32_t*>(d_out_counts);
    uint32_t* out_num = static_cast<uint32_t*>(d_out_num);
    const K* src = static_cast<const K*>(d_keys);
    h->last_n = n;
    h->last_value_type = (uint32_t)vt;
    h->last_op = (uint32_t)op;
    if (!sorted) {  // the input as it lies
        reduce_enqueue<K>(h, l, src, d_values, n, vt, op, out_keys, d_out_values, out_counts, out_num, s);
        GS_HIP(hipGetLastError());
        h->last_route = route;
        return GS_OK;
    }
    K* keys = reinterpret_cast<K*>(h->ws.dev + l.keys);
    K* alt_keys = reinterpret_cast<K*>(h->ws.dev + l.alt_keys);
    char* vals = h->ws.dev + l.vals;
    char* alt_vals = h->ws.dev + l.alt_vals;
    const uint32_t prep_grid = div_up(n, gs::UQ_PREP_TILE);
    if (h->value_bytes == 8u)
        hipLaunchKernelGGL((gs::rd_prepare_kernel<K, uint64_t>), dim3(prep_grid), dim3(gs::UQ_PREP_THREADS), 0, s, src, static_cast<const uint64_t*>(d_values), n,
                           keys, reinterpret_cast<uint64_t*>(vals));
    else
        hipLaunchKernelGGL((gs::rd_prepare_kernel<K, uint32_t>), dim3(prep_grid), dim3(gs::UQ_PREP_THREADS), 0, s, src, static_cast<const uint32_t*>(d_values), n,
                           keys, reinterpret_cast<uint32_t*>(vals));
    GS_HIP(hipGetLastError());
    const gs_status st = gs_onesweep_sort_pairs(h->engine, keys, vals, alt_keys, alt_vals, n, kt, order, s);
    h->last_route = route;
    if (st != GS_OK) {
        h->sort_failed = true;
        return st;
    }
    reduce_enqueue<K>(h, l, keys, vals, n, vt, op, out_keys, d_out_values, out_counts, out_num, s);
    GS_HIP(hipGetLastError());
    return GS_OK;
#else
    (void)s;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_reduce_temp_bytes(uint32_t max_keys, uint32_t value_bytes) {
    if (!reduce_sizes_ok(max_keys) || !reduce_width_ok(value_bytes)) return 0;
    return reduce_layout(max_keys, value_bytes).total + gs_onesweep_temp_bytes(max_keys);
}

gs_status gs_reduce_create(gs_reduce** out, uint32_t max_keys, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!reduce_sizes_ok(max_keys)) return GS_ERR_SIZE;
    if (!reduce_width_ok(value_bytes)) return GS_ERR_MODE;  // (before anything looks for a device)
    return handle_create(out, true, GS_MODE_PAIRS, value_bytes, [&](gs_reduce* h) {
        h->max_keys = max_keys;
        const gs_status st = gs_onesweep_create(&h->engine, max_keys, GS_MODE_PAIRS, value_bytes);  // (the pairs sorter keeps its defaults)
        if (st != GS_OK) return st;
        const ReduceLayout l = reduce_layout(max_keys, value_bytes);
        h->ws_bytes = l.total;
        return h->ws.alloc(l.total, l.ctl, gs::UQC_WORDS, gs::UQC_WORDS);
    });
}

gs_status gs_reduce_destroy(gs_reduce* h) { return handle_destroy(h); }  // (the engine with it: ~gs_reduce)

gs_status gs_reduce_by_key(gs_reduce* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values, void* d_out_counts,
                           void* d_out_num, gs_key_type key_type, gs_order order, gs_value_type value_type, gs_reduce_op op, void* stream) {
    return reduce_impl<uint32_t>(h, d_keys, d_values, n, d_out_keys, d_out_values, d_out_counts, d_out_num, key_type, order, value_type, op,
                       static_cast<hipStream_t>(stream), GS_REDUCE_ROUTE_SORTED);
}

gs_status gs_reduce_by_key_consecutive(gs_reduce* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values,
                                       void* d_out_counts, void* d_out_num, gs_value_type value_type, gs_reduce_op op, void* stream) {
    return reduce_impl<uint32_t>(h, d_keys, d_values, n, d_out_keys, d_out_values, d_out_counts, d_out_num, GS_KEY_UINT32, GS_ORDER_ASCENDING, value_type, op,
                       static_cast<hipStream_t>(stream), GS_REDUCE_ROUTE_CONSECUTIVE);
}

gs_status gs_reduce_check(gs_reduce* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    const uint32_t* c = h->ws.pinned;
    if (h->sort_failed || (c[gs::UQC_STATUS] & gs::UQ_ST_INTERNAL) || c[gs::UQC_U] != c[gs::UQC_WRITTEN]) return GS_ERR_HIP;
    return h->last_route == GS_REDUCE_ROUTE_SORTED ? gs_onesweep_check(h->engine, stream) : GS_OK;
}

gs_status gs_reduce_last(gs_reduce* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_REDUCE_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_REDUCE_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_REDUCE_R_ROUTE] = h->last_route;
    report[GS_REDUCE_R_STATUS] = h->ws.pinned[gs::UQC_STATUS];
    report[GS_REDUCE_R_RANK] = (uint32_t)gs_onesweep_get_rank_mode(h->engine);
    if (h->last_route == GS_REDUCE_ROUTE_NONE) return GS_OK;
    report[GS_REDUCE_R_N] = h->last_n;
    report[GS_REDUCE_R_U] = h->ws.pinned[gs::UQC_U];
    report[GS_REDUCE_R_RANGES] = h->last_plan[0];
    report[GS_REDUCE_R_PER_RANGE] = h->last_plan[1];
    report[GS_REDUCE_R_TILE] = h->last_plan[2];
    report[GS_REDUCE_R_VALUE_TYPE] = h->last_value_type;
    report[GS_REDUCE_R_OP] = h->last_op;
    return GS_OK;
}

}  // extern "C"
