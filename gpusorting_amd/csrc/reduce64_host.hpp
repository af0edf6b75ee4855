// reduce64_host.hpp — part of the gpusort_capi.hip translation unit: the gs_reduce64 handle and its entries: gs_reduce_* on 8-byte keys
// (GS_KEY_UINT64 / INT64 / FLOAT64).  The handle is gs_reduce's with 8-byte key copies in its workspace; the argument checks, their
// order, the routes and the launches are reduce_host.hpp's reduce_impl on the key word uint64_t, the kernels reduce_kernels.hpp's on
// that word (the tree of a float sum is the same one), the plan gs_unique_plan.  No counterpart in the reference project.
struct gs_reduce64 : gs_reduce {};

extern "C" {

size_t gs_reduce64_temp_bytes(uint32_t max_keys, uint32_t value_bytes) {
    if (!reduce_sizes_ok(max_keys) || !reduce_width_ok(value_bytes)) return 0;
    return reduce_layout(max_keys, value_bytes, 8u).total + gs_onesweep_temp_bytes(max_keys);
}

gs_status gs_reduce64_create(gs_reduce64** out, uint32_t max_keys, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!reduce_sizes_ok(max_keys)) return GS_ERR_SIZE;
    if (!reduce_width_ok(value_bytes)) return GS_ERR_MODE;  // (before anything looks for a device)
    return handle_create(out, true, GS_MODE_PAIRS, value_bytes, [&](gs_reduce64* h) {
        h->max_keys = max_keys;
        const gs_status st = gs_onesweep_create(&h->engine, max_keys, GS_MODE_PAIRS, value_bytes);
        if (st != GS_OK) return st;
        const ReduceLayout l = reduce_layout(max_keys, value_bytes, 8u);
        h->ws_bytes = l.total;
        return h->ws.alloc(l.total, l.ctl, gs::UQC_WORDS, gs::UQC_WORDS);
    });
}

gs_status gs_reduce64_destroy(gs_reduce64* h) { return handle_destroy(h); }  // (the engine with it: ~gs_reduce)

gs_status gs_reduce64_by_key(gs_reduce64* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values,
                             void* d_out_counts, void* d_out_num, gs_key_type key_type, gs_order order, gs_value_type value_type, gs_reduce_op op,
                             void* stream) {
    return reduce_impl<uint64_t>(h, d_keys, d_values, n, d_out_keys, d_out_values, d_out_counts, d_out_num, key_type, order, value_type, op,
                                 static_cast<hipStream_t>(stream), GS_REDUCE_ROUTE_SORTED);
}

gs_status gs_reduce64_by_key_consecutive(gs_reduce64* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values,
                                         void* d_out_counts, void* d_out_num, gs_value_type value_type, gs_reduce_op op, void* stream) {
    return reduce_impl<uint64_t>(h, d_keys, d_values, n, d_out_keys, d_out_values, d_out_counts, d_out_num, GS_KEY_UINT64, GS_ORDER_ASCENDING, value_type,
                                 op, static_cast<hipStream_t>(stream), GS_REDUCE_ROUTE_CONSECUTIVE);
}

gs_status gs_reduce64_check(gs_reduce64* h, void* stream) { return gs_reduce_check(h, stream); }

gs_status gs_reduce64_last(gs_reduce64* h, uint32_t* report, uint32_t words, void* stream) { return gs_reduce_last(h, report, words, stream); }

}  // extern "C"
