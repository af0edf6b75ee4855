// unique64_host.hpp — part of the gpusort_capi.hip translation unit: the gs_unique64 handle and its entries: gs_unique_* on 8-byte keys
// (GS_KEY_UINT64 / INT64 / FLOAT64).  The handle is gs_unique's with 8-byte key copies in its workspace; the argument checks, their
// order, the routes and the launches are unique_host.hpp's unique_impl on the key word uint64_t, the kernels unique_kernels.hpp's on
// that word, the plan gs_unique_plan.  The embedded gs_onesweep keeps its defaults on both handles: the engine's 64-bit route never
// takes position chains (sort_route), so the keys-only caveat of gs_unique_create does not arise.  No counterpart in the reference project.
struct gs_unique64 : gs_unique {};

extern "C" {

size_t gs_unique64_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (!unique_sizes_ok(max_keys) || !unique_mode_ok(mode, value_bytes)) return 0;
    return unique_layout(max_keys, mode == GS_MODE_PAIRS, 8u).total + gs_onesweep_temp_bytes(max_keys);
}

gs_status gs_unique64_create(gs_unique64** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!unique_sizes_ok(max_keys)) return GS_ERR_SIZE;
    if (!unique_mode_ok(mode, value_bytes)) return GS_ERR_MODE;  // (8-byte values: before anything looks for a device)
    return handle_create(out, true, mode, value_bytes, [&](gs_unique64* h) {
        h->max_keys = max_keys;
        const gs_status st = gs_onesweep_create(&h->engine, max_keys, mode, value_bytes);
        if (st != GS_OK) return st;
        const UniqueLayout l = unique_layout(max_keys, mode == GS_MODE_PAIRS, 8u);
        return h->ws.alloc(l.total, l.ctl, gs::UQC_WORDS, gs::UQC_WORDS);
    });
}

gs_status gs_unique64_destroy(gs_unique64* h) { return handle_destroy(h); }  // (the engine with it: ~gs_unique)

gs_status gs_unique64_keys(gs_unique64* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_num, gs_key_type key_type,
                           gs_order order, void* stream) {
    return unique_impl<uint64_t>(h, d_keys, n, d_out_keys, d_out_counts, nullptr, nullptr, d_out_num, key_type, order, static_cast<hipStream_t>(stream),
                                 GS_UNIQUE_ROUTE_KEYS);
}

gs_status gs_unique64_positions(gs_unique64* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first,
                                void* d_out_inverse, void* d_out_num, gs_key_type key_type, gs_order order, void* stream) {
    return unique_impl<uint64_t>(h, d_keys, n, d_out_keys, d_out_counts, d_out_first, d_out_inverse, d_out_num, key_type, order,
                                 static_cast<hipStream_t>(stream), GS_UNIQUE_ROUTE_POSITIONS);
}

gs_status gs_unique64_consecutive(gs_unique64* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_inverse,
                                  void* d_out_num, void* stream) {
    return unique_impl<uint64_t>(h, d_keys, n, d_out_keys, d_out_counts, nullptr, d_out_inverse, d_out_num, GS_KEY_UINT64, GS_ORDER_ASCENDING,
                                 static_cast<hipStream_t>(stream), GS_UNIQUE_ROUTE_CONSECUTIVE);
}

gs_status gs_unique64_check(gs_unique64* h, void* stream) { return gs_unique_check(h, stream); }

gs_status gs_unique64_last(gs_unique64* h, uint32_t* report, uint32_t words, void* stream) { return gs_unique_last(h, report, words, stream); }

}  // extern "C"
