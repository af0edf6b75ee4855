// merge_host.hpp — part of the gpusort_capi.hip translation unit: the gs_merge handle (merge_kernels.hpp) and its entries: the plan, the
// three forms and the report.  Allocation, the create frame and the control read-back are handle_core.hpp's.  The handle owns the
// control block and nothing that grows with n; there is no engine.  No counterpart in the reference project.
struct gs_merge {
    uint32_t max_keys = 0, key_bytes = 0;
    gs_mode mode = GS_MODE_KEYS_ONLY;  // (handle_core's frame)
    uint32_t value_bytes = 0;
    int rank_mode = 0;
    Workspace ws;  // the control block
    uint32_t last_form = GS_MERGE_FORM_NONE, last_na = 0, last_nb = 0, last_plan[GS_MERGE_PLAN_WORDS] = {};
};

namespace {
inline size_t merge_layout_bytes() {
    Arena a;
    (void)a.take(gs::MGC_WORDS * 4u);
    return a.total();
}
inline bool merge_sizes_ok(uint32_t max_keys) { return max_keys != 0 && max_keys <= GS_MAX_KEYS; }

// gs_merge_plan's words for na + nb = n outputs of key_bytes bytes (sizes checked by the caller)
void merge_plan(uint32_t n, uint32_t key_bytes, uint32_t plan[GS_MERGE_PLAN_WORDS]) {
    const uint32_t T = key_bytes == 8u ? gs::MgShape<uint64_t>::T : gs::MgShape<uint32_t>::T;
    for (uint32_t i = 0; i < GS_MERGE_PLAN_WORDS; ++i) plan[i] = 0;
    plan[GS_MERGE_P_TILE] = T;
    plan[GS_MERGE_P_VT] = T / gs::MG_THREADS;
    plan[GS_MERGE_P_THREADS] = gs::MG_THREADS;
    plan[GS_MERGE_P_GRID] = div_up(n, T);
    plan[GS_MERGE_P_LDS_BYTES] = T * (key_bytes + 2u) + 8u;  // the words, the 16-bit indices (pairs and positions), the two splits
}

#if GS_SORT16_BUILT
template <class K, uint32_t FORM>
void merge_launch(gs_merge* h, const void* a, uint32_t na, const void* b, uint32_t nb, void* out, const void* av, const void* bv, void* aux,
                  gs_key_type kt, gs_order order, hipStream_t s) {
    hipLaunchKernelGGL((gs::mg_tile_kernel<K, FORM>), dim3(h->last_plan[GS_MERGE_P_GRID]), dim3(gs::MG_THREADS), 0, s, static_cast<const K*>(a), na,
                       static_cast<const K*>(b), nb, static_cast<K*>(out), av, bv, aux, (uint32_t)kt, order == GS_ORDER_DESCENDING ? 1u : 0u,
                       h->ws.ctl());
}
template <class K>
void merge_launch_form(gs_merge* h, uint32_t form, const void* a, uint32_t na, const void* b, uint32_t nb, void* out, const void* av, const void* bv,
                       void* aux, gs_key_type kt, gs_order order, hipStream_t s) {
    switch (form) {
        case gs::MG_KEYS: merge_launch<K, gs::MG_KEYS>(h, a, na, b, nb, out, av, bv, aux, kt, order, s); break;
        case gs::MG_PAIRS4: merge_launch<K, gs::MG_PAIRS4>(h, a, na, b, nb, out, av, bv, aux, kt, order, s); break;
        case gs::MG_PAIRS8: merge_launch<K, gs::MG_PAIRS8>(h, a, na, b, nb, out, av, bv, aux, kt, order, s); break;
        default: merge_launch<K, gs::MG_POSITIONS>(h, a, na, b, nb, out, av, bv, aux, kt, order, s); break;
    }
}
#endif

// One call of any form.  aux_bytes: the width of an element of the auxiliary output (0 keys; the values' width; 4 positions);
// with_vals: the call has a_vals / b_vals.  The checks stand in the order include/gpusort.h fixes.
gs_status merge_call(gs_merge* h, uint32_t form, const void* a, const void* av, uint32_t na, const void* b, const void* bv, uint32_t nb, void* out,
                     void* aux, uint32_t aux_bytes, bool with_vals, gs_key_type kt, gs_order order, void* stream) {
    if (!h) return GS_ERR_ARG;
    h->last_form = GS_MERGE_FORM_NONE;  // a refused call leaves no form behind
    const bool has_aux = form != GS_MERGE_FORM_KEYS;
    if ((na != 0 && (!a || misaligned(a))) || (nb != 0 && (!b || misaligned(b))) || !out || misaligned(out)) return GS_ERR_ARG;
    if (has_aux && (!aux || misaligned(aux))) return GS_ERR_ARG;
    if (with_vals && ((na != 0 && (!av || misaligned(av))) || (nb != 0 && (!bv || misaligned(bv))))) return GS_ERR_ARG;
    if (!(h->key_bytes == 8u ? is_key64_type(kt) : is_key32_type(kt)) || !valid_order(order)) return GS_ERR_ARG;
    if (with_vals && aux_bytes != 4u && aux_bytes != 8u) return GS_ERR_MODE;
    const uint64_t n64 = (uint64_t)na + nb;
    if (n64 == 0 || n64 > h->max_keys) return GS_ERR_SIZE;
    const uint32_t n = (uint32_t)n64;
    {  // no buffer of the call on another (an empty side has no bytes and overlaps nothing)
        const void* p[6] = {a, b, out, aux, av, bv};
        const size_t by[6] = {(size_t)na * h->key_bytes, (size_t)nb * h->key_bytes, (size_t)n * h->key_bytes, has_aux ? (size_t)n * aux_bytes : 0u,
                              with_vals ? (size_t)na * aux_bytes : 0u, with_vals ? (size_t)nb * aux_bytes : 0u};
        const void* q[6];
        size_t qb[6];
        int count = 0;
        for (int i = 0; i < 6; ++i)
            if (by[i] != 0) {
                q[count] = p[i];
                qb[count++] = by[i];
            }
        if (any_overlap(q, qb, count)) return GS_ERR_ARG;
    }
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no merge kernels
#if GS_SORT16_BUILT
    merge_plan(n, h->key_bytes, h->last_plan);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t kform = form == GS_MERGE_FORM_KEYS ? gs::MG_KEYS
                           : form == GS_MERGE_FORM_POSITIONS ? gs::MG_POSITIONS
                           : aux_bytes == 8u ? gs::MG_PAIRS8 : gs::MG_PAIRS4;
    hipLaunchKernelGGL(gs::mg_reset_kernel, dim3(1), dim3(gs::MGC_WORDS), 0, s, h->ws.ctl());
    if (h->key_bytes == 8u) merge_launch_form<uint64_t>(h, kform, a, na, b, nb, out, av, bv, aux, kt, order, s);
    else merge_launch_form<uint32_t>(h, kform, a, na, b, nb, out, av, bv, aux, kt, order, s);
    GS_HIP(hipGetLastError());
    h->last_form = form;
    h->last_na = na;
    h->last_nb = nb;
    return GS_OK;
#else
    (void)stream;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_merge_temp_bytes(uint32_t max_keys, uint32_t key_bytes) {
    if (!merge_sizes_ok(max_keys) || (key_bytes != 4u && key_bytes != 8u)) return 0;
    return merge_layout_bytes();
}

gs_status gs_merge_create(gs_merge** out, uint32_t max_keys, uint32_t key_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!merge_sizes_ok(max_keys)) return GS_ERR_SIZE;
    if (key_bytes != 4u && key_bytes != 8u) return GS_ERR_ARG;  // (2-byte keys: a follow-up)
    return handle_create(out, true, GS_MODE_KEYS_ONLY, 0u, [&](gs_merge* h) {
        h->max_keys = max_keys;
        h->key_bytes = key_bytes;
        return h->ws.alloc(merge_layout_bytes(), 0, gs::MGC_WORDS, gs::MGC_WORDS);
    });
}

gs_status gs_merge_destroy(gs_merge* h) { return handle_destroy(h); }

gs_status gs_merge_plan(uint32_t na, uint32_t nb, uint32_t key_bytes, uint32_t plan[GS_MERGE_PLAN_WORDS]) {
    if (!plan) return GS_ERR_ARG;
    const uint64_t n = (uint64_t)na + nb;
    if (n == 0 || n > GS_MAX_KEYS) return GS_ERR_SIZE;  // (sizes in front of the key width, as gs_merge_create)
    if (key_bytes != 4u && key_bytes != 8u) return GS_ERR_ARG;
    merge_plan((uint32_t)n, key_bytes, plan);
    return GS_OK;
}

gs_status gs_merge_keys(gs_merge* h, const void* d_a, uint32_t na, const void* d_b, uint32_t nb, void* d_out, gs_key_type key_type, gs_order order,
                        void* stream) {
    return merge_call(h, GS_MERGE_FORM_KEYS, d_a, nullptr, na, d_b, nullptr, nb, d_out, nullptr, 0u, false, key_type, order, stream);
}

gs_status gs_merge_pairs(gs_merge* h, const void* d_a_keys, const void* d_a_vals, uint32_t na, const void* d_b_keys, const void* d_b_vals, uint32_t nb,
                         void* d_out_keys, void* d_out_vals, uint32_t value_bytes, gs_key_type key_type, gs_order order, void* stream) {
    return merge_call(h, GS_MERGE_FORM_PAIRS, d_a_keys, d_a_vals, na, d_b_keys, d_b_vals, nb, d_out_keys, d_out_vals, value_bytes, true, key_type,
                      order, stream);
}

gs_status gs_merge_positions(gs_merge* h, const void* d_a, uint32_t na, const void* d_b, uint32_t nb, void* d_out_keys, void* d_out_src,
                             gs_key_type key_type, gs_order order, void* stream) {
    return merge_call(h, GS_MERGE_FORM_POSITIONS, d_a, nullptr, na, d_b, nullptr, nb, d_out_keys, d_out_src, 4u, false, key_type, order, stream);
}

gs_status gs_merge_last(gs_merge* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_MERGE_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_MERGE_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_MERGE_R_FORM] = h->last_form;
    if (h->last_form == GS_MERGE_FORM_NONE) return GS_OK;
    report[GS_MERGE_R_NA] = h->last_na;
    report[GS_MERGE_R_NB] = h->last_nb;
    for (uint32_t sh = 0; sh < gs::MGC_SHARDS; ++sh) {  // the counters are sharded over 128-byte lines (merge_kernels.hpp)
        report[GS_MERGE_R_TILES] += h->ws.pinned[sh * gs::MGC_STRIDE + gs::MGC_TILES];
        report[GS_MERGE_R_COPY_TILES] += h->ws.pinned[sh * gs::MGC_STRIDE + gs::MGC_COPY_TILES];
    }
    for (uint32_t i = 0; i < GS_MERGE_PLAN_WORDS; ++i) report[GS_MERGE_R_PLAN + i] = h->last_plan[i];
    return GS_OK;
}

}  // extern "C"
