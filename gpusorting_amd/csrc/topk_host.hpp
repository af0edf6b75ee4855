// topk_host.hpp — part of the gpusort_capi.hip translation unit: the gs_topk handle (topk_kernels.hpp) and its entries.
// The handle's own: the engine, the 1-D routes, the row-wise routes and the LOOP route's staging.  The layout arena and the control
// block's allocation and read-back are handle_core.hpp's.  No counterpart in the reference project.
struct gs_topk {
    uint32_t max_keys, max_k, sort_cap;
    gs_mode mode;
    uint32_t value_bytes;
    gs_onesweep* engine = nullptr;  // the final sort of the k selected elements (and the single-tile route's sort)
    Workspace ws;                   // one allocation: see topk_layout
    uint32_t last_route = GS_TOPK_ROUTE_NONE, last_flip = 0;
    bool sort_failed = false;       // the engine refused a call on the host side
    // the last row-wise call (gs_topk_rows_last)
    uint32_t rows_route = GS_TOPK_ROWS_ROUTE_NONE, rows_rows = 0, rows_len = 0, rows_k = 0;
    char* loop_stage = nullptr;     // GS_TOPK_ROWS_ROUTE_LOOP: aligned copies of a row and of its output (loop_stage_layout): allocated
                                    // once, at the handle's largest size, by the first call that needs it; freed by destroy only
};

namespace {
// Large k: there is no full-sort route — the select route serves every k <= n, at k = n it is a partition that keeps everything
// followed by the sort; the measured rows for k = 2^20 are in DESIGN.md 3.9.  What the single-tile route takes is the one routing
// constant: n up to the single-tile sort's capacity for the value width (one launch instead of eleven).
inline uint32_t topk_single_max(uint32_t vb) { return gs::seg_max_lds(vb); }
constexpr uint32_t TOPK_SINGLE_MAX_ANY = 32768;  // the largest of them (keys only): bounds the handle's sort capacity

struct TopkLayout {
    size_t ctl, extra, sums, rc, slices, cand_keys, cand_vals, alt_keys, alt_vals, total;
};
inline size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }
inline uint32_t topk_sort_cap(uint32_t max_keys, uint32_t max_k) {
    const uint32_t small = max_keys < TOPK_SINGLE_MAX_ANY ? max_keys : TOPK_SINGLE_MAX_ANY;
    return max_k > small ? max_k : small;
}
TopkLayout topk_layout(uint32_t max_keys, uint32_t max_k, uint32_t vb) {
    TopkLayout l{};
    const size_t cap = topk_sort_cap(max_keys, max_k);
    Arena a;
    l.ctl = a.take(gs::TKC_WORDS * 4u);
    l.extra = a.take(2u * gs::TK_BINS * 4u);
    l.sums = a.take(gs::TK_BINS * 4u);
    l.rc = a.take(2u * 2u * gs::TK_MAX_RANGES * 4u);
    l.slices = a.take((size_t)gs::TK_MAX_RANGES * gs::TK_SLICE_WORDS * 4u);
    l.cand_keys = a.take((size_t)max_keys * 4u);
    l.cand_vals = a.take((size_t)max_keys * vb);
    l.alt_keys = a.take(cap * 4u);
    l.alt_vals = a.take(cap * vb);
    l.total = a.total();
    return l;
}

using TkScatter = void (*)(hipStream_t, const uint32_t* src, const void* src_vals, uint32_t* ctl, uint32_t level, uint32_t kt, uint32_t flip,
                           const uint32_t* rc, uint32_t* out, void* out_vals, uint32_t k, uint32_t* cand, void* cand_vals, uint32_t cand_cap);
template <int VM>
void launch_tk_scatter(hipStream_t s, const uint32_t* src, const void* src_vals, uint32_t* ctl, uint32_t level, uint32_t kt, uint32_t flip,
                       const uint32_t* rc, uint32_t* out, void* out_vals, uint32_t k, uint32_t* cand, void* cand_vals, uint32_t cand_cap) {
    hipLaunchKernelGGL((gs::tk_scatter_kernel<VM>), dim3(gs::TK_MAX_RANGES), dim3(gs::TK_THREADS), 0, s, src, src_vals, ctl, level, kt, flip, rc,
                       out, out_vals, k, cand, cand_vals, cand_cap);
}
inline TkScatter tk_scatter(uint32_t vm) {
    return vm == 0 ? launch_tk_scatter<0> : vm == 1 ? launch_tk_scatter<1> : vm == 4 ? launch_tk_scatter<4> : launch_tk_scatter<8>;
}

gs_status topk_run(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals,
                   gs_key_type kt, gs_order order, hipStream_t s, bool pairs);

gs_status topk_impl(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals,
                    gs_key_type kt, gs_order order, hipStream_t s, bool pairs) {
    if (!h || !d_keys || !d_out_keys || misaligned(d_keys) || misaligned(d_out_keys) || !is_key32_type(kt) || !valid_order(order))
        return GS_ERR_ARG;  // (64-bit key types: out of scope)
    if (pairs != (h->mode == GS_MODE_PAIRS)) return GS_ERR_MODE;
    const uint32_t vb = h->value_bytes;
    const bool pos = pairs && !d_vals;  // the value is the element's position
    if (pairs && (!d_out_vals || misaligned(d_out_vals) || (pos ? vb != 4u : misaligned(d_vals)))) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys || k == 0 || k > n || k > h->max_k) return GS_ERR_SIZE;
    if (buffers_overlap(d_keys, (size_t)n * 4u, d_out_keys, (size_t)k * 4u) ||
        (pairs && !pos && buffers_overlap(d_vals, (size_t)n * vb, d_out_vals, (size_t)k * vb)))
        return GS_ERR_ARG;
    if (!TK_BUILT) return GS_ERR_MODE;  // this build flavour has no selection
    return topk_run(h, d_keys, d_vals, n, k, d_out_keys, d_out_vals, kt, order, s, pairs);
}

// the 1-D routes on checked arguments (the row-wise LOOP route calls it row by row: there the values need element alignment only)
gs_status topk_run(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals,
                   gs_key_type kt, gs_order order, hipStream_t s, bool pairs) {
    const uint32_t vb = h->value_bytes;
    const bool pos = pairs && !d_vals;
    const TopkLayout l = topk_layout(h->max_keys, h->max_k, vb);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    uint32_t* cand_keys = reinterpret_cast<uint32_t*>(h->ws.dev + l.cand_keys);
    void* cand_vals = h->ws.dev + l.cand_vals;
    uint32_t* alt_keys = reinterpret_cast<uint32_t*>(h->ws.dev + l.alt_keys);
    void* alt_vals = h->ws.dev + l.alt_vals;
    const uint32_t* keys = static_cast<const uint32_t*>(d_keys);
    uint32_t* out = static_cast<uint32_t*>(d_out_keys);
    h->sort_failed = false;
    h->last_route = GS_TOPK_ROUTE_NONE;
    auto sort = [&](uint32_t* sk, void* sv, uint32_t m) {
        const gs_status st = engine_sort(h->engine, pairs, sk, sv, alt_keys, alt_vals, m, kt, order, s);
        if (st != GS_OK) h->sort_failed = true;
        return st;
    };
    if (n <= topk_single_max(vb)) {  // one tile: sort a copy, emit the head
        GS_HIP(hipMemcpyAsync(cand_keys, keys, (size_t)n * 4u, hipMemcpyDeviceToDevice, s));
        if (pos) hipLaunchKernelGGL(gs::tk_iota_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, static_cast<uint32_t*>(cand_vals), n);
        else if (pairs) GS_HIP(hipMemcpyAsync(cand_vals, d_vals, (size_t)n * vb, hipMemcpyDeviceToDevice, s));
        GS_HIP(hipGetLastError());
        const gs_status st = sort(cand_keys, cand_vals, n);
        if (st != GS_OK) return st;
        GS_HIP(hipMemcpyAsync(out, cand_keys, (size_t)k * 4u, hipMemcpyDeviceToDevice, s));
        if (pairs) GS_HIP(hipMemcpyAsync(d_out_vals, cand_vals, (size_t)k * vb, hipMemcpyDeviceToDevice, s));
        h->last_route = GS_TOPK_ROUTE_SINGLE_TILE;
        return GS_OK;
    }
    uint32_t* extra = reinterpret_cast<uint32_t*>(h->ws.dev + l.extra);
    uint32_t* sums = reinterpret_cast<uint32_t*>(h->ws.dev + l.sums);
    uint32_t* rc = reinterpret_cast<uint32_t*>(h->ws.dev + l.rc);
    uint32_t* slices = reinterpret_cast<uint32_t*>(h->ws.dev + l.slices);
    const uint32_t flip = order == GS_ORDER_DESCENDING ? 0xffffffffu : 0u, ktu = (uint32_t)kt;
    hipLaunchKernelGGL(gs::tk_init_kernel, dim3(2u * gs::TK_BINS / 4u / 256u), dim3(256), 0, s, ctl, extra, n, k);
    for (uint32_t level = 0; level < 2; ++level) {
        const uint32_t* src = level == 0 ? keys : cand_keys;
        const void* src_vals = level == 0 ? d_vals : cand_vals;
        // level 1 of the position mode makes the index the value; level 2 carries it as a 4-byte value
        const uint32_t vm = !pairs ? 0u : (pos && level == 0) ? 1u : vb;
        hipLaunchKernelGGL(gs::tk_hist_kernel, dim3(gs::TK_MAX_RANGES), dim3(gs::TK_THREADS), 0, s, src, ctl, level, ktu, flip, slices, extra);
        hipLaunchKernelGGL(gs::tk_reduce_kernel, dim3(gs::TK_TABLE_WORDS / 256u), dim3(256), 0, s, slices, ctl, level, extra, sums);
        hipLaunchKernelGGL(gs::tk_threshold_kernel, dim3(1), dim3(1024), 0, s, sums, ctl, level);
        hipLaunchKernelGGL(gs::tk_rangecount_kernel, dim3(gs::TK_MAX_RANGES), dim3(256), 0, s, src, slices, ctl, level, ktu, flip, rc);
        tk_scatter(vm)(s, src, src_vals, ctl, level, ktu, flip, rc, out, d_out_vals, k, cand_keys, cand_vals, h->max_keys);
    }
    GS_HIP(hipGetLastError());
    h->last_route = GS_TOPK_ROUTE_SELECT;
    h->last_flip = flip;
    return sort(out, d_out_vals, k);
}

// ---- row-wise selection (topk_rows_kernels.hpp) ---------------------------------------------------------------------------------
// Routes by row length, then k: WAVE and TILE sort the row in LDS and take every k; STREAM takes k <= TKR_STAGE; LOOP, everything
// else, is the 1-D select route enqueued row by row: rows x (its eleven launches, the final sort, one status launch), still without
// a host round trip.  The 2-byte key types (is_key16; these two entries only) take the same routes on the kernels of
// topk_rows16_kernels.hpp, LOOP excepted.

// The staging of the LOOP route, sized by the handle alone so that it is never regrown: a captured graph holds its address for as long
// as the handle lives.  Only calls of two rows and more stage, and their rows are at most max_keys / 2 long
// ((rows - 1) * row_stride + row_len <= max_keys with row_stride >= row_len).
struct LoopStage {
    size_t outk, outv, total;  // (the row's copy lies at 0)
};
inline LoopStage loop_stage_layout(const gs_topk* h) {
    const size_t row = h->max_keys / 2u, k = h->max_k < row ? h->max_k : row;
    LoopStage l{};
    l.outk = up16(row * 4u);
    l.outv = l.outk + up16(k * 4u);
    l.total = l.outv + up16(k * h->value_bytes);
    return l;
}

gs_status rows_loop(gs_topk* h, const uint32_t* keys, const char* vals, uint32_t rows, uint32_t row_len, uint32_t row_stride, uint32_t k,
                    uint32_t* out_keys, char* out_vals, gs_key_type kt, gs_order order, hipStream_t s, bool pairs) {
    // The 1-D kernels load the keys 16 bytes at a time and the engine sorts the output in place: a row or an output row that starts
    // off a 16-byte boundary goes through an aligned copy.  The first call that needs the staging allocates it (synchronously, and
    // not while the stream is capturing: GS_ERR_MODE then, with the capture left intact); no later call frees or moves it.
    const uint32_t vb = h->value_bytes;
    const LoopStage l = loop_stage_layout(h);
    const bool staged = rows > 1 && (((row_stride | k) & 3u) != 0);
    if (staged && !h->loop_stage) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        GS_HIP(hipStreamIsCapturing(s, &cap));
        if (cap != hipStreamCaptureStatusNone) return GS_ERR_MODE;
        GS_HIP(hipMalloc(&h->loop_stage, l.total));
    }
    uint32_t* ctl = h->ws.ctl();
    hipLaunchKernelGGL(gs::tkr_reset_kernel, dim3(1), dim3(64), 0, s, ctl);  // (the status gathered over the rows starts at 0)
    char* st_in = h->loop_stage;
    char* st_outk = h->loop_stage + l.outk;
    char* st_outv = h->loop_stage + l.outv;
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t* rk = keys + (size_t)r * row_stride;
        const char* rv = vals ? vals + (size_t)r * row_stride * vb : nullptr;
        uint32_t* ok = out_keys + (size_t)r * k;
        char* ov = pairs ? out_vals + (size_t)r * k * vb : nullptr;
        const bool in_staged = misaligned(rk), out_staged = misaligned(ok) || (pairs && misaligned(ov));
        if (in_staged) GS_HIP(hipMemcpyAsync(st_in, rk, (size_t)row_len * 4u, hipMemcpyDeviceToDevice, s));
        const gs_status st = topk_run(h, in_staged ? static_cast<const void*>(st_in) : rk, rv, row_len, k, out_staged ? static_cast<void*>(st_outk) : ok,
                                      pairs ? (out_staged ? static_cast<void*>(st_outv) : ov) : nullptr, kt, order, s, pairs);
        if (st != GS_OK) return st;
        if (out_staged) {
            GS_HIP(hipMemcpyAsync(ok, st_outk, (size_t)k * 4u, hipMemcpyDeviceToDevice, s));
            if (pairs) GS_HIP(hipMemcpyAsync(ov, st_outv, (size_t)k * vb, hipMemcpyDeviceToDevice, s));
        }
        // every row's 1-D call starts from a clean control block: its status joins the call's, which the last row leaves in TKC_STATUS
        hipLaunchKernelGGL(gs::tkr_status_kernel, dim3(1), dim3(64), 0, s, ctl);
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

gs_status rows_impl(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t rows, uint32_t row_len, uint32_t row_stride, uint32_t k,
                    void* d_out_keys, void* d_out_vals, gs_key_type kt, gs_order order, hipStream_t s, bool pairs) {
    const bool key16 = is_key16(kt);  // 2-byte elements in d_keys and d_out_keys (topk_rows16_kernels.hpp)
    if (!h || !d_keys || !d_out_keys || misaligned(d_keys) || misaligned(d_out_keys) || !(is_key32_type(kt) || key16) || !valid_order(order))
        return GS_ERR_ARG;  // (64-bit key types: out of scope)
    if (pairs != (h->mode == GS_MODE_PAIRS)) return GS_ERR_MODE;
    const uint32_t vb = h->value_bytes, kb = key16 ? 2u : 4u;
    const bool pos = pairs && !d_vals;  // the value is the element's position in its row
    if (pairs && (!d_out_vals || misaligned(d_out_vals) || (pos ? vb != 4u : misaligned(d_vals)))) return GS_ERR_ARG;
    if (rows == 0 || row_len == 0 || k == 0 || k > row_len || k > h->max_k) return GS_ERR_SIZE;
    if (row_stride < row_len) return GS_ERR_ARG;
    const unsigned long long extent = (unsigned long long)(rows - 1u) * row_stride + row_len;
    if (extent > h->max_keys) return GS_ERR_SIZE;
    const size_t out_elems = (size_t)rows * k;
    if (buffers_overlap(d_keys, (size_t)extent * kb, d_out_keys, out_elems * kb) ||
        (pairs && !pos && buffers_overlap(d_vals, (size_t)extent * vb, d_out_vals, out_elems * vb)))
        return GS_ERR_ARG;
    if (!TK_BUILT) return GS_ERR_MODE;  // this build flavour has no selection
    h->sort_failed = false;
    h->last_route = GS_TOPK_ROUTE_NONE;
    h->rows_route = GS_TOPK_ROWS_ROUTE_NONE;
    h->rows_rows = rows;
    h->rows_len = row_len;
    h->rows_k = k;
    uint32_t* ctl = h->ws.ctl();
    // few, very long rows: one workgroup per row leaves the other CUs idle, and the 1-D route row by row is faster.  Measured (DESIGN.md
    // 3.10): STREAM costs 0.415 ms per 2^20 elements of a row, LOOP 0.078 ms + 0.022 ms per 2^20 elements for every row; LOOP where
    // rows * (0.078 + 0.022 L) <= 0.415 L, in integers below, for the row lengths that were measured (2^19 and up)
    const bool few_long = row_len >= (1u << 19) && (unsigned long long)rows * ((unsigned long long)row_len + (7ull << 19)) <= 19ull * row_len;
    // 2-byte keys have no LOOP route (the 1-D select is a 32-bit algorithm): every k <= TKR_STAGE of a long row takes STREAM, few, very
    // long rows included (unmeasured there), and a larger k is refused before anything is launched
    const uint32_t route = row_len <= gs::SEG_WAVE_MAX ? GS_TOPK_ROWS_ROUTE_WAVE : row_len <= gs::seg_max_lds(vb) ? GS_TOPK_ROWS_ROUTE_TILE
                           : k <= gs::TKR_STAGE && (key16 || !few_long) ? GS_TOPK_ROWS_ROUTE_STREAM : GS_TOPK_ROWS_ROUTE_LOOP;
    if (route == GS_TOPK_ROWS_ROUTE_LOOP) {
        if (key16) return GS_ERR_SIZE;
        const gs_status st = rows_loop(h, static_cast<const uint32_t*>(d_keys), static_cast<const char*>(d_vals), rows, row_len, row_stride, k,
                                       static_cast<uint32_t*>(d_out_keys), static_cast<char*>(d_out_vals), kt, order, s, pairs);
        if (st == GS_OK) h->rows_route = route;
        return st;
    }
    const gs::TkrArgs a{static_cast<const uint32_t*>(d_keys), d_vals, static_cast<uint32_t*>(d_out_keys), d_out_vals, rows, row_len, row_stride, k,
                        (uint32_t)kt, order == GS_ORDER_DESCENDING ? 1u : 0u, ctl};
    const uint32_t vm = !pairs ? 0u : pos ? 1u : vb;
    hipLaunchKernelGGL(gs::tkr_reset_kernel, dim3(1), dim3(64), 0, s, ctl);
    if (route == GS_TOPK_ROWS_ROUTE_WAVE) {
        tkr_vm(key16, vm).wave(s, div_up(rows, gs::TKR_WAVE_ROWS), a);
    } else if (route == GS_TOPK_ROWS_ROUTE_TILE) {
        const TkrLauncher f = tkr_tile_launcher(key16, (int)gs::seg_class_of(row_len, vb) - 3, h->engine->rank_mode, vm);
        if (!f) return GS_ERR_MODE;
        f(s, rows, a);
    } else {
        tkr_vm(key16, vm).stream(s, rows, a);
    }
    GS_HIP(hipGetLastError());
    h->rows_route = route;
    return GS_OK;
}
}  // namespace

extern "C" {

size_t gs_topk_temp_bytes(uint32_t max_keys, uint32_t max_k, uint32_t value_bytes) {
    return topk_layout(max_keys, max_k, value_bytes).total + gs_onesweep_temp_bytes(topk_sort_cap(max_keys, max_k));
}

gs_status gs_topk_create(gs_topk** out, uint32_t max_keys, uint32_t max_k, gs_mode mode, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (max_keys == 0 || max_keys > GS_MAX_KEYS || max_k == 0 || max_k > max_keys) return GS_ERR_SIZE;
    gs_onesweep* engine = nullptr;
    const uint32_t cap = topk_sort_cap(max_keys, max_k);
    const gs_status st = gs_onesweep_create(&engine, cap, mode, value_bytes);  // checks mode and value width
    if (st != GS_OK) return st;
    gs_topk* h = new (std::nothrow) gs_topk();
    if (!h) { (void)gs_onesweep_destroy(engine); return GS_ERR_ARG; }
    h->max_keys = max_keys;
    h->max_k = max_k;
    h->sort_cap = cap;
    h->mode = mode;
    h->value_bytes = mode == GS_MODE_PAIRS ? value_bytes : 0u;
    h->engine = engine;
    const TopkLayout l = topk_layout(max_keys, max_k, h->value_bytes);
    const gs_status ws = h->ws.alloc(l.total, l.ctl, gs::TKC_WORDS, gs::TKC_WORDS);
    if (ws != GS_OK) {
        (void)gs_topk_destroy(h);  // the engine with it
        return ws;
    }
    *out = h;
    return GS_OK;
}

gs_status gs_topk_destroy(gs_topk* h) {
    if (!h) return GS_ERR_ARG;
    h->ws.release();
    if (h->loop_stage) (void)hipFree(h->loop_stage);
    if (h->engine) (void)gs_onesweep_destroy(h->engine);
    delete h;
    return GS_OK;
}

gs_status gs_topk_select_keys(gs_topk* h, const void* d_keys, uint32_t n, uint32_t k, void* d_out_keys, gs_key_type key_type, gs_order order,
                              void* stream) {
    return topk_impl(h, d_keys, nullptr, n, k, d_out_keys, nullptr, key_type, order, static_cast<hipStream_t>(stream), false);
}

gs_status gs_topk_select_pairs(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys, void* d_out_vals,
                               gs_key_type key_type, gs_order order, void* stream) {
    return topk_impl(h, d_keys, d_vals, n, k, d_out_keys, d_out_vals, key_type, order, static_cast<hipStream_t>(stream), true);
}

gs_status gs_topk_select_rows_keys(gs_topk* h, const void* d_keys, uint32_t rows, uint32_t row_len, uint32_t row_stride, uint32_t k,
                                   void* d_out_keys, gs_key_type key_type, gs_order order, void* stream) {
    return rows_impl(h, d_keys, nullptr, rows, row_len, row_stride, k, d_out_keys, nullptr, key_type, order, static_cast<hipStream_t>(stream), false);
}

gs_status gs_topk_select_rows_pairs(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t rows, uint32_t row_len, uint32_t row_stride,
                                    uint32_t k, void* d_out_keys, void* d_out_vals, gs_key_type key_type, gs_order order, void* stream) {
    return rows_impl(h, d_keys, d_vals, rows, row_len, row_stride, k, d_out_keys, d_out_vals, key_type, order, static_cast<hipStream_t>(stream), true);
}

uint32_t gs_topk_rows_max_k(gs_mode mode, uint32_t value_bytes) {
    if (mode == GS_MODE_KEYS_ONLY) return gs::TKR_STAGE;
    return mode == GS_MODE_PAIRS && (value_bytes == 4u || value_bytes == 8u) ? gs::TKR_STAGE : 0u;  // (values are fetched by position: no LDS of theirs)
}

gs_status gs_topk_rows_last(gs_topk* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_TOPK_ROWS_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_TOPK_ROWS_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_TOPK_ROWS_R_ROUTE] = h->rows_route;
    report[GS_TOPK_ROWS_R_ROWS] = h->rows_rows;
    report[GS_TOPK_ROWS_R_ROW_LEN] = h->rows_len;
    report[GS_TOPK_ROWS_R_K] = h->rows_k;
    report[GS_TOPK_ROWS_R_STATUS] = h->ws.pinned[gs::TKC_STATUS];
    if (h->rows_route == GS_TOPK_ROWS_ROUTE_STREAM) report[GS_TOPK_ROWS_R_READS] = h->ws.pinned[gs::TKR_CTL_READS];
    return GS_OK;
}

gs_onesweep* gs_topk_engine(gs_topk* h) { return h ? h->engine : nullptr; }

gs_status gs_topk_check(gs_topk* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    if (h->sort_failed || (h->ws.pinned[gs::TKC_STATUS] & gs::TK_ST_INTERNAL)) return GS_ERR_HIP;
    return gs_onesweep_check(h->engine, stream);  // the final sort
}

gs_status gs_topk_last(gs_topk* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_TOPK_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_TOPK_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_TOPK_R_ROUTE] = h->last_route;
    if (h->last_route != GS_TOPK_ROUTE_SELECT) return GS_OK;
    const uint32_t* l1 = h->ws.pinned + gs::TKC_LEVEL;
    const uint32_t* l2 = l1 + gs::TKL_WORDS;
    report[GS_TOPK_R_THRESHOLD] = ((l1[gs::TKL_BIN] << 16) | l2[gs::TKL_BIN]) ^ h->last_flip;
    report[GS_TOPK_R_IN_FRONT] = l1[gs::TKL_FRONT] + l2[gs::TKL_FRONT];
    report[GS_TOPK_R_EQUAL] = l2[gs::TKL_EQUAL];
    report[GS_TOPK_R_TAKEN] = l2[gs::TKL_TAKE];
    report[GS_TOPK_R_CANDIDATES] = l1[gs::TKL_EQUAL];
    report[GS_TOPK_R_LEVEL2] = 1u;  // the select route always runs both levels
    report[GS_TOPK_R_RANGES] = l1[gs::TKL_RANGES] | (l2[gs::TKL_RANGES] << 16);
    return GS_OK;
}

}  // extern "C"
