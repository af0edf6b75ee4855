// segsort_host.hpp — part of the gpusort_capi.hip translation unit: the gs_segsort handle (segsort_kernels.hpp) and its entries.
// Replaces SplitSortAllocateTempMemory / SplitSortPairs / SplitSortFreeTempMemory (GPUSortingCUDA/SegSort/SplitSort/SplitSort.cuh:674-709).
// The handle's own: the engine, the two long routes and their buffers, the launches of the LDS classes (shared with the row-wise sort).
// The control block's allocation and read-back, the buffer predicates, the ping-pong and the head of a segmented call are
// handle_core.hpp's.
struct gs_segsort {
    uint32_t max_keys, max_segments;
    gs_mode mode;
    uint32_t value_bytes;
    gs_onesweep* engine = nullptr;  // long segments (and the rank mode of the workgroup classes)
    Workspace ws;                   // device: gs::SEGC_WORDS control words, then the class lists (max_segments words);
                                    // pinned: the control block + SEG_LONG_CHUNK list entries + a segment's two offsets (the host long route)
    bool long_failed = false;       // a long segment's engine call failed on the host side
    uint32_t long_route = GS_SEGSORT_LONG_HOST;
    char* long_dev = nullptr;       // the device route's buffers (seg_long_layout), from the first switch to it until destroy
    // the last call (gs_segsort_last)
    uint32_t last_route = 0, last_forms = 0, last_unit_cap = 0, last_n = 0;
};

static_assert(GS_SEGSORT_CLASSES == gs::SEG_CLASSES, "header and kernels agree on the classes");
static_assert(GS_SEGSORT_LONG_PASSES == gs::SR_PASSES && GS_SEGSORT_LONG_PASSES % 2u == 0 && GS_SEGSORT_LONG_PART % GS_SORT_ROWS_TILE == 0 &&
                  GS_SORT_ROWS_TILE == gs::SR_TILE,
              "header and kernels agree on the plan: a part is whole tiles, and an even number of passes ends in the caller's buffers");
namespace {
constexpr uint32_t SEG_LONG_CHUNK = 1024;  // long-list entries per read-back
inline uint32_t* seg_list(const gs_segsort* h) { return h->ws.ctl() + gs::SEGC_WORDS; }

// workgroups of a fixed-grid class kernel: what the chip holds at once (waves and LDS), never more than the class can have segments
uint32_t seg_grid(uint32_t bound, uint32_t waves, size_t lds_bytes) {
    uint32_t per_cu = 32u / waves;
    const uint32_t by_lds = (uint32_t)((160u * 1024u) / lds_bytes);
    if (by_lds < per_cu) per_cu = by_lds;
    if (per_cu == 0) per_cu = 1;
    const uint32_t g = cu_count() * per_cu;
    return bound < g ? (bound ? bound : 1u) : g;
}

// The launches of every class that fits LDS (0 .. 7, up to `top`): reset, classify, fill, packed, wave, workgroup classes.  ctl: a
// control block of gs::SEGC_WORDS words with the class lists behind it; rank_mode: the ranking of the workgroup classes.  No host
// wait.  Shared with the row-wise sort (sortrows_host.hpp), whose short rows are segments at uniform offsets.
gs_status seg_enqueue_lds(uint32_t* ctl, int rank_mode, uint32_t vb, uint32_t* keys, void* d_vals, uint32_t n, const uint32_t* d_offsets,
                          uint32_t num_segments, uint32_t max_len, uint32_t top, gs_key_type kt, uint32_t desc, hipStream_t s) {
    uint32_t* list = ctl + gs::SEGC_WORDS;
    seg_enqueue_head(ctl, d_offsets, num_segments, n, vb, max_len, top, s);
    const SegVbLaunchers& f = seg_vb(vb);
    if (top >= 1) f.packed(s, div_up(num_segments, 64), keys, d_vals, d_offsets, num_segments, max_len, (uint32_t)kt, desc, ctl);
    if (top >= 2 && n > gs::SEG_PACK_MAX)
        f.wave(s, seg_grid(seg_class_bound(n, num_segments, gs::SEG_PACK_MAX + 1), 1, gs::SEG_WAVE_MAX * (8 + vb)), keys, d_vals, d_offsets, list, ctl, num_segments,
               (uint32_t)kt, desc);
    for (uint32_t c = 3; c <= 7 && c <= top; ++c) {
        const uint32_t min_len = gs::SEG_CLASS_MAX[c - 1] + 1;
        if (n < min_len || gs::SEG_CLASS_MAX[c] > gs::seg_max_lds(vb)) continue;
        const Shape sh = g_small_class[c - 3];
        const SegWgLauncher wg = seg_wg_launcher((int)c - 3, rank_mode, vb, (int)kt);
        if (!wg) return GS_ERR_MODE;
        const uint32_t bound = seg_class_bound(n, num_segments, min_len);
        wg(s, SEG_WG_LOOP(sh.threads, sh.kpt) ? seg_grid(bound, (uint32_t)sh.threads / 64, seg_wg_lds_bytes(sh, vb)) : bound, keys, d_vals, d_offsets, list, ctl,
           num_segments, c, desc);
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// ---- long segments on the device: sizes shared with the 16-bit sort (segsort16_host.hpp), the part size as a parameter ----
// most long segments of a call, and the bound on its (segment, part) units: a segment of length len has at most len / part + 1 parts
uint32_t seg_long_cap(uint32_t n, uint32_t num_segments, uint32_t vb) {
    const uint32_t by_len = n / (gs::seg_max_lds(vb) + 1u);
    return by_len < num_segments ? by_len : num_segments;
}
uint32_t seg_long_units(uint32_t n, uint32_t num_segments, uint32_t vb, uint32_t part) { return n / part + seg_long_cap(n, num_segments, vb); }
bool seg_long_sizes_ok(uint32_t n, uint32_t num_segments, gs_mode mode, uint32_t vb) {
    return n != 0 && n <= GS_MAX_KEYS && num_segments != 0 && num_segments <= GS_MAX_KEYS && mode_value_ok(mode, vb);
}

struct SegLongLayout {
    size_t desc, rec, table, bases, total;
};
// desc: one uint4 per unit; rec: one uint4 per long segment; table, bases: units x 256 words each
SegLongLayout seg_long_layout(uint32_t max_keys, uint32_t max_segments, uint32_t vb) {
    SegLongLayout l{};
    Arena a;
    const size_t units = seg_long_units(max_keys, max_segments, vb, GS_SEGSORT_LONG_PART), longs = seg_long_cap(max_keys, max_segments, vb);
    l.desc = a.take(units * 16u);
    l.rec = a.take(longs * 16u);
    l.table = a.take(units * gs::RADIX * 4u);
    l.bases = a.take(units * gs::RADIX * 4u);
    l.total = a.total();
    return l;
}

#if GS_SORT_ROWS_BUILT
// the kernels are launched directly (no registry family; gs_segsort_last's forms word accounts for them)
using SegLongScatter = void (*)(hipStream_t, uint32_t grid, const uint32_t*, const void*, uint32_t*, void*, const uint4* desc, uint32_t unit_cap, uint32_t kt,
                                uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl);
template <int VB, int RANK>
void launch_segl_scatter(hipStream_t s, uint32_t grid, const uint32_t* kin, const void* vin, uint32_t* kout, void* vout, const uint4* desc, uint32_t unit_cap,
                         uint32_t kt, uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl) {
    hipLaunchKernelGGL((gs::segl_scatter_kernel<VB, RANK>), dim3(grid), dim3(gs::SR_THREADS), 0, s, kin, vin, kout, vout, desc, unit_cap, kt, shift, reverse,
                       bases, ctl);
}
constexpr auto g_segl_scatter = Table<2, 3>::make([](auto r, auto v) -> SegLongScatter { return launch_segl_scatter<VB_OF[v], r>; });  // [rank mode][vb index]

// The long segments of a call on the device route, behind seg_enqueue_lds: the work list, then four passes, ping-pong between the
// caller's buffers and the alternates.  No host wait.
gs_status seg_enqueue_long(gs_segsort* h, uint32_t* keys, void* vals, uint32_t* alt_keys, void* alt_vals, uint32_t n, const uint32_t* d_offsets,
                           uint32_t num_segments, uint32_t kt, bool descending, hipStream_t s) {
    const uint32_t vb = h->value_bytes, v = vb / 4u, rank = h->engine->rank_mode ? 1u : 0u;
    const SegLongLayout l = seg_long_layout(h->max_keys, h->max_segments, vb);
    const uint32_t unit_cap = seg_long_units(n, num_segments, vb, GS_SEGSORT_LONG_PART), long_cap = seg_long_cap(n, num_segments, vb);
    uint32_t* ctl = h->ws.ctl();
    uint4* desc4 = reinterpret_cast<uint4*>(h->long_dev + l.desc);
    uint4* rec = reinterpret_cast<uint4*>(h->long_dev + l.rec);
    uint32_t* table = reinterpret_cast<uint32_t*>(h->long_dev + l.table);
    uint32_t* bases = reinterpret_cast<uint32_t*>(h->long_dev + l.bases);
    h->last_unit_cap = unit_cap;
    hipLaunchKernelGGL(gs::seg16_units_kernel, dim3(div_up(long_cap, 256)), dim3(256), 0, s, d_offsets, seg_list(h), ctl, num_segments, GS_SEGSORT_LONG_PART,
                       unit_cap, long_cap, desc4, rec);
    h->last_forms |= GS_SEGSORT_LF_UNITS | GS_SEGSORT_LF_COUNT | GS_SEGSORT_LF_SCAN;
    for (uint32_t pass = 0; pass < GS_SEGSORT_LONG_PASSES; ++pass) {
        const bool last = pass + 1u == GS_SEGSORT_LONG_PASSES;
        const PingPong<uint32_t> b = ping_pong(pass, keys, vals, alt_keys, alt_vals);
        hipLaunchKernelGGL(gs::segl_count_kernel, dim3(unit_cap), dim3(gs::SR_THREADS), 0, s, b.kin, desc4, ctl, unit_cap, kt, pass * 8u, table);
        hipLaunchKernelGGL(gs::seg16_scan_kernel, dim3(long_cap), dim3(gs::RADIX), 0, s, table, bases, rec, ctl, unit_cap, long_cap);
        g_segl_scatter[Table<2, 3>::index({(int)rank, (int)v})](s, unit_cap, b.kin, b.vin, b.kout, b.vout, desc4, unit_cap, kt, pass * 8u,
                                                               (descending && last) ? 1u : 0u, bases, ctl);
    }
    h->last_forms |= GS_SEGSORT_LF_SCATTER << (2u * v + rank);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
#endif

gs_status segsort_impl(gs_segsort* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n, const uint32_t* d_offsets,
                       uint32_t num_segments, uint32_t max_len, gs_key_type kt, gs_order order, hipStream_t s, bool pairs) {
    if (!h || !d_keys || !d_offsets || misaligned(d_keys) || (reinterpret_cast<uintptr_t>(d_offsets) & 3u) || !is_key32_type(kt) || !valid_order(order))
        return GS_ERR_ARG;  // (64-bit key types: out of scope)
    if (pairs != (h->mode == GS_MODE_PAIRS)) return GS_ERR_MODE;
    if (pairs && (!d_vals || misaligned(d_vals))) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys || num_segments == 0 || num_segments > h->max_segments) return GS_ERR_SIZE;
    const uint32_t vb = h->value_bytes;
    const bool allow_long = max_len == 0u || max_len > gs::seg_max_lds(vb);
    if (allow_long && !alt_buffers_present(d_alt_keys, d_alt_vals, pairs)) return GS_ERR_ARG;
    if (allow_long && h->long_route == GS_SEGSORT_LONG_DEVICE && !alt_buffers_disjoint(d_keys, d_alt_keys, d_vals, d_alt_vals, n, 4u, vb, pairs))
        return GS_ERR_ARG;  // (the device route's passes read one buffer while they write the other)
    if (!SEG_BUILT) return GS_ERR_MODE;  // this build flavour has no segmented-sort kernels
    const uint32_t top = allow_long ? gs::SEG_CLASS_LONG : gs::seg_class_of(max_len, vb);  // the highest class a segment can fall in
    const uint32_t desc = order == GS_ORDER_DESCENDING ? 1u : 0u;
    uint32_t* keys = static_cast<uint32_t*>(d_keys);
    h->long_failed = false;
    h->last_route = h->long_route;
    h->last_forms = h->last_unit_cap = 0;
    h->last_n = n;
    const gs_status lds = seg_enqueue_lds(h->ws.ctl(), h->engine->rank_mode, vb, keys, d_vals, n, d_offsets, num_segments, max_len, top, kt, desc, s);
    if (lds != GS_OK) return lds;
    if (!allow_long || n <= gs::seg_max_lds(vb)) return GS_OK;
#if GS_SORT_ROWS_BUILT
    if (h->long_route == GS_SEGSORT_LONG_DEVICE)
        return seg_enqueue_long(h, keys, d_vals, static_cast<uint32_t*>(d_alt_keys), d_alt_vals, n, d_offsets, num_segments, (uint32_t)kt, desc != 0u, s);
#endif
    // ---- long segments: the one host wait.  Control block + the head of the long list (it starts the list array) ----
    const SegVbLaunchers& f = seg_vb(vb);
    const uint32_t by_len = n / (gs::seg_max_lds(vb) + 1), most = by_len < num_segments ? by_len : num_segments;  // long segments at most
    uint32_t* pinned = h->ws.pinned;
    const gs_status rd = h->ws.read_ctl(s, gs::SEGC_WORDS + (most < SEG_LONG_CHUNK ? most : SEG_LONG_CHUNK));
    if (rd != GS_OK) return rd;
    if (pinned[gs::SEGC_STATUS] & gs::SEG_ST_ARG) return GS_OK;  // reported by gs_segsort_check; nothing was sorted
    const uint32_t count = pinned[gs::SEGC_COUNT + gs::SEG_CLASS_LONG];
    if (count > most) return GS_ERR_HIP;  // (cannot happen: the classify kernel counted more long segments than n holds)
    char* vals = static_cast<char*>(d_vals);
    char* alt_vals = static_cast<char*>(d_alt_vals);
    uint32_t* alt_keys = static_cast<uint32_t*>(d_alt_keys);
    for (uint32_t first = 0; first < count; first += SEG_LONG_CHUNK) {
        const uint32_t chunk = count - first < SEG_LONG_CHUNK ? count - first : SEG_LONG_CHUNK;
        if (first != 0) {
            GS_HIP(hipMemcpyAsync(pinned + gs::SEGC_WORDS, seg_list(h) + first, chunk * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            GS_HIP(hipStreamSynchronize(s));
        }
        // the chunk's offsets: segment numbers come from the device's own (validated) classification
        uint32_t* bounds = pinned + gs::SEGC_WORDS + SEG_LONG_CHUNK;
        for (uint32_t i = 0; i < chunk; ++i) {
            const uint32_t seg = pinned[gs::SEGC_WORDS + i];
            if (seg >= num_segments) return GS_ERR_HIP;
            GS_HIP(hipMemcpyAsync(bounds, d_offsets + seg, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            GS_HIP(hipStreamSynchronize(s));
            const uint32_t start = bounds[0], end = bounds[1];
            if (end > n || start >= end) return GS_ERR_HIP;
            // the engine wants 16-byte aligned buffers: it sorts [start + head, end), seg_merge_head_kernel merges the head in
            const uint32_t head = (4u - (start & 3u)) & 3u, a = start + head, len = end - start;
            const gs_status st = engine_sort(h->engine, pairs, keys + a, vals + (size_t)a * vb, alt_keys + a, alt_vals + (size_t)a * vb, len - head, kt, order, s);
            if (st != GS_OK) { h->long_failed = true; return st; }
            if (head != 0) {
                const uint32_t grid = div_up(len, 256 * 8);
                f.merge_head(s, grid < 4096 ? grid : 4096, keys, d_vals, alt_keys, d_alt_vals, start, head, len, (uint32_t)kt, desc);
                GS_HIP(hipMemcpyAsync(keys + start, alt_keys + start, (size_t)len * 4, hipMemcpyDeviceToDevice, s));
                if (pairs) GS_HIP(hipMemcpyAsync(vals + (size_t)start * vb, alt_vals + (size_t)start * vb, (size_t)len * vb, hipMemcpyDeviceToDevice, s));
            }
        }
    }
    return GS_OK;
}
}  // namespace

extern "C" {

size_t gs_segsort_temp_bytes(uint32_t max_keys, uint32_t max_segments) {
    return gs_onesweep_temp_bytes(max_keys) + ((size_t)gs::SEGC_WORDS + max_segments) * sizeof(uint32_t);
}
uint32_t gs_segsort_class_of(uint32_t length, gs_mode mode, uint32_t value_bytes) {
    return gs::seg_class_of(length, mode == GS_MODE_PAIRS ? value_bytes : 0);
}
uint32_t gs_segsort_max_lds_segment(gs_mode mode, uint32_t value_bytes) { return gs::seg_max_lds(mode == GS_MODE_PAIRS ? value_bytes : 0); }

uint32_t gs_segsort_long_units(uint32_t n, uint32_t num_segments, gs_mode mode, uint32_t value_bytes) {
    return seg_long_sizes_ok(n, num_segments, mode, value_bytes) ? seg_long_units(n, num_segments, value_bytes, GS_SEGSORT_LONG_PART) : 0u;
}
size_t gs_segsort_long_temp_bytes(uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes) {
    return seg_long_sizes_ok(max_keys, max_segments, mode, value_bytes) ? seg_long_layout(max_keys, max_segments, value_bytes).total : 0;
}

gs_status gs_segsort_create(gs_segsort** out, uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (max_segments == 0 || max_segments > GS_MAX_KEYS) return GS_ERR_SIZE;
    gs_onesweep* engine = nullptr;
    const gs_status st = gs_onesweep_create(&engine, max_keys, mode, value_bytes);  // checks max_keys, mode and value width
    if (st != GS_OK) return st;
    gs_segsort* h = new (std::nothrow) gs_segsort();
    if (!h) { (void)gs_onesweep_destroy(engine); return GS_ERR_ARG; }
    h->max_keys = max_keys;
    h->max_segments = max_segments;
    h->mode = mode;
    h->value_bytes = value_bytes;
    h->engine = engine;
    const gs_status ws = h->ws.alloc(((size_t)gs::SEGC_WORDS + max_segments) * sizeof(uint32_t), 0, gs::SEGC_WORDS, gs::SEGC_WORDS + SEG_LONG_CHUNK + 2);
    if (ws != GS_OK) {
        (void)gs_segsort_destroy(h);  // the engine with it
        return ws;
    }
    *out = h;
    return GS_OK;
}

gs_status gs_segsort_destroy(gs_segsort* h) {
    if (!h) return GS_ERR_ARG;
    h->ws.release();
    if (h->long_dev) (void)hipFree(h->long_dev);
    if (h->engine) (void)gs_onesweep_destroy(h->engine);
    delete h;
    return GS_OK;
}

gs_status gs_segsort_sort_keys(gs_segsort* h, void* d_keys, void* d_alt, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments,
                               uint32_t max_segment_len, gs_key_type key_type, gs_order order, void* stream) {
    return segsort_impl(h, d_keys, nullptr, d_alt, nullptr, n, d_offsets, num_segments, max_segment_len, key_type, order,
                        static_cast<hipStream_t>(stream), false);
}

gs_status gs_segsort_sort_pairs(gs_segsort* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n,
                                const uint32_t* d_offsets, uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type, gs_order order,
                                void* stream) {
    return segsort_impl(h, d_keys, d_vals, d_alt_keys, d_alt_vals, n, d_offsets, num_segments, max_segment_len, key_type, order,
                        static_cast<hipStream_t>(stream), true);
}

gs_status gs_segsort_check(gs_segsort* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    const uint32_t st = h->ws.pinned[gs::SEGC_STATUS];
    if (st & gs::SEG_ST_ARG) return GS_ERR_ARG;
    if (h->long_failed || h->ws.pinned[gs::SEG16C_INTERNAL] != 0u) return GS_ERR_HIP;  // (the word is the device route's: a long segment's counts did not add up)
    if (st & gs::SEG_ST_SIZE) return GS_ERR_SIZE;
    return gs_onesweep_check(h->engine, stream);  // the long segments' sorts
}

gs_onesweep* gs_segsort_engine(gs_segsort* h) { return h ? h->engine : nullptr; }

gs_status gs_segsort_set_long_route(gs_segsort* h, uint32_t route) {
    if (!h || (route != GS_SEGSORT_LONG_HOST && route != GS_SEGSORT_LONG_DEVICE)) return GS_ERR_ARG;
    if (route == GS_SEGSORT_LONG_DEVICE) {
        if (!GS_SORT_ROWS_BUILT) return GS_ERR_MODE;  // this build flavour has no pass kernels
        if (!h->long_dev) {
            const hipError_t e = hipMalloc(&h->long_dev, seg_long_layout(h->max_keys, h->max_segments, h->value_bytes).total);
            if (e != hipSuccess) {
                g_last_hip_error = (int)e;
                h->long_dev = nullptr;
                return GS_ERR_HIP;
            }
        }
    }
    h->long_route = route;
    return GS_OK;
}

uint32_t gs_segsort_get_long_route(gs_segsort* h) { return h ? h->long_route : 0xffffffffu; }

gs_status gs_segsort_last(gs_segsort* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SEGSORT_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SEGSORT_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_SEGSORT_R_ROUTE] = h->last_route;
    if (h->last_route == GS_SEGSORT_LONG_DEVICE) {
        report[GS_SEGSORT_R_UNITS] = h->ws.pinned[gs::SEG16C_UNITS];
        report[GS_SEGSORT_R_UNIT_CAP] = h->last_unit_cap;
        report[GS_SEGSORT_R_FORMS] = h->last_forms;
    }
    report[GS_SEGSORT_R_LONG] = h->ws.pinned[gs::SEGC_COUNT + gs::SEG_CLASS_LONG];
    report[GS_SEGSORT_R_STATUS] = h->ws.pinned[gs::SEGC_STATUS] | (h->ws.pinned[gs::SEG16C_INTERNAL] != 0u ? 256u : 0u);
    report[GS_SEGSORT_R_RANK] = (uint32_t)h->engine->rank_mode;
    report[GS_SEGSORT_R_N] = h->last_n;
    return GS_OK;
}

gs_status gs_segsort_last_classes(gs_segsort* h, uint32_t* counts, uint32_t words, void* stream) {
    if (!h || !counts || words < GS_SEGSORT_CLASSES + 1) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t c = 0; c < GS_SEGSORT_CLASSES; ++c) counts[c] = h->ws.pinned[gs::SEGC_COUNT + c];
    counts[GS_SEGSORT_CLASSES] = h->ws.pinned[gs::SEGC_MAXLEN];
    return GS_OK;
}

}  // extern "C"
