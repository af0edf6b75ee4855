// segsort16_host.hpp — part of the gpusort_capi.hip translation unit: the gs_segsort16 handle (segsort16_kernels.hpp) and its
// entries: the layout, the launchers, every launch of a call and the reports.  Allocation, create/destroy, the control read-back, the
// rank mode, the buffer predicate, the ping-pong and the head of a segmented call are handle_core.hpp's.  No counterpart in the
// reference project.
struct gs_segsort16 {
    uint32_t max_keys, max_segments;
    gs_mode mode;
    uint32_t value_bytes;
    int rank_mode;               // the ranking of the workgroup classes and of the long route's scatter (probed at create)
    Workspace ws;                // one allocation: see segsort16_layout
    // the last call (gs_segsort16_last)
    uint32_t last_forms = 0, last_wg_forms = 0, last_unit_cap = 0, last_n = 0;
};

namespace {
static_assert(GS_SEGSORT16_PASSES == gs::SR16_PASSES && GS_SEGSORT16_PART % GS_SORT_ROWS_TILE == 0 && GS_SORT_ROWS_TILE == gs::SR_TILE,
              "header and kernels agree on the plan: a part is whole tiles");

// most long segments of a call and the bound on its (segment, part) units: seg_long_cap / seg_long_units / seg_long_sizes_ok of
// segsort_host.hpp, shared with the 32-bit sort's device route, with this sort's part
uint32_t segsort16_long_cap(uint32_t n, uint32_t num_segments, uint32_t vb) { return seg_long_cap(n, num_segments, vb); }
uint32_t segsort16_units(uint32_t n, uint32_t num_segments, uint32_t vb) { return seg_long_units(n, num_segments, vb, GS_SEGSORT16_PART); }
bool segsort16_sizes_ok(uint32_t n, uint32_t num_segments, gs_mode mode, uint32_t vb) { return seg_long_sizes_ok(n, num_segments, mode, vb); }

struct SegSort16Layout {
    size_t ctl, desc, rec, table, bases, total;
};
// ctl: the segmented sort's control block with the class lists behind it; desc: one uint4 per unit; rec: one uint4 per long segment;
// table, bases: units x 256 words each
SegSort16Layout segsort16_layout(uint32_t max_keys, uint32_t max_segments, uint32_t vb) {
    SegSort16Layout l{};
    Arena a;
    const size_t units = segsort16_units(max_keys, max_segments, vb), longs = segsort16_long_cap(max_keys, max_segments, vb);
    l.ctl = a.take(((size_t)gs::SEGC_WORDS + max_segments) * 4u);
    l.desc = a.take(units * 16u);
    l.rec = a.take(longs * 16u);
    l.table = a.take(units * gs::RADIX * 4u);
    l.bases = a.take(units * gs::RADIX * 4u);
    l.total = a.total();
    return l;
}

#if GS_SORT_ROWS_BUILT
// ---- launchers: the new kernels are launched directly (no registry family; gs_segsort16_last's forms words account for them) ----
struct Seg16VmLaunchers {
    void (*packed)(hipStream_t, uint32_t grid, uint16_t* keys, void* vals, const uint32_t* off, uint32_t num_segments, uint32_t max_len, uint32_t kt,
                   uint32_t descending, const uint32_t* ctl);
    void (*wave)(hipStream_t, uint32_t grid, uint16_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
                 uint32_t num_segments, uint32_t kt, uint32_t descending);
};
template <int VM>
constexpr Seg16VmLaunchers seg16_vm_launchers() {
    return {[](hipStream_t s, uint32_t grid, uint16_t* keys, void* vals, const uint32_t* off, uint32_t num_segments, uint32_t max_len, uint32_t kt,
               uint32_t descending, const uint32_t* ctl) {
                hipLaunchKernelGGL((gs::seg16_packed_kernel<VM>), dim3(grid), dim3(64), 0, s, keys, vals, off, num_segments, max_len, kt, descending, ctl);
            },
            [](hipStream_t s, uint32_t grid, uint16_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
               uint32_t num_segments, uint32_t kt, uint32_t descending) {
                hipLaunchKernelGGL((gs::seg16_wave_kernel<VM>), dim3(grid), dim3(64), 0, s, keys, vals, off, list, ctl, num_segments, kt, descending);
            }};
}
constexpr auto g_seg16_vm = Table<4>::make([](auto v) -> Seg16VmLaunchers { return seg16_vm_launchers<VM_OF[v]>(); });  // [vm index]

using Seg16WgLauncher = void (*)(hipStream_t, uint32_t grid, uint16_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
                                 uint32_t num_segments, uint32_t cls, uint32_t kt, uint32_t descending);
template <int T, int K, int VM, int RANK>
void launch_seg16_wg(hipStream_t s, uint32_t grid, uint16_t* keys, void* vals, const uint32_t* off, const uint32_t* list, const uint32_t* ctl,
                     uint32_t num_segments, uint32_t cls, uint32_t kt, uint32_t descending) {
    hipLaunchKernelGGL((gs::seg16_wg_kernel<T, K, VM, RANK, SEG_WG_LOOP(T, K)>), dim3(grid), dim3(T), 0, s, keys, vals, off, list, ctl, num_segments, cls,
                       kt, descending);
}
// workgroup class c runs on g_small_class[c] with the value modes that shape holds, as the row-wise top-k's tile kernel (tkr_tile_built)
using Seg16WgTable = Table<5, 2, 4>;  // [workgroup class][rank mode][vm index]
constexpr auto g_seg16_wg = Seg16WgTable::make([](auto c, auto r, auto v) -> Seg16WgLauncher {
    if constexpr (tkr_tile_built(c, VM_OF[v])) return launch_seg16_wg<g_small_class[c].threads, g_small_class[c].kpt, VM_OF[v], r>;
    else return nullptr;
});

using Seg16Scatter = void (*)(hipStream_t, uint32_t grid, const uint16_t*, const void*, uint16_t*, void*, const uint4* desc, uint32_t unit_cap, uint32_t kt,
                              uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl);
template <int VM, int RANK>
void launch_seg16_scatter(hipStream_t s, uint32_t grid, const uint16_t* kin, const void* vin, uint16_t* kout, void* vout, const uint4* desc, uint32_t unit_cap,
                          uint32_t kt, uint32_t shift, uint32_t reverse, const uint32_t* bases, uint32_t* ctl) {
    hipLaunchKernelGGL((gs::seg16_scatter_kernel<VM, RANK>), dim3(grid), dim3(gs::SR_THREADS), 0, s, kin, vin, kout, vout, desc, unit_cap, kt, shift, reverse,
                       bases, ctl);
}
constexpr auto g_seg16_scatter = Table<2, 4>::make([](auto r, auto v) -> Seg16Scatter { return launch_seg16_scatter<VM_OF[v], r>; });  // [rank mode][vm index]

// every launch of a call.  vm: 0 keys only, 1 positions (argsort), 4, 8
gs_status segsort16_enqueue(gs_segsort16* h, const SegSort16Layout& l, uint16_t* keys, void* vals, uint16_t* alt_keys, void* alt_vals, uint32_t n,
                            const uint32_t* d_offsets, uint32_t num_segments, uint32_t max_len, uint32_t top, bool allow_long, uint32_t kt, bool descending,
                            uint32_t vm, hipStream_t s) {
    const uint32_t vb = h->value_bytes, v = (uint32_t)vm_index(vm), desc = descending ? 1u : 0u, rank = h->rank_mode ? 1u : 0u;
    uint32_t* ctl = reinterpret_cast<uint32_t*>(h->ws.dev + l.ctl);
    uint32_t* list = ctl + gs::SEGC_WORDS;
    seg_enqueue_head(ctl, d_offsets, num_segments, n, vb, max_len, top, s);
    h->last_forms = GS_SEGSORT16_F_CLASSIFY | (top >= 2 ? GS_SEGSORT16_F_FILL : 0u);
    const Seg16VmLaunchers& f = g_seg16_vm[v];
    if (top >= 1 || vm == 1u) {  // (the argsort form writes the position of a segment of one element)
        f.packed(s, div_up(num_segments, 64), keys, vals, d_offsets, num_segments, max_len, kt, desc, ctl);
        h->last_forms |= GS_SEGSORT16_F_PACKED << v;
    }
    if (top >= 2 && n > gs::SEG_PACK_MAX) {
        f.wave(s, seg_grid(seg_class_bound(n, num_segments, gs::SEG_PACK_MAX + 1), 1, gs::SEG_WAVE_MAX * (8 + (vm == 1u ? 4u : vm))), keys, vals, d_offsets, list,
               ctl, num_segments, kt, desc);
        h->last_forms |= GS_SEGSORT16_F_WAVE << v;
    }
    for (uint32_t c = 3; c <= 7 && c <= top; ++c) {
        const uint32_t min_len = gs::SEG_CLASS_MAX[c - 1] + 1;
        if (n < min_len || gs::SEG_CLASS_MAX[c] > gs::seg_max_lds(vb)) continue;
        const Shape sh = g_small_class[c - 3];
        const Seg16WgLauncher wg = g_seg16_wg[Seg16WgTable::index({(int)c - 3, (int)rank, (int)v})];
        if (!wg) return GS_ERR_MODE;
        const uint32_t bound = seg_class_bound(n, num_segments, min_len);
        wg(s, SEG_WG_LOOP(sh.threads, sh.kpt) ? seg_grid(bound, (uint32_t)sh.threads / 64, seg_wg_lds_bytes(sh, vb)) : bound, keys, vals, d_offsets, list, ctl,
           num_segments, c, kt, desc);
        h->last_wg_forms |= GS_SEGSORT16_WG_FORM(c, v, rank);
    }
    // ---- long segments: the work list, then two passes, the low byte into the alternates, the high byte back ----
    if (allow_long && n > gs::seg_max_lds(vb)) {
        const uint32_t unit_cap = segsort16_units(n, num_segments, vb), long_cap = segsort16_long_cap(n, num_segments, vb);
        uint4* desc4 = reinterpret_cast<uint4*>(h->ws.dev + l.desc);
        uint4* rec = reinterpret_cast<uint4*>(h->ws.dev + l.rec);
        uint32_t* table = reinterpret_cast<uint32_t*>(h->ws.dev + l.table);
        uint32_t* bases = reinterpret_cast<uint32_t*>(h->ws.dev + l.bases);
        h->last_unit_cap = unit_cap;
        hipLaunchKernelGGL(gs::seg16_units_kernel, dim3(div_up(long_cap, 256)), dim3(256), 0, s, d_offsets, list, ctl, num_segments, GS_SEGSORT16_PART, unit_cap,
                           long_cap, desc4, rec);
        h->last_forms |= GS_SEGSORT16_F_UNITS | GS_SEGSORT16_F_COUNT | GS_SEGSORT16_F_SCAN;
        for (uint32_t pass = 0; pass < gs::SR16_PASSES; ++pass) {
            const bool fwd = pass == 0u;
            const PingPong<uint16_t> b = ping_pong(pass, keys, vals, alt_keys, alt_vals);
            const uint32_t pv = (uint32_t)vm_index((vm == 1u && !fwd) ? 4u : vm);  // the argsort's second pass carries the positions as 4-byte values
            hipLaunchKernelGGL(gs::seg16_count_kernel, dim3(unit_cap), dim3(gs::SR_THREADS), 0, s, b.kin, desc4, ctl, unit_cap, kt, pass * 8u, table);
            hipLaunchKernelGGL(gs::seg16_scan_kernel, dim3(long_cap), dim3(gs::RADIX), 0, s, table, bases, rec, ctl, unit_cap, long_cap);
            g_seg16_scatter[Table<2, 4>::index({(int)rank, (int)pv})](s, unit_cap, b.kin, b.vin, b.kout, b.vout, desc4, unit_cap, kt, pass * 8u,
                                                                     (descending && !fwd) ? 1u : 0u, bases, ctl);
            h->last_forms |= GS_SEGSORT16_F_SCATTER << (2u * pv + rank);
        }
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}
#endif

// what: 0 keys, 1 pairs, 2 argsort.  The order of the checks is sort_rows16_impl's.
gs_status segsort16_impl(gs_segsort16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n, const uint32_t* d_offsets,
                         uint32_t num_segments, uint32_t max_len, gs_key_type kt, gs_order order, hipStream_t s, int what) {
    if (!h || !d_keys || misaligned(d_keys) || !d_offsets || (reinterpret_cast<uintptr_t>(d_offsets) & 3u) || !is_key16(kt) || !valid_order(order))
        return GS_ERR_ARG;  // (32- and 64-bit key types: gs_segsort_*, out of scope)
    const bool pairs = what != 0;
    if (pairs != (h->mode == GS_MODE_PAIRS) || (what == 2 && h->value_bytes != 4u)) return GS_ERR_MODE;
    if (pairs && (!d_vals || misaligned(d_vals))) return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys || num_segments == 0 || num_segments > h->max_segments) return GS_ERR_SIZE;
    const uint32_t vb = h->value_bytes;
    const bool allow_long = max_len == 0u || max_len > gs::seg_max_lds(vb);
    if (allow_long && !alt_buffers_ok(d_keys, d_alt_keys, d_vals, d_alt_vals, n, 2u, vb, pairs)) return GS_ERR_ARG;
    if (!SR_BUILT) return GS_ERR_MODE;  // this build flavour has no segmented sort
#if GS_SORT_ROWS_BUILT
    const uint32_t top = allow_long ? gs::SEG_CLASS_LONG : gs::seg_class_of(max_len, vb);  // the highest class a segment can fall in
    h->last_forms = h->last_wg_forms = h->last_unit_cap = 0;
    h->last_n = n;
    return segsort16_enqueue(h, segsort16_layout(h->max_keys, h->max_segments, vb), static_cast<uint16_t*>(d_keys), d_vals, static_cast<uint16_t*>(d_alt_keys),
                             d_alt_vals, n, d_offsets, num_segments, max_len, top, allow_long, (uint32_t)kt, order == GS_ORDER_DESCENDING,
                             what == 0 ? 0u : what == 2 ? 1u : vb, s);
#else
    (void)s; (void)d_alt_keys; (void)d_alt_vals; (void)d_vals; (void)max_len; (void)allow_long;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

uint32_t gs_segsort16_units(uint32_t n, uint32_t num_segments, gs_mode mode, uint32_t value_bytes) {
    return segsort16_sizes_ok(n, num_segments, mode, value_bytes) ? segsort16_units(n, num_segments, value_bytes) : 0u;
}

size_t gs_segsort16_temp_bytes(uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes) {
    return segsort16_sizes_ok(max_keys, max_segments, mode, value_bytes) ? segsort16_layout(max_keys, max_segments, value_bytes).total : 0;
}

gs_status gs_segsort16_create(gs_segsort16** out, uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes) {
    const bool sizes_ok = max_keys != 0 && max_keys <= GS_MAX_KEYS && max_segments != 0 && max_segments <= GS_MAX_KEYS;
    return handle_create(out, sizes_ok, mode, value_bytes, [&](gs_segsort16* h) {
        h->max_keys = max_keys;
        h->max_segments = max_segments;
        const SegSort16Layout l = segsort16_layout(max_keys, max_segments, value_bytes);
        return h->ws.alloc(l.total, l.ctl, gs::SEGC_WORDS, gs::SEGC_WORDS);
    });
}

gs_status gs_segsort16_destroy(gs_segsort16* h) { return handle_destroy(h); }

gs_status gs_segsort16_sort_keys(gs_segsort16* h, void* d_keys, void* d_alt, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments,
                                 uint32_t max_segment_len, gs_key_type key_type, gs_order order, void* stream) {
    return segsort16_impl(h, d_keys, nullptr, d_alt, nullptr, n, d_offsets, num_segments, max_segment_len, key_type, order, static_cast<hipStream_t>(stream), 0);
}

gs_status gs_segsort16_sort_pairs(gs_segsort16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n, const uint32_t* d_offsets,
                                  uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type, gs_order order, void* stream) {
    return segsort16_impl(h, d_keys, d_vals, d_alt_keys, d_alt_vals, n, d_offsets, num_segments, max_segment_len, key_type, order,
                          static_cast<hipStream_t>(stream), 1);
}

gs_status gs_segsort16_argsort(gs_segsort16* h, void* d_keys, void* d_pos, void* d_alt_keys, void* d_alt_pos, uint32_t n, const uint32_t* d_offsets,
                               uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type, gs_order order, void* stream) {
    return segsort16_impl(h, d_keys, d_pos, d_alt_keys, d_alt_pos, n, d_offsets, num_segments, max_segment_len, key_type, order,
                          static_cast<hipStream_t>(stream), 2);
}

gs_status gs_segsort16_check(gs_segsort16* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    const uint32_t st = h->ws.pinned[gs::SEGC_STATUS];
    if (st & gs::SEG_ST_ARG) return GS_ERR_ARG;
    if (h->ws.pinned[gs::SEG16C_INTERNAL] != 0u) return GS_ERR_HIP;
    if (st & gs::SEG_ST_SIZE) return GS_ERR_SIZE;
    return GS_OK;
}

gs_status gs_segsort16_last_classes(gs_segsort16* h, uint32_t* counts, uint32_t words, void* stream) {
    if (!h || !counts || words < GS_SEGSORT_CLASSES + 1) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t c = 0; c < GS_SEGSORT_CLASSES; ++c) counts[c] = h->ws.pinned[gs::SEGC_COUNT + c];
    counts[GS_SEGSORT_CLASSES] = h->ws.pinned[gs::SEGC_MAXLEN];
    return GS_OK;
}

gs_status gs_segsort16_last(gs_segsort16* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_SEGSORT16_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_SEGSORT16_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_SEGSORT16_R_UNITS] = h->ws.pinned[gs::SEG16C_UNITS];
    report[GS_SEGSORT16_R_FORMS] = h->last_forms;
    report[GS_SEGSORT16_R_WG_FORMS] = h->last_wg_forms;
    report[GS_SEGSORT16_R_STATUS] = h->ws.pinned[gs::SEGC_STATUS] | (h->ws.pinned[gs::SEG16C_INTERNAL] != 0u ? 256u : 0u);
    report[GS_SEGSORT16_R_RANK] = (uint32_t)h->rank_mode;
    report[GS_SEGSORT16_R_LONG] = h->ws.pinned[gs::SEGC_COUNT + gs::SEG_CLASS_LONG];
    report[GS_SEGSORT16_R_UNIT_CAP] = h->last_unit_cap;
    report[GS_SEGSORT16_R_N] = h->last_n;
    return GS_OK;
}

gs_status gs_segsort16_set_rank_mode(gs_segsort16* h, int mode) { return handle_set_rank_mode(h, mode); }

int gs_segsort16_get_rank_mode(gs_segsort16* h) { return handle_get_rank_mode(h); }

}  // extern "C"
