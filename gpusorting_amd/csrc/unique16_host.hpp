// unique16_host.hpp — part of the gpusort_capi.hip translation unit: the gs_unique16 handle (unique16_kernels.hpp) and its entries:
// the layout, the two routes and the report.  Allocation, the create frame and the control read-back are handle_core.hpp's; the
// histogram's plan is sort16_host.hpp's, the run-length stage's unique_host.hpp's.  No counterpart in the reference project.
struct gs_unique16 {
    uint32_t max_keys = 0;
    gs_mode mode = GS_MODE_KEYS_ONLY;  // (handle_core's frame: one handle kind)
    uint32_t value_bytes = 0;
    int rank_mode = 0;
    Workspace ws;  // one allocation: see unique16_layout; the control block lies at its start, the histogram directly behind it
    uint32_t inverse_form = GS_UNIQUE16_INVERSE_AUTO;  // gs_unique16_set_inverse_form
    uint32_t last_route = GS_UNIQUE16_ROUTE_NONE, last_n = 0, last_ran = 0, last_plan[4] = {0u, 0u, 0u, 0u}, last_first_ranges = 0,
             last_inverse_ranges = 0;
};

namespace {
struct Unique16Layout {
    size_t ctl, hist, first, rank, rc, rl, base, prev, total;
};
// Nothing here grows with max_keys: the 65 536-bin histogram is the exact answer.
Unique16Layout unique16_layout() {
    Unique16Layout l{};
    Arena a;
    l.ctl = a.take(gs::UQC_WORDS * 4u);
    l.hist = a.take(gs::S16_BINS * 4u);
    l.first = a.take(gs::S16_BINS * 4u);
    l.rank = a.take(gs::S16_BINS * 2u);
    l.rc = a.take(gs::UQ_CAP * 4u);
    l.rl = a.take(gs::UQ_CAP * 4u);
    l.base = a.take(gs::UQ_CAP * 4u);
    l.prev = a.take(gs::UQ_CAP * 4u);
    l.total = a.total();
    return l;
}
inline bool unique16_sizes_ok(uint32_t max_keys) { return max_keys != 0 && max_keys <= GS_MAX_KEYS; }
// ranges of at least `min_tiles` whole tiles, at most `cap` of them: elements per range
inline uint32_t unique16_per_range(uint32_t n, uint32_t cap, uint32_t min_tiles) {
    const uint32_t tiles = div_up(div_up(n, cap), gs::U16_TILE);
    return (tiles < min_tiles ? min_tiles : tiles) * gs::U16_TILE;
}

// consecutive: the input as it lies
gs_status unique16_impl(gs_unique16* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first, void* d_out_inverse,
                        void* d_out_num, gs_key_type kt, gs_order order, hipStream_t s, bool consecutive) {
    if (!h) return GS_ERR_ARG;
    h->last_route = GS_UNIQUE16_ROUTE_NONE;  // a refused call leaves no route behind
    if (!d_keys || !d_out_keys || misaligned(d_keys) || misaligned(d_out_keys)) return GS_ERR_ARG;
    if (!consecutive && (!is_key16(kt) || !valid_order(order))) return GS_ERR_ARG;
    if ((d_out_counts && misaligned(d_out_counts)) || (d_out_first && misaligned(d_out_first)) || (d_out_inverse && misaligned(d_out_inverse)) ||
        (reinterpret_cast<uintptr_t>(d_out_num) & 3u) != 0)
        return GS_ERR_ARG;
    if (n == 0 || n > h->max_keys) return GS_ERR_SIZE;
    {  // no buffer of the call on another: outputs at their capacities, one word at d_out_num; a null pointer takes no room
        const size_t cap = consecutive || n < gs::S16_BINS ? n : gs::S16_BINS;
        const void* p[6] = {d_keys, d_out_keys, d_out_counts, d_out_first, d_out_inverse, d_out_num};
        const size_t b[6] = {(size_t)n * 2u, cap * 2u, d_out_counts ? cap * 4u : 0u, d_out_first ? cap * 4u : 0u, d_out_inverse ? (size_t)n * 4u : 0u,
                             d_out_num ? 4u : 0u};
        for (int i = 0; i < 6; ++i)
            for (int j = i + 1; j < 6; ++j)
                if (b[i] && b[j] && buffers_overlap(p[i], b[i], p[j], b[j])) return GS_ERR_ARG;
    }
    if (!S16_BUILT) return GS_ERR_MODE;  // this build flavour has no 16-bit kernels
#if GS_SORT16_BUILT
    const Unique16Layout l = unique16_layout();
    char* dev = h->ws.dev;
    uint32_t* ctl = h->ws.ctl();
    const uint16_t* keys = static_cast<const uint16_t*>(d_keys);
    uint16_t* out_keys = static_cast<uint16_t*>(d_out_keys);
    uint32_t* out_counts = static_cast<uint32_t*>(d_out_counts);
    uint32_t* out_first = static_cast<uint32_t*>(d_out_first);
    uint32_t* out_inverse = static_cast<uint32_t*>(d_out_inverse);
    uint32_t* out_num = static_cast<uint32_t*>(d_out_num);
    h->last_n = n;
    h->last_ran = h->last_first_ranges = h->last_inverse_ranges = 0;
    if (consecutive) {  // count, scan, compact: every grid is the plan's, a function of n alone
        uint32_t* rc = reinterpret_cast<uint32_t*>(dev + l.rc);
        uint32_t* rl = reinterpret_cast<uint32_t*>(dev + l.rl);
        uint32_t* base = reinterpret_cast<uint32_t*>(dev + l.base);
        uint32_t* prev = reinterpret_cast<uint32_t*>(dev + l.prev);
        unique_plan(n, h->last_plan);
        h->last_plan[3] = gs::UQ_CAP;
        const uint32_t ranges = h->last_plan[0], per = h->last_plan[1];
        hipLaunchKernelGGL(gs::u16_count_kernel, dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, n, per, rc, rl);
        hipLaunchKernelGGL(gs::uq_scan_kernel, dim3(1), dim3(gs::UQ_CAP), 0, s, rc, rl, ranges, n, base, prev, out_num, ctl);
        hipLaunchKernelGGL(gs::u16_compact_kernel, dim3(ranges), dim3(gs::UQ_THREADS), 0, s, keys, n, per, base, prev, rc, out_keys, out_counts, out_inverse,
                           ctl);
        GS_HIP(hipGetLastError());
        h->last_route = GS_UNIQUE16_ROUTE_CONSECUTIVE;
        return GS_OK;
    }
    uint32_t* hist = reinterpret_cast<uint32_t*>(dev + l.hist);
    uint32_t* first = reinterpret_cast<uint32_t*>(dev + l.first);
    uint16_t* rank = reinterpret_cast<uint16_t*>(dev + l.rank);
    const uint32_t flip = order == GS_ORDER_DESCENDING ? 0xffffu : 0u, ktu = (uint32_t)kt;
    sort16_plan(n, false, h->last_plan);
    const uint32_t clear_groups = (uint32_t)((l.first - l.ctl) / 16u);  // the control block and the histogram behind it
    hipLaunchKernelGGL(gs::s16_clear_kernel, dim3(div_up(clear_groups, 256)), dim3(256), 0, s, reinterpret_cast<uint4*>(ctl), clear_groups);
    if (out_first) hipLaunchKernelGGL(gs::u16_fill_kernel, dim3(gs::S16_BINS / 4u / 256u), dim3(256), 0, s, reinterpret_cast<uint4*>(first), gs::S16_BINS / 4u);
    hipLaunchKernelGGL(gs::s16_hist_kernel, dim3(2u * h->last_plan[0]), dim3(gs::S16_KTHREADS), 0, s, keys, n, h->last_plan[1], ktu, flip, hist);
    if (out_first) {
        const uint32_t per = unique16_per_range(n, gs::U16_FCAP, gs::U16_FMIN_TILES);
        h->last_first_ranges = div_up(n, per);
        hipLaunchKernelGGL(gs::u16_first_kernel, dim3(h->last_first_ranges), dim3(gs::U16_THREADS), 0, s, keys, n, per, ktu, flip, first);
        h->last_ran |= GS_UNIQUE16_K_FIRST;
    }
    hipLaunchKernelGGL(gs::u16_rank_kernel, dim3(1), dim3(gs::S16_KTHREADS), 0, s, hist, first, n, ktu, flip, rank, out_keys, out_counts, out_first, out_num, ctl);
    if (out_inverse) {
        const bool lds = h->inverse_form == GS_UNIQUE16_INVERSE_LDS || (h->inverse_form == GS_UNIQUE16_INVERSE_AUTO && n >= GS_UNIQUE16_INVERSE_LDS_MIN);
        h->last_inverse_ranges = div_up(n, gs::U16_TILE);
        if (lds) {
            const uint32_t per = unique16_per_range(n, gs::U16_ICAP, gs::U16_IMIN_TILES);
            h->last_inverse_ranges = div_up(n, per);
            hipLaunchKernelGGL(gs::u16_inverse_kernel<true>, dim3(h->last_inverse_ranges), dim3(gs::U16_THREADS), 0, s, keys, n, per, ktu, flip, rank, out_inverse, ctl);
        } else {  // ranges of one tile
            hipLaunchKernelGGL(gs::u16_inverse_kernel<false>, dim3(div_up(n, gs::U16_TILE)), dim3(gs::U16_THREADS), 0, s, keys, n, gs::U16_TILE, ktu, flip, rank,
                               out_inverse, ctl);
        }
        h->last_ran |= lds ? GS_UNIQUE16_K_INVERSE_LDS : GS_UNIQUE16_K_INVERSE_GATHER;
    }
    GS_HIP(hipGetLastError());
    h->last_route = GS_UNIQUE16_ROUTE_HISTOGRAM;
    return GS_OK;
#else
    (void)s;
    return GS_ERR_MODE;
#endif
}
}  // namespace

extern "C" {

size_t gs_unique16_temp_bytes(uint32_t max_keys) { return unique16_sizes_ok(max_keys) ? unique16_layout().total : 0; }

gs_status gs_unique16_create(gs_unique16** out, uint32_t max_keys) {
    return handle_create(out, unique16_sizes_ok(max_keys), GS_MODE_KEYS_ONLY, 0u, [&](gs_unique16* h) {
        h->max_keys = max_keys;
        const Unique16Layout l = unique16_layout();
        return h->ws.alloc(l.total, l.ctl, gs::UQC_WORDS, gs::UQC_WORDS);
    });
}

gs_status gs_unique16_destroy(gs_unique16* h) { return handle_destroy(h); }

gs_status gs_unique16_unique(gs_unique16* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first, void* d_out_inverse,
                             void* d_out_num, gs_key_type key_type, gs_order order, void* stream) {
    return unique16_impl(h, d_keys, n, d_out_keys, d_out_counts, d_out_first, d_out_inverse, d_out_num, key_type, order, static_cast<hipStream_t>(stream), false);
}

gs_status gs_unique16_consecutive(gs_unique16* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_inverse, void* d_out_num,
                                  void* stream) {
    return unique16_impl(h, d_keys, n, d_out_keys, d_out_counts, nullptr, d_out_inverse, d_out_num, GS_KEY_UINT16, GS_ORDER_ASCENDING,
                         static_cast<hipStream_t>(stream), true);
}

gs_status gs_unique16_check(gs_unique16* h, void* stream) {
    if (!h) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    const uint32_t* c = h->ws.pinned;
    return ((c[gs::UQC_STATUS] & gs::UQ_ST_INTERNAL) || c[gs::UQC_U] != c[gs::UQC_WRITTEN]) ? GS_ERR_HIP : GS_OK;
}

gs_status gs_unique16_last(gs_unique16* h, uint32_t* report, uint32_t words, void* stream) {
    if (!h || !report || words < GS_UNIQUE16_REPORT_WORDS) return GS_ERR_ARG;
    const gs_status rd = h->ws.read_ctl(static_cast<hipStream_t>(stream));
    if (rd != GS_OK) return rd;
    for (uint32_t i = 0; i < GS_UNIQUE16_REPORT_WORDS; ++i) report[i] = 0;
    report[GS_UNIQUE16_R_ROUTE] = h->last_route;
    report[GS_UNIQUE16_R_STATUS] = h->ws.pinned[gs::UQC_STATUS];
    if (h->last_route == GS_UNIQUE16_ROUTE_NONE) return GS_OK;
    report[GS_UNIQUE16_R_N] = h->last_n;
    report[GS_UNIQUE16_R_U] = h->ws.pinned[gs::UQC_U];
    report[GS_UNIQUE16_R_RAN] = h->last_ran;
    report[GS_UNIQUE16_R_RANGES] = h->last_plan[0];
    report[GS_UNIQUE16_R_PER_RANGE] = h->last_plan[1];
    report[GS_UNIQUE16_R_TILE] = h->last_plan[2];
    report[GS_UNIQUE16_R_FIRST_RANGES] = h->last_first_ranges;
    report[GS_UNIQUE16_R_INVERSE_RANGES] = h->last_inverse_ranges;
    return GS_OK;
}

gs_status gs_unique16_set_inverse_form(gs_unique16* h, uint32_t which) {
    if (!h || which > GS_UNIQUE16_INVERSE_GATHER) return GS_ERR_ARG;
    h->inverse_form = which;
    return GS_OK;
}

}  // extern "C"
