// topk_seg16_host.hpp — part of the gpusort_capi.hip translation unit: the gs_segtopk16 handle (topk_seg16_kernels.hpp) and its
// entries.  No counterpart in the reference project.
//
// A gs_segtopk16 is a gs_segtopk (topk_seg_host.hpp): the same control block, class lists, report and rank mode; nothing in the
// handle depends on the key width.  What differs is decided per call by a TksRoutes: 2-byte elements in the overlap checks, the four
// 16-bit key types, and the kernels of topk_seg16_kernels.hpp on the grids segtopk_impl computes.  The handle type is its own so
// that a caller cannot hand a 32-bit handle's entries 2-byte keys or the reverse without a cast.
namespace {
inline gs_segtopk* tks16_handle(gs_segtopk16* h) { return reinterpret_cast<gs_segtopk*>(h); }

// The kernels of 1024 threads — the tile shapes 1024 x 16 and 1024 x 32 and the stream kernel — take one workgroup per slot their class
// can have (n / the class's shortest length) instead of a grid-stride loop over the list, as the 1024 x 32 shape does in every
// handle: inside the loop tks16_tile_kernel<1024, 16, 1 / 4, 0> spilled one VGPR and tks16_stream_kernel four to seven to scratch,
// without it they take the registers of tkr16_tile_kernel and tkr16_stream_kernel and no scratch.
constexpr bool tks16_tile_loops(int threads, int) { return threads < 1024; }

// the kernels are launched directly (no registry family; gs_segtopk16_last's forms word accounts for them)
template <int VM>
void launch_tks16_packed(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t) {
    hipLaunchKernelGGL((gs::tks16_packed_kernel<VM>), dim3(grid), dim3(64), 0, s, a);
}
template <int VM>
void launch_tks16_wave(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t) {
    hipLaunchKernelGGL((gs::tks16_wave_kernel<VM>), dim3(grid), dim3(64 * gs::TKR_WAVE_ROWS), 0, s, a);
}
template <int VM>
void launch_tks16_stream(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t) {
    hipLaunchKernelGGL((gs::tks16_stream_kernel<VM, 0>), dim3(grid), dim3(gs::TKR_THREADS), 0, s, a);  // (RANK 0, as tkr16_stream_kernel)
}
template <int T, int K, int VM, int RANK>
void launch_tks16_tile(hipStream_t s, uint32_t grid, const gs::TksArgs& a, uint32_t cls) {
    hipLaunchKernelGGL((gs::tks16_tile_kernel<T, K, VM, RANK, tks16_tile_loops(T, K)>), dim3(grid), dim3(T), 0, s, a, cls);
}
constexpr auto g_tks16_vm = Table<4>::make([](auto v) -> TksVmLaunchers {  // [vm index]
    if constexpr (TK_BUILT) return TksVmLaunchers{launch_tks16_packed<VM_OF[v]>, launch_tks16_wave<VM_OF[v]>, launch_tks16_stream<VM_OF[v]>};
    else return TksVmLaunchers{nullptr, nullptr, nullptr};
});
constexpr auto g_tks16_tile = TksTileTable::make([](auto c, auto r, auto v) -> TksLauncher {  // the cells of g_tks_tile
    if constexpr (tkr_tile_built(c, VM_OF[v])) return launch_tks16_tile<g_small_class[c].threads, g_small_class[c].kpt, VM_OF[v], r>;
    else return nullptr;
});
constexpr TksRoutes g_tks_routes16{2u, g_tks16_vm.data(), g_tks16_tile.data(), tks16_tile_loops, false};
}  // namespace

extern "C" {

size_t gs_segtopk16_temp_bytes(uint32_t max_segments) { return segtopk_bytes(max_segments); }

gs_status gs_segtopk16_create(gs_segtopk16** out, uint32_t max_keys, uint32_t max_segments, uint32_t max_k, gs_mode mode, uint32_t value_bytes) {
    if (!out) return GS_ERR_ARG;
    gs_segtopk* h = nullptr;
    const gs_status st = gs_segtopk_create(&h, max_keys, max_segments, max_k, mode, value_bytes);
    *out = reinterpret_cast<gs_segtopk16*>(h);
    return st;
}

gs_status gs_segtopk16_destroy(gs_segtopk16* h) { return gs_segtopk_destroy(tks16_handle(h)); }

gs_status gs_segtopk16_select_keys(gs_segtopk16* h, const void* d_keys, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments, uint32_t k,
                                   uint32_t max_segment_len, void* d_out_keys, gs_key_type key_type, gs_order order, void* stream) {
    return segtopk_impl(g_tks_routes16, tks16_handle(h), d_keys, nullptr, n, d_offsets, num_segments, k, max_segment_len, d_out_keys, nullptr,
                        key_type, order, static_cast<hipStream_t>(stream), false);
}

gs_status gs_segtopk16_select_pairs(gs_segtopk16* h, const void* d_keys, const void* d_vals, uint32_t n, const uint32_t* d_offsets,
                                    uint32_t num_segments, uint32_t k, uint32_t max_segment_len, void* d_out_keys, void* d_out_vals,
                                    gs_key_type key_type, gs_order order, void* stream) {
    return segtopk_impl(g_tks_routes16, tks16_handle(h), d_keys, d_vals, n, d_offsets, num_segments, k, max_segment_len, d_out_keys, d_out_vals,
                        key_type, order, static_cast<hipStream_t>(stream), true);
}

gs_status gs_segtopk16_check(gs_segtopk16* h, void* stream) { return gs_segtopk_check(tks16_handle(h), stream); }

gs_status gs_segtopk16_last(gs_segtopk16* h, uint32_t* report, uint32_t words, void* stream) {
    return gs_segtopk_last(tks16_handle(h), report, words, stream);
}

gs_status gs_segtopk16_set_rank_mode(gs_segtopk16* h, int mode) { return gs_segtopk_set_rank_mode(tks16_handle(h), mode); }

int gs_segtopk16_get_rank_mode(gs_segtopk16* h) { return gs_segtopk_get_rank_mode(tks16_handle(h)); }

}  // extern "C"
