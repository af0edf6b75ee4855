// handle_core.hpp — part of the gpusort_capi.hip translation unit: the scaffolding the handles of the *_host.hpp files share.  Each
// piece stands here once: the layout arena (256-byte granules), the workspace a handle embeds (device block, pinned block, the
// control block's read-back), the create/destroy frame, the rank-mode setter and getter, the alternate-buffer predicates, the
// ping-pong of a pass loop, and the head of a segmented call (reset, classify, fill; a class's segment bound and LDS bytes).
// gs_onesweep and gs_mgpu do not use it.
namespace {

bool lds_atomic_order_ok();  // onesweep_host.hpp: the probe of gs_onesweep_create, once per device

// ---- layout arena: offsets into one allocation, every block on a 256-byte granule ----
struct Arena {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t a = at; at += (bytes + 255u) & ~(size_t)255u; return a; }
    size_t total() const { return at; }
};

// ---- workspace: what a handle owns on the device and in pinned memory ----
struct Workspace {
    char* dev = nullptr;         // one allocation: see the handle's layout function
    uint32_t* pinned = nullptr;  // read-back of the control block (pinned_words words)
    size_t ctl_offset = 0;       // the control block inside dev
    uint32_t ctl_words = 0, pinned_words = 0;

    uint32_t* ctl() const { return reinterpret_cast<uint32_t*>(dev + ctl_offset); }
    // the device block, its control words zeroed (a handle's check may run before any call), and the pinned block
    gs_status alloc(size_t total_bytes, size_t ctl_off, uint32_t ctl_w, uint32_t pinned_w) {
        ctl_offset = ctl_off;
        ctl_words = ctl_w;
        pinned_words = pinned_w;
        hipError_t e = hipMalloc(&dev, total_bytes);
        if (e == hipSuccess) e = hipMemset(dev + ctl_offset, 0, ctl_words * sizeof(uint32_t));
        if (e == hipSuccess) e = hipHostMalloc(&pinned, pinned_words * sizeof(uint32_t), hipHostMallocDefault);
        if (e == hipSuccess) return GS_OK;
        g_last_hip_error = (int)e;
        return GS_ERR_HIP;
    }
    void release() {
        if (pinned) (void)hipHostFree(pinned);
        if (dev) (void)hipFree(dev);
        pinned = nullptr;
        dev = nullptr;
    }
    // the first `words` words of the control block -> pinned (synchronises)
    gs_status read_ctl(hipStream_t s, uint32_t words) {
        if (words > pinned_words) return GS_ERR_ARG;
        GS_HIP(hipMemcpyAsync(pinned, dev + ctl_offset, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        return GS_OK;
    }
    gs_status read_ctl(hipStream_t s) { return read_ctl(s, ctl_words); }
};

// ---- create / destroy of a handle H with the members mode, value_bytes, rank_mode and ws ----
// fill(h) copies the handle's own sizes and allocates h->ws for its layout; its status is create's.
template <class H>
gs_status handle_destroy(H* h) {
    if (!h) return GS_ERR_ARG;
    h->ws.release();
    delete h;
    return GS_OK;
}
template <class H, class Fill>
gs_status handle_create(H** out, bool sizes_ok, gs_mode mode, uint32_t value_bytes, Fill fill) {
    if (!out) return GS_ERR_ARG;
    *out = nullptr;
    if (!sizes_ok) return GS_ERR_SIZE;
    if (!mode_value_ok(mode, value_bytes)) return GS_ERR_MODE;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GS_ERR_NO_DEVICE;
    H* h = new (std::nothrow) H();
    if (!h) return GS_ERR_ARG;
    h->mode = mode;
    h->value_bytes = value_bytes;
    h->rank_mode = lds_atomic_order_ok() ? 1 : 0;
    const gs_status st = fill(h);
    if (st != GS_OK) {
        (void)handle_destroy(h);
        return st;
    }
    *out = h;
    return GS_OK;
}

// ---- the ranking of a handle's scatter and workgroup classes: 0 ballot multi-split, 1 returning LDS atomic ----
template <class H>
gs_status handle_set_rank_mode(H* h, int mode) {
    if (!h || (mode != 0 && mode != 1)) return GS_ERR_ARG;
    h->rank_mode = mode;
    return GS_OK;
}
template <class H>
int handle_get_rank_mode(const H* h) { return h ? h->rank_mode : -1; }

// ---- the alternate buffers of a pass route ----
// there and 16-byte aligned (the values' one with pairs only)
inline bool alt_buffers_present(const void* alt_keys, const void* alt_vals, bool pairs) {
    return alt_keys && !misaligned(alt_keys) && (!pairs || (alt_vals && !misaligned(alt_vals)));
}
// no two of {keys, alt_keys, vals, alt_vals} of n elements share a byte: the passes read one buffer while they write the other
inline bool alt_buffers_disjoint(const void* keys, const void* alt_keys, const void* vals, const void* alt_vals, uint32_t n, uint32_t key_bytes,
                                 uint32_t value_bytes, bool pairs) {
    const size_t kb = (size_t)n * key_bytes, vb = (size_t)n * value_bytes;
    const void* p[4] = {keys, alt_keys, vals, alt_vals};
    const size_t b[4] = {kb, kb, vb, vb};
    return !any_overlap(p, b, pairs ? 4 : 2);
}
inline bool alt_buffers_ok(const void* keys, const void* alt_keys, const void* vals, const void* alt_vals, uint32_t n, uint32_t key_bytes,
                           uint32_t value_bytes, bool pairs) {
    return alt_buffers_present(alt_keys, alt_vals, pairs) && alt_buffers_disjoint(keys, alt_keys, vals, alt_vals, n, key_bytes, value_bytes, pairs);
}

// ---- the ping-pong of a pass loop: even passes go from the caller's buffers into the alternates, odd ones back ----
template <class K>
struct PingPong {
    const K* kin;
    K* kout;
    const void* vin;
    void* vout;
};
template <class K>
inline PingPong<K> ping_pong(uint32_t pass, K* keys, void* vals, K* alt_keys, void* alt_vals) {
    if ((pass & 1u) == 0u) return {keys, alt_keys, vals, alt_vals};
    return {alt_keys, keys, alt_vals, vals};
}

// ---- the head of a segmented call.  ctl: a control block of gs::SEGC_WORDS words with the class lists behind it ----
// reset, classify, and the class lists when a segment can fall in class 2 or higher.  No host wait.
inline void seg_enqueue_head(uint32_t* ctl, const uint32_t* d_offsets, uint32_t num_segments, uint32_t n, uint32_t vb, uint32_t max_len, uint32_t top,
                             hipStream_t s) {
    hipLaunchKernelGGL(gs::seg_reset_kernel, dim3(1), dim3(64), 0, s, ctl);
    const uint32_t seg_blocks = div_up(num_segments, 256);
    hipLaunchKernelGGL(gs::seg_classify_kernel, dim3(seg_blocks), dim3(256), 0, s, d_offsets, num_segments, n, vb, max_len, ctl);
    if (top >= 2) hipLaunchKernelGGL(gs::seg_fill_kernel, dim3(seg_blocks), dim3(256), 0, s, d_offsets, num_segments, vb, max_len, ctl, ctl + gs::SEGC_WORDS);
}
// a class whose shortest segment has min_len elements holds at most n / min_len segments
inline uint32_t seg_class_bound(uint32_t n, uint32_t num_segments, uint32_t min_len) {
    const uint32_t b = n / min_len;
    return b < num_segments ? b : num_segments;
}
// LDS of a workgroup class's kernel on shape sh: the tile's keys and values, a digit table per wave, the header
inline size_t seg_wg_lds_bytes(Shape sh, uint32_t vb) { return (size_t)sh.threads * sh.kpt * (4 + vb) + (size_t)sh.threads / 64 * gs::RADIX * 4 + 64; }

}  // namespace
