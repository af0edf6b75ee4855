// host_common.hpp — part of the gpusort_capi.hip translation unit: what every host file of the C-ABI shares — the HIP error
// macro, the argument predicates, small arithmetic, and the device scratch word(s) of the diagnostic entries.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <utility>

namespace {

thread_local int g_last_hip_error = 0;

#define GS_HIP(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) {                        \
            g_last_hip_error = (int)e_;                \
            return GS_ERR_HIP;                         \
        }                                              \
    } while (0)

inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// ---- argument predicates: every test of a key type or an order in the host files goes through these ----
inline bool valid_key_type(gs_key_type kt) { return (int)kt >= 0 && (int)kt <= 5; }
inline bool is_key32_type(gs_key_type kt) { return (int)kt >= 0 && (int)kt <= 2; }  // what the 32-bit-only entries accept
inline bool is_key64(gs_key_type kt) { return (int)kt >= 3; }
inline bool is_key16(gs_key_type kt) { return (int)kt >= 6 && (int)kt <= 9; }  // 2-byte keys: the row-wise top-k entries only
inline bool valid_order(gs_order order) { return order == GS_ORDER_ASCENDING || order == GS_ORDER_DESCENDING; }

// a handle's mode and value width: keys only without values, pairs with 4- or 8-byte values
inline bool mode_value_ok(gs_mode mode, uint32_t vb) {
    return mode == GS_MODE_KEYS_ONLY ? vb == 0u : mode == GS_MODE_PAIRS && (vb == 4u || vb == 8u);
}
// do [a, a + na) and [b, b + nb) share a byte
inline bool buffers_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}
// do any two of the first `count` buffers p[i] of bytes[i] bytes share a byte
inline bool any_overlap(const void* const* p, const size_t* bytes, int count) {
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if (buffers_overlap(p[i], bytes[i], p[j], bytes[j])) return true;
    return false;
}

// compute units of the device (read once per process; 256 if it cannot be read)
uint32_t cu_count() {
    static const uint32_t cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return (uint32_t)v;
    }();
    return cus;
}

// Device scratch of a diagnostic entry (a counter or a small report): allocated and zeroed on the stream, read back with a wait,
// freed when the entry returns — whichever way it returns.
struct DeviceScratch {
    void* d = nullptr;
    const size_t bytes;
    explicit DeviceScratch(size_t n) : bytes(n) {}
    DeviceScratch(const DeviceScratch&) = delete;
    ~DeviceScratch() {
        if (d) (void)hipFree(d);
    }
    template <class T> T* as() const { return static_cast<T*>(d); }
    gs_status alloc_zeroed(hipStream_t s) {
        GS_HIP(hipMalloc(&d, bytes));
        GS_HIP(hipMemsetAsync(d, 0, bytes, s));
        return GS_OK;
    }
    gs_status read_back(void* host, hipStream_t s) {
        GS_HIP(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        return GS_OK;
    }
};

}  // namespace
