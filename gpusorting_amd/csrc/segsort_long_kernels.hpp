// segsort_long_kernels.hpp — gfx950 (wave64) device code of the segmented sort's device route for long segments of 32-bit keys
// (GS_SEGSORT_LONG_DEVICE of gs_segsort_set_long_route in include/gpusort.h).  No counterpart in the reference project.
//
// Segments longer than LDS holds (class 8) take GS_SEGSORT_LONG_PASSES stable 8-bit LSD passes over ALL long segments at once, ping-pong
// between the caller's buffers and the alternates, with NO host round trip.  Behind the launches of the classes that fit LDS:
//   seg16_units_kernel    as it is (segsort16_kernels.hpp: it does not depend on the key width), with parts of GS_SEGSORT_LONG_PART
//                         elements: the (segment, part) work list and one record per long segment, built on the device
//   per pass: segl_count_kernel (one 256-bin table per unit, 4-byte keys), seg16_scan_kernel as it is (one workgroup per long segment;
//                         the counts must add up to its length), segl_scatter_kernel (one workgroup per unit, its tiles in order)
// on fixed grids sized by the host's bound on units and long segments (gs_segsort_long_units): workgroups beyond the device's own counts
// leave at once.  Count, scan and scatter are the bodies of radix_pass.hpp, which tells the pass's structure and invariants, with a
// long segment as the row and a unit descriptor as its part.
//
// A segment starts at any element: every key load and store is one dword per lane, and an 8-byte value at an odd element index is
// naturally aligned because the value buffer is 16-byte aligned.  Nothing is merged or copied afterwards.
// No kernel waits on another workgroup.  The guards are those of the 16-bit kernels: a unit beyond the device's count, or an
// internal status already set, reads nothing; a scatter that finds the status set writes nothing.  Registers, LDS and scratch per
// kernel: DESIGN.md 3.16.
#pragma once
#include "segsort16_kernels.hpp"  // seg16_units_kernel, seg16_scan_kernel, SEG16C_*; through it radix_pass.hpp

namespace gs {

#if GS_SORT_ROWS_BUILT

// table[unit][d] = keys of the unit's part whose byte at `shift` of the sortable bits is d.  Workgroup = unit (fixed grid).
__global__ __launch_bounds__(SR_THREADS) void segl_count_kernel(const uint32_t* __restrict__ keys, const uint4* __restrict__ desc,
                                                                const uint32_t* __restrict__ ctl, uint32_t unit_cap, uint32_t kt, uint32_t shift,
                                                                uint32_t* __restrict__ table) {
    const uint32_t u = blockIdx.x;
    // (uniform; bad offsets claim no units; a rejected claim leaves descriptors unwritten: nothing is read through them)
    if (u >= unit_cap || u >= ctl[SEG16C_UNITS] || ctl[SEG16C_INTERNAL] != 0u) return;
    const uint4 d = desc[u];  // (start, length, part's first element, part's end)
    const uint32_t len = (d.z < d.w && d.w <= d.y) ? d.w - d.z : 0u;
    pass_count32_body(keys + d.x + d.z, len, kt, shift, table + (size_t)u * RADIX);
}

// One workgroup per unit (fixed grid), its tiles in order: seg16_scatter_kernel on 4-byte keys.  VB: 0 keys only, 4 / 8 = values of
// that width (the argsort passes an index array as values).  Positions are relative to the segment.
template <int VB, int RANK>
__global__ __launch_bounds__(SR_THREADS) void segl_scatter_kernel(const uint32_t* __restrict__ kin, const void* __restrict__ vin_, uint32_t* __restrict__ kout,
                                                                  void* __restrict__ vout_, const uint4* __restrict__ desc, uint32_t unit_cap, uint32_t kt,
                                                                  uint32_t shift, uint32_t reverse, const uint32_t* __restrict__ bases,
                                                                  uint32_t* __restrict__ ctl) {
    static_assert(VB == 0 || VB == 4 || VB == 8, "no positions made in registers on this route");
    using V = typename S16Val<VB>::type;
    const uint32_t u = blockIdx.x;
    if (u >= unit_cap || u >= ctl[SEG16C_UNITS]) return;  // (uniform)
    const uint4 d = desc[u];  // (start, length, part's first element, part's end)
    if (d.w > d.y) return;
    pass_scatter_body<uint32_t, VB, RANK>(kin + d.x, static_cast<const V*>(vin_) + (VB != 0 ? d.x : 0u), kout + d.x,
                                          static_cast<V*>(vout_) + (VB != 0 ? d.x : 0u), d.y, d.z, d.w, 0u, kt, shift, reverse,
                                          bases + (size_t)u * RADIX, ctl + SEG16C_INTERNAL);
}

#endif  // GS_SORT_ROWS_BUILT

}  // namespace gs
