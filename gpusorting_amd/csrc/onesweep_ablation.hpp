// onesweep_ablation.hpp — tracing and fault-injection hooks of the OneSweep kernels.  NOT part of the product build:
// onesweep_kernels.hpp includes this file only when GS_EXP != 0 (tools/README.md "experiment builds",
// tests/test_gpu_fault.py), and it rejects every GS_EXP bit but these two:
//   2   per-tile phase timestamps (10 ns ticks, lane 0 of wave 0) into the buffer whose address the host stored in
//       the slab at STATUS+8; 8 words per (pass, block) — tools/trace_tiles.py
//   8   fault injection (cf. the reference's EmulatedDeadlocking.cu:36-37,339-345): tile 5 of chain 3 never publishes
//       its descriptor, as if its workgroup had stalled.  With the fallback (default) its successors recount it and
//       the sort is exact; with -DGS_FALLBACK=0 every later tile of that chain runs into the bounded spin, the sort
//       still finishes, and gs_onesweep_check says GS_ERR_TIMEOUT.
#pragma once

#define GS_FAULT_TILE(chain, tile) (((GS_EXP)&8) && (chain) == 3u && (tile) == 5u)
// ... and in the two-launch mid-size sort every fourth workgroup of K1 behaves as if it had never been dispatched (the
// others adopt its tile)
#define GS_FAULT_MID_ABSENT(block) (((GS_EXP)&8) && ((block)&3u) == 1u)
// ... and, in the build WITHOUT the fallback (-DGS_FALLBACK=0: the one that must report GS_ERR_TIMEOUT), workgroup 2 of K1 claims its
// tile and never publishes its counts: nobody can adopt a claimed tile, so every waiter must run into its bounded spin
#define GS_FAULT_MID_SILENT(block) (((GS_EXP)&8) && !GS_FALLBACK && (block) == 2u)

#if (GS_EXP & 2)
#define GS_TRACE_SETUP()                                                                                                  \
    uint32_t* trace = reinterpret_cast<uint32_t*>(((unsigned long long)status[9] << 32) | status[8]) +                    \
                      ((size_t)(shift >> 3) * gridDim.x + blockIdx.x) * 8;                                                \
    uint32_t trace_trips = 0
#define GS_TRACE(slot) do { if (tid == 0) trace[(slot)] = (uint32_t)wall_clock64(); } while (0)
#define GS_TRACE_TRIP() ++trace_trips
#define GS_TRACE_END(chain) do { if (tid == 0) trace[7] = trace_trips | ((chain) << 16) | (1u << 31); } while (0)
#else
#define GS_TRACE_SETUP() do { } while (0)
#define GS_TRACE(slot) do { } while (0)
#define GS_TRACE_TRIP() do { } while (0)
#define GS_TRACE_END(chain) do { } while (0)
#endif
