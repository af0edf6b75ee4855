/*
 * gpusort.h — C-ABI of the MI355X-native OneSweep radix sort (libgpusort.so).
 *
 * This is the drop-in boundary for the reference's OneSweep path
 * (b0nes164/GPUSorting @ 2024_10_08).  The reference has no FFI: its boundary
 * is a C++ class per backend.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference root).  On top of
 * this header, include/gpusort/OneSweepDispatcher.hpp re-creates the CUDA
 * tree's `OneSweepDispatcher` class verbatim (same method names, arguments
 * and print format) so GPUSortingCUDA/GPUSortingCUDA.cu:20-23,36-39 compiles
 * unchanged against it; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no HIP/torch types: streams are passed as void* (a hipStream_t;
 *     NULL = the null stream); device pointers are void* and caller-owned.
 *   - every call returns a gs_status; nothing throws across the boundary.
 *   - all calls are asynchronous on `stream` unless stated otherwise.
 *   - key/value device buffers must be 16-byte aligned.
 *   - 1 <= n <= GS_MAX_KEYS (30-bit tile-descriptor payload, same limit as the
 *     reference: GPUSortingCUDA/SegSort/SplitSort/SplitSortLarge.cuh:795-800).
 *   - a handle serialises its sorts: one in-flight sort per handle (it owns the
 *     chained-scan state).  Use one handle per stream.
 */
#ifndef GPUSORT_H
#define GPUSORT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_MAX_KEYS ((1u << 30) - 1u)

typedef enum gs_status {
    GS_OK = 0,
    GS_ERR_ARG = 1,      /* NULL / misaligned pointer, bad enum */
    GS_ERR_SIZE = 2,     /* n == 0, n > max_keys of the handle, n > GS_MAX_KEYS */
    GS_ERR_HIP = 3,      /* a HIP runtime call failed (gs_last_hip_error() has the code) */
    GS_ERR_TIMEOUT = 4,  /* a bounded look-back spin expired on the device */
    GS_ERR_MODE = 5,     /* pairs call on a keys-only handle / value width mismatch */
    GS_ERR_NO_DEVICE = 6, /* no gfx950 device visible */
    GS_ERR_COMM = 7       /* multi-GPU: RCCL could not be loaded or a collective failed (gs_last_rccl_error()) */
} gs_status;

/* GPUSortingD3D12/GPUSorting.h:40-45 */
typedef enum gs_mode { GS_MODE_KEYS_ONLY = 0, GS_MODE_PAIRS = 1 } gs_mode;
/* GPUSortingD3D12/GPUSorting.h:47-52 */
typedef enum gs_order { GS_ORDER_ASCENDING = 0, GS_ORDER_DESCENDING = 1 } gs_order;
/* GPUSortingD3D12/GPUSorting.h:54-60 */
typedef enum gs_key_type {
    GS_KEY_UINT32 = 0, GS_KEY_INT32 = 1, GS_KEY_FLOAT32 = 2,
    /* 64-bit keys (the reference has 32-bit keys only): 8-byte elements in d_keys / d_alt, sorted by
     * eight stable passes of the same kernels, planned by ONE GlobalHistogram sweep + Scan (identity passes are dropped
     * in pairs across the whole key); values as for 32-bit keys.  Accepted by
     * gs_onesweep_sort_keys / _sort_pairs / _digit_pass (pass 0..7) and gs_validate; not by the histogram read-back,
     * the MSD split and the generator, which are 32-bit. */
    GS_KEY_UINT64 = 3, GS_KEY_INT64 = 4, GS_KEY_FLOAT64 = 5,
    /* 16-bit keys: 2-byte elements, FLOAT16 is IEEE binary16.  Accepted by gs_topk_select_rows_keys / _pairs (see there) and by the
     * gs_sort16_* family (gs_sort16_sort_keys / _sort_pairs / _argsort, at the end of this header), which takes nothing else; every
     * other entry that takes a gs_key_type treats them as it treats any value it does not know. */
    GS_KEY_UINT16 = 6, GS_KEY_INT16 = 7, GS_KEY_FLOAT16 = 8, GS_KEY_BFLOAT16 = 9
} gs_key_type;
/* GPUSortingCUDA/UtilityKernels.cuh:16-24 (value = number of extra AND-ed draws) */
typedef enum gs_entropy_preset {
    GS_ENTROPY_PRESET_1 = 0, GS_ENTROPY_PRESET_2 = 1, GS_ENTROPY_PRESET_3 = 2,
    GS_ENTROPY_PRESET_4 = 3, GS_ENTROPY_PRESET_5 = 4
} gs_entropy_preset;

typedef struct gs_onesweep gs_onesweep; /* opaque sorter state */

const char* gs_version(void);
const char* gs_status_string(gs_status s);
int gs_last_hip_error(void); /* hipError_t of the last failing HIP call on this thread */

/* ---- sorter object -------------------------------------------------------
 * Replaces: OneSweepDispatcher::OneSweepDispatcher(bool keysOnly, uint32_t maxSize)
 * / ~OneSweepDispatcher (GPUSortingCUDA/Sort/OneSweepDispatcher.cuh:42-83) for
 * the scan state (m_index, m_globalHistogram, m_*PassHistogram), and the temp
 * buffers of Unity's OneSweep ctor (GPUSortingUnity/Runtime/OneSweep.cs:27-81).
 * Key/value/alt buffers stay with the caller (Unity ownership model).
 * value_bytes: 0 (keys only), 4 or 8.  Synchronous (allocates). */
gs_status gs_onesweep_create(gs_onesweep** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
gs_status gs_onesweep_destroy(gs_onesweep* h);

/* Everything that can be chosen about a sorter, in one place (the analogue of the reference's GPUSortingConfig + DeviceInfo,
 * GPUSortingD3D12/GPUSorting.h:40-86: mode / order / key type / payload type travel with the calls here; what is left are the
 * algorithm switches below).  The library itself reads NO environment variables: gs_onesweep_create uses the defaults;
 * harnesses that want GPUSORT_* variables (gpusorting_amd/onesweep.py, tools/) translate them into this struct.
 * Fill it with gs_onesweep_options_default() first; struct_size lets the struct grow. */
typedef struct gs_onesweep_options {
    uint32_t struct_size;            /* sizeof(gs_onesweep_options) */
    uint32_t shape_threads;          /* tile shape, threads x keys per thread; 0 x 0 (default) = the library picks by size and mode */
    uint32_t shape_keys_per_thread;
    int32_t rank_mode;               /* -1 (default) probe the device: 1 if its LDS serves same-address lanes in lane order, else 0;
                                        0 = 64-lane ballot multi-split, 1 = one returning LDS atomic per key */
    int32_t small_path;              /* 1 (default): n <= 8192 .. 32 768 keys in ONE workgroup; 0: always tiled */
    int32_t mid_path;                /* 1 (default): up to 2^20 .. 2^22 keys in two launches (MSD pass + bucket sorts) */
    int32_t skip_passes;             /* 1 (default): identity passes (a constant byte) are dropped in pairs on the device */
    int32_t position_chains;         /* skewed keys: 1 (default) position-chain plan when the histogram kernel finds the digit
                                        groups uneven, 0 never, 2 always (tests, tuning) */
    uint32_t position_chains_min_log2;  /* ... from 2^this keys up (20 .. 30); the default, 25, means 2^25 + 1: up to 2^25 keys the smaller tile shape wins */
    int32_t key64_sweeps;            /* 64-bit keys: 1 (default) one histogram sweep plans all eight passes, 2 one sweep per word */
    int32_t plan;                    /* gs_onesweep_set_plan: 0 (default) the library picks — the two-level plan for large sorts whose
                                        keys turn out near-uniform, the four LSD passes otherwise; 1 LSD passes only; 2 two-level plan wherever it can run */
    int32_t first_pass_big;          /* 1 (default): keys-only mid sizes run their first pass on the 16 384-key tile */
    uint32_t hist_blocks;            /* workgroups of the GlobalHistogram kernel; 0 (default) = one per CU (tuning aid) */
    uint32_t debug_flags;            /* 0.  Every build but the tuning build (-DGS_TUNING) ignores every bit.  There, bit 30 = the two-level
                                        plan stops behind its second pass (tools/hy_bringup.py; the result is NOT sorted) */
} gs_onesweep_options;
void gs_onesweep_options_default(gs_onesweep_options* o);
/* gs_onesweep_create with explicit options (NULL = defaults).  GS_ERR_ARG for a struct_size this library does not know, a tile
 * shape it was not built with, or a value out of range. */
gs_status gs_onesweep_create_ex(gs_onesweep** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes, const gs_onesweep_options* options);

/* Bytes of device memory a handle for max_keys allocates (descriptors + histograms + the two-level plan's tables): an upper
 * bound over modes and options (default hist_blocks). */
size_t gs_onesweep_temp_bytes(uint32_t max_keys);
/* Keys per binning tile of this build (the reference's k_partitionSize = 7680,
 * OneSweepDispatcher.cuh:23; tests ladder sizes over [P, 2P]). */
uint32_t gs_onesweep_partition_size(gs_mode mode, uint32_t value_bytes);

/* ---- the hot path ---------------------------------------------------------
 * Replaces: OneSweepDispatcher::DispatchKernelsKeysOnly(uint32_t size)
 * (OneSweepDispatcher.cuh:311-336) and Unity OneSweep.Sort(...) keys overload
 * (GPUSortingUnity/Runtime/OneSweep.cs:297-323).  Sorts d_keys[0..n) in place
 * (result in d_keys, as in the reference after 4 passes); d_alt is scratch of
 * n keys.  key_type/order as D3D12 GPUSortBase (GPUSortingD3D12/OneSweep.h:16-27). */
gs_status gs_onesweep_sort_keys(gs_onesweep* h, void* d_keys, void* d_alt, uint32_t n,
                                gs_key_type key_type, gs_order order, void* stream);

/* Replaces: OneSweepDispatcher::DispatchKernelsPairs (OneSweepDispatcher.cuh:338-363)
 * and Unity OneSweep.Sort pairs overload (OneSweep.cs:358-390).  Values are
 * bit-copied (value_bytes of the handle); stable by key; descending = exact
 * reverse of the stable ascending result (SortCommon.hlsl:594-597,645-656). */
gs_status gs_onesweep_sort_pairs(gs_onesweep* h, void* d_keys, void* d_vals, void* d_alt_keys,
                                 void* d_alt_vals, uint32_t n, gs_key_type key_type,
                                 gs_order order, void* stream);

/* Synchronises `stream` and reads the device status word of the last sort:
 * GS_OK or GS_ERR_TIMEOUT.  With the look-back fallback of the default build (a tile that
 * waits too long recounts its predecessor itself) a timeout cannot occur; the word exists
 * for builds without it (-DGS_FALLBACK=0), whose bounded spins report here instead of hanging.
 * Every sort resets the word itself, whatever route it takes.
 * (The reference checks nothing; D3D12 only warns, GPUSortingD3D12/SweepBase.h:52-53.) */
gs_status gs_onesweep_check(gs_onesweep* h, void* stream);

/* ---- tuning (no reference counterpart at run time; the reference fixes its
 * tile shape with #defines, GPUSortingCUDA/Sort/OneSweep.cu:30-36, and the D3D12
 * tree picks one per device in Tuner.h) -------------------------------------
 * Select one of the compiled tile shapes (threads x keys-per-thread).  Without a
 * choice the library picks: the shape gs_onesweep_partition_size() reports for large
 * sorts (512x32 keys-only and 8-byte values, 1024x16 4-byte values) and 512x16
 * (8192-key tiles) up to 2^23 / 2^24 / 2^25 keys (keys-only / 4-byte / 8-byte values),
 * where it is faster.  512x32, 1024x16 and 512x16 exist for every key and value type
 * (the tuning build libgpusort_tuning.so adds 256x32, 256x16 and 512x20 for uint32 keys).  (gs_onesweep_options::shape_threads / shape_keys_per_thread at create.) */
gs_status gs_onesweep_set_shape(gs_onesweep* h, uint32_t threads, uint32_t keys_per_thread);
uint32_t gs_onesweep_get_partition_size(gs_onesweep* h);
/* Ranking algorithm inside a tile: 0 = 64-lane ballot multi-split (the
 * reference's WLMS, OneSweep.cu:207-253, re-derived for wave64); 1 = one
 * returning LDS atomic per key, valid only if gs_selftest_lds_atomic_order()
 * reports 0 failures on this device. */
gs_status gs_onesweep_set_rank_mode(gs_onesweep* h, int mode);
int gs_onesweep_get_rank_mode(gs_onesweep* h); /* the mode in use (after the create-time probe): 0 or 1; -1 for a null handle */
/* Small inputs are sorted by ONE workgroup in one launch (all four passes in LDS): n <= 8192 in every
 * mode, n <= 16384 for keys-only and 4-byte values, n <= 32768 for keys-only — unless this is switched off
 * (tests use 0 to push small sizes through the tiled path as well). */
gs_status gs_onesweep_set_small_path(gs_onesweep* h, int on);
/* Mid sizes (single-tile limit < n <= 2^20; 4-byte values up to 2^22 pairs, keys-only up to 2^23; 32-bit keys) are
 * sorted in TWO launches instead of seven: one MSD pass on the
 * top byte (its workgroups claim their tiles and adopt the tiles of workgroups that were never dispatched: no residency
 * requirement) and one workgroup per top-byte bucket that sorts the remaining 24
 * bits in LDS; a top byte too skewed for that (a bucket above what the class's workgroup holds: 8192 … 34 816 keys) is noticed on the device and the first kernel
 * runs the four LSD passes itself (reference size sweep GPUSortingD3D12/Tests.h:392-393,415-416).  Same
 * result either way; 0 sends these sizes through the general path.  Only used while the library picks the tile shape.
 * Default 1 (gs_onesweep_options::mid_path at create). */
gs_status gs_onesweep_set_mid_path(gs_onesweep* h, int on);
/* A pass whose digit is the same for every key (e.g. the upper bytes of 16-bit keys) is the
 * identity permutation.  The Scan kernel sees that in the histogram and drops such passes in
 * pairs, on the device, with no host round trip (the reference always runs
 * four passes).  Results are identical either way; 0 runs all four passes.  Default 1;
 * (gs_onesweep_options::skip_passes at create). */
gs_status gs_onesweep_set_skip_passes(gs_onesweep* h, int on);
/* Plan of large sorts of 32-bit keys — keys-only and pairs (library-picked shape, rank mode 1, position chains allowed).
 * The reference's pipeline is GlobalHistogram + Scan + four 8-bit LSD DigitBinningPasses (GPUSortingCUDA/Sort/OneSweep.cu:44-344,
 * dispatch OneSweepDispatcher.cuh:311-336): 36 bytes of memory traffic per key.  The TWO-LEVEL plan (hybrid_kernels.hpp) runs the same
 * kernels in another order — one histogram sweep over the keys' top 16 bits, a Scan, a DigitBinningPass on the top byte, a
 * DigitBinningPass on byte 2 inside the top-byte buckets (256 chains), then one workgroup per 16-bit-prefix bucket sorts the low
 * 16 bits in LDS, in place: 28 bytes per key, the same result bit for bit.  It needs buckets that fit a workgroup (near-uniform top
 * 16 bits); whether they do is decided ON THE DEVICE from the histogram (no host round trip): otherwise the same launches run the
 * four LSD passes on position chains.
 *   0 (default): the two-level plan is offered from 3 x 2^24 (50 M) keys up, to pairs from 2^25 + 1 (measured crossovers);  1: never (the
 *   LSD passes only);  2 (tests): offered at every size from gs_onesweep_options::position_chains_min_log2 up.  A handle that was
 *   created without the plan's tables (below the plan's default size, or with plan 1) gets them allocated by gs_onesweep_set_plan(h, 2)
 *   — call it with no sort of the handle in flight; GS_ERR_MODE for max_keys <= 2^20 (neither the plan nor its fall-back runs there).  Pairs: the values travel with their keys through
 *   both DigitBinningPasses and are moved once more by the bucket-local sort — 52 / 76 bytes per pair instead of 68 / 100.
 * gs_onesweep_last_plan (synchronous) reports what the device decided for the last sort: *plan = 1 the two-level plan ran, 0 the LSD
 * passes (or a one- / two-launch route); *largest_bucket (may be NULL) = the largest 16-bit-prefix bucket it saw (0 if not offered). */
gs_status gs_onesweep_set_plan(gs_onesweep* h, int plan);
gs_status gs_onesweep_last_plan(gs_onesweep* h, uint32_t* plan, uint32_t* largest_bucket, void* stream);
/* Device probe: do same-address lanes of one LDS atomic get their results in
 * ascending lane order?  Synchronous; *h_failures = mismatching lanes. */
gs_status gs_selftest_lds_atomic_order(uint32_t iters, uint32_t seed, uint64_t* h_failures, void* stream);
/* Self-test of the wave-level primitives (wave64 scans by shuffle and by DPP, reduction, 64-bit ballot, mbcnt lane rank, the
 * eight-ballot multi-split) — what the reference builds from PTX and 32-lane *_sync intrinsics in GPUSortingCUDA/Utils.cuh:22-126 and
 * OneSweep.cu:207-253.  Enqueues one kernel: `waves` (a multiple of 4) waves each write 8 rows of 64 words to d_out
 * (waves x 512 uint32); row layout and the input word of a lane: onesweep_kernels.hpp, wave_primitives_kernel.  The caller compares. */
gs_status gs_selftest_wave_primitives(uint32_t seed, uint32_t waves, uint32_t* d_out, void* stream);
/* Instrumented builds only (-DGS_EXP=2, tools/trace_tiles.py): device buffer of 4 passes x grid x 8 words that
 * receives per-tile phase timestamps.  A no-op in the product build. */
gs_status gs_debug_set_trace(gs_onesweep* h, void* d_buf);

/* Debug: post-call invariants of the handle's chained-scan state (the analogue of the reference's
 * ValidateInitialOneSweepState + index checks, GPUSortingCUDA/UtilityKernels.cuh:482-502, which the reference never
 * calls after a sort).  Synchronous.  After any tiled call that completed: report[0] descriptor rows that are not
 * INCLUSIVE, [1] rows whose inclusive count decreased along their chain, [2] chains whose ticket counter is below
 * their tile count, [3] non-zero words left in the histogram region (it must be zero whenever no call is in
 * flight) — all four must be 0 — and [4 + q] the keys the descriptors of the call's q-th pass account for (== n
 * for every pass that ran, 0 for a dropped identity pass).  All zero after a single-tile sort (no scan state). */
gs_status gs_debug_check_state(gs_onesweep* h, uint64_t report[8], void* stream);
/* Test hook: overwrite the device status word gs_onesweep_check() reads (e.g. GS_ERR_TIMEOUT) — every sort must reset it
 * itself, whatever route it takes.  Synchronous. */
gs_status gs_debug_poke_status(gs_onesweep* h, uint32_t word, void* stream);
/* Test / tuning hook: copies `count` words of the handle's state slab, from word `first_word`, to the host.  Synchronous. */
gs_status gs_debug_read_slab(gs_onesweep* h, uint32_t first_word, uint32_t count, uint32_t* h_out, void* stream);
/* Test hook, host only (no device work, no allocation): which way gs_onesweep_sort_keys / _sort_pairs would send a sort of n
 * elements of key_type on this handle as it is set up now (mode and value width are the handle's) — what the library decides from
 * sizes, modes and options alone; what the keys look like is the device's business (gs_debug_pass_flags, gs_onesweep_last_plan).
 * report[GS_ROUTE_R_*]; GS_ERR_ARG for a null handle or report or a key type the sorts do not take, GS_ERR_SIZE for n == 0 or
 * n > max_keys. */
#define GS_ROUTE_NONE 0xffffffffu
#define GS_ROUTE_R_SMALL 0   /* single-tile route: its size class 0 .. 4 (up to 1024 / 2048 / 8192 / 16 384 / 32 768 elements), else GS_ROUTE_NONE */
#define GS_ROUTE_R_MID 1     /* two-launch mid-size route: its class 0 .. 4, else GS_ROUTE_NONE (-1); the words below describe the general
                                pipeline, which runs when both are GS_ROUTE_NONE */
#define GS_ROUTE_R_SHAPE 2   /* tile shape of the binning passes: 0 = 512 x 32, 1 = 1024 x 16, 2 = 512 x 16 (the tuning build has three more) */
#define GS_ROUTE_R_SHAPE0 3  /* ... of the first pass */
#define GS_ROUTE_R_DYN 4     /* 2: the Scan kernel plans the passes on the device (identity passes dropped, source buffers); 0: fixed ping-pong */
#define GS_ROUTE_R_POS 5     /* 0, or — the sort may be planned on position chains — the tile word of those passes: keys per tile, bit 31 set
                                if the plan's last pass runs on that tile too */
#define GS_ROUTE_R_HY 6      /* 1: the sort is offered the two-level plan */
#define GS_ROUTE_R_RANK 7    /* the handle's rank mode, as gs_onesweep_get_rank_mode */
gs_status gs_debug_sort_route(gs_onesweep* h, uint32_t n, gs_key_type key_type, uint32_t report[8]);
/* Test hook, host only (no device work): the size class of the two-level plan's bucket-local sort — 0 .. 3: a workgroup of
 * 256 x 12, 512 x 12, 1024 x 12, 1024 x 24 keys — is picked from n alone (class 0 up to 2^27 keys, 1 up to 2^28, 2 up to 2^29, 3 above);
 * cls = 0 .. 3 forces that class for every later sort of the handle, whatever its n: the bucket limit the device judges the plan by and
 * the bucket-local kernel follow it, so a bucket of exactly the class's capacity is a few thousand keys of a small sort.  -1 (the
 * default of every handle): by n.  A sort whose forced class has no kernel for its value width and key type (8-byte values, class 3)
 * is not offered the plan (GS_ROUTE_R_HY 0) and runs on the LSD passes.  GS_ERR_ARG for a null handle or any other cls.  Call it with no
 * sort of the handle in flight. */
gs_status gs_debug_set_hy_class(gs_onesweep* h, int cls);
/* Test hook, host only (no device work): the grid of the handle's position-chain launches — the persistent workgroups that run a
 * keys-only sort's passes on either plan, and the position-chain form of a pairs sort's passes — is two workgroups per CU.  At
 * 2^20 .. 2^23 keys each of them sees one tile, so what a workgroup keeps ACROSS its tiles (the packed next-digit table and its
 * overflow guard, the next digit it leaves out, tiles taken from other chains) is only reached at full size.  workgroups >= 16 (the
 * chains of a pass) sets that grid for every later sort of the handle; 0 restores the default.  Any such grid is correct: a workgroup
 * draws tickets on chain blockIdx % 16 — group by group on the 256 chains of the two-level plan's second pass — and then takes tiles of
 * whichever chain still has some, and no tile waits for a workgroup that has not started.  (The plain persistent form of a pairs sort
 * on the two-level plan and the bucket-local sorts keep their grids.)  GS_ERR_ARG for a null handle, 1 .. 15, or more than 65 535.
 * Call it with no sort of the handle in flight.
 * What such a sort leaves in its status block, readable until the next sort of the handle (gs_debug_read_slab, first_word =
 * GS_SLAB_STATUS_WORD + ...): word GS_ST_GUARD_HANDOVERS = counters of the packed next-digit tables that went to the next pass's
 * counts early (at 0xC000), word GS_ST_STOLEN_TILES = tiles a counting position-chain workgroup took from another chain than its own. */
#define GS_SLAB_STATUS_WORD 67584u
#define GS_ST_GUARD_HANDOVERS 4u
#define GS_ST_STOLEN_TILES 5u
gs_status gs_debug_set_pos_grid(gs_onesweep* h, uint32_t workgroups);
/* Test hook: flags[q] = the flag word the Scan kernel and the passes left in the info block of the last sort's q-th pass (32-bit keys
 * use the first four, 64-bit keys planned by one sweep all eight) — which passes ran, from which buffer, in which form.  All zero
 * after a sort that left no scan state (the single-tile and mid-size routes).  Synchronous. */
#define GS_PF_SKEW 1u     /* some digit holds more than 1/16 of the keys: the pass ranks with wave-aggregated adds (8-byte values on the
                             512 x 32 tile: the two-round form of the pass works, the one-round form exits) */
#define GS_PF_SKIP 2u     /* the pass was dropped: every key has the same digit, and so has another pass */
#define GS_PF_SRC_ALT 4u  /* an odd number of earlier passes ran: this pass reads the alternate buffers */
#define GS_PF_LAST 8u     /* the last pass that runs */
#define GS_PF_POS 16u     /* the sort runs on position chains: the position-chain form of the pass works */
#define GS_PF_HALF16 32u  /* the second pass of a keys-only sort on the two-level plan: it hands the bucket-local sort the keys' low 16 bits
                             alone, two bytes per key (gs_debug_hy_half_slot); never set for pairs or on the LSD passes */
gs_status gs_debug_pass_flags(gs_onesweep* h, uint32_t flags[8], void* stream);
/* Test hook, host only (no device work): where the second pass of a keys-only sort on the two-level plan puts the low 16 bits of a key.
 * The bucket of a 16-bit prefix holds the keys whose sorted ascending positions are [base_p, base_p1); its final range starts at key
 * index at = base_p (ascending) or n - base_p1 (descending != 0).  With the key buffer viewed as uint16[2 n], the key that pass ranks
 * `rank` (0 .. base_p1 - base_p - 1) inside the bucket goes to halfword 2 at + rank — the value returned: the first half of the bucket's
 * own bytes.  The kernels compute their addresses with the same function. */
uint32_t gs_debug_hy_half_slot(uint32_t base_p, uint32_t base_p1, uint32_t n, uint32_t descending, uint32_t rank);
/* Test hooks, host only (they work without a GPU): the kernel registry of this build — one launcher table per kernel family
 * (GS_KF_*), indexed by tile shape or size class, rank mode, value width and key type.  gs_debug_registry_dims: dims[0 .. r) = the
 * table's extents, the rest 1; returns r, -1 for an unknown family or null dims.  gs_debug_registry_cell: 1 if this build compiled
 * the kernel(s) of the cell at coord[0 .. r) (coord[r .. 5) must be 0), 0 if not, -1 for an unknown family or a coordinate outside
 * the table.  Index orders (vb: 0 / 1 / 2 = no / 4-byte / 8-byte values; vm: 0 / 1 / 2 / 3 = keys only / positions / 4- / 8-byte
 * values; kt: gs_key_type 0 .. 5; rank: the rank mode; class: the family's size class): */
#define GS_KF_BIN 0u             /* [two-round form][shape][rank][vb][kt]   digit_binning_kernel */
#define GS_KF_POS 1u             /* [vb][last pass][kt]                     the position-chain forms of the pass */
#define GS_KF_PERSIST 2u         /* [8-byte values][kt]                     the two-level plan's passes for pairs */
#define GS_KF_SMALL 3u           /* [class][rank][vb][kt]                   the single-tile sort */
#define GS_KF_MID 4u             /* [class][rank][vb][kt]                   the mid-size route's two kernels */
#define GS_KF_SEG_WG 5u          /* [class][rank][vb][32-bit kt]            segmented sort, one workgroup per segment */
#define GS_KF_SEG_VB 6u          /* [vb]                                    segmented sort: packed, wave, head merge */
#define GS_KF_TKR_TILE 7u        /* [2-byte keys][class][rank][vm]          row-wise top-k, one workgroup per row */
#define GS_KF_TKR_VM 8u          /* [2-byte keys][vm]                       row-wise top-k: wave and stream kernels */
#define GS_KF_HIST 9u            /* [kt]                                    GlobalHistogram */
#define GS_KF_HY_HIST 10u        /* [kt]                                    the two-level plan's histogram */
#define GS_KF_HY_LOCAL 11u       /* [class][kt]                             ... its bucket-local sort, keys only */
#define GS_KF_HY_LOCAL_PAIRS 12u /* [8-byte values][class][kt]              ... and for pairs */
#define GS_KF_COUNT 13u
int gs_debug_registry_dims(uint32_t family, int32_t dims[5]);
int gs_debug_registry_cell(uint32_t family, const int32_t coord[5]);

/* ---- structural entry points (parity tests, MSD split) --------------------
 * GlobalHistogram + Scan only (GPUSortingCUDA/Sort/OneSweep.cu:44-162): writes
 * the four 256-bin histograms (counts, not prefixes) to h_hist[1024] on the
 * host.  Synchronous. */
gs_status gs_onesweep_global_histogram(gs_onesweep* h, const void* d_keys, uint32_t n,
                                       gs_key_type key_type, uint32_t* h_hist, void* stream);
/* GlobalHistogram + Scan, and what the Scan kernel left for the passes (GPUSortingCUDA/Sort/OneSweep.cu:125-162, the
 * store of :141-158): h_rows[q * 256 + d] = the RAW descriptor word of digit d in the first row of pass q, which is
 * (exclusive prefix of histogram q at d) << 2 | FLAG_INCLUSIVE (2) — the reference's passHistogram_q[d] before any tile has run.
 * Synchronous.  (The direct parity check of row A2 of SURVEY.md 8a: tests diff it against the CPU restatement of the reference's Scan.) */
gs_status gs_onesweep_scan(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type key_type, uint32_t* h_rows,
                           void* stream);
/* One stable DigitBinningPass (OneSweep.cu:164-344 / :346-600) on byte `pass`
 * (0..3) from d_keys_in to d_keys_out (values optional, NULL for keys-only).
 * reverse_index != 0 applies the reference's descending rule to this pass.
 * Self-contained (clears state, histograms, scans, runs the one pass).  With
 * pass = 3 this is the multi-GPU MSD partition step. */
gs_status gs_onesweep_digit_pass(gs_onesweep* h, const void* d_keys_in, void* d_keys_out,
                                 const void* d_vals_in, void* d_vals_out, uint32_t n,
                                 uint32_t pass, gs_key_type key_type, int reverse_index,
                                 void* stream);

/* The multi-GPU MSD split in two steps that share ONE histogram + scan of the shard (no reference
 * counterpart).  prepare: top-byte histogram of d_keys[0..n) to h_hist256[256] on the
 * host (synchronous).  partition: the stable DigitBinningPass on the top byte of the SAME buffer and n;
 * must be the next call on this handle (GS_ERR_ARG otherwise). */
gs_status gs_onesweep_msd_prepare(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type key_type,
                                  uint32_t* h_hist256, void* stream);
gs_status gs_onesweep_msd_partition(gs_onesweep* h, const void* d_keys_in, void* d_keys_out,
                                    const void* d_vals_in, void* d_vals_out, uint32_t n, void* stream);

/* ---- profiling hook --------------------------------------------------------
 * Replaces the cudaEvent pair of BatchTiming* (OneSweepDispatcher.cuh:207-229)
 * with per-kernel HIP events recorded on the sort's own stream.
 * Slots: 0 state clear (0 since the clear is folded into the GlobalHistogram kernel), 1 GlobalHistogram,
 * 2 Scan, 3..6 DigitBinningPass 0..3, 7 whole sort. */
#define GS_PROFILE_SLOTS 8
gs_status gs_onesweep_set_profiling(gs_onesweep* h, int enabled);
/* Synchronises the last profiled sort and returns milliseconds per slot. */
gs_status gs_onesweep_get_profile(gs_onesweep* h, float ms[GS_PROFILE_SLOTS]);

/* ---- fixtures exported for parity tests ------------------------------------
 * Replaces: InitRandom<<<256,256>>> keys / pairs (GPUSortingCUDA/UtilityKernels.cuh:53-117).
 * d_vals may be NULL; value_bytes 0/4/8 (value = key, zero-extended for 8). */
gs_status gs_init_random(void* d_keys, void* d_vals, uint32_t value_bytes, uint32_t and_count,
                         uint32_t seed, uint32_t n, void* stream);
/* Replaces: Validate keys / pairs (UtilityKernels.cuh:402-479) + the 4-byte
 * read-back of DispatchValidateKeys/Pairs (OneSweepDispatcher.cuh:365-391),
 * order/type-aware as GPUSortingD3D12/Shaders/Utility.hlsl:147-230.
 * Synchronous; *h_err_count = number of adjacent inversions.  64-bit key types: the keys' order only (d_vals ignored). */
gs_status gs_validate(const void* d_keys, const void* d_vals, uint32_t value_bytes, uint32_t n,
                      gs_key_type key_type, gs_order order, uint32_t* h_err_count, void* stream);

/* ---- multi-GPU MSD split helper (host only; no reference counterpart) ------
 * From the all-reduced top-byte histogram pick the first top-byte bin each of
 * `world` ranks owns: first_bin[0] = 0 ... first_bin[world] = 256. */
gs_status gs_msd_splitters(const uint64_t hist256[256], uint32_t world, uint32_t* first_bin);
/* The same over any number of bins (first_bin[world] = nbins). */
gs_status gs_msd_splitters_n(const uint64_t* hist, uint32_t nbins, uint32_t world, uint32_t* first_bin);
/* Finer split for skewed shards (top-byte buckets can overflow): the 4096-bin histogram of the
 * 12-bit key prefix, bin = top_byte * 16 + (next byte >> 4), read back to the host (synchronous).  A shard sorted
 * by its top two bytes (two gs_onesweep_digit_pass calls: pass 2, then pass 3) is contiguous in that prefix. */
gs_status gs_onesweep_msd_fine_histogram(gs_onesweep* h, const void* d_keys, uint32_t n, gs_key_type key_type,
                                         uint32_t* h_hist4096, void* stream);

/* ---- multi-GPU: one process per GPU, MSD bucket split + RCCL exchange + per-GPU OneSweep -------------------
 * BASELINE.json configs[3].  No reference counterpart (the reference is single-GPU; SURVEY.md 5.8, 8b proposed
 * gs_onesweep_sort_sharded(gs_mgpu*, ...)).  Every rank of the job owns one gs_mgpu context; all calls below that
 * say "collective" must be made by every rank, in the same order.
 *
 * Bootstrap as with NCCL: one rank calls gs_mgpu_get_unique_id and hands the 128 bytes to every rank over whatever
 * it has (MPI, torch.distributed, a file); then every rank calls gs_mgpu_create (collective: ncclCommInitRank).
 * RCCL (librccl.so.1) is loaded on first use; libgpusort.so does not depend on it otherwise. */
#define GS_MGPU_UNIQUE_ID_BYTES 128
typedef struct gs_mgpu gs_mgpu;
gs_status gs_mgpu_get_unique_id(uint8_t id[GS_MGPU_UNIQUE_ID_BYTES]);
/* shard_keys: most keys a rank passes in; capacity (>= shard_keys): most keys a rank can receive (its bucket of the
 * global result; 1.25 x shard_keys is plenty for uniform keys).  Allocates the local sorter's scan state and one
 * scratch array per key/value array (max(shard_keys, capacity) elements).  value_bytes 0 / 4 / 8 as gs_onesweep_create. */
gs_status gs_mgpu_create(gs_mgpu** out, const uint8_t id[GS_MGPU_UNIQUE_ID_BYTES], uint32_t rank, uint32_t world,
                         uint32_t shard_keys, uint32_t capacity, gs_mode mode, uint32_t value_bytes);
/* Options of a sharded-sort context (the library reads no environment variables; gs_mgpu_create uses the defaults). */
typedef struct gs_mgpu_options {
    uint32_t struct_size;   /* sizeof(gs_mgpu_options) */
    int32_t force_exchange; /* 0 (default); 1: a single rank runs partition + exchange too (tests: world == 1 normally just sorts) */
    int32_t overlap;        /* 1 (default): pairs send their values on a second stream / communicator behind the keys; 0: one group */
    int32_t alltoallv;      /* 0 (default): grouped ncclSend / ncclRecv; 1: ncclAllToAllv (also switchable later: gs_mgpu_set_alltoallv) */
    int32_t by_bin;         /* 1 (default): the grouped exchange goes one message per (peer, top byte), so that a bucket offered the two-level plan
                               is landed bin-major and its local sort starts at the plan's second pass (gs_mgpu_last_layout); 0: one message
                               per peer, source-major landing, full local sort (round 5's exchange; what ncclAllToAllv and the 12-bit split always use) */
    gs_onesweep_options sorter;  /* options of the context's local sorter (gs_mgpu_sorter); struct_size 0 = defaults */
} gs_mgpu_options;
void gs_mgpu_options_default(gs_mgpu_options* o);
gs_status gs_mgpu_create_ex(gs_mgpu** out, const uint8_t id[GS_MGPU_UNIQUE_ID_BYTES], uint32_t rank, uint32_t world,
                            uint32_t shard_keys, uint32_t capacity, gs_mode mode, uint32_t value_bytes, const gs_mgpu_options* options);
/* The bucket exchange of the RCCL transport: 0 grouped ncclSend / ncclRecv, 1 ncclAllToAllv.  Every rank must choose alike.
 * Takes effect from the next gs_onesweep_sort_sharded (a harness can time both on one context). */
gs_status gs_mgpu_set_alltoallv(gs_mgpu* ctx, int on);
gs_status gs_mgpu_destroy(gs_mgpu* ctx);
/* The sorted array is the concatenation over ranks of what each rank gets back.  Collective.  d_keys[0..n) (and
 * d_vals) is this rank's shard (n may be 0; unchanged on return); d_out_keys / d_out_vals are caller-owned buffers
 * of `capacity` elements that receive this rank's contiguous range of the global result, *out_n its length.  Stable
 * (received order = source rank, source position).  Asynchronous on `stream` except for ONE wait on a few dozen
 * words (per-peer counts: RCCL's send/recv take them as host integers).  Pairs: the values travel on a second stream and (RCCL)
 * a second communicator behind the keys, and the local sort's GlobalHistogram + Scan run on the received keys meanwhile;
 * gs_mgpu_options::overlap = 0 keeps keys and values in one group, ::alltoallv = 1 / gs_mgpu_set_alltoallv uses ncclAllToAllv
 * instead of grouped send / recv.  GS_ERR_SIZE on EVERY rank if a bucket does not fit `capacity` even at
 * 12-bit-prefix granularity; GS_ERR_COMM on every rank if some rank failed before the histogram gather (see gs_mgpu_check for
 * failures after it).  ARGUMENT errors (GS_ERR_ARG / GS_ERR_SIZE / GS_ERR_MODE: null or misaligned pointers, n > shard_keys, a
 * key type other than the three 32-bit ones) are returned BEFORE the first collective, on the calling rank only: like the
 * arguments of any collective they must be valid on every rank or on none.  64-bit keys are not accepted here: the split
 * works on the top byte of a 32-bit key and the exchange moves 4-byte keys; sort 64-bit keys per GPU (gs_onesweep_sort_keys). */
gs_status gs_onesweep_sort_sharded(gs_mgpu* ctx, const void* d_keys, const void* d_vals, uint32_t n, gs_key_type key_type,
                                   void* d_out_keys, void* d_out_vals, uint32_t* out_n, void* stream);
/* Synchronises `stream` and reports the last call's outcome: GS_ERR_COMM if SOME rank carried an error of its own through the
 * exchange (every rank's status is all-gathered at the end of the call: its peers were served, its own result is not there, and
 * the global result is incomplete), otherwise gs_onesweep_check() of the local sorter.  (A rank that fails BEFORE the histogram
 * gather poisons its row instead, and every rank's gs_onesweep_sort_sharded returns GS_ERR_COMM at once.)  If the last
 * gs_onesweep_sort_sharded itself returned an error on this rank, the gathered words on the device belong to an EARLIER call: nothing
 * is read, GS_ERR_COMM is returned and the context stays marked as failed (its teardown aborts the communicators) until a later
 * call has completed cleanly on every rank. */
gs_status gs_mgpu_check(gs_mgpu* ctx, void* stream);
/* Test hook: the next gs_onesweep_sort_sharded on this rank fails on its own — 1: before the histogram gather, 2: after the plan
 * (as if a HIP launch had failed) — to exercise the failure agreement with the peers.  0 clears it. */
gs_status gs_mgpu_debug_fail(gs_mgpu* ctx, int where);
/* Phase times of the last gs_onesweep_sort_sharded on this rank (HIP events on its stream; synchronises):
 * ms[0] split (histogram + all-gather + plan + the host wait + partition pass), ms[1] bucket exchange,
 * ms[2] local sort, ms[3] total; bytes this rank sent to / received from OTHER ranks; whether the 12-bit split ran. */
gs_status gs_mgpu_get_profile(gs_mgpu* ctx, float ms[4], uint64_t* bytes_sent, uint64_t* bytes_received, uint32_t* fine_split);
/* The exchange plan of the last call (host memory, no synchronisation): [0] keys received, [1] overflow, [2] largest bucket,
 * [3] 1 if the split ran at the 12-bit prefix, then
 * send_counts[world], recv_counts[world], first_bin[world + 1]; `words` >= 4 + 3 * world + 1. */
gs_status gs_mgpu_last_plan(gs_mgpu* ctx, uint32_t* plan, uint32_t words);
gs_onesweep* gs_mgpu_sorter(gs_mgpu* ctx);               /* the local engine (tuning switches, gs_onesweep_check) */
gs_status gs_mgpu_set_force_exchange(gs_mgpu* ctx, int on); /* run split + exchange even with one rank (tests) */
/* How the last gs_onesweep_sort_sharded landed its bucket (host state, no synchronisation): *bin_major = 1 — the bucket exchange went
 * one message per (peer, top byte) and this rank placed the segments top byte by top byte in the local sort's alternate buffer, so the
 * local sort started at the two-level plan's second pass (the sender's split WAS its top-byte partition); 0 — source by source in the
 * output buffer, full local sort (buckets below the two-level plan's size, the 12-bit split, ncclAllToAllv, world 1 without exchange). */
gs_status gs_mgpu_last_layout(gs_mgpu* ctx, uint32_t* bin_major);
int gs_last_rccl_error(void);                             /* ncclResult_t of the last failing RCCL call on this thread */

/* The transport the pipeline runs on: RCCL by default; tests run several ranks on ONE GPU over a host-staged one.
 * Both functions take device pointers and either enqueue on `stream` or complete before returning; 0 = success.
 * exchange: for every array a < n_arrays and every peer p, send_counts[p] elements of elem_bytes[a] bytes from
 * d_send[a] + send_displs[p] go to peer p, which receives them at d_recv[a] + recv_displs[self]; counts and
 * displacements are host arrays of `world` entries, shared by all arrays. */
typedef struct gs_mgpu_transport {
    void* user;
    int (*all_gather_u32)(void* user, const void* d_send, void* d_recv, size_t count, void* stream);
    int (*exchange)(void* user, uint32_t n_arrays, const void* const* d_send, void* const* d_recv, const uint32_t* elem_bytes,
                    const uint32_t* send_counts, const uint32_t* send_displs, const uint32_t* recv_counts,
                    const uint32_t* recv_displs, void* stream);
} gs_mgpu_transport;
gs_status gs_mgpu_create_with_transport_ex(gs_mgpu** out, const gs_mgpu_transport* transport, uint32_t rank, uint32_t world,
                                           uint32_t shard_keys, uint32_t capacity, gs_mode mode, uint32_t value_bytes, const gs_mgpu_options* options);
gs_status gs_mgpu_create_with_transport(gs_mgpu** out, const gs_mgpu_transport* transport, uint32_t rank, uint32_t world,
                                        uint32_t shard_keys, uint32_t capacity, gs_mode mode, uint32_t value_bytes);
/* The plan as a host function (same rule as the device kernel; CPU tests, other transports): table[src * nbins + b] =
 * keys of rank src in MSD bin b. */
gs_status gs_msd_plan(const uint32_t* table, uint32_t nbins, uint32_t world, uint32_t rank, uint32_t capacity, uint32_t* plan);
/* One round of the per-(peer, top byte) bucket exchange as gs_onesweep_sort_sharded runs it (host function, no GPU: CPU tests, other
 * transports).  table[src * 256 + b] = keys of rank src under top byte b (the gathered table of the coarse split); first_bin[world + 1] =
 * the plan's splitters.  Round `round` carries, for every peer p, byte first_bin[p] + round of p's range: send_counts / send_displs[p]
 * (elements, in this rank's shard grouped by top byte) and recv_counts / recv_displs[q] for this rank's own byte first_bin[rank] + round
 * from every source q — landed bin-major (bin_major != 0: byte by byte, sources in rank order inside a byte = the stable top-byte
 * partition of the concatenated sources) or source-major.  *rounds (may be NULL) = rounds of a call = the widest rank's byte count. */
gs_status gs_msd_exchange_round(const uint32_t* table, uint32_t world, uint32_t rank, const uint32_t* first_bin, int bin_major, uint32_t round,
                                uint32_t* send_counts, uint32_t* send_displs, uint32_t* recv_counts, uint32_t* recv_displs, uint32_t* rounds);
/* Test hook: the device plan kernel on a host table (nbins 256 or 4096); synchronous. */
gs_status gs_debug_msd_plan_device(const uint32_t* h_table, uint32_t nbins, uint32_t world, uint32_t rank, uint32_t capacity,
                                   uint32_t* h_plan, void* stream);

/* ---- segmented sort: many independent segments of one array in one call ------------------------------------
 * Replaces: SplitSortAllocateTempMemory / SplitSortPairs / SplitSortFreeTempMemory
 * (GPUSortingCUDA/SegSort/SplitSort/SplitSort.cuh:674-709).  The reference takes the segment STARTS plus the total
 * length; this interface takes CSR offsets: d_offsets[0 .. num_segments] (num_segments + 1 uint32 words in device
 * memory), segment s = [d_offsets[s], d_offsets[s + 1]).
 *
 * Every segment is sorted on its own, in place, and ends up exactly as gs_onesweep_sort_keys / _sort_pairs would leave
 * that slice: stable by key, descending = exact reverse of the stable ascending result, floats by the order-preserving
 * bit flip, values bit-copied.  Empty segments and segments of one element are legal anywhere; elements in front of
 * d_offsets[0] and behind d_offsets[num_segments] are not touched.  32-bit key types only: GS_KEY_UINT64 / INT64 /
 * FLOAT64 return GS_ERR_ARG (out of scope).  1 <= n <= max_keys, 1 <= num_segments <= max_segments (GS_ERR_SIZE).
 *
 * The offsets are validated ON THE DEVICE before anything is loaded through them (non-decreasing, last <= n): with bad
 * offsets nothing is written to keys or values and gs_segsort_check reports GS_ERR_ARG.
 *
 * Length classes (gs_segsort_class_of; GS_SEGSORT_CLASSES of them), each with a kernel of its own, all enqueued by one call:
 *   0  length 0 or 1: nothing to do (also counts the segments that broke the caller's promise, below)
 *   1  2 .. 32: packed, 64 consecutive segments per wave, counting rank inside the segment
 *   2  33 .. 256: one segment per wave, sorted in LDS
 *   3 .. 7  up to 1024 / 2048 / 8192 / 16 384 / 32 768: one segment per workgroup, sorted in LDS by the single-tile sort
 *      (class 6 not with 8-byte values, class 7 keys-only: what 160 KiB of LDS hold)
 *   8  longer than gs_segsort_max_lds_segment(): sorted one by one by the handle's own gs_onesweep engine (the default), or all at
 *      once by four passes on the device (gs_segsort_set_long_route)
 *
 * max_segment_len is a promise by the caller.  Non-zero and <= gs_segsort_max_lds_segment(): the call is asynchronous on
 * `stream`, never touches the host after its launches (it can be captured into a graph) and d_alt* may be NULL; a segment
 * that breaks the promise is left unsorted — noticed on the device — and gs_segsort_check reports GS_ERR_SIZE.  0 (unknown)
 * or larger: long segments are allowed, d_alt* (n elements each, scratch) are required, and on the default long route
 * (GS_SEGSORT_LONG_HOST) the call WAITS ON THE HOST ONCE for the list of long segments (then once per long segment for its two
 * offsets) before it enqueues their sorts.  gs_segsort_set_long_route(h, GS_SEGSORT_LONG_DEVICE) selects a route that never waits
 * (below).
 * One in-flight call per handle. */
#define GS_SEGSORT_CLASSES 9
typedef struct gs_segsort gs_segsort;
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create.  Synchronous (allocates gs_segsort_temp_bytes of device memory). */
gs_status gs_segsort_create(gs_segsort** out, uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes);
gs_status gs_segsort_destroy(gs_segsort* h);
/* Host only.  gs_onesweep_temp_bytes(max_keys) (the embedded engine for long segments) + 4 x max_segments (the class lists: ONE
 * array, filled class by class) + 256 (control block).  The reference needs 12 x max_segments plus small change for its bins
 * (SplitSort.cuh:674-690). */
size_t gs_segsort_temp_bytes(uint32_t max_keys, uint32_t max_segments);
/* Host only: the class a segment of this length falls in (monotone in the length), and the longest segment sorted in LDS:
 * 32 768 keys-only, 16 384 with 4-byte values, 8192 with 8-byte values. */
uint32_t gs_segsort_class_of(uint32_t length, gs_mode mode, uint32_t value_bytes);
uint32_t gs_segsort_max_lds_segment(gs_mode mode, uint32_t value_bytes);
gs_status gs_segsort_sort_keys(gs_segsort* h, void* d_keys, void* d_alt, uint32_t n, const uint32_t* d_offsets,
                               uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type, gs_order order, void* stream);
gs_status gs_segsort_sort_pairs(gs_segsort* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n,
                                const uint32_t* d_offsets, uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type,
                                gs_order order, void* stream);
/* Synchronises `stream` and reports the last call: GS_OK, GS_ERR_ARG (bad offsets: nothing was sorted), GS_ERR_SIZE (a segment
 * longer than promised: that one is unsorted, every other one sorted), or what gs_onesweep_check says about the long segments'
 * sorts.  Every call resets the status word itself. */
gs_status gs_segsort_check(gs_segsort* h, void* stream);
/* Synchronous: counts[c] = segments of class c in the last call, c < GS_SEGSORT_CLASSES; counts[GS_SEGSORT_CLASSES] = the longest
 * segment seen.  words >= GS_SEGSORT_CLASSES + 1. */
gs_status gs_segsort_last_classes(gs_segsort* h, uint32_t* counts, uint32_t words, void* stream);
/* The handle's embedded engine, borrowed (as gs_mgpu_sorter; NULL for a null handle): it sorts the long segments and its rank mode is
 * the one the workgroup classes run with.  For gs_onesweep_set_rank_mode / gs_onesweep_get_rank_mode / gs_onesweep_check, with no call of
 * the handle in flight; the handle destroys it. */
gs_onesweep* gs_segsort_engine(gs_segsort* h);

/* The route of the long segments (class 8), chosen per handle; the default is GS_SEGSORT_LONG_HOST, so a handle that never switches
 * behaves as described above.
 *
 * GS_SEGSORT_LONG_DEVICE: GS_SEGSORT_LONG_PASSES stable 8-bit LSD passes over ALL long segments at once, ping-pong between the caller's
 * buffers and d_alt* (the result is back in the caller's buffers).  The (segment, part) work list — parts of GS_SEGSORT_LONG_PART
 * elements — is built on the device, and each pass is a count, a scan and a scatter launch on fixed grids sized by
 * gs_segsort_long_units: 1 + 3 x GS_SEGSORT_LONG_PASSES launches whatever the number of long segments.  The call NEVER waits on the
 * host, whatever the lengths: with max_segment_len = 0 it can be captured on one linear stream and every node is a kernel launch.  No
 * kernel waits on another workgroup.  A segment starts at any element; nothing is merged or copied afterwards.
 *
 * Results are those of the host route bit for bit, keys and values; max_segment_len, the promise and gs_segsort_last_classes mean what
 * they mean there.  On this route only, after the size checks: GS_ERR_ARG if any two of d_keys, d_vals, d_alt_keys, d_alt_vals (n
 * elements each) overlap.  gs_segsort_check: GS_ERR_ARG (bad offsets), then GS_ERR_HIP if a long segment's counts did not add up (the
 * scatters then wrote nothing), then GS_ERR_SIZE, then what it reports on the host route.
 *
 * It moves about 4 x (4 count + 4 read + 4 write) bytes per key where the engine's two-level plan moves 28: the host route stays the
 * better one for a handful of huge segments (DESIGN.md 3.16 has the measured table). */
#define GS_SEGSORT_LONG_HOST 0u   /* default: one host wait + one per long segment, the embedded engine sorts each */
#define GS_SEGSORT_LONG_DEVICE 1u /* GS_SEGSORT_LONG_PASSES stable 8-bit LSD passes over ALL long segments at once, no host wait */
#define GS_SEGSORT_LONG_PASSES 4u
#define GS_SEGSORT_LONG_PART (4u * GS_SORT_ROWS_TILE) /* elements of a part of a long segment: 4 tiles (measured against 8 and 16) */
/* With no call of the handle in flight and not while a stream is capturing.  The first switch to GS_SEGSORT_LONG_DEVICE allocates
 * gs_segsort_long_temp_bytes(max_keys, max_segments, mode, value_bytes) of device memory, synchronously; the buffers are neither moved
 * nor freed before gs_segsort_destroy (a captured graph stays valid), and switching back keeps them.  GS_ERR_ARG: null handle or
 * unknown route.  GS_ERR_MODE: GS_SEGSORT_LONG_DEVICE on a build flavour without the pass kernels (the tuning and fault-injection
 * libraries).  GS_ERR_HIP: the allocation failed; the route stays GS_SEGSORT_LONG_HOST. */
gs_status gs_segsort_set_long_route(gs_segsort* h, uint32_t route);
/* GS_SEGSORT_LONG_*; 0xffffffff for a null handle. */
uint32_t gs_segsort_get_long_route(gs_segsort* h);
/* Host only: the bound on the (segment, part) units of a device-route call, the fixed grid of its count and scatter launches.  With
 * L = gs_segsort_max_lds_segment(mode, value_bytes), n / GS_SEGSORT_LONG_PART + min(num_segments, n / (L + 1)) — a segment of length len
 * has at most len / GS_SEGSORT_LONG_PART + 1 parts, and at most n / (L + 1) segments are long.  0 for the arguments gs_segsort16_units
 * refuses. */
uint32_t gs_segsort_long_units(uint32_t n, uint32_t num_segments, gs_mode mode, uint32_t value_bytes);
/* Host only.  With U = gs_segsort_long_units(max_keys, max_segments, ..) and G = min(max_segments, max_keys / (L + 1)): the unit
 * descriptors (16 x U), the long-segment records (16 x G), the table and the bases (U x 256 words each), each rounded up to 256 bytes.
 * 0 for arguments gs_segsort_long_units refuses. */
size_t gs_segsort_long_temp_bytes(uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes);
/* gs_segsort_last: report[GS_SEGSORT_R_*].  On the host route every word but R_ROUTE, R_LONG, R_STATUS, R_RANK and R_N is 0. */
#define GS_SEGSORT_R_ROUTE 0     /* the long route the last call was set to */
#define GS_SEGSORT_R_UNITS 1     /* (segment, part) units claimed on the device */
#define GS_SEGSORT_R_LONG 2      /* long segments counted on the device */
#define GS_SEGSORT_R_UNIT_CAP 3  /* gs_segsort_long_units of the call: the fixed grid (0: the long launches were skipped) */
#define GS_SEGSORT_R_FORMS 4     /* GS_SEGSORT_LF_*: the kernel forms of the long route the call launched */
#define GS_SEGSORT_R_STATUS 5    /* the device status: bit 0 bad offsets, bit 1 a promise broken; bit 8: a long segment's counts did not add up */
#define GS_SEGSORT_R_RANK 6      /* the embedded engine's rank mode */
#define GS_SEGSORT_R_N 7
#define GS_SEGSORT_REPORT_WORDS 8
/* v: 0 keys only, 1 4-byte values, 2 8-byte values */
#define GS_SEGSORT_LF_UNITS 1u
#define GS_SEGSORT_LF_COUNT 2u
#define GS_SEGSORT_LF_SCAN 4u
#define GS_SEGSORT_LF_SCATTER 8u /* << (2 x v + rank mode): bits 3 .. 8 */
#define GS_SEGSORT_LF_ALL 0x1ffu
/* Synchronous diagnostics of the last call: report[GS_SEGSORT_R_*], words >= GS_SEGSORT_REPORT_WORDS. */
gs_status gs_segsort_last(gs_segsort* h, uint32_t* report, uint32_t words, void* stream);

/* ---- top-k selection: the first k elements of the sorted order without sorting the rest --------------------
 * No counterpart in the reference project.
 *
 * For 1 <= k <= n the output is exactly the first k elements of what gs_onesweep_sort_keys / _sort_pairs with the same key
 * type and order would leave for that input, keys and values, bit for bit: ascending = the k smallest, descending = the k
 * largest, delivered in sorted order; floats by the order-preserving bit flip (-0 < +0, NaNs by bit pattern: above +inf or
 * below -inf by their sign — the library's order, not a "NaN is largest" rule); ties are deterministic: ascending, among the
 * elements equal to the k-th key those at the LOWEST input positions are taken and equal keys come out in increasing position;
 * descending is the exact reverse of the stable ascending result, so those at the HIGHEST positions are taken and equal keys
 * come out in decreasing position.  Values are bit-copied.  The input arrays are not written; the output arrays hold k
 * elements, must not overlap the input (GS_ERR_ARG) and nothing behind their k-th element is touched.
 *
 * 32-bit key types only: GS_KEY_UINT64 / INT64 / FLOAT64 return GS_ERR_ARG.  k == 0, k > n, k > max_k, n == 0, n > max_keys
 * return GS_ERR_SIZE; NULL or not 16-byte aligned pointers GS_ERR_ARG; select_pairs on a keys-only handle (and the reverse)
 * GS_ERR_MODE.  On a handle with 4-byte values d_vals == NULL means "the value is the element's input position" (uint32): the
 * kernels produce the index themselves, no n-sized index array exists anywhere.
 *
 * Asynchronous on `stream`, no host round trip: every launch is enqueued up front (the output count is k whatever the data), so
 * a call can be captured into a graph.  No kernel waits on another workgroup.  One in-flight call per handle.
 *
 * Routes (gs_topk_last): GS_TOPK_ROUTE_SINGLE_TILE for n up to the single-tile sort's capacity (32 768 keys only, 16 384 with
 * 4-byte values, 8192 with 8-byte values): a copy is sorted in one launch and its head emitted.  GS_TOPK_ROUTE_SELECT otherwise, for
 * every k: a two-level radix select (16 + 16 bits) finds the bit pattern T of the k-th element, gathers the elements in front of T
 * and the wanted share of those equal to T into the output in input order — two reads of the keys, 8 bytes per key, for keys that
 * spread over their top 16 bits, 20 at most — and the handle's embedded engine sorts those k.  GS_TOPK_ROUTE_FULL_SORT is reserved:
 * no handle takes it today. */
typedef struct gs_topk gs_topk;
#define GS_TOPK_ROUTE_NONE 0u
#define GS_TOPK_ROUTE_SELECT 1u
#define GS_TOPK_ROUTE_FULL_SORT 2u
#define GS_TOPK_ROUTE_SINGLE_TILE 3u
/* gs_topk_last report words */
#define GS_TOPK_R_ROUTE 0      /* GS_TOPK_ROUTE_* of the last call; the words below are zero unless it is GS_TOPK_ROUTE_SELECT */
#define GS_TOPK_R_THRESHOLD 1  /* T: the k-th element's key as sortable bits (unsigned order = key order) */
#define GS_TOPK_R_IN_FRONT 2   /* elements strictly in front of T in the requested order (< k) */
#define GS_TOPK_R_EQUAL 3      /* elements equal to T (in_front + equal >= k) */
#define GS_TOPK_R_TAKEN 4      /* how many of those were taken: k - in_front */
#define GS_TOPK_R_CANDIDATES 5 /* elements left after the first level: those that share T's top 16 bits */
#define GS_TOPK_R_LEVEL2 6     /* 1: the second level ran (always on the select route) */
#define GS_TOPK_R_RANGES 7     /* workgroup ranges of level 1 | level 2 << 16 */
#define GS_TOPK_REPORT_WORDS 8
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create; 1 <= max_k <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE).  Synchronous
 * (allocates gs_topk_temp_bytes of device memory). */
gs_status gs_topk_create(gs_topk** out, uint32_t max_keys, uint32_t max_k, gs_mode mode, uint32_t value_bytes);
gs_status gs_topk_destroy(gs_topk* h);
/* Host only.  With e = 4 + value_bytes, c = max(max_k, min(max_keys, 32 768)) (what the embedded engine sorts at most) and
 * every term rounded up to 256 bytes:
 *     max_keys x e            candidate buffer: the elements that share T's top 16 bits, all of them in the worst case
 *   + c x e                   the embedded engine's second buffer
 *   + gs_onesweep_temp_bytes(c)
 *   + 256 x 131 088           histogram slices: 256 workgroup ranges x (65 536 packed 16-bit counters + 16 bytes)
 *   + 3 x 262 144             two recount histograms and the summed histogram
 *   + 4096 + 256              per-range counts of both levels, control block
 * Sort-and-slice needs gs_onesweep_temp_bytes(max_keys) + 2 x max_keys x e. */
size_t gs_topk_temp_bytes(uint32_t max_keys, uint32_t max_k, uint32_t value_bytes);
gs_status gs_topk_select_keys(gs_topk* h, const void* d_keys, uint32_t n, uint32_t k, void* d_out_keys, gs_key_type key_type,
                              gs_order order, void* stream);
/* d_vals == NULL on a handle with 4-byte values: the values are the input positions 0 .. n - 1. */
gs_status gs_topk_select_pairs(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys,
                               void* d_out_vals, gs_key_type key_type, gs_order order, void* stream);
/* Synchronises `stream` and reports the last call: GS_OK, GS_ERR_HIP (a count of the selection did not add up — cannot happen; no
 * store leaves its buffer — or the engine refused the final sort), or what gs_onesweep_check says about the final sort
 * (GS_ERR_TIMEOUT). */
gs_status gs_topk_check(gs_topk* h, void* stream);
/* Synchronous diagnostics of the last call: report[GS_TOPK_R_*], words >= GS_TOPK_REPORT_WORDS. */
gs_status gs_topk_last(gs_topk* h, uint32_t* report, uint32_t words, void* stream);
/* The handle's embedded engine, borrowed (as gs_mgpu_sorter; NULL for a null handle): it runs the single-tile route and the final sort
 * of k, and its rank mode is the one the row-wise tile kernels run with.  For gs_onesweep_set_rank_mode / gs_onesweep_get_rank_mode /
 * gs_onesweep_check, with no call of the handle in flight; the handle destroys it. */
gs_onesweep* gs_topk_engine(gs_topk* h);

/* ---- Row-wise top-k: the first k of every row of a [rows, row_len] matrix in one call, on the same handle ----
 * Row r of the output is what gs_topk_select_keys / _pairs delivers for keys[r * row_stride .. r * row_stride + row_len) with the same
 * k, key type and order, bit for bit: sorted, floats by the order-preserving bit flip, ties by position (ascending the lowest
 * positions, in rising position; descending the exact reverse of the stable ascending result), values bit-copied.  d_vals == NULL on
 * a handle with 4-byte values: the value is the element's position WITHIN ITS ROW (what torch.topk returns as indices).  The inputs
 * are not written.  The output is dense, [rows, k] with row stride k; nothing behind element rows * k is touched.
 *
 * row_stride counts elements, for keys and values alike; any value >= row_len, it need not be a multiple of 4: only the base
 * pointers must be 16-byte aligned, rows may start at any element.
 *
 * GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned base pointer, 64-bit or unknown key type,
 * row_stride < row_len, output overlapping input.  GS_ERR_MODE: pairs call on a keys-only handle or the reverse.  GS_ERR_SIZE:
 * rows, row_len or k zero, k > row_len, k > max_k, (rows - 1) * row_stride + row_len > max_keys (in 64 bits).
 *
 * Asynchronous on `stream`, every launch enqueued up front, no host round trip, no kernel waits on another workgroup; a call can be
 * captured into a graph.  gs_topk_check reports the call as it does a 1-D one.  No temp memory beyond gs_topk_temp_bytes on the
 * one-launch routes (gs_topk_rows_last):
 *   GS_TOPK_ROWS_ROUTE_WAVE    row_len <= 256: one wave per row, the row sorted in LDS, its head written; every k.
 *   GS_TOPK_ROWS_ROUTE_TILE    row_len <= gs_segsort_max_lds_segment: one workgroup per row, the single-tile sort; every k.
 *   GS_TOPK_ROWS_ROUTE_STREAM  longer rows, k <= gs_topk_rows_max_k: one workgroup per row, a radix select on LDS histograms:
 *                              2 to 3 reads of the row (a 4th for a row in which more than gs_topk_rows_max_k elements share the
 *                              top 24 bits of the k-th), the selected elements sorted in LDS, 1 write of k.
 *   GS_TOPK_ROWS_ROUTE_LOOP    everything else, and few, very long rows whatever k is (row_len >= 2^19 and
 *                              rows * (row_len + 7 * 2^19) <= 19 * row_len: 2 rows of 2^19, 4 of 2^20, 10 of 2^22; measured, DESIGN.md
 *                              3.10): the 1-D select route enqueued row by row (rows x its eleven launches and final
 *                              sort, one launch that gathers the rows' status: gs_topk_check and gs_topk_rows_last speak
 *                              for every row).  With two rows or more and a row_stride or k that is no multiple of 4, rows and
 *                              output rows pass through an aligned staging buffer of the handle: max_keys / 2 keys and
 *                              min(max_k, max_keys / 2) outputs, its size fixed by the handle, allocated once by the first
 *                              call that needs it and neither moved nor freed before gs_topk_destroy, so a captured graph stays
 *                              valid whatever calls follow.  That first call allocates synchronously; made while `stream` is
 *                              capturing it returns GS_ERR_MODE instead, launches nothing and leaves the capture intact: make
 *                              one plain call of such a shape on the handle before capturing. */
/* 16-bit keys (GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16), these two entries only: the elements of d_keys and d_out_keys are 2 bytes,
 * read at that width (no widened copy, no staging, no temp memory beyond gs_topk_temp_bytes, which is unchanged).  row_stride, row_len,
 * k, positions and max_keys keep counting ELEMENTS; values stay 4 or 8 bytes under the same element index.  The base pointers stay
 * 16-byte aligned; rows and output rows may start at any element, so at 2-byte alignment.  The overlap test takes the keys' 2-byte
 * extent, and nothing behind element rows * k of either output is written, at 2-byte granularity for the keys.  Everything said above
 * holds on the 16 bits: uint16 sorts as it is, int16 with the sign bit flipped, float16 and bfloat16 by the order-preserving flip (sign
 * bit set: all 16 bits inverted; otherwise the sign bit flipped: -0 < +0, NaNs by bit pattern).
 * Routes: WAVE, TILE and STREAM at the same row lengths as for 32-bit keys.  There is NO LOOP route (the 1-D select is a 32-bit
 * algorithm): a row longer than gs_segsort_max_lds_segment with k > gs_topk_rows_max_k returns GS_ERR_SIZE before anything is
 * launched (gs_topk_rows_last then reports GS_TOPK_ROWS_ROUTE_NONE), and the "few, very long rows" rule is not applied: such shapes
 * take STREAM.  GS_TOPK_ROWS_R_READS is 2 or 3, never 4: the select is exact after two levels (12 + 4 bits). */
#define GS_TOPK_ROWS_ROUTE_NONE 0u
#define GS_TOPK_ROWS_ROUTE_WAVE 1u
#define GS_TOPK_ROWS_ROUTE_TILE 2u
#define GS_TOPK_ROWS_ROUTE_STREAM 3u
#define GS_TOPK_ROWS_ROUTE_LOOP 4u
/* gs_topk_rows_last report words */
#define GS_TOPK_ROWS_R_ROUTE 0   /* GS_TOPK_ROWS_ROUTE_* of the last row-wise call */
#define GS_TOPK_ROWS_R_ROWS 1
#define GS_TOPK_ROWS_R_ROW_LEN 2
#define GS_TOPK_ROWS_R_K 3
#define GS_TOPK_ROWS_R_STATUS 4  /* the device status word: 0, or 1 if a count did not add up (gs_topk_check: GS_ERR_HIP) */
#define GS_TOPK_ROWS_R_READS 5   /* GS_TOPK_ROWS_ROUTE_STREAM: the most reads of its row any row took (2 .. 4; 16-bit keys: 2 .. 3); otherwise 0 */
#define GS_TOPK_ROWS_REPORT_WORDS 8
gs_status gs_topk_select_rows_keys(gs_topk* h, const void* d_keys, uint32_t rows, uint32_t row_len, uint32_t row_stride, uint32_t k,
                                   void* d_out_keys, gs_key_type key_type, gs_order order, void* stream);
gs_status gs_topk_select_rows_pairs(gs_topk* h, const void* d_keys, const void* d_vals, uint32_t rows, uint32_t row_len,
                                    uint32_t row_stride, uint32_t k, void* d_out_keys, void* d_out_vals, gs_key_type key_type,
                                    gs_order order, void* stream);
/* Host only: the largest k the one-launch routes take for rows longer than LDS holds (0 for an invalid mode or value width). */
uint32_t gs_topk_rows_max_k(gs_mode mode, uint32_t value_bytes);
/* Synchronous diagnostics of the last row-wise call: report[GS_TOPK_ROWS_R_*], words >= GS_TOPK_ROWS_REPORT_WORDS. */
gs_status gs_topk_rows_last(gs_topk* h, uint32_t* report, uint32_t words, void* stream);

/* ---- sort of 16-bit keys: GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 at their own width, keys, pairs and argsort -----------------
 * No counterpart in the reference project.  The library's own semantics on 16 bits: uint16 sorts as it is, int16 with the sign bit
 * flipped, float16 and bfloat16 by the order-preserving flip (sign bit set: all 16 bits inverted; otherwise the sign bit flipped:
 * -0 < +0, NaNs by bit pattern); stable by key; descending = the exact reverse of the stable ascending result (equal keys come out in
 * falling position); values are bit-copied; every key bit pattern is preserved exactly (NaN payloads, subnormals, -0).
 *
 * Keys only is a counting sort: one histogram over all 65 536 patterns (the array is cut into ranges, gs_sort16_plan, and every
 * range is read by two workgroups, one per half of the bin space: 4 bytes read per key), a scan, and a fill that writes the sorted
 * array from the histogram (2 bytes written per key) — in place, no n-sized scratch, three launches and a clear.  Pairs and argsort are
 * two stable 8-bit passes (low byte into d_alt_*, high byte back), each a count, a scan and a scatter launch: one workgroup per range
 * walks its tiles in order with running per-digit bases.  No kernel waits on another workgroup.
 *
 * 1 <= n <= max_keys <= GS_MAX_KEYS; base pointers 16-byte aligned; key elements are 2 bytes; nothing at or behind element n of any
 * buffer is written, at 2-byte granularity for the keys.
 * GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned pointer, a key type outside 6 .. 9, any two of the
 * call's buffers overlapping.  GS_ERR_MODE: keys call on a pairs handle or the reverse, gs_sort16_argsort on anything but a handle with
 * 4-byte values (and every sort call on a build flavour without these kernels: the tuning and fault-injection libraries).
 * GS_ERR_SIZE: n == 0 or n > max_keys.
 * Precedence, as in gs_topk_select_*: GS_ERR_ARG for the handle, d_keys, the key type and the order; then GS_ERR_MODE; then GS_ERR_ARG
 * for the value and alternate pointers of a pairs call; then GS_ERR_SIZE; then GS_ERR_ARG for overlapping buffers (the overlap test
 * needs a valid n).
 * Asynchronous on `stream`, every launch enqueued up front, no host round trip: a call can be captured into a graph.  One in-flight
 * call per handle. */
typedef struct gs_sort16 gs_sort16;
#define GS_SORT16_ROUTE_NONE 0u
#define GS_SORT16_ROUTE_KEYS 1u    /* histogram, scan, fill */
#define GS_SORT16_ROUTE_PAIRS 2u   /* two passes of count, scan, scatter (gs_sort16_sort_pairs and gs_sort16_argsort) */
/* gs_sort16_last report words */
#define GS_SORT16_R_ROUTE 0      /* GS_SORT16_ROUTE_* of the last call */
#define GS_SORT16_R_RANGES 1     /* as gs_sort16_plan: ranges, */
#define GS_SORT16_R_PER_RANGE 2  /* elements per range, */
#define GS_SORT16_R_TILE 3       /* tile */
#define GS_SORT16_R_FORMS 4      /* GS_SORT16_F_*: the kernel forms the call launched */
#define GS_SORT16_R_STATUS 5     /* the device status word: 0, or 1 if a count did not add up (gs_sort16_check: GS_ERR_HIP) */
#define GS_SORT16_R_N 6
#define GS_SORT16_R_RANK 7       /* the handle's rank mode */
#define GS_SORT16_REPORT_WORDS 8
#define GS_SORT16_F_HIST 1u
#define GS_SORT16_F_SCAN 2u
#define GS_SORT16_F_FILL 4u
#define GS_SORT16_F_COUNT 8u
#define GS_SORT16_F_PSCAN 16u
#define GS_SORT16_F_SCATTER 32u  /* << (2 x v + rank mode), v = 0 positions made in registers (argsort, first pass), 1 4-byte, 2 8-byte values: bits 5 .. 10 */
#define GS_SORT16_F_ALL 0x7ffu
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create.  Synchronous (allocates gs_sort16_temp_bytes of device memory). */
gs_status gs_sort16_create(gs_sort16** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
gs_status gs_sort16_destroy(gs_sort16* h);
/* Host only.  Keys only: a 256-byte control block + the 65 536-word histogram + its 65 537-word prefix; pairs: the control block + two
 * tables of (range cap) x 256 words.  Independent of max_keys; 0 for an invalid size, mode or value width. */
size_t gs_sort16_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* In place; no scratch array. */
gs_status gs_sort16_sort_keys(gs_sort16* h, void* d_keys, uint32_t n, gs_key_type key_type, gs_order order, void* stream);
/* Result in d_keys / d_vals; d_alt_* are scratch of n elements each. */
gs_status gs_sort16_sort_pairs(gs_sort16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n,
                               gs_key_type key_type, gs_order order, void* stream);
/* Handle with 4-byte values: d_pos is OUTPUT only (the uint32 input positions of the sorted order) and never read on entry: the first
 * pass makes the positions in registers. */
gs_status gs_sort16_argsort(gs_sort16* h, void* d_keys, void* d_pos, void* d_alt_keys, void* d_alt_pos, uint32_t n,
                            gs_key_type key_type, gs_order order, void* stream);
/* Synchronises `stream` and reads the device status word, which every call resets: GS_OK, or GS_ERR_HIP if a count did not add up
 * (cannot happen; no store leaves its buffer either way). */
gs_status gs_sort16_check(gs_sort16* h, void* stream);
/* Synchronous diagnostics of the last call: report[GS_SORT16_R_*], words >= GS_SORT16_REPORT_WORDS. */
gs_status gs_sort16_last(gs_sort16* h, uint32_t* report, uint32_t words, void* stream);
/* Host only: how a sort of n elements is cut — plan[0] ranges, [1] elements per range (a multiple of the tile; the smallest range is
 * one tile), [2] tile (8192 keys only, 4096 pairs), [3] range cap (128 keys only, 512 pairs).  ranges x per-range >= n.  GS_ERR_ARG
 * for a null plan, GS_ERR_MODE for an invalid mode or value width, GS_ERR_SIZE for n == 0 or n > GS_MAX_KEYS. */
gs_status gs_sort16_plan(uint32_t n, gs_mode mode, uint32_t value_bytes, uint32_t plan[4]);
/* The scatter's ranking inside a tile, as gs_onesweep_set_rank_mode: 0 = 64-lane ballot multi-split, 1 = one returning LDS atomic per
 * key; gs_sort16_create probes the device as gs_onesweep_create does.  get: -1 for a null handle. */
gs_status gs_sort16_set_rank_mode(gs_sort16* h, int mode);
int gs_sort16_get_rank_mode(gs_sort16* h);

/* ---- 1-D top-k on 16-bit keys: GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 at their own width, keys, pairs and positions -------------
 * No counterpart in the reference project.  gs_topk_select_* on 2-BYTE ELEMENTS in d_keys and d_out_keys, with a handle of its own.
 *
 * Result.  For 1 <= k <= n the output is, bit for bit, the first k elements of what gs_sort16_sort_keys / _sort_pairs / _argsort with
 * the same key type and order leaves for that input: ordered by the sortable 16 bits (uint16 as it is, int16 with the sign bit
 * flipped, float16 and bfloat16 by the order-preserving flip: -0 < +0, NaNs by bit pattern); ties ascending: the LOWEST positions are
 * taken and equal keys come out in rising position; descending is the exact reverse of the stable ascending result, so the HIGHEST
 * positions are taken and equal keys come out in falling position.  Every key bit pattern is preserved, values are bit-copied.  On a
 * handle with 4-byte values d_vals == NULL means "the value is the element's input position" (uint32): the positions are made in
 * registers, no index array exists anywhere.
 *
 * Buffers.  The inputs are not written.  Key elements are 2 bytes; nothing at or behind element k of an output is written, at 2-byte
 * granularity for the keys (an odd k is legal).  Base pointers are 16-byte aligned.  No output may overlap an input or the other output;
 * the extents are counted in 2-byte elements for the keys, so an output at d_keys + 2 * n bytes is legal.
 *
 * Errors, in this order.  GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned d_keys / d_out_keys, a key type
 * outside 6 .. 9 (the 32-bit key types go to gs_topk_select_*, the 64-bit ones nowhere), a bad order.  GS_ERR_MODE: a keys call on a pairs
 * handle or the reverse.  GS_ERR_ARG: null or misaligned d_out_vals, misaligned d_vals, d_vals == NULL on a handle whose value_bytes is not
 * 4.  GS_ERR_SIZE: n == 0, n > max_keys, k == 0, k > n, k > max_k.  GS_ERR_ARG: overlapping buffers (the test needs valid sizes).
 * GS_ERR_MODE: every select call on a build flavour without these kernels (the tuning and fault-injection libraries).  A refused call
 * launches nothing, writes nothing and leaves GS_TOPK16_ROUTE_NONE in the report.
 *
 * Execution.  Asynchronous on `stream`; every launch is enqueued up front (the output count is k whatever the data), there is no host
 * round trip and every node is a kernel launch, so a call can be captured into a graph.  No kernel waits on another workgroup.  One call
 * in flight per handle.
 *
 * Routes (gs_topk16_last).  bin = sortable bits ^ (descending ? 0xFFFF : 0), so both orders look for the k smallest bins:
 *   GS_TOPK16_ROUTE_TILE    n <= gs_segsort_max_lds_segment(mode, value_bytes): one launch of the row-wise 16-bit wave / tile kernel of
 *                           gs_topk_select_rows_* on the one row.
 *   GS_TOPK16_ROUTE_COUNT   keys only, longer arrays: a histogram of all 65 536 bins, a scan to prefix[65 537], and a fill of outputs
 *                           [0, k) FROM THE PREFIX: the keys are read by the histogram only.  Two histograms (gs_topk16_set_count_histogram;
 *                           measured): from GS_TOPK16_COUNT_SLICES_MIN elements on GS_TOPK16_HIST_SLICES, the per-range
 *                           slices of the SELECT route and their sum (one read of the keys, 2 bytes per key, and a fixed 64 MiB of
 *                           slice traffic); below it GS_TOPK16_HIST_GLOBAL, the histogram kernel of gs_sort16_sort_keys (every range read
 *                           by two workgroups, one per half of the bin space: 4 bytes per key, no slices).
 *   GS_TOPK16_ROUTE_SELECT  pairs and positions, longer arrays: the same histograms and their sum, the threshold bin P with
 *                           in_front < k <= in_front + equal, per-range counts from the histograms, and an ordered scatter (second
 *                           read: 4 bytes per key in total) that puts the elements in front of P and, by position rank, the wanted share
 *                           of those in P into the output in input order; the handle's embedded gs_sort16 pairs handle then sorts
 *                           those k in place.
 * The 16 bits are one level of gs_topk's two-level select: the histogram is exact, there is no second level and no candidate buffer. */
typedef struct gs_topk16 gs_topk16;
#define GS_TOPK16_ROUTE_NONE 0u
#define GS_TOPK16_ROUTE_TILE 1u
#define GS_TOPK16_ROUTE_COUNT 2u
#define GS_TOPK16_ROUTE_SELECT 3u
/* gs_topk16_last report words */
#define GS_TOPK16_R_ROUTE 0      /* GS_TOPK16_ROUTE_* of the last call; words 1 .. 5, 7 and 8 are zero unless it is COUNT or SELECT */
#define GS_TOPK16_R_THRESHOLD 1  /* T: the k-th element's key as sortable 16 bits (unsigned order = key order) */
#define GS_TOPK16_R_IN_FRONT 2   /* elements strictly in front of T in the requested order (< k) */
#define GS_TOPK16_R_EQUAL 3      /* elements equal to T (in_front + equal >= k) */
#define GS_TOPK16_R_TAKEN 4      /* how many of those are in the output: k - in_front */
#define GS_TOPK16_R_RANGES 5     /* workgroup ranges of the histogram: ceil(n / per-range) */
#define GS_TOPK16_R_STATUS 6     /* the device status word: 0, or 1 if a count did not add up (gs_topk16_check: GS_ERR_HIP) */
#define GS_TOPK16_R_PER_RANGE 7  /* elements per range: max(32 768, ceil(ceil(n / 256) / 8192) x 8192); GS_TOPK16_HIST_GLOBAL: as gs_sort16_plan */
#define GS_TOPK16_R_HIST 8       /* GS_TOPK16_ROUTE_COUNT: the histogram that ran, GS_TOPK16_HIST_SLICES or _GLOBAL; SELECT: _SLICES; otherwise 0 */
#define GS_TOPK16_REPORT_WORDS 9
/* the COUNT route's histogram */
#define GS_TOPK16_HIST_AUTO 0u    /* by n: GS_TOPK16_HIST_GLOBAL below GS_TOPK16_COUNT_SLICES_MIN elements, GS_TOPK16_HIST_SLICES from there on */
#define GS_TOPK16_HIST_SLICES 1u
#define GS_TOPK16_HIST_GLOBAL 2u
#define GS_TOPK16_COUNT_SLICES_MIN 134217728u  /* 2^27 */
/* No counterpart in the reference project.  value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create (GS_ERR_MODE);
 * 1 <= max_k <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE).  Synchronous (allocates gs_topk16_temp_bytes of device memory). */
gs_status gs_topk16_create(gs_topk16** out, uint32_t max_keys, uint32_t max_k, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_topk16_destroy(gs_topk16* h);
/* No counterpart in the reference project.  Host only; 0 for invalid sizes, mode or value width.  NO TERM GROWS WITH max_keys.  Every
 * term rounded up to 256 bytes:
 *     256                     control block
 *   + 2 x 262 144             the recount histogram and the summed histogram
 *   + 256 x 131 088           histogram slices: 256 workgroup ranges x (65 536 packed 16-bit counters + 16 bytes)
 * keys only:
 *   + 262 148                 prefix[65 537]
 * pairs:
 *   + 2048                    per-range counts
 *   + max_k x 2 + max_k x value_bytes   the final sort's second buffers
 *   + gs_sort16_temp_bytes(max_k, GS_MODE_PAIRS, value_bytes)   the embedded sorter */
size_t gs_topk16_temp_bytes(uint32_t max_keys, uint32_t max_k, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_topk16_select_keys(gs_topk16* h, const void* d_keys, uint32_t n, uint32_t k, void* d_out_keys, gs_key_type key_type,
                                gs_order order, void* stream);
/* No counterpart in the reference project.  d_vals == NULL on a handle with 4-byte values: the values are the input positions 0 .. n - 1. */
gs_status gs_topk16_select_pairs(gs_topk16* h, const void* d_keys, const void* d_vals, uint32_t n, uint32_t k, void* d_out_keys,
                                 void* d_out_vals, gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project.  Synchronises `stream` and reports the last call: GS_OK, GS_ERR_HIP (a count did not add up —
 * cannot happen; no store leaves its buffer — or the embedded sorter refused the final sort), or what gs_sort16_check says about the
 * final sort of a SELECT call. */
gs_status gs_topk16_check(gs_topk16* h, void* stream);
/* No counterpart in the reference project.  Synchronous diagnostics of the last call: report[GS_TOPK16_R_*], words >= GS_TOPK16_REPORT_WORDS. */
gs_status gs_topk16_last(gs_topk16* h, uint32_t* report, uint32_t words, void* stream);
/* No counterpart in the reference project.  Which histogram the COUNT route runs from the next call on: GS_TOPK16_HIST_AUTO (the
 * default), _SLICES or _GLOBAL; the result is the same bit for bit.  With no call of the handle in flight.  GS_ERR_ARG: null handle, any
 * other value. */
gs_status gs_topk16_set_count_histogram(gs_topk16* h, uint32_t which);

/* ---- row-wise sort: every row of a contiguous [rows, row_len] matrix of 32-bit keys sorted on its own, in one call ------------------
 * No counterpart in the reference project.  Row r is elements [r * row_len, (r + 1) * row_len) of the array; after the call every row
 * holds exactly what gs_onesweep_sort_keys / _sort_pairs leaves for that slice, bit for bit: stable by key, descending = the exact
 * reverse of the row's stable ascending result, floats by the order-preserving bit flip, values bit-copied.  Strided rows are not
 * taken.  Key types GS_KEY_UINT32 / INT32 / FLOAT32.
 *
 * Routes (gs_sort_rows_plan says which; gs_sort_rows_last reports the one taken):
 *   GS_SORT_ROWS_ROUTE_LDS     row_len <= gs_segsort_max_lds_segment(mode, value_bytes): the packed / wave / workgroup kernels of the
 *                              segmented sort on uniform offsets that a small kernel writes into the handle's temp memory.  In place;
 *                              d_alt* are not touched and may be NULL.
 *   GS_SORT_ROWS_ROUTE_PASSES  longer rows: GS_SORT_ROWS_PASSES stable 8-bit LSD passes over all rows at once, ping-pong between the
 *                              caller's buffers and d_alt* (the result is back in the caller's buffers), each a count, a scan and a
 *                              scatter launch behind one clear: 13 launches whatever `rows` is.  Every row is cut into `parts` ranges of
 *                              whole tiles (a tile never straddles two rows); one workgroup per (row, part) counts, one per row scans,
 *                              one per (row, part) walks its tiles in order with running per-digit bases.  No kernel waits on another
 *                              workgroup.  d_alt* are required: rows * row_len elements of scratch each.
 *
 * rows >= 1, row_len >= 1, rows * row_len <= max_keys <= GS_MAX_KEYS; only the base pointers need 16-byte alignment (rows start
 * wherever they start; there is no head-merge step); nothing at or behind element rows * row_len of any buffer is written.
 * GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned d_keys, a key type outside 0 .. 2 (the 64-bit and the
 * 16-bit ones), a bad order; then GS_ERR_MODE: keys call on a pairs handle or the reverse (and every call on a build flavour without
 * these kernels: the tuning and fault-injection libraries); then GS_ERR_ARG for a null or misaligned d_vals; then GS_ERR_SIZE: rows == 0,
 * row_len == 0 or rows * row_len > max_keys; then, on the pass route, GS_ERR_ARG for a null or misaligned d_alt* and for any two of the
 * call's buffers overlapping.
 * Asynchronous on `stream`, every launch enqueued up front, the host is never waited on: a call can be captured into a graph, and
 * every node of a captured call is a kernel launch.  One in-flight call per handle. */
typedef struct gs_sort_rows gs_sort_rows;
#define GS_SORT_ROWS_ROUTE_NONE 0u
#define GS_SORT_ROWS_ROUTE_LDS 1u
#define GS_SORT_ROWS_ROUTE_PASSES 2u
#define GS_SORT_ROWS_TILE 4096u   /* elements a workgroup of the pass route ranks and stages at a time */
#define GS_SORT_ROWS_PCAP 1024u   /* workgroups rows x parts aims at; with parts > 1 it is never above it */
#define GS_SORT_ROWS_MIN_TILES 2u /* tiles of a range at least (a row of fewer tiles is one range) */
#define GS_SORT_ROWS_PASSES 4u
/* gs_sort_rows_plan words */
#define GS_SORT_ROWS_P_ROUTE 0     /* GS_SORT_ROWS_ROUTE_LDS / _PASSES */
#define GS_SORT_ROWS_P_PARTS 1     /* ranges per row (LDS route: 1) */
#define GS_SORT_ROWS_P_PER_PART 2  /* elements per range: a multiple of the tile, parts x per-part >= row_len > (parts - 1) x per-part (LDS route: row_len) */
#define GS_SORT_ROWS_P_TILE 3      /* GS_SORT_ROWS_TILE (LDS route: 0) */
#define GS_SORT_ROWS_P_PASSES 4    /* GS_SORT_ROWS_PASSES (LDS route: 0) */
#define GS_SORT_ROWS_P_CAP 5       /* max(rows, GS_SORT_ROWS_PCAP): rows x parts never exceeds it */
#define GS_SORT_ROWS_PLAN_WORDS 8
/* gs_sort_rows_last report words */
#define GS_SORT_ROWS_R_ROUTE 0     /* GS_SORT_ROWS_ROUTE_* of the last call */
#define GS_SORT_ROWS_R_ROWS 1
#define GS_SORT_ROWS_R_ROW_LEN 2
#define GS_SORT_ROWS_R_PARTS 3     /* as gs_sort_rows_plan */
#define GS_SORT_ROWS_R_FORMS 4     /* GS_SORT_ROWS_F_*: the kernel forms the call launched */
#define GS_SORT_ROWS_R_STATUS 5    /* the device status: 0; bit 0: a row's counts did not add up or a position left its row (pass route); bits 8 .. : the segmented sort's status word (LDS route) */
#define GS_SORT_ROWS_R_RANK 6      /* the handle's rank mode */
#define GS_SORT_ROWS_R_PER_PART 7  /* as gs_sort_rows_plan */
#define GS_SORT_ROWS_REPORT_WORDS 8
#define GS_SORT_ROWS_F_CLEAR 1u
#define GS_SORT_ROWS_F_OFFSETS 2u
#define GS_SORT_ROWS_F_LDS 4u      /* the segmented sort's kernels for the row's length class */
#define GS_SORT_ROWS_F_COUNT 8u
#define GS_SORT_ROWS_F_SCAN 16u
#define GS_SORT_ROWS_F_SCATTER 32u /* << (2 x v + rank mode), v = 0 keys only, 1 4-byte, 2 8-byte values: bits 5 .. 10 */
#define GS_SORT_ROWS_F_ALL 0x7ffu
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create.  Synchronous (allocates gs_sort_rows_temp_bytes of device memory). */
gs_status gs_sort_rows_create(gs_sort_rows** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
gs_status gs_sort_rows_destroy(gs_sort_rows* h);
/* Host only.  With L = gs_segsort_max_lds_segment(mode, value_bytes), R = max_keys / (L + 1) (the most rows of a pass-route call) and
 * U = R == 0 ? 0 : min(max(R, GS_SORT_ROWS_PCAP), max_keys / GS_SORT_ROWS_TILE + R) (the most rows x parts), each term rounded up to
 * 256 bytes: a 256-byte control block + the segmented sort's (64 + max_keys / 33 + 1 words) + the offsets (max_keys + 1 words) + the
 * table and the bases (U x 256 words each).  0 for an invalid size, mode or value width. */
size_t gs_sort_rows_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* Host only: how a call is routed and cut — plan[GS_SORT_ROWS_P_*], GS_SORT_ROWS_PLAN_WORDS words.  Pass route: parts =
 * max(1, min(tiles of a row / GS_SORT_ROWS_MIN_TILES, GS_SORT_ROWS_PCAP / rows)), evened out over whole tiles.  GS_ERR_ARG for a null plan, GS_ERR_MODE for an
 * invalid mode or value width, GS_ERR_SIZE for rows == 0, row_len == 0 or rows * row_len > GS_MAX_KEYS. */
gs_status gs_sort_rows_plan(uint32_t rows, uint32_t row_len, gs_mode mode, uint32_t value_bytes, uint32_t* plan);
/* Result in d_keys; d_alt: scratch of rows * row_len keys (pass route; may be NULL on the LDS route). */
gs_status gs_sort_rows_keys(gs_sort_rows* h, void* d_keys, void* d_alt, uint32_t rows, uint32_t row_len, gs_key_type key_type,
                            gs_order order, void* stream);
/* Result in d_keys / d_vals; d_alt_*: scratch of rows * row_len elements each (pass route; may be NULL on the LDS route). */
gs_status gs_sort_rows_pairs(gs_sort_rows* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t rows,
                             uint32_t row_len, gs_key_type key_type, gs_order order, void* stream);
/* Synchronises `stream` and reads the device status, which every call resets: GS_OK, or GS_ERR_HIP if a row's counts did not add up
 * (cannot happen; the scatter then writes nothing, and no store leaves its row either way). */
gs_status gs_sort_rows_check(gs_sort_rows* h, void* stream);
/* Synchronous diagnostics of the last call: report[GS_SORT_ROWS_R_*], words >= GS_SORT_ROWS_REPORT_WORDS. */
gs_status gs_sort_rows_last(gs_sort_rows* h, uint32_t* report, uint32_t words, void* stream);
/* The ranking inside a tile (the pass route's scatter and the LDS route's workgroup classes), as gs_sort16_set_rank_mode: 0 = 64-lane
 * ballot multi-split, 1 = one returning LDS atomic per key; gs_sort_rows_create probes the device.  get: -1 for a null handle. */
gs_status gs_sort_rows_set_rank_mode(gs_sort_rows* h, int mode);
int gs_sort_rows_get_rank_mode(gs_sort_rows* h);

/* ---- row-wise sort on 16-bit keys: every row of a contiguous [rows, row_len] matrix of GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 ----
 * No counterpart in the reference project.  Row r is the 2-byte elements [r * row_len, (r + 1) * row_len) of the array; after the call
 * every row holds exactly what gs_sort16_sort_pairs / gs_sort16_argsort leaves for that slice alone, bit for bit, with positions
 * relative to the row: stable by the sortable 16 bits, descending = the exact reverse of the row's stable ascending result, floats by
 * the order-preserving bit flip (-0 < +0, NaNs by bit pattern), every key bit pattern preserved, values bit-copied.  Strided rows are
 * not taken.  The 32-bit key types stay with gs_sort_rows_* (which keeps answering GS_ERR_ARG for the 16-bit ones).
 *
 * Routes (the words of gs_sort_rows_plan and gs_sort_rows_last, GS_SORT_ROWS_P_* / _R_* / _ROUTE_*, are reused):
 *   GS_SORT_ROWS_ROUTE_LDS     row_len <= gs_segsort_max_lds_segment(mode, value_bytes) (positions count as 4-byte values): ONE launch
 *                              behind the clear, the 2-byte LDS sorts of the row-wise top-k with k = row_len, in place: one wave per row
 *                              up to 256 elements, one workgroup per row above.  d_alt* are not touched and may be NULL.
 *   GS_SORT_ROWS_ROUTE_PASSES  longer rows: GS_SORT_ROWS16_PASSES stable 8-bit LSD passes over all rows at once, the low byte from the
 *                              caller's buffers into d_alt*, the high byte back, each a count, a scan and a scatter launch behind one
 *                              clear: 7 launches whatever `rows` is.  Rows are cut into parts of whole tiles exactly as gs_sort_rows_plan
 *                              cuts them (GS_SORT_ROWS_TILE, _PCAP, _MIN_TILES).  No kernel waits on another workgroup.  d_alt* are
 *                              required: rows * row_len elements of scratch each.
 *
 * rows >= 1, row_len >= 1, rows * row_len <= max_keys <= GS_MAX_KEYS; only the base pointers need 16-byte alignment (row r starts
 * wherever r * row_len * 2 bytes falls); nothing at or behind element rows * row_len of any buffer is written, at 2-byte granularity
 * for the keys.
 * GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned d_keys, a key type outside 6 .. 9 (the 32- and the
 * 64-bit ones), a bad order; then GS_ERR_MODE: keys call on a pairs handle or the reverse, gs_sort_rows16_argsort on anything but a
 * handle with 4-byte values (and every call on a build flavour without these kernels: the tuning and fault-injection libraries); then
 * GS_ERR_ARG for a null or misaligned d_vals / d_pos; then GS_ERR_SIZE: rows == 0, row_len == 0 or rows * row_len > max_keys; then, on
 * the pass route, GS_ERR_ARG for a null or misaligned d_alt* and for any two of the call's buffers overlapping.  A refused call writes
 * nothing.
 * Asynchronous on `stream`, every launch enqueued up front, the host is never waited on: a call can be captured into a graph on one
 * linear stream, and every node of a captured call is a kernel launch.  One in-flight call per handle. */
typedef struct gs_sort_rows16 gs_sort_rows16;
#define GS_SORT_ROWS16_PASSES 2u
/* gs_sort_rows16_last: report[GS_SORT_ROWS_R_FORMS], the kernel forms the call launched */
#define GS_SORT_ROWS16_F_CLEAR 1u
#define GS_SORT_ROWS16_F_LDS_WAVE 2u  /* tkr16_wave_kernel: rows of up to 256 elements */
#define GS_SORT_ROWS16_F_LDS_TILE 4u  /* tkr16_tile_kernel of the row length's class */
#define GS_SORT_ROWS16_F_COUNT 8u
#define GS_SORT_ROWS16_F_SCAN 16u
#define GS_SORT_ROWS16_F_SCATTER 32u  /* << (2 x v + rank mode), v = 0 keys only, 1 positions made in registers (argsort, first pass), 2 4-byte, 3 8-byte values: bits 5 .. 12 */
#define GS_SORT_ROWS16_F_ALL 0x1fffu
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create.  Synchronous (allocates gs_sort_rows16_temp_bytes of device memory). */
gs_status gs_sort_rows16_create(gs_sort_rows16** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
gs_status gs_sort_rows16_destroy(gs_sort_rows16* h);
/* Host only.  With U as in gs_sort_rows_temp_bytes (the most rows x parts of a pass-route call): a 256-byte control block + the table
 * and the bases (U x 256 words each, rounded up to 256 bytes).  0 for an invalid size, mode or value width. */
size_t gs_sort_rows16_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* Host only: plan[GS_SORT_ROWS_P_*], GS_SORT_ROWS_PLAN_WORDS words, as gs_sort_rows_plan — the same route border and the same cut — with
 * plan[GS_SORT_ROWS_P_PASSES] = GS_SORT_ROWS16_PASSES on the pass route.  Same errors. */
gs_status gs_sort_rows16_plan(uint32_t rows, uint32_t row_len, gs_mode mode, uint32_t value_bytes, uint32_t* plan);
/* Result in d_keys; d_alt: scratch of rows * row_len keys (pass route; may be NULL on the LDS route). */
gs_status gs_sort_rows16_keys(gs_sort_rows16* h, void* d_keys, void* d_alt, uint32_t rows, uint32_t row_len, gs_key_type key_type,
                              gs_order order, void* stream);
/* Result in d_keys / d_vals; d_alt_*: scratch of rows * row_len elements each (pass route; may be NULL on the LDS route). */
gs_status gs_sort_rows16_pairs(gs_sort_rows16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t rows,
                               uint32_t row_len, gs_key_type key_type, gs_order order, void* stream);
/* Handle with 4-byte values: d_pos is OUTPUT only (the uint32 positions within the row of the sorted order) and never read on entry:
 * the kernels make the positions in registers. */
gs_status gs_sort_rows16_argsort(gs_sort_rows16* h, void* d_keys, void* d_pos, void* d_alt_keys, void* d_alt_pos, uint32_t rows,
                                 uint32_t row_len, gs_key_type key_type, gs_order order, void* stream);
/* Synchronises `stream` and reads the device status, which every call resets: GS_OK, or GS_ERR_HIP if a row's counts did not add up
 * (cannot happen; the scatter then writes nothing, and no store leaves its row either way). */
gs_status gs_sort_rows16_check(gs_sort_rows16* h, void* stream);
/* Synchronous diagnostics of the last call: report[GS_SORT_ROWS_R_*], words >= GS_SORT_ROWS_REPORT_WORDS; the forms are GS_SORT_ROWS16_F_*. */
gs_status gs_sort_rows16_last(gs_sort_rows16* h, uint32_t* report, uint32_t words, void* stream);
/* The ranking inside a tile (the pass route's scatter and the LDS route's workgroup kernel), as gs_sort_rows_set_rank_mode. */
gs_status gs_sort_rows16_set_rank_mode(gs_sort_rows16* h, int mode);
int gs_sort_rows16_get_rank_mode(gs_sort_rows16* h);

/* ---- segmented sort on 16-bit keys: many independent segments of one array of GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 in one call ----
 * No counterpart in the reference project.  gs_segsort_* on 2-byte elements: CSR offsets d_offsets[0 .. num_segments] (num_segments + 1
 * uint32 words in device memory, counting elements), segment s = [d_offsets[s], d_offsets[s + 1]).  Every segment is sorted on its own,
 * in place, and ends exactly as gs_sort16_sort_keys / _sort_pairs would leave that slice alone: stable by the sortable 16 bits,
 * descending = the exact reverse of the stable ascending result, floats by the order-preserving bit flip (-0 < +0, NaNs by bit pattern),
 * every key bit pattern preserved, values bit-copied.  Empty segments and segments of one element are legal anywhere.  Elements in front
 * of d_offsets[0] and behind d_offsets[num_segments] are never written — at 2-byte granularity: not even the other half of a dword they
 * share with a segment.  The 32-bit key types stay with gs_segsort_* (which keeps answering GS_ERR_ARG for the 16-bit ones).
 *
 * The offsets are validated ON THE DEVICE before anything is loaded through them (non-decreasing, last <= n): with bad offsets nothing
 * is written and gs_segsort16_check reports GS_ERR_ARG.
 *
 * Length classes: those of gs_segsort_class_of, with the same LDS limits (gs_segsort_max_lds_segment: 32 768 keys-only, 16 384 with
 * 4-byte values or positions, 8192 with 8-byte values; a key occupies a 32-bit register and LDS word while it is ranked).  Classes
 * 1 .. 7 are sorted in LDS by two 8-bit ranking passes, in place.  Class 8 (longer) takes GS_SEGSORT16_PASSES stable 8-bit LSD passes
 * over ALL long segments at once, the low byte from the caller's buffers into d_alt*, the high byte back: the (segment, part) work list
 * — parts of GS_SEGSORT16_PART elements — is built on the device, and each pass is a count, a scan and a scatter launch on fixed
 * grids sized by gs_segsort16_units.  No kernel waits on another workgroup.
 *
 * max_segment_len is a promise by the caller, as in gs_segsort_*: a segment that breaks it is left unsorted — noticed on the device —
 * and gs_segsort16_check reports GS_ERR_SIZE.  Non-zero and <= gs_segsort_max_lds_segment(): d_alt* are not touched and may be NULL.  0
 * (unknown) or larger: long segments are allowed and d_alt* (n elements each, scratch) are required.  UNLIKE gs_segsort_*, the call
 * never waits on the host, whatever the segment lengths: every launch is enqueued up front and a call can be captured into a graph on
 * one linear stream with max_segment_len = 0; every node of a captured call is a kernel launch.
 *
 * 1 <= n <= max_keys, 1 <= num_segments <= max_segments; only the base pointers need 16-byte alignment.
 * GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned d_keys, null d_offsets or one off a 4-byte boundary,
 * a key type outside 6 .. 9 (the 32- and the 64-bit ones), a bad order; then GS_ERR_MODE: keys call on a pairs handle or the reverse,
 * gs_segsort16_argsort on anything but a handle with 4-byte values (and every call on a build flavour without these kernels: the
 * tuning and fault-injection libraries); then GS_ERR_ARG for a null or misaligned d_vals / d_pos; then GS_ERR_SIZE: n == 0,
 * n > max_keys, num_segments == 0 or num_segments > max_segments; then, where long segments are allowed, GS_ERR_ARG for a null or
 * misaligned d_alt* and for any two of the call's buffers overlapping.  A refused call writes nothing.  One in-flight call per handle. */
typedef struct gs_segsort16 gs_segsort16;
#define GS_SEGSORT16_PASSES 2u
#define GS_SEGSORT16_PART (8u * GS_SORT_ROWS_TILE)  /* elements of a part of a long segment: 8 tiles (measured against 4 and 16) */
/* gs_segsort16_last: report[GS_SEGSORT16_R_*] */
#define GS_SEGSORT16_R_UNITS 0     /* (segment, part) units counted on the device (0: no long segment, or the long launches were skipped) */
#define GS_SEGSORT16_R_FORMS 1     /* GS_SEGSORT16_F_*: the kernel forms the call launched */
#define GS_SEGSORT16_R_WG_FORMS 2  /* the workgroup-class kernels among them: bit GS_SEGSORT16_WG_FORM(class, v, rank mode) */
#define GS_SEGSORT16_R_STATUS 3    /* the device status: bit 0 bad offsets, bit 1 a promise broken (the segmented sort's status word); bit 8: a long segment's counts did not add up */
#define GS_SEGSORT16_R_RANK 4      /* the handle's rank mode */
#define GS_SEGSORT16_R_LONG 5      /* long segments counted on the device */
#define GS_SEGSORT16_R_UNIT_CAP 6  /* gs_segsort16_units of the call: the fixed grids (0: the long launches were skipped) */
#define GS_SEGSORT16_R_N 7
#define GS_SEGSORT16_REPORT_WORDS 8
/* v below: 0 keys only, 1 positions made in registers (argsort; in the long route its first pass only), 2 4-byte, 3 8-byte values */
#define GS_SEGSORT16_F_CLASSIFY 1u     /* seg_reset_kernel + seg_classify_kernel */
#define GS_SEGSORT16_F_FILL 2u         /* seg_fill_kernel */
#define GS_SEGSORT16_F_PACKED 4u       /* << v: bits 2 .. 5 */
#define GS_SEGSORT16_F_WAVE 64u        /* << v: bits 6 .. 9 */
#define GS_SEGSORT16_F_UNITS 1024u
#define GS_SEGSORT16_F_COUNT 2048u
#define GS_SEGSORT16_F_SCAN 4096u
#define GS_SEGSORT16_F_SCATTER 8192u   /* << (2 x v + rank mode): bits 13 .. 20 */
#define GS_SEGSORT16_F_ALL 0x1fffffu
/* The workgroup-class kernels that exist: classes 3 .. 5 with every v, class 6 without 8-byte values, class 7 keys only: 16 per rank
 * mode.  Bit = 16 x rank mode + 4 x (class - 3) + v for classes 3 .. 5, 12 + v for class 6, 15 for class 7. */
#define GS_SEGSORT16_WG_FORM(cls, v, rank) (1u << (16u * (rank) + ((cls) <= 5u ? 4u * ((cls) - 3u) + (v) : (cls) == 6u ? 12u + (v) : 15u)))
#define GS_SEGSORT16_WG_ALL 0xffffffffu
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create.  Synchronous (allocates gs_segsort16_temp_bytes of device memory). */
gs_status gs_segsort16_create(gs_segsort16** out, uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes);
gs_status gs_segsort16_destroy(gs_segsort16* h);
/* Host only.  The bound on (segment, part) units of a call, which sizes the tables and the fixed grids of the long route: with
 * L = gs_segsort_max_lds_segment(mode, value_bytes), n / GS_SEGSORT16_PART + min(num_segments, n / (L + 1)) — a segment of length len
 * has at most len / GS_SEGSORT16_PART + 1 parts, and at most n / (L + 1) segments are long.  0 for n == 0, n > GS_MAX_KEYS,
 * num_segments == 0, num_segments > GS_MAX_KEYS or an invalid mode or value width. */
uint32_t gs_segsort16_units(uint32_t n, uint32_t num_segments, gs_mode mode, uint32_t value_bytes);
/* Host only.  With U = gs_segsort16_units(max_keys, max_segments, ..) and G = min(max_segments, max_keys / (L + 1)): a 256-byte
 * control block + the class lists (4 x max_segments) + 16 x U (unit descriptors) + 16 x G (long-segment records) + the table and the
 * bases (U x 256 words each), each rounded up to 256 bytes.  0 for arguments gs_segsort16_units refuses. */
size_t gs_segsort16_temp_bytes(uint32_t max_keys, uint32_t max_segments, gs_mode mode, uint32_t value_bytes);
/* Result in d_keys; d_alt: scratch of n keys (required where long segments are allowed). */
gs_status gs_segsort16_sort_keys(gs_segsort16* h, void* d_keys, void* d_alt, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments,
                                 uint32_t max_segment_len, gs_key_type key_type, gs_order order, void* stream);
/* Result in d_keys / d_vals; d_alt_*: scratch of n elements each (required where long segments are allowed). */
gs_status gs_segsort16_sort_pairs(gs_segsort16* h, void* d_keys, void* d_vals, void* d_alt_keys, void* d_alt_vals, uint32_t n,
                                  const uint32_t* d_offsets, uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type,
                                  gs_order order, void* stream);
/* Handle with 4-byte values: d_pos is OUTPUT only and never read on entry.  For every i inside the segments, d_pos[i] = the ARRAY index
 * (segment start + position in the segment) of the element the order puts at i; a segment of one element gets its own index; d_pos
 * outside the segments, and inside a segment that broke the promise, is not written. */
gs_status gs_segsort16_argsort(gs_segsort16* h, void* d_keys, void* d_pos, void* d_alt_keys, void* d_alt_pos, uint32_t n,
                               const uint32_t* d_offsets, uint32_t num_segments, uint32_t max_segment_len, gs_key_type key_type,
                               gs_order order, void* stream);
/* Synchronises `stream` and reports the last call: GS_OK, GS_ERR_ARG (bad offsets: nothing was sorted), GS_ERR_HIP (a long segment's
 * counts did not add up — cannot happen; the scatters then write nothing), GS_ERR_SIZE (a segment longer than promised: that one is
 * unsorted, every other one sorted).  Every call resets the status itself. */
gs_status gs_segsort16_check(gs_segsort16* h, void* stream);
/* Synchronous, as gs_segsort_last_classes: counts[c] = segments of class c in the last call, counts[GS_SEGSORT_CLASSES] = the longest
 * segment seen.  words >= GS_SEGSORT_CLASSES + 1. */
gs_status gs_segsort16_last_classes(gs_segsort16* h, uint32_t* counts, uint32_t words, void* stream);
/* Synchronous diagnostics of the last call: report[GS_SEGSORT16_R_*], words >= GS_SEGSORT16_REPORT_WORDS. */
gs_status gs_segsort16_last(gs_segsort16* h, uint32_t* report, uint32_t words, void* stream);
/* The ranking inside a tile (the workgroup classes and the long route's scatter), as gs_sort_rows16_set_rank_mode. */
gs_status gs_segsort16_set_rank_mode(gs_segsort16* h, int mode);
int gs_segsort16_get_rank_mode(gs_segsort16* h);

/* ---- segmented top-k: the first k of every segment of one array in one call -------------------------------------------------------
 * No counterpart in the reference project.  Segment s is keys[off[s] .. off[s + 1]) (CSR offsets d_offsets[0 .. num_segments], as
 * gs_segsort_*; elements outside [off[0], off[num_segments]) belong to no segment).  With m_s = min(k, len_s), output row s is
 * out[s * k .. s * k + m_s): bit for bit the first m_s elements that gs_segsort_sort_keys / _sort_pairs would leave in that segment —
 * for len_s >= k what gs_topk_select_keys / _pairs delivers for that slice.  Sorted, floats by the order-preserving bit flip, ties by
 * position (ascending the lowest positions, in rising position; descending the exact reverse of the stable ascending result), values
 * bit-copied.  The output is dense, [num_segments, k] with row stride k.  Slots m_s .. k of a short or empty segment's row are NOT
 * WRITTEN; nothing behind element num_segments * k is touched; the inputs are not written.
 *
 * d_vals == NULL on a handle with 4-byte values: the value is the element's position in the WHOLE ARRAY, off[s] plus the position in
 * the segment (the convention of the segmented argsort).  The kernels produce it themselves: no n-sized index array exists.
 *
 * Key types: GS_KEY_UINT32 / INT32 / FLOAT32; the 64-bit and 16-bit ones return GS_ERR_ARG (16-bit keys: gs_segtopk16_* below).
 *
 * The offsets are validated on the device before anything is loaded through them (non-decreasing, last <= n); with bad offsets no
 * output is written and gs_segtopk_check reports GS_ERR_ARG.  max_segment_len is the promise of gs_segsort_*: 0 = unknown; a segment
 * longer than a non-zero promise gets no output row — noticed on the device — and gs_segtopk_check reports GS_ERR_SIZE.
 *
 * THE CALL NEVER WAITS ON THE HOST, whatever the lengths and whatever max_segment_len is: every launch is enqueued up front on fixed
 * grids (reset, classify, fill, then one kernel per length class that can occur), no kernel waits on another workgroup, nothing is
 * allocated after create, and a call can be captured on one linear stream with every node a kernel launch.
 * Kernels by segment length (the classes of gs_segsort_class_of):
 *   1 .. 32      packed: 64 consecutive segments per wave, a counting rank inside the segment (length 1 is emitted here)
 *   33 .. 256    one wave per segment, the segment sorted in LDS, its head written
 *   classes 3 .. 7, up to gs_segsort_max_lds_segment(): one workgroup per segment, the single-tile sort, its head written; every k
 *   longer       one workgroup per segment, the radix select of GS_TOPK_ROWS_ROUTE_STREAM: k <= gs_topk_rows_max_k (4096)
 * Lengths are known on the device only, so the rule for k is one the host can check: k > gs_topk_rows_max_k is accepted only with a
 * non-zero promise max_segment_len <= gs_segsort_max_lds_segment(mode, value_bytes); otherwise the call returns GS_ERR_SIZE before
 * anything is launched.  There is no row-by-row route and no embedded engine.
 *
 * GS_ERR_ARG: null handle (before anything else is looked at), a null or not 16-byte aligned base pointer (d_offsets: 4-byte aligned),
 * a key type other than the three above, an output ([num_segments * k] elements, computed in 64 bits) overlapping an input or the
 * other output.  GS_ERR_MODE: a keys call on a pairs handle or the reverse; every call on the build flavours without the selection
 * kernels (the tuning and fault-injection libraries).  GS_ERR_SIZE: n, num_segments or k zero or above the handle's maxima, and the
 * rule for k above. */
typedef struct gs_segtopk gs_segtopk;
/* value_bytes 0 (keys only), 4 or 8, as gs_onesweep_create.  Synchronous (allocates gs_segtopk_temp_bytes of device memory).
 * GS_ERR_SIZE: max_keys, max_segments or max_k zero or above GS_MAX_KEYS.  GS_ERR_MODE: mode and value_bytes do not fit. */
gs_status gs_segtopk_create(gs_segtopk** out, uint32_t max_keys, uint32_t max_segments, uint32_t max_k, gs_mode mode, uint32_t value_bytes);
gs_status gs_segtopk_destroy(gs_segtopk* h);
/* Host only: the control block (64 words) and the class lists (max_segments words), 4 bytes each, rounded up to 256 bytes:
 * ((64 + max_segments) * 4 + 255) & ~255.  Independent of max_keys and max_k: no n-sized scratch exists. */
size_t gs_segtopk_temp_bytes(uint32_t max_segments);
gs_status gs_segtopk_select_keys(gs_segtopk* h, const void* d_keys, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments, uint32_t k,
                                 uint32_t max_segment_len, void* d_out_keys, gs_key_type key_type, gs_order order, void* stream);
gs_status gs_segtopk_select_pairs(gs_segtopk* h, const void* d_keys, const void* d_vals, uint32_t n, const uint32_t* d_offsets,
                                  uint32_t num_segments, uint32_t k, uint32_t max_segment_len, void* d_out_keys, void* d_out_vals,
                                  gs_key_type key_type, gs_order order, void* stream);
/* Synchronises `stream` and reports the last call: GS_OK, GS_ERR_ARG (bad offsets: nothing was written), GS_ERR_HIP (a count did not
 * add up in a long segment — cannot happen; that row is unwritten), GS_ERR_SIZE (a segment longer than promised: that row is unwritten,
 * every other one is right), in that order.  Every call resets the status itself. */
gs_status gs_segtopk_check(gs_segtopk* h, void* stream);
/* gs_segtopk_last: report[GS_SEGTOPK_R_*] */
#define GS_SEGTOPK_R_CLASSES 0  /* [GS_SEGSORT_CLASSES] words: segments per class of gs_segsort_class_of (class 0: empty, length 1, and longer than promised) */
#define GS_SEGTOPK_R_LONGEST 9  /* the longest segment seen */
#define GS_SEGTOPK_R_STATUS 10  /* the device status: bit 0 bad offsets, bit 1 a promise broken; bit 8: a count did not add up */
#define GS_SEGTOPK_R_READS 11   /* the most reads of its segment any long segment took (2 .. 4, as GS_TOPK_ROWS_R_READS); 0 without long segments */
#define GS_SEGTOPK_R_FORMS 12   /* GS_SEGTOPK_F_*: the kernel forms the call launched */
#define GS_SEGTOPK_R_RANK 13    /* the rank mode of the tile classes */
#define GS_SEGTOPK_R_K 14
#define GS_SEGTOPK_R_PACKED 15  /* segments the packed kernel emitted: those of length 1 .. 32 within the promise */
#define GS_SEGTOPK_REPORT_WORDS 16
/* the kernel forms of a call, one bit each */
#define GS_SEGTOPK_F_PACKED 1u
#define GS_SEGTOPK_F_WAVE 2u
#define GS_SEGTOPK_F_STREAM 4u
#define GS_SEGTOPK_F_TILE(cls, rank) (8u << (((cls) - 3u) + 5u * (rank))) /* class 3 .. 7, rank mode 0 / 1: bits 3 .. 12 */
#define GS_SEGTOPK_F_VM 0x10000u /* << (0 keys only, 1 positions, 2 4-byte values, 3 8-byte values): the value mode every kernel of the call ran in */
/* Synchronous diagnostics of the last call: report[GS_SEGTOPK_R_*], words >= GS_SEGTOPK_REPORT_WORDS. */
gs_status gs_segtopk_last(gs_segtopk* h, uint32_t* report, uint32_t words, void* stream);
/* The ranking inside a tile (classes 3 .. 7), as gs_sort16_set_rank_mode: 0 = 64-lane ballot multi-split, 1 = returning LDS atomic;
 * probed at create.  With no call of the handle in flight.  get: -1 for a null handle. */
gs_status gs_segtopk_set_rank_mode(gs_segtopk* h, int mode);
int gs_segtopk_get_rank_mode(gs_segtopk* h);

/* ---- segmented top-k on 16-bit keys: GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 -----------------------------------------------------
 * No counterpart in the reference project.  gs_segtopk_* on 2-BYTE ELEMENTS in d_keys and d_out_keys, read once at their own width:
 * row s of the dense [num_segments, k] output holds the first m_s = min(k, len_s) elements that gs_segsort16_sort_keys / _sort_pairs
 * would leave in segment s; slots m_s .. k are NOT WRITTEN — the key stores are 2-byte stores, so an unwritten slot keeps its content
 * even where it shares a 32-bit word with a written one (odd k).  Keys are ordered by the 16-bit order-preserving flip (unsigned as
 * they are, signed with the sign bit flipped, both float formats with all bits of negatives flipped too: -0 < +0, NaNs by bit
 * pattern); ties by position, descending the exact reverse of the stable ascending result.  Offsets, n, k, max_segment_len and the
 * positions count elements; values are 4 or 8 bytes wide under the same index; d_vals == NULL on a 4-byte handle delivers the position
 * in the whole array.  Everything else is what the section above says of gs_segtopk_*: the offsets are validated on the device (bad
 * offsets: nothing written, GS_ERR_ARG at check), a segment longer than a non-zero promise gets no output row (GS_ERR_SIZE at check),
 * the call never waits on the host, allocates nothing after create, needs no n-sized scratch and can be captured on one linear stream
 * with every node a kernel launch; k > gs_topk_rows_max_k (4096) is accepted only with a non-zero promise max_segment_len <=
 * gs_segsort_max_lds_segment(mode, value_bytes) and returns GS_ERR_SIZE before anything is launched otherwise.
 * Kernels by segment length, the classes and the LDS limit of gs_segsort_class_of as in the 32-bit call: packed (1 .. 32), one wave
 * per segment (33 .. 256), one workgroup per segment (classes 3 .. 7), and for longer segments the 16-bit radix select of the row-wise
 * top-k (12 + 4 bits: a segment is read 2 or 3 times, never 4).
 *
 * GS_ERR_ARG: null handle, a null or not 16-byte aligned base pointer (d_offsets: 4-byte aligned; segments and output rows start at
 * 2-byte alignment only), a key type other than the four 16-bit ones, an output overlapping an input or the other output — in 2-byte
 * key sizes, so an output at d_keys + 2 * n bytes is legal.  GS_ERR_MODE and GS_ERR_SIZE as gs_segtopk_select_*. */
typedef struct gs_segtopk16 gs_segtopk16;
/* No counterpart in the reference project.  As gs_segtopk_create; the handle holds nothing that depends on the key width. */
gs_status gs_segtopk16_create(gs_segtopk16** out, uint32_t max_keys, uint32_t max_segments, uint32_t max_k, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_segtopk16_destroy(gs_segtopk16* h);
/* No counterpart in the reference project.  Host only: gs_segtopk_temp_bytes(max_segments), ((64 + max_segments) * 4 + 255) & ~255. */
size_t gs_segtopk16_temp_bytes(uint32_t max_segments);
/* No counterpart in the reference project. */
gs_status gs_segtopk16_select_keys(gs_segtopk16* h, const void* d_keys, uint32_t n, const uint32_t* d_offsets, uint32_t num_segments, uint32_t k,
                                   uint32_t max_segment_len, void* d_out_keys, gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project. */
gs_status gs_segtopk16_select_pairs(gs_segtopk16* h, const void* d_keys, const void* d_vals, uint32_t n, const uint32_t* d_offsets,
                                    uint32_t num_segments, uint32_t k, uint32_t max_segment_len, void* d_out_keys, void* d_out_vals,
                                    gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project.  As gs_segtopk_check: GS_OK, GS_ERR_ARG, GS_ERR_HIP, GS_ERR_SIZE, in that order. */
gs_status gs_segtopk16_check(gs_segtopk16* h, void* stream);
/* No counterpart in the reference project.  The 16-word report of gs_segtopk_last in the same layout: the GS_SEGTOPK_R_* words and
 * GS_SEGTOPK_F_* bits above are reused, there is no second set; words >= GS_SEGTOPK_REPORT_WORDS.  report[GS_SEGTOPK_R_READS] is 2 or
 * 3 here (0 without long segments), never 4. */
gs_status gs_segtopk16_last(gs_segtopk16* h, uint32_t* report, uint32_t words, void* stream);
/* No counterpart in the reference project.  As gs_segtopk_set_rank_mode / _get_rank_mode. */
gs_status gs_segtopk16_set_rank_mode(gs_segtopk16* h, int mode);
int gs_segtopk16_get_rank_mode(gs_segtopk16* h);

/* ---- unique / run-length encode: the distinct keys of an array, their counts, first positions and the inverse map ------------------
 * No counterpart in the reference project.  For n keys of GS_KEY_UINT32 / INT32 / FLOAT32 and an order, with u distinct keys:
 *   out_keys[0 .. u)    the distinct key BIT PATTERNS in the order gs_onesweep_sort_keys would leave them (floats by the order-preserving
 *                       flip).  Equality is BITWISE: -0.0 and +0.0 are two keys and every NaN pattern is a key of its own — unlike
 *                       torch.unique / numpy.unique, which compare values (-0.0 == +0.0 there, and NaNs are placed by their own rules).
 *   out_counts[j]       (uint32) how many inputs equal out_keys[j]; the counts add up to n.
 *   out_first[j]        (uint32) the LOWEST input position that holds out_keys[j], in either order (numpy's return_index).  Descending
 *                       is the exact reverse of the stable ascending sort, so there the lowest position lies at the run's tail.
 *   out_inverse[i]      (uint32, n entries) the j with out_keys[j] bitwise equal to keys[i].
 *   *d_out_num          u, one uint32 ON THE DEVICE, so that a following kernel can use it without a host wait; gs_unique_last reports
 *                       it too.
 * The input is not written.  Every output pointer but d_out_keys may be NULL: not wanted.  The caller provides n elements for each of
 * out_keys, out_counts, out_first and out_inverse and one word at d_out_num; NOTHING AT OR BEHIND ELEMENT u of out_keys, out_counts or
 * out_first IS WRITTEN, and nothing intermediate passes through them.  Base pointers are 16-byte aligned (d_out_num: 4-byte); no
 * buffer of the call overlaps another.  The call is asynchronous on `stream`: every launch is enqueued up front with no host round
 * trip, every node is a kernel launch, and every grid is fixed by n, never by u — a call can be captured into a graph and replayed on
 * new data with another u.  No kernel waits on another workgroup.  One call in flight per handle.  The 64-bit and 16-bit key types
 * return GS_ERR_ARG (a 65 536-bin histogram answers the 16-bit case: gs_unique16_* below).
 *
 * Handles: (GS_MODE_KEYS_ONLY, 0) for keys and counts; (GS_MODE_PAIRS, 4) adds first and inverse — its embedded gs_onesweep sorts
 * (key, position) pairs.  Anything else: GS_ERR_MODE.
 *   gs_unique_keys         either handle: copies the keys into the workspace, sorts them there, then the run-length stage.
 *   gs_unique_positions    the pairs handle only: one kernel copies the keys and writes the positions 0 .. n - 1 beside them, the
 *                          engine's pairs sort, then the run-length stage with the sorted positions as a second input.
 *   gs_unique_consecutive  either handle: the run-length encode of the input AS IT LIES, no sort, no key type: runs of bitwise-equal
 *                          neighbours (torch.unique_consecutive); out_inverse[i] is the index of the run that holds i.  It is the second
 *                          half of the two calls above.
 * The result does not depend on the route the engine takes (single tile, mid, two-level, LSD passes).  Both engines are created
 * with the library's defaults (gs_onesweep_create).
 * The run-length stage: the array is cut into gs_unique_plan's ranges of whole tiles; count (one workgroup per range: the heads of the
 * range — element i is a head when i == 0 or key[i] != key[i - 1] — and its last head's position), scan (one workgroup: heads and last
 * head in front of every range, u), compact (the head of rank r writes out_keys[r] and closes run r - 1: out_counts[r - 1] = its
 * position - the previous head's; the workgroup that holds element n - 1 closes the last run).
 *
 * Errors, in this order.  GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned d_keys / d_out_keys, a key type
 * outside 0 .. 2, a bad order (gs_unique_consecutive has neither).  GS_ERR_MODE: gs_unique_positions on a keys-only handle.
 * GS_ERR_ARG: a misaligned d_out_counts / d_out_first / d_out_inverse / d_out_num.  GS_ERR_SIZE: n == 0 or n > max_keys.  GS_ERR_ARG:
 * any two of the call's buffers overlapping (outputs at their capacity of n elements).  GS_ERR_MODE: every call on a build flavour
 * without these kernels (the tuning and fault-injection libraries).  A refused call launches nothing and leaves route NONE. */
typedef struct gs_unique gs_unique;
#define GS_UNIQUE_ROUTE_NONE 0
#define GS_UNIQUE_ROUTE_KEYS 1
#define GS_UNIQUE_ROUTE_POSITIONS 2
#define GS_UNIQUE_ROUTE_CONSECUTIVE 3
/* gs_unique_last report words */
#define GS_UNIQUE_R_ROUTE 0
#define GS_UNIQUE_R_N 1
#define GS_UNIQUE_R_U 2          /* distinct keys (runs) of the last call */
#define GS_UNIQUE_R_RANGES 3     /* the run-length stage's plan: gs_unique_plan(n) */
#define GS_UNIQUE_R_PER_RANGE 4
#define GS_UNIQUE_R_TILE 5
#define GS_UNIQUE_R_STATUS 6     /* the device status word: 0, or 1 if a count did not add up (gs_unique_check: GS_ERR_HIP) */
#define GS_UNIQUE_R_RANK 7       /* the embedded engine's rank mode (gs_onesweep_get_rank_mode) */
#define GS_UNIQUE_REPORT_WORDS 8
/* No counterpart in the reference project.  1 <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE), then (mode, value_bytes) as above (GS_ERR_MODE),
 * both answered before a device is looked for.  Synchronous (allocates gs_unique_temp_bytes of device memory). */
gs_status gs_unique_create(gs_unique** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_unique_destroy(gs_unique* h);
/* No counterpart in the reference project.  Host only.  With A(x) = (x + 255) & ~255:
 *     A(64 * 4)                            the control block
 *   + 4 * A(1024 * 4)                      per range: heads, last head, heads in front, last head in front
 *   + 2 * A(4 * max_keys)                  the copy of the keys the engine sorts, and its alternate buffer
 *   + 2 * A(4 * max_keys)  pairs only      the positions and their alternate buffer
 *   + gs_onesweep_temp_bytes(max_keys)     the embedded engine
 * 0 for invalid sizes, mode or value width. */
size_t gs_unique_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_unique_keys(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_num, gs_key_type key_type,
                         gs_order order, void* stream);
/* No counterpart in the reference project. */
gs_status gs_unique_positions(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first,
                              void* d_out_inverse, void* d_out_num, gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project. */
gs_status gs_unique_consecutive(gs_unique* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_inverse,
                                void* d_out_num, void* stream);
/* No counterpart in the reference project.  Host only: the run-length stage's plan for n elements: plan[0] ranges (at most 1024),
 * [1] elements per range = ceil(ceil(n / 1024) / tile) * tile, [2] tile (4096).  ranges x per-range >= n.  GS_ERR_ARG for a null plan,
 * GS_ERR_SIZE for n == 0 or n > GS_MAX_KEYS. */
gs_status gs_unique_plan(uint32_t n, uint32_t plan[3]);
/* No counterpart in the reference project.  Synchronises `stream` and reports the last call: GS_ERR_HIP if the heads counted and the
 * heads written disagree (cannot happen; the compact then wrote nothing or stopped) or the engine refused its sort; otherwise, after
 * gs_unique_keys / _positions, what gs_onesweep_check says of the engine (GS_ERR_TIMEOUT); GS_OK. */
gs_status gs_unique_check(gs_unique* h, void* stream);
/* No counterpart in the reference project.  Synchronous diagnostics of the last call: report[GS_UNIQUE_R_*], words >= GS_UNIQUE_REPORT_WORDS. */
gs_status gs_unique_last(gs_unique* h, uint32_t* report, uint32_t words, void* stream);

/* ---- unique / run-length encode on 16-bit keys: one histogram, no sort ------------------------------------------------------------------
 * No counterpart in the reference project.  gs_unique_positions restated for n keys of GS_KEY_UINT16 / INT16 / FLOAT16 / BFLOAT16 at
 * their own width, with u distinct keys:
 *   out_keys[0 .. u)    (2-byte elements) the distinct key BIT PATTERNS in the order gs_sort16_sort_keys would leave them.  Equality is
 *                       BITWISE: -0.0 and +0.0 are two keys and every NaN pattern is a key of its own.
 *   out_counts[j]       (uint32) how many inputs equal out_keys[j]; the counts add up to n.
 *   out_first[j]        (uint32) the LOWEST input position that holds out_keys[j], in either order.
 *   out_inverse[i]      (uint32, n entries) the j with out_keys[j] bitwise equal to keys[i].
 *   *d_out_num          u, one uint32 ON THE DEVICE; gs_unique16_last reports it too.
 * The input is not written.  Every output pointer but d_out_keys may be NULL: not wanted (d_out_num as well, as in gs_unique_*).
 * gs_unique16_unique: the caller provides min(n, 65 536) elements for each of out_keys, out_counts and out_first (u cannot be larger)
 * and n for out_inverse; gs_unique16_consecutive: n elements each (u can reach n).  NOTHING AT OR BEHIND ELEMENT u of out_keys,
 * out_counts or out_first IS WRITTEN, and out_keys is written with 2-byte stores: an unwritten 2-byte neighbour of a written element
 * survives.  Base pointers are 16-byte aligned (d_out_num: 4-byte); no buffer of the call overlaps another.  The call is asynchronous
 * on `stream`: every launch is enqueued up front, every node is a kernel launch, every grid is fixed by n, never by u — a call can be
 * captured into a graph and replayed on new data with another u.  No kernel waits on another workgroup.  One call in flight per handle.
 *
 * One handle kind: there is no sorter to choose.
 *   gs_unique16_unique       A 16-bit key has 65 536 patterns, so one histogram of bin = sortable bits ^ (descending ? 0xFFFF : 0) is the
 *                            exact answer: a clear; the histogram kernel of gs_sort16 on gs_sort16_plan's ranges; with d_out_first the
 *                            lowest position per bin (a filtered atomic minimum into a 65 536-word table); one workgroup that scans the
 *                            non-empty bins, writes u, the table of the bins' ranks, out_keys, out_counts and out_first; with
 *                            d_out_inverse the lookup out_inverse[i] = rank[bin(keys[i])].  No sort, no scratch that grows with n.
 *                            The lookup has two forms, chosen by n (GS_UNIQUE16_INVERSE_LDS_MIN; gs_unique16_set_inverse_form): the
 *                            rank table in LDS (one workgroup per range of at most 256), or gathered from global memory.
 *   gs_unique16_consecutive  the run-length encode of the input AS IT LIES (torch.unique_consecutive): no key type, no order.  The
 *                            count / scan / compact stage of gs_unique_consecutive on 2-byte loads, on gs_unique_plan's ranges.
 *
 * Errors, in this order.  GS_ERR_ARG: null handle (before anything else is looked at); null or misaligned d_keys / d_out_keys, a key
 * type outside the four 16-bit ones, a bad order (gs_unique16_consecutive has neither); a misaligned d_out_counts / d_out_first /
 * d_out_inverse / d_out_num.  GS_ERR_SIZE: n == 0 or n > max_keys.  GS_ERR_ARG: any two of the call's buffers overlapping (outputs at
 * the capacities above).  GS_ERR_MODE: every call on a build flavour without these kernels (the tuning and fault-injection
 * libraries).  A refused call launches nothing and leaves route NONE. */
typedef struct gs_unique16 gs_unique16;
#define GS_UNIQUE16_ROUTE_NONE 0
#define GS_UNIQUE16_ROUTE_HISTOGRAM 1
#define GS_UNIQUE16_ROUTE_CONSECUTIVE 2
/* gs_unique16_last report words */
#define GS_UNIQUE16_R_ROUTE 0
#define GS_UNIQUE16_R_N 1
#define GS_UNIQUE16_R_U 2          /* distinct keys (runs) of the last call */
#define GS_UNIQUE16_R_STATUS 3     /* the device status word: 0, or 1 if a count did not add up (gs_unique16_check: GS_ERR_HIP) */
#define GS_UNIQUE16_R_RAN 4        /* GS_UNIQUE16_K_* bits: the optional kernels the last call launched */
#define GS_UNIQUE16_R_RANGES 5     /* HISTOGRAM: gs_sort16_plan(n) of the histogram; CONSECUTIVE: gs_unique_plan(n) */
#define GS_UNIQUE16_R_PER_RANGE 6
#define GS_UNIQUE16_R_TILE 7
#define GS_UNIQUE16_R_FIRST_RANGES 8    /* workgroups of the first-position kernel: ranges of max(4, ceil(ceil(n / 256) / 8192)) tiles of 8192 */
#define GS_UNIQUE16_R_INVERSE_RANGES 9  /* workgroups of the inverse: LDS ranges of max(8, ceil(ceil(n / 256) / 8192)) tiles; GATHER one tile each */
#define GS_UNIQUE16_REPORT_WORDS 10
#define GS_UNIQUE16_K_FIRST 1u           /* the first-position kernel (d_out_first given) */
#define GS_UNIQUE16_K_INVERSE_LDS 2u     /* the inverse with the rank table in LDS */
#define GS_UNIQUE16_K_INVERSE_GATHER 4u  /* the inverse gathering from the global rank table */
/* gs_unique16_set_inverse_form */
#define GS_UNIQUE16_INVERSE_AUTO 0
#define GS_UNIQUE16_INVERSE_LDS 1
#define GS_UNIQUE16_INVERSE_GATHER 2
/* AUTO: the gather below this many keys, the LDS table from there on (measured: DESIGN.md 3.22) */
#define GS_UNIQUE16_INVERSE_LDS_MIN (1u << 22)
/* No counterpart in the reference project.  1 <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE), answered before a device is looked for.
 * Synchronous (allocates gs_unique16_temp_bytes of device memory). */
gs_status gs_unique16_create(gs_unique16** out, uint32_t max_keys);
/* No counterpart in the reference project. */
gs_status gs_unique16_destroy(gs_unique16* h);
/* No counterpart in the reference project.  Host only.  With A(x) = (x + 255) & ~255:
 *     A(64 * 4)            the control block
 *   + A(65536 * 4)         the histogram (directly behind the control block: one clear)
 *   + A(65536 * 4)         the first position per bin
 *   + A(65536 * 2)         the rank per bin
 *   + 4 * A(1024 * 4)      the run-length stage, per range: heads, last head, heads in front, last head in front
 * = 672 000 bytes whatever max_keys is.  0 for max_keys == 0 or above GS_MAX_KEYS. */
size_t gs_unique16_temp_bytes(uint32_t max_keys);
/* No counterpart in the reference project. */
gs_status gs_unique16_unique(gs_unique16* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first,
                             void* d_out_inverse, void* d_out_num, gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project. */
gs_status gs_unique16_consecutive(gs_unique16* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_inverse,
                                  void* d_out_num, void* stream);
/* No counterpart in the reference project.  Synchronises `stream` and reports the last call: GS_ERR_HIP if a count did not add up
 * (cannot happen; the kernels behind then wrote nothing); GS_OK. */
gs_status gs_unique16_check(gs_unique16* h, void* stream);
/* No counterpart in the reference project.  Synchronous diagnostics of the last call: report[GS_UNIQUE16_R_*], words >=
 * GS_UNIQUE16_REPORT_WORDS. */
gs_status gs_unique16_last(gs_unique16* h, uint32_t* report, uint32_t words, void* stream);
/* No counterpart in the reference project.  Which form of the inverse lookup gs_unique16_unique runs from the next call on:
 * GS_UNIQUE16_INVERSE_AUTO (by n, the default), _LDS or _GATHER; the result is the same bit for bit.  GS_ERR_ARG for a null handle
 * or another value. */
gs_status gs_unique16_set_inverse_form(gs_unique16* h, uint32_t which);

/* ---- reduce by key: one sum, minimum or maximum per distinct key ----------------------------------------------------------------------
 * No counterpart in the reference project.  For n keys of GS_KEY_UINT32 / INT32 / FLOAT32, n values of one gs_value_type and an order,
 * with u distinct keys:
 *   out_keys[0 .. u)    exactly what gs_unique_keys delivers: the distinct key BIT PATTERNS in the engine's order.  Equality is BITWISE.
 *   out_values[j]       (the value type) the reduction, by one gs_reduce_op, of all values whose key equals out_keys[j].
 *   out_counts[j]       (uint32) how many inputs equal out_keys[j]; the counts add up to n.
 *   *d_out_num          u, one uint32 ON THE DEVICE; gs_reduce_last reports it too.
 * It is what unique(return_inverse) + index_add_ / scatter_reduce computes, without the inverse, without a gather and without atomics
 * on the values: a stable sort of (key, value) pairs followed by one segmented reduction.
 *
 * The operations.
 *   GS_REDUCE_SUM on integers wraps modulo 2^32 / 2^64 (signed and unsigned are the same bits).
 *   GS_REDUCE_MIN / _MAX on integers are the usual ones.
 *   GS_REDUCE_MIN / _MAX on floats use this library's TOTAL ORDER of float keys, the sortable-bits order
 *       -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN
 *     They return one of the inputs bit for bit and are exact and independent of the order of the inputs.  THIS DIFFERS from torch.amin /
 *     amax (a NaN in the run makes the result NaN) and from fmin / fmax (NaNs are dropped): here a negative NaN is the smallest value, a
 *     positive NaN the largest, and -0.0 lies below +0.0.
 *   GS_REDUCE_SUM on floats is the fold of the run's values in the STABLE SORTED ORDER: for ascending the order of the input, for
 *     descending its exact reverse (descending is the reverse of the stable ascending sort, as for gs_unique_positions).  The values
 *     are combined in a tree fixed by n and the run's place in the sorted array (eight values per thread left to right, the threads of
 *     a wave by a scan of distances 1 .. 32, then waves, tiles and ranges left to right); the tree never depends on timing, on how the
 *     grid is scheduled or on the route the engine takes.  No identity element is combined in anywhere: a run of length 1 returns its
 *     value bit for bit (NaN payloads included) and a run of -0.0s returns -0.0.  Consequences: two calls on the same input give
 *     bitwise identical output; the result is NOT the left-to-right sequential sum; ascending and descending may differ in the last bits.
 *
 * The inputs are not written.  d_out_counts and d_out_num may be NULL: not wanted.  The caller provides n elements for each of
 * out_keys, out_values and out_counts and one word at d_out_num; NOTHING AT OR BEHIND ELEMENT u of out_keys, out_values or out_counts IS
 * WRITTEN, and nothing intermediate passes through them.  Base pointers are 16-byte aligned (d_out_num: 4-byte); no two of the call's
 * buffers overlap (keys, values, the three outputs, d_out_num, and the handle's own workspace: seven, pairwise).  The call is
 * asynchronous on `stream`: every launch is enqueued up front with no host round trip, every node is a kernel launch, and every grid
 * is fixed by n, never by u — a call can be captured into a graph and replayed on new data with another u.  No kernel waits on
 * another workgroup and no value goes through an atomic.  One call in flight per handle.
 *
 * A handle is made for one value WIDTH (4 or 8 bytes); its embedded gs_onesweep sorts (key, value) pairs of that width.
 *   gs_reduce_by_key              one kernel copies keys and values into the workspace, gs_onesweep_sort_pairs runs on the copy, then
 *                                 the reduce stage.
 *   gs_reduce_by_key_consecutive  the stage alone on the input AS IT LIES: runs of bitwise-equal neighbouring keys are reduced (thrust's
 *                                 reduce_by_key); no key type, no order.
 * The stage works on gs_unique_plan's ranges of whole tiles, in three launches: count (one workgroup per range: its heads, its last
 * head's position and its open partial — the reduction from its last head to its end, or of the whole range if it holds no head),
 * scan (one workgroup: heads and last head in front of every range, u, and the carry into every range), reduce (a segmented scan per
 * tile; the head of rank r writes out_keys[r] and closes run r - 1: its count and its total, each written exactly once; the thread
 * that holds element n - 1 closes the last run).
 *
 * Errors, in this order.  GS_ERR_ARG: null handle (before anything else is looked at); null or misaligned d_keys / d_values / d_out_keys
 * / d_out_values; a key type outside 0 .. 2, a bad order (gs_reduce_by_key_consecutive has neither); a value type outside 0 .. 5, an
 * op outside 0 .. 2.  GS_ERR_MODE: a value type whose width is not the handle's.  GS_ERR_ARG: a misaligned d_out_counts / d_out_num.
 * GS_ERR_SIZE: n == 0 or n > max_keys.  GS_ERR_ARG: any two of the seven buffers overlapping (outputs at their capacity of n elements).
 * GS_ERR_MODE: every call on a build flavour without these kernels (the tuning and fault-injection libraries).  A refused call
 * launches nothing and leaves route NONE. */
typedef struct gs_reduce gs_reduce;
typedef enum gs_value_type {
    GS_VALUE_INT32 = 0,
    GS_VALUE_UINT32 = 1,
    GS_VALUE_FLOAT32 = 2,
    GS_VALUE_INT64 = 3,
    GS_VALUE_UINT64 = 4,
    GS_VALUE_FLOAT64 = 5
} gs_value_type;
typedef enum gs_reduce_op { GS_REDUCE_SUM = 0, GS_REDUCE_MIN = 1, GS_REDUCE_MAX = 2 } gs_reduce_op;
#define GS_REDUCE_ROUTE_NONE 0
#define GS_REDUCE_ROUTE_SORTED 1
#define GS_REDUCE_ROUTE_CONSECUTIVE 2
/* gs_reduce_last report words */
#define GS_REDUCE_R_ROUTE 0
#define GS_REDUCE_R_N 1
#define GS_REDUCE_R_U 2           /* distinct keys (runs) of the last call */
#define GS_REDUCE_R_RANGES 3      /* the stage's plan: gs_unique_plan(n) */
#define GS_REDUCE_R_PER_RANGE 4
#define GS_REDUCE_R_TILE 5
#define GS_REDUCE_R_STATUS 6      /* the device status word: 0, or 1 if a count did not add up (gs_reduce_check: GS_ERR_HIP) */
#define GS_REDUCE_R_RANK 7        /* the embedded engine's rank mode (gs_onesweep_get_rank_mode) */
#define GS_REDUCE_R_VALUE_TYPE 8  /* the gs_value_type of the last call */
#define GS_REDUCE_R_OP 9          /* its gs_reduce_op */
#define GS_REDUCE_REPORT_WORDS 10
/* No counterpart in the reference project.  1 <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE), then value_bytes 4 or 8 (GS_ERR_MODE), both
 * answered before a device is looked for.  Synchronous (allocates gs_reduce_temp_bytes of device memory). */
gs_status gs_reduce_create(gs_reduce** out, uint32_t max_keys, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_reduce_destroy(gs_reduce* h);
/* No counterpart in the reference project.  Host only.  With A(x) = (x + 255) & ~255:
 *     A(64 * 4)                            the control block
 *   + 4 * A(1024 * 4)                      per range: heads, last head, heads in front, last head in front
 *   + 2 * A(1024 * 8)                      per range: the open partial and the carry (8 bytes each, whatever the width)
 *   + 2 * A(4 * max_keys)                  the copy of the keys the engine sorts, and its alternate buffer
 *   + 2 * A(value_bytes * max_keys)        the copy of the values, and its alternate buffer
 *   + gs_onesweep_temp_bytes(max_keys)     the embedded engine
 * 0 for invalid sizes or value width. */
size_t gs_reduce_temp_bytes(uint32_t max_keys, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_reduce_by_key(gs_reduce* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values,
                           void* d_out_counts, void* d_out_num, gs_key_type key_type, gs_order order, gs_value_type value_type, gs_reduce_op op,
                           void* stream);
/* No counterpart in the reference project. */
gs_status gs_reduce_by_key_consecutive(gs_reduce* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values,
                                       void* d_out_counts, void* d_out_num, gs_value_type value_type, gs_reduce_op op, void* stream);
/* No counterpart in the reference project.  Synchronises `stream` and reports the last call: GS_ERR_HIP if the heads counted and the
 * heads written disagree (cannot happen; the reduce then wrote nothing or stopped) or the engine refused its sort; otherwise, after
 * gs_reduce_by_key, what gs_onesweep_check says of the engine (GS_ERR_TIMEOUT); GS_OK. */
gs_status gs_reduce_check(gs_reduce* h, void* stream);
/* No counterpart in the reference project.  Synchronous diagnostics of the last call: report[GS_REDUCE_R_*], words >= GS_REDUCE_REPORT_WORDS. */
gs_status gs_reduce_last(gs_reduce* h, uint32_t* report, uint32_t words, void* stream);

/* ---- unique / run-length encode on 64-bit keys: GS_KEY_UINT64 / INT64 / FLOAT64 ------------------------------------------------------------
 * No counterpart in the reference project.  gs_unique_* restated for n keys of 8 bytes, as gs_unique16_* restates it for 2-byte keys:
 * the outputs, what may be NULL, what is never written (NOTHING AT OR BEHIND ELEMENT u of out_keys, out_counts or out_first), the
 * alignment, the asynchrony (every node a kernel, every grid fixed by n through gs_unique_plan, capturable and replayable with another
 * u), one call in flight per handle, the three routes and the two handles ((GS_MODE_KEYS_ONLY, 0): keys and counts; (GS_MODE_PAIRS, 4):
 * first and inverse as well) are those of gs_unique_*.  What differs:
 *   - d_keys and d_out_keys hold 8-byte elements; out_keys are the distinct BIT PATTERNS in the order gs_onesweep_sort_keys leaves
 *     64-bit keys (floats by the order-preserving flip), and equality is BITWISE on all 64 bits: -0.0 and +0.0 are two keys, every NaN
 *     pattern is one of its own.  A head is a key that differs from its left neighbour in either word.
 *   - key types are 3 .. 5; the 32-bit and the 16-bit key types return GS_ERR_ARG (gs_unique_*, gs_unique16_*).
 *   - counts, first, inverse and *d_out_num stay uint32 (n <= GS_MAX_KEYS); out_first is the LOWEST input position in either order.
 *   - the overlap check takes 8 n bytes for d_keys and d_out_keys and 4 n for the other outputs.
 *   - both handles' embedded gs_onesweep keep their defaults: the engine's 64-bit route has no position-chain plan, so the caveat of
 *     gs_unique_create does not arise.  The engine drops constant bytes of the keys in pairs on the device: keys below 2^32 (ids) cost
 *     four passes, not eight.
 * The run-length stage is the one of gs_unique_* on 8-byte loads (four 16-byte loads per thread and tile of 4096; the left neighbour
 * of a thread's eight keys comes from the lane below as both words, lane 0 reads it from memory); the scan kernel between count and
 * compact is the same kernel.
 *
 * Errors, in this order, as gs_unique_*.  GS_ERR_ARG: null handle (before anything else is looked at), null or misaligned d_keys /
 * d_out_keys, a key type outside 3 .. 5, a bad order (gs_unique64_consecutive has neither).  GS_ERR_MODE: gs_unique64_positions on a
 * keys-only handle.  GS_ERR_ARG: a misaligned d_out_counts / d_out_first / d_out_inverse / d_out_num.  GS_ERR_SIZE: n == 0 or
 * n > max_keys.  GS_ERR_ARG: any two of the call's buffers overlapping (outputs at their capacity of n elements).  GS_ERR_MODE: every
 * call on a build flavour without these kernels (the tuning and fault-injection libraries).  A refused call launches nothing and
 * leaves route NONE.  Routes and report words are gs_unique's. */
typedef struct gs_unique64 gs_unique64;
#define GS_UNIQUE64_ROUTE_NONE 0
#define GS_UNIQUE64_ROUTE_KEYS 1
#define GS_UNIQUE64_ROUTE_POSITIONS 2
#define GS_UNIQUE64_ROUTE_CONSECUTIVE 3
/* gs_unique64_last report words: those of gs_unique_last */
#define GS_UNIQUE64_R_ROUTE 0
#define GS_UNIQUE64_R_N 1
#define GS_UNIQUE64_R_U 2
#define GS_UNIQUE64_R_RANGES 3
#define GS_UNIQUE64_R_PER_RANGE 4
#define GS_UNIQUE64_R_TILE 5
#define GS_UNIQUE64_R_STATUS 6
#define GS_UNIQUE64_R_RANK 7
#define GS_UNIQUE64_REPORT_WORDS 8
/* No counterpart in the reference project.  1 <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE), then (mode, value_bytes) as gs_unique_create
 * (GS_ERR_MODE), both answered before a device is looked for.  Synchronous (allocates gs_unique64_temp_bytes of device memory). */
gs_status gs_unique64_create(gs_unique64** out, uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_unique64_destroy(gs_unique64* h);
/* No counterpart in the reference project.  Host only.  With A(x) = (x + 255) & ~255:
 *     A(64 * 4)                            the control block
 *   + 4 * A(1024 * 4)                      per range: heads, last head, heads in front, last head in front
 *   + 2 * A(8 * max_keys)                  the copy of the keys the engine sorts, and its alternate buffer
 *   + 2 * A(4 * max_keys)  pairs only      the positions and their alternate buffer
 *   + gs_onesweep_temp_bytes(max_keys)     the embedded engine
 * 0 for invalid sizes, mode or value width. */
size_t gs_unique64_temp_bytes(uint32_t max_keys, gs_mode mode, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_unique64_keys(gs_unique64* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_num,
                           gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project. */
gs_status gs_unique64_positions(gs_unique64* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_first,
                                void* d_out_inverse, void* d_out_num, gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project. */
gs_status gs_unique64_consecutive(gs_unique64* h, const void* d_keys, uint32_t n, void* d_out_keys, void* d_out_counts, void* d_out_inverse,
                                  void* d_out_num, void* stream);
/* No counterpart in the reference project.  As gs_unique_check. */
gs_status gs_unique64_check(gs_unique64* h, void* stream);
/* No counterpart in the reference project.  As gs_unique_last: report[GS_UNIQUE64_R_*], words >= GS_UNIQUE64_REPORT_WORDS. */
gs_status gs_unique64_last(gs_unique64* h, uint32_t* report, uint32_t words, void* stream);

/* ---- reduce by key on 64-bit keys: GS_KEY_UINT64 / INT64 / FLOAT64 -------------------------------------------------------------------------
 * No counterpart in the reference project.  gs_reduce_* restated for n keys of 8 bytes: the outputs, the operations (integer sums wrap;
 * MIN / MAX on floats follow the library's total order of floats and return one of the inputs bit for bit), what may be NULL, what is
 * never written (NOTHING AT OR BEHIND ELEMENT u of out_keys, out_values or out_counts), the alignment, the seven buffers that must not
 * overlap, the asynchrony (every node a kernel, every grid fixed by n through gs_unique_plan, capturable), one call in flight per
 * handle, one value WIDTH (4 or 8 bytes) per handle and the two routes are those of gs_reduce_*.  What differs:
 *   - d_keys and d_out_keys hold 8-byte elements; out_keys are exactly what gs_unique64_keys delivers; equality is BITWISE on 64 bits.
 *   - key types are 3 .. 5; the 32-bit and the 16-bit key types return GS_ERR_ARG.
 *   - counts and *d_out_num stay uint32; the overlap check takes 8 n bytes for d_keys and d_out_keys.
 * GS_REDUCE_SUM on floats is THE SAME TREE as gs_reduce_*: eight values per thread left to right, the threads of a wave by a scan of
 * distances 1 .. 32, then waves, tiles and ranges left to right, over gs_unique_plan's ranges; no identity element is combined in.  The
 * tree depends on n and on where the runs lie, not on the width of the keys: ON KEYS THAT ARE ZERO-EXTENDED 32-BIT KEYS (of
 * GS_KEY_UINT32, sorted as GS_KEY_UINT64) THE REDUCED VALUES ARE BIT FOR BIT THOSE OF gs_reduce_by_key, and two calls, or two handles,
 * give bitwise identical output.
 *
 * Errors, in this order, as gs_reduce_*.  GS_ERR_ARG: null handle (before anything else is looked at); null or misaligned d_keys /
 * d_values / d_out_keys / d_out_values; a key type outside 3 .. 5, a bad order (gs_reduce64_by_key_consecutive has neither); a value
 * type outside 0 .. 5, an op outside 0 .. 2.  GS_ERR_MODE: a value type whose width is not the handle's.  GS_ERR_ARG: a misaligned
 * d_out_counts / d_out_num.  GS_ERR_SIZE: n == 0 or n > max_keys.  GS_ERR_ARG: any two of the seven buffers overlapping (outputs at
 * their capacity of n elements).  GS_ERR_MODE: every call on a build flavour without these kernels (the tuning and fault-injection
 * libraries).  A refused call launches nothing and leaves route NONE.  Routes and report words are gs_reduce's. */
typedef struct gs_reduce64 gs_reduce64;
#define GS_REDUCE64_ROUTE_NONE 0
#define GS_REDUCE64_ROUTE_SORTED 1
#define GS_REDUCE64_ROUTE_CONSECUTIVE 2
/* gs_reduce64_last report words: those of gs_reduce_last */
#define GS_REDUCE64_R_ROUTE 0
#define GS_REDUCE64_R_N 1
#define GS_REDUCE64_R_U 2
#define GS_REDUCE64_R_RANGES 3
#define GS_REDUCE64_R_PER_RANGE 4
#define GS_REDUCE64_R_TILE 5
#define GS_REDUCE64_R_STATUS 6
#define GS_REDUCE64_R_RANK 7
#define GS_REDUCE64_R_VALUE_TYPE 8
#define GS_REDUCE64_R_OP 9
#define GS_REDUCE64_REPORT_WORDS 10
/* No counterpart in the reference project.  1 <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE), then value_bytes 4 or 8 (GS_ERR_MODE), both
 * answered before a device is looked for.  Synchronous (allocates gs_reduce64_temp_bytes of device memory). */
gs_status gs_reduce64_create(gs_reduce64** out, uint32_t max_keys, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_reduce64_destroy(gs_reduce64* h);
/* No counterpart in the reference project.  Host only.  With A(x) = (x + 255) & ~255:
 *     A(64 * 4)                            the control block
 *   + 4 * A(1024 * 4)                      per range: heads, last head, heads in front, last head in front
 *   + 2 * A(1024 * 8)                      per range: the open partial and the carry (8 bytes each, whatever the width)
 *   + 2 * A(8 * max_keys)                  the copy of the keys the engine sorts, and its alternate buffer
 *   + 2 * A(value_bytes * max_keys)        the copy of the values, and its alternate buffer
 *   + gs_onesweep_temp_bytes(max_keys)     the embedded engine
 * 0 for invalid sizes or value width. */
size_t gs_reduce64_temp_bytes(uint32_t max_keys, uint32_t value_bytes);
/* No counterpart in the reference project. */
gs_status gs_reduce64_by_key(gs_reduce64* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys, void* d_out_values,
                             void* d_out_counts, void* d_out_num, gs_key_type key_type, gs_order order, gs_value_type value_type,
                             gs_reduce_op op, void* stream);
/* No counterpart in the reference project. */
gs_status gs_reduce64_by_key_consecutive(gs_reduce64* h, const void* d_keys, const void* d_values, uint32_t n, void* d_out_keys,
                                         void* d_out_values, void* d_out_counts, void* d_out_num, gs_value_type value_type, gs_reduce_op op,
                                         void* stream);
/* No counterpart in the reference project.  As gs_reduce_check. */
gs_status gs_reduce64_check(gs_reduce64* h, void* stream);
/* No counterpart in the reference project.  As gs_reduce_last: report[GS_REDUCE64_R_*], words >= GS_REDUCE64_REPORT_WORDS. */
gs_status gs_reduce64_last(gs_reduce64* h, uint32_t* report, uint32_t words, void* stream);

/* ---- sorted search: the lower / upper bound of many queries in a sorted array ------------------------------------------------------------
 * No counterpart in the reference project.  What a caller of the sorts, of gs_unique_* or of gs_reduce_* does next: where does this key
 * fall in the sorted keys I already have.
 *
 * hay[0 .. n) is sorted in `order` under the library's total order of key_type: GS_KEY_UINT32 / INT32 / FLOAT32 on a handle created
 * with key_bytes 4, GS_KEY_UINT64 / INT64 / FLOAT64 on one created with key_bytes 8 (floats by the order-preserving flip:
 * -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN).  The 16-bit key types are refused with GS_ERR_ARG.  q[0 .. m) holds keys of the
 * same type.  out[j] is a uint32 in [0, n]:
 *
 *                        GS_SEARCH_LEFT                                  GS_SEARCH_RIGHT
 *     ascending          number of hay keys strictly below q[j]          number of hay keys below or equal
 *     descending         number of hay keys strictly above q[j]          number of hay keys above or equal
 *
 * the insertion position that keeps hay sorted, before (LEFT) or after (RIGHT) the keys equal to the query.  Equality is BITWISE in the
 * flipped domain: -0.0 and +0.0 are two keys and every NaN pattern is a key of its own.  On integers, ascending, the result is
 * torch.searchsorted(hay, q, right = ...)'s.
 *
 * THE ORDER OF hay IS NOT CHECKED.  If hay is not sorted as declared the positions are unspecified, and so they are if queries declared
 * sorted are not.  Even then every out[j] lies in [0, n], no byte outside the call's buffers is read or written, and the call ends:
 * every window is clamped to lo <= hi <= n and every loop is bounded by the sizes, not by the data.
 *
 * Three routes (gs_search_last reports the one taken, gs_search_set_route forces one; GS_SEARCH_ROUTE_AUTO is the default):
 *   GS_SEARCH_ROUTE_TILE    queries in order.  One workgroup per tile of GS_SEARCH_P_TILE queries finds the tile's window of hay with
 *                           two searches (LEFT of its first query, RIGHT of its last); a window of at most GS_SEARCH_P_WINDOW keys is
 *                           staged into LDS and every query answered there; a wider one (sparse queries) is searched in global
 *                           memory narrowed to the window.  The decision is made per tile on the device.
 *   GS_SEARCH_ROUTE_SORT    queries in any order, through TILE: the queries are copied with their positions 0 .. m - 1, the embedded
 *                           stable pairs engine sorts (query, position) in `order`, the tile kernel runs on the sorted copy and
 *                           stores out[position].  Needs a handle created with sort_queries = 1.
 *   GS_SEARCH_ROUTE_BINARY  queries in any order without a sort: one thread per query.  With the sample table (GS_SEARCH_R_TABLE = 1)
 *                           every GS_SEARCH_P_STRIDE-th key of hay is written into a table of at most 64 KiB in the workspace, a
 *                           workgroup stages it into LDS once and serves many queries: the samples in LDS, then the keys between two
 *                           samples in global memory.  Without it every level is a global load.  gs_search_set_table forces the
 *                           form; AUTO takes the table from GS_SEARCH_TABLE_MIN_QUERIES queries on.
 * AUTO: queries_sorted != 0 -> TILE.  Otherwise, on a handle with the engine, SORT when m >= GS_SEARCH_SORT_MIN_QUERIES and
 * n >= GS_SEARCH_SORT_MIN_KEYS, else BINARY; on a handle without it BINARY.
 *
 * Buffers: d_hay, d_queries and d_out 16-byte aligned; d_out holds m uint32 and nothing at or behind element m is written; hay and the
 * queries are not written.  No host wait; every node is a kernel and every grid is a function of (n, m) alone (gs_search_plan), so a
 * call can be captured in a graph and replayed on other contents of the same sizes.  One call in flight per handle.
 *
 * Errors of gs_search_sorted, in this order.  GS_ERR_ARG: null handle (before anything else is looked at); a null or misaligned
 * d_hay / d_queries / d_out; a key type whose width is not the handle's (the 16-bit ones included), a bad order, a bad side.
 * GS_ERR_MODE: route SORT forced on a handle created without sort_queries.  GS_ERR_SIZE: n == 0, m == 0, n > max_keys or
 * m > max_queries.  GS_ERR_ARG: any two of the three buffers overlapping.  GS_ERR_MODE: every call on a build flavour without these
 * kernels (the tuning and fault-injection libraries).  A refused call launches nothing and leaves route NONE. */
typedef struct gs_search gs_search;
typedef enum gs_search_side { GS_SEARCH_LEFT = 0, GS_SEARCH_RIGHT = 1 } gs_search_side;
#define GS_SEARCH_ROUTE_AUTO 0   /* gs_search_set_route only */
#define GS_SEARCH_ROUTE_NONE 0   /* gs_search_last: no call yet, or the last one was refused */
#define GS_SEARCH_ROUTE_TILE 1
#define GS_SEARCH_ROUTE_SORT 2
#define GS_SEARCH_ROUTE_BINARY 3
#define GS_SEARCH_TABLE_AUTO 0   /* gs_search_set_table */
#define GS_SEARCH_TABLE_ON 1
#define GS_SEARCH_TABLE_OFF 2
/* the AUTO rule's constants (measured: DESIGN.md 3.25) */
#define GS_SEARCH_TABLE_MIN_QUERIES 262144u  /* level with the plain form at 2^18 queries, ahead from 2^20 on, behind at 2^16 */
#define GS_SEARCH_SORT_MIN_QUERIES 4194304u  /* SORT is ahead of BINARY at 2^22 queries in 2^22 keys and more, behind at 2^20 of either */
#define GS_SEARCH_SORT_MIN_KEYS 4194304u
/* gs_search_plan words */
#define GS_SEARCH_P_TILE 0              /* T: queries per workgroup of the tile kernel */
#define GS_SEARCH_P_WINDOW 1            /* W: the most keys of a window in LDS (32 KiB / key_bytes) */
#define GS_SEARCH_P_SAMPLES 2           /* samples in the table: n / S */
#define GS_SEARCH_P_STRIDE 3            /* S: the smallest power of two with ceil(n / S) <= 64 KiB / key_bytes; 1: the table is hay */
#define GS_SEARCH_P_TILE_GRID 4         /* ceil(m / T) */
#define GS_SEARCH_P_BINARY_GRID 5       /* the BINARY route's grid in the form AUTO takes */
#define GS_SEARCH_P_SAMPLE_GRID 6       /* the sample kernel's grid */
#define GS_SEARCH_P_TABLE 7             /* 1: AUTO's BINARY uses the sample table for this m */
#define GS_SEARCH_P_ROUTE_SORTED 8      /* AUTO's route for queries_sorted != 0 */
#define GS_SEARCH_P_ROUTE_UNSORTED 9    /* ... for queries in no order on a handle with the engine */
#define GS_SEARCH_P_ROUTE_NO_ENGINE 10  /* ... on a handle without it */
#define GS_SEARCH_PLAN_WORDS 12
/* gs_search_last report words */
#define GS_SEARCH_R_ROUTE 0
#define GS_SEARCH_R_N 1
#define GS_SEARCH_R_M 2
#define GS_SEARCH_R_TABLE 3         /* BINARY: 1 with the sample table, 0 plain */
#define GS_SEARCH_R_LDS_TILES 4     /* TILE / SORT: tiles answered in LDS ... */
#define GS_SEARCH_R_GLOBAL_TILES 5  /* ... and tiles whose window was wider than W */
#define GS_SEARCH_R_ENGINE 6        /* 1: the handle sorts queries */
#define GS_SEARCH_R_PLAN 8          /* the GS_SEARCH_PLAN_WORDS words of gs_search_plan(n, m, key_bytes) */
#define GS_SEARCH_REPORT_WORDS 20
/* No counterpart in the reference project.  1 <= max_keys, max_queries <= GS_MAX_KEYS (GS_ERR_SIZE), then key_bytes 4 or 8 and
 * sort_queries 0 or 1 (GS_ERR_ARG; 2-byte keys are a follow-up), both answered before a device is looked for.  sort_queries = 1 embeds
 * a gs_onesweep pairs engine of capacity max_queries with 4-byte values and allocates the copy of the queries, its alternate and two
 * position buffers; without it the handle allocates only the control block and the sample table.  Synchronous. */
gs_status gs_search_create(gs_search** out, uint32_t max_keys, uint32_t max_queries, uint32_t key_bytes, int sort_queries);
/* No counterpart in the reference project. */
gs_status gs_search_destroy(gs_search* h);
/* No counterpart in the reference project.  Host only.  With A(x) = (x + 255) & ~255:
 *     A(64 * 4) + A(65536)                         the control block and the sample table
 *   + 2 * A(key_bytes * max_queries)               sort_queries only: the copy of the queries and its alternate buffer
 *   + 2 * A(4 * max_queries)                       sort_queries only: the positions and their alternate buffer
 *   + gs_onesweep_temp_bytes(max_queries)          sort_queries only: the embedded engine
 * 0 for invalid arguments. */
size_t gs_search_temp_bytes(uint32_t max_keys, uint32_t max_queries, uint32_t key_bytes, int sort_queries);
/* No counterpart in the reference project.  Host only: plan[GS_SEARCH_P_*] for n keys and m queries of key_bytes bytes.  In the order
 * of gs_search_create: GS_ERR_ARG: null plan; GS_ERR_SIZE: n or m 0 or above GS_MAX_KEYS; GS_ERR_ARG: key_bytes not 4 or 8. */
gs_status gs_search_plan(uint32_t n, uint32_t m, uint32_t key_bytes, uint32_t plan[GS_SEARCH_PLAN_WORDS]);
/* No counterpart in the reference project.  See above.  queries_sorted != 0 declares q sorted in the same `order`. */
gs_status gs_search_sorted(gs_search* h, const void* d_hay, uint32_t n, const void* d_queries, uint32_t m, void* d_out, gs_key_type key_type,
                           gs_order order, gs_search_side side, int queries_sorted, void* stream);
/* No counterpart in the reference project.  GS_SEARCH_ROUTE_AUTO / _TILE / _SORT / _BINARY for the calls that follow, whatever
 * queries_sorted says (GS_ERR_ARG: null handle, another value).  SORT on a handle without the engine is refused by the call. */
gs_status gs_search_set_route(gs_search* h, uint32_t route);
/* No counterpart in the reference project.  The form of the BINARY route: GS_SEARCH_TABLE_AUTO / _ON / _OFF (GS_ERR_ARG otherwise). */
gs_status gs_search_set_table(gs_search* h, uint32_t table);
/* No counterpart in the reference project.  Synchronous diagnostics of the last call: report[GS_SEARCH_R_*], words >= GS_SEARCH_REPORT_WORDS. */
gs_status gs_search_last(gs_search* h, uint32_t* report, uint32_t words, void* stream);

/* ---- merge: two sorted arrays into one: keys, pairs or positions --------------------------------------------------------------------------
 * No counterpart in the reference project.  What a caller who holds keys sorted by this library does with new ones: gs_search_sorted says
 * where each belongs, this moves the data, reading every element once and writing it once.
 *
 * A[0 .. na) and B[0 .. nb) are sorted in `order` under the library's total order of key_type: GS_KEY_UINT32 / INT32 / FLOAT32 on a handle
 * created with key_bytes 4, GS_KEY_UINT64 / INT64 / FLOAT64 on one created with key_bytes 8 (floats by the order-preserving flip:
 * -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN).  The 16-bit key types are refused with GS_ERR_ARG.  out[0 .. na + nb) is the
 * STABLE merge: sorted in the same order, and among keys with the same word all of A's come before all of B's, each side in its input
 * order: A[i] lands at i + #{B in front of A[i]}, B[j] at j + #{A in front of or equal to B[j]}.  Equality is BITWISE in the flipped
 * domain: -0.0 and +0.0 are two keys and every NaN pattern is a key of its own.  The result is that of a stable pairs sort of the
 * concatenation [A; B].  Three forms:
 *
 *     gs_merge_keys        out_keys
 *     gs_merge_pairs       out_keys, out_vals: the values follow their keys; value_bytes 4 or 8, given per call, the same for A and B
 *     gs_merge_positions   out_keys, out_src: uint32, i for A[i] and na + j for B[j]: the "argmerge"; a caller gathers any payload through it
 *
 * THE ORDER OF THE INPUTS IS NOT CHECKED.  If A or B is not sorted as declared the output is unspecified.  Even then the call ends (every
 * kernel loop is bounded by the sizes, not by the data), every output slot [0, na + nb) is written exactly once, every out_src value is
 * below na + nb, and no byte outside the call's buffers is read or written.
 *
 * One kernel: a workgroup per tile of GS_MERGE_P_TILE consecutive outputs finds its two merge-path diagonals with 64-way searches,
 * stages its piece of A and of B into LDS and merges there, GS_MERGE_P_VT outputs per thread; a tile that lies wholly in one input is a
 * copy (gs_merge_last counts them).
 *
 * Buffers: either side may be empty, but not both, and a side of length 0 may be passed as null pointers; 1 <= na + nb <= max_keys;
 * every base pointer 16-byte aligned; the inputs are not written; nothing at or behind element na + nb of an output is written; no buffer
 * of the call may overlap another.  No host wait; every node is a kernel and the grid is a function of na + nb alone (gs_merge_plan), so
 * a call can be captured in a graph and replayed on other contents of the same sizes.  One call in flight per handle.
 *
 * Errors of gs_merge_keys / _pairs / _positions, in this order.  GS_ERR_ARG: null handle (before anything else is looked at).
 * GS_ERR_ARG: a null or misaligned pointer of a non-empty side or of an output; a key type whose width is not the handle's (the 16-bit
 * ones included); a bad order.  GS_ERR_MODE: value_bytes not 4 or 8.  GS_ERR_SIZE: na + nb == 0 or na + nb > max_keys (the sum in 64
 * bits).  GS_ERR_ARG: any two buffers of the call overlapping.  GS_ERR_MODE: every call on a build flavour without these kernels (the
 * tuning and fault-injection libraries).  A refused call launches nothing and leaves form NONE. */
typedef struct gs_merge gs_merge;
#define GS_MERGE_FORM_NONE 0 /* gs_merge_last: no call yet, or the last one was refused */
#define GS_MERGE_FORM_KEYS 1
#define GS_MERGE_FORM_PAIRS 2
#define GS_MERGE_FORM_POSITIONS 3
/* gs_merge_plan words */
#define GS_MERGE_P_TILE 0      /* T: outputs per workgroup */
#define GS_MERGE_P_VT 1        /* VT: outputs per thread, T / threads */
#define GS_MERGE_P_THREADS 2   /* threads per workgroup */
#define GS_MERGE_P_GRID 3      /* ceil((na + nb) / T) */
#define GS_MERGE_P_LDS_BYTES 4 /* LDS of the pairs and positions forms: T * (key_bytes + 2) + 8; the keys form has no indices: T * key_bytes + 8 */
#define GS_MERGE_PLAN_WORDS 8
/* gs_merge_last report words */
#define GS_MERGE_R_FORM 0
#define GS_MERGE_R_NA 1
#define GS_MERGE_R_NB 2
#define GS_MERGE_R_TILES 3      /* tiles run: the plan's grid */
#define GS_MERGE_R_COPY_TILES 4 /* ... of which lay wholly in one input and were copied */
#define GS_MERGE_R_PLAN 8       /* the GS_MERGE_PLAN_WORDS words of gs_merge_plan(na, nb, key_bytes) */
#define GS_MERGE_REPORT_WORDS 16
/* No counterpart in the reference project.  1 <= max_keys <= GS_MAX_KEYS (GS_ERR_SIZE), then key_bytes 4 or 8 (GS_ERR_ARG; 2-byte keys
 * are a follow-up), both answered before a device is looked for.  The handle allocates the control block only.  Synchronous. */
gs_status gs_merge_create(gs_merge** out, uint32_t max_keys, uint32_t key_bytes);
/* No counterpart in the reference project. */
gs_status gs_merge_destroy(gs_merge* h);
/* No counterpart in the reference project.  Host only.  4096: the control block (32 pairs of counters, each pair on a 128-byte line of its own);
 * nothing grows with max_keys.  0 for invalid arguments. */
size_t gs_merge_temp_bytes(uint32_t max_keys, uint32_t key_bytes);
/* No counterpart in the reference project.  Host only: plan[GS_MERGE_P_*] for na + nb outputs of key_bytes bytes.  GS_ERR_ARG: null plan;
 * GS_ERR_SIZE: na + nb 0 or above GS_MAX_KEYS (the sum in 64 bits); GS_ERR_ARG: key_bytes not 4 or 8. */
gs_status gs_merge_plan(uint32_t na, uint32_t nb, uint32_t key_bytes, uint32_t plan[GS_MERGE_PLAN_WORDS]);
/* No counterpart in the reference project.  See above. */
gs_status gs_merge_keys(gs_merge* h, const void* d_a, uint32_t na, const void* d_b, uint32_t nb, void* d_out, gs_key_type key_type, gs_order order,
                        void* stream);
/* No counterpart in the reference project.  See above. */
gs_status gs_merge_pairs(gs_merge* h, const void* d_a_keys, const void* d_a_vals, uint32_t na, const void* d_b_keys, const void* d_b_vals, uint32_t nb,
                         void* d_out_keys, void* d_out_vals, uint32_t value_bytes, gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project.  See above. */
gs_status gs_merge_positions(gs_merge* h, const void* d_a, uint32_t na, const void* d_b, uint32_t nb, void* d_out_keys, void* d_out_src,
                             gs_key_type key_type, gs_order order, void* stream);
/* No counterpart in the reference project.  Synchronous diagnostics of the last call: report[GS_MERGE_R_*], words >= GS_MERGE_REPORT_WORDS. */
gs_status gs_merge_last(gs_merge* h, uint32_t* report, uint32_t words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPUSORT_H */
