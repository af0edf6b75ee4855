"""ctypes binding of libgpusort.so (the C-ABI of include/gpusort.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``make`` into ``gpusorting_amd/lib/libgpusort.so``.  There is NO fallback: if
the library is missing, importing the binding raises — the product path never
routes through the CPU oracle or any eager PyTorch op.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPUSORT_LIB") or os.path.join(_HERE, "lib", "libgpusort.so")  # env: other builds (tuning, trace, fault)

GS_OK, GS_ERR_ARG, GS_ERR_SIZE, GS_ERR_HIP, GS_ERR_TIMEOUT, GS_ERR_MODE, GS_ERR_NO_DEVICE, GS_ERR_COMM = range(8)
GS_MGPU_UNIQUE_ID_BYTES = 128
GS_MAX_KEYS = (1 << 30) - 1
GS_PROFILE_SLOTS = 8
GS_SEGSORT_CLASSES = 9
GS_TOPK_REPORT_WORDS = 8
GS_TOPK_ROWS_REPORT_WORDS = 8
# gs_sort16_last: report words, routes and the kernel-form bits
GS_SORT16_REPORT_WORDS = 8
GS_SORT16_ROUTE_NONE, GS_SORT16_ROUTE_KEYS, GS_SORT16_ROUTE_PAIRS = 0, 1, 2
(GS_SORT16_R_ROUTE, GS_SORT16_R_RANGES, GS_SORT16_R_PER_RANGE, GS_SORT16_R_TILE, GS_SORT16_R_FORMS, GS_SORT16_R_STATUS, GS_SORT16_R_N,
 GS_SORT16_R_RANK) = range(8)
GS_SORT16_F_HIST, GS_SORT16_F_SCAN, GS_SORT16_F_FILL, GS_SORT16_F_COUNT, GS_SORT16_F_PSCAN, GS_SORT16_F_SCATTER = 1, 2, 4, 8, 16, 32
GS_SORT16_F_ALL = 0x7FF
# gs_topk16_last: routes and report words
GS_TOPK16_ROUTE_NONE, GS_TOPK16_ROUTE_TILE, GS_TOPK16_ROUTE_COUNT, GS_TOPK16_ROUTE_SELECT = 0, 1, 2, 3
(GS_TOPK16_R_ROUTE, GS_TOPK16_R_THRESHOLD, GS_TOPK16_R_IN_FRONT, GS_TOPK16_R_EQUAL, GS_TOPK16_R_TAKEN, GS_TOPK16_R_RANGES, GS_TOPK16_R_STATUS,
 GS_TOPK16_R_PER_RANGE, GS_TOPK16_R_HIST) = range(9)
GS_TOPK16_REPORT_WORDS = 9
GS_TOPK16_HIST_AUTO, GS_TOPK16_HIST_SLICES, GS_TOPK16_HIST_GLOBAL = 0, 1, 2
GS_TOPK16_COUNT_SLICES_MIN = 1 << 27
# gs_sort_rows_plan / gs_sort_rows_last: plan and report words, routes and the kernel-form bits
GS_SORT_ROWS_PLAN_WORDS = GS_SORT_ROWS_REPORT_WORDS = 8
GS_SORT_ROWS_ROUTE_NONE, GS_SORT_ROWS_ROUTE_LDS, GS_SORT_ROWS_ROUTE_PASSES = 0, 1, 2
GS_SORT_ROWS_TILE, GS_SORT_ROWS_PCAP, GS_SORT_ROWS_MIN_TILES, GS_SORT_ROWS_PASSES = 4096, 1024, 2, 4
(GS_SORT_ROWS_P_ROUTE, GS_SORT_ROWS_P_PARTS, GS_SORT_ROWS_P_PER_PART, GS_SORT_ROWS_P_TILE, GS_SORT_ROWS_P_PASSES, GS_SORT_ROWS_P_CAP) = range(6)
(GS_SORT_ROWS_R_ROUTE, GS_SORT_ROWS_R_ROWS, GS_SORT_ROWS_R_ROW_LEN, GS_SORT_ROWS_R_PARTS, GS_SORT_ROWS_R_FORMS, GS_SORT_ROWS_R_STATUS,
 GS_SORT_ROWS_R_RANK, GS_SORT_ROWS_R_PER_PART) = range(8)
(GS_SORT_ROWS_F_CLEAR, GS_SORT_ROWS_F_OFFSETS, GS_SORT_ROWS_F_LDS, GS_SORT_ROWS_F_COUNT, GS_SORT_ROWS_F_SCAN,
 GS_SORT_ROWS_F_SCATTER) = 1, 2, 4, 8, 16, 32
GS_SORT_ROWS_F_ALL = 0x7FF
# gs_sort_rows16_*: the plan and report words and the routes are gs_sort_rows_*'s; two passes, and its own kernel-form bits
GS_SORT_ROWS16_PASSES = 2
(GS_SORT_ROWS16_F_CLEAR, GS_SORT_ROWS16_F_LDS_WAVE, GS_SORT_ROWS16_F_LDS_TILE, GS_SORT_ROWS16_F_COUNT, GS_SORT_ROWS16_F_SCAN,
 GS_SORT_ROWS16_F_SCATTER) = 1, 2, 4, 8, 16, 32
GS_SORT_ROWS16_F_ALL = 0x1FFF
# gs_segsort16_*: two passes over parts of GS_SEGSORT16_PART elements, the report words and the kernel-form bits
GS_SEGSORT16_PASSES = 2
GS_SEGSORT16_PART = 8 * GS_SORT_ROWS_TILE
(GS_SEGSORT16_R_UNITS, GS_SEGSORT16_R_FORMS, GS_SEGSORT16_R_WG_FORMS, GS_SEGSORT16_R_STATUS, GS_SEGSORT16_R_RANK, GS_SEGSORT16_R_LONG,
 GS_SEGSORT16_R_UNIT_CAP, GS_SEGSORT16_R_N) = range(8)
GS_SEGSORT16_REPORT_WORDS = 8
(GS_SEGSORT16_F_CLASSIFY, GS_SEGSORT16_F_FILL, GS_SEGSORT16_F_PACKED, GS_SEGSORT16_F_WAVE, GS_SEGSORT16_F_UNITS, GS_SEGSORT16_F_COUNT,
 GS_SEGSORT16_F_SCAN, GS_SEGSORT16_F_SCATTER) = 1, 2, 4, 64, 1024, 2048, 4096, 8192
GS_SEGSORT16_F_ALL = 0x1FFFFF
GS_SEGSORT16_WG_ALL = 0xFFFFFFFF


def GS_SEGSORT16_WG_FORM(cls: int, v: int, rank: int) -> int:
    """The bit of a workgroup-class kernel in report[GS_SEGSORT16_R_WG_FORMS] (the macro of include/gpusort.h)."""
    return 1 << (16 * rank + (4 * (cls - 3) + v if cls <= 5 else 12 + v if cls == 6 else 15))


# gs_segsort_set_long_route / gs_segsort_last: the long routes, the device route's plan, the report words and the kernel-form bits
GS_SEGSORT_LONG_HOST, GS_SEGSORT_LONG_DEVICE = 0, 1
GS_SEGSORT_LONG_PASSES = 4
GS_SEGSORT_LONG_PART = 4 * GS_SORT_ROWS_TILE
(GS_SEGSORT_R_ROUTE, GS_SEGSORT_R_UNITS, GS_SEGSORT_R_LONG, GS_SEGSORT_R_UNIT_CAP, GS_SEGSORT_R_FORMS, GS_SEGSORT_R_STATUS, GS_SEGSORT_R_RANK,
 GS_SEGSORT_R_N) = range(8)
GS_SEGSORT_REPORT_WORDS = 8
GS_SEGSORT_LF_UNITS, GS_SEGSORT_LF_COUNT, GS_SEGSORT_LF_SCAN, GS_SEGSORT_LF_SCATTER = 1, 2, 4, 8
GS_SEGSORT_LF_ALL = 0x1FF

# gs_segtopk_last: the report words and the kernel-form bits
GS_SEGTOPK_R_CLASSES = 0
(GS_SEGTOPK_R_LONGEST, GS_SEGTOPK_R_STATUS, GS_SEGTOPK_R_READS, GS_SEGTOPK_R_FORMS, GS_SEGTOPK_R_RANK, GS_SEGTOPK_R_K,
 GS_SEGTOPK_R_PACKED) = range(9, 16)
GS_SEGTOPK_REPORT_WORDS = 16
GS_SEGTOPK_F_PACKED, GS_SEGTOPK_F_WAVE, GS_SEGTOPK_F_STREAM, GS_SEGTOPK_F_VM = 1, 2, 4, 0x10000


def GS_SEGTOPK_F_TILE(cls: int, rank: int) -> int:
    """The bit of a tile-class kernel (class 3 .. 7, rank mode 0 / 1) in report[GS_SEGTOPK_R_FORMS] (the macro of include/gpusort.h)."""
    return 8 << ((cls - 3) + 5 * rank)


# gs_unique_last: routes and report words
GS_UNIQUE_ROUTE_NONE, GS_UNIQUE_ROUTE_KEYS, GS_UNIQUE_ROUTE_POSITIONS, GS_UNIQUE_ROUTE_CONSECUTIVE = 0, 1, 2, 3
(GS_UNIQUE_R_ROUTE, GS_UNIQUE_R_N, GS_UNIQUE_R_U, GS_UNIQUE_R_RANGES, GS_UNIQUE_R_PER_RANGE, GS_UNIQUE_R_TILE, GS_UNIQUE_R_STATUS,
 GS_UNIQUE_R_RANK) = range(8)
GS_UNIQUE_REPORT_WORDS = 8
# gs_unique16_last: routes, report words, the optional-kernel bits; gs_unique16_set_inverse_form
GS_UNIQUE16_ROUTE_NONE, GS_UNIQUE16_ROUTE_HISTOGRAM, GS_UNIQUE16_ROUTE_CONSECUTIVE = 0, 1, 2
(GS_UNIQUE16_R_ROUTE, GS_UNIQUE16_R_N, GS_UNIQUE16_R_U, GS_UNIQUE16_R_STATUS, GS_UNIQUE16_R_RAN, GS_UNIQUE16_R_RANGES, GS_UNIQUE16_R_PER_RANGE,
 GS_UNIQUE16_R_TILE, GS_UNIQUE16_R_FIRST_RANGES, GS_UNIQUE16_R_INVERSE_RANGES) = range(10)
GS_UNIQUE16_REPORT_WORDS = 10
GS_UNIQUE16_K_FIRST, GS_UNIQUE16_K_INVERSE_LDS, GS_UNIQUE16_K_INVERSE_GATHER = 1, 2, 4
GS_UNIQUE16_INVERSE_AUTO, GS_UNIQUE16_INVERSE_LDS, GS_UNIQUE16_INVERSE_GATHER = 0, 1, 2
GS_UNIQUE16_INVERSE_LDS_MIN = 1 << 22
# gs_reduce_*: value types, operations, routes and report words
GS_VALUE_INT32, GS_VALUE_UINT32, GS_VALUE_FLOAT32, GS_VALUE_INT64, GS_VALUE_UINT64, GS_VALUE_FLOAT64 = range(6)
GS_REDUCE_SUM, GS_REDUCE_MIN, GS_REDUCE_MAX = 0, 1, 2
GS_REDUCE_ROUTE_NONE, GS_REDUCE_ROUTE_SORTED, GS_REDUCE_ROUTE_CONSECUTIVE = 0, 1, 2
(GS_REDUCE_R_ROUTE, GS_REDUCE_R_N, GS_REDUCE_R_U, GS_REDUCE_R_RANGES, GS_REDUCE_R_PER_RANGE, GS_REDUCE_R_TILE, GS_REDUCE_R_STATUS, GS_REDUCE_R_RANK,
 GS_REDUCE_R_VALUE_TYPE, GS_REDUCE_R_OP) = range(10)
GS_REDUCE_REPORT_WORDS = 10
# gs_unique64_* / gs_reduce64_*: the routes and report words of the 32-bit families under their own names
GS_UNIQUE64_ROUTE_NONE, GS_UNIQUE64_ROUTE_KEYS, GS_UNIQUE64_ROUTE_POSITIONS, GS_UNIQUE64_ROUTE_CONSECUTIVE = 0, 1, 2, 3
(GS_UNIQUE64_R_ROUTE, GS_UNIQUE64_R_N, GS_UNIQUE64_R_U, GS_UNIQUE64_R_RANGES, GS_UNIQUE64_R_PER_RANGE, GS_UNIQUE64_R_TILE, GS_UNIQUE64_R_STATUS,
 GS_UNIQUE64_R_RANK) = range(8)
GS_UNIQUE64_REPORT_WORDS = 8
GS_REDUCE64_ROUTE_NONE, GS_REDUCE64_ROUTE_SORTED, GS_REDUCE64_ROUTE_CONSECUTIVE = 0, 1, 2
(GS_REDUCE64_R_ROUTE, GS_REDUCE64_R_N, GS_REDUCE64_R_U, GS_REDUCE64_R_RANGES, GS_REDUCE64_R_PER_RANGE, GS_REDUCE64_R_TILE, GS_REDUCE64_R_STATUS,
 GS_REDUCE64_R_RANK, GS_REDUCE64_R_VALUE_TYPE, GS_REDUCE64_R_OP) = range(10)
GS_REDUCE64_REPORT_WORDS = 10
# gs_search_*: sides, routes, table forms, the AUTO rule's constants, plan and report words
GS_SEARCH_LEFT, GS_SEARCH_RIGHT = 0, 1
GS_SEARCH_ROUTE_AUTO = GS_SEARCH_ROUTE_NONE = 0
GS_SEARCH_ROUTE_TILE, GS_SEARCH_ROUTE_SORT, GS_SEARCH_ROUTE_BINARY = 1, 2, 3
GS_SEARCH_TABLE_AUTO, GS_SEARCH_TABLE_ON, GS_SEARCH_TABLE_OFF = 0, 1, 2
GS_SEARCH_TABLE_MIN_QUERIES, GS_SEARCH_SORT_MIN_QUERIES, GS_SEARCH_SORT_MIN_KEYS = 1 << 18, 1 << 22, 1 << 22
(GS_SEARCH_P_TILE, GS_SEARCH_P_WINDOW, GS_SEARCH_P_SAMPLES, GS_SEARCH_P_STRIDE, GS_SEARCH_P_TILE_GRID, GS_SEARCH_P_BINARY_GRID,
 GS_SEARCH_P_SAMPLE_GRID, GS_SEARCH_P_TABLE, GS_SEARCH_P_ROUTE_SORTED, GS_SEARCH_P_ROUTE_UNSORTED, GS_SEARCH_P_ROUTE_NO_ENGINE) = range(11)
GS_SEARCH_PLAN_WORDS = 12
(GS_SEARCH_R_ROUTE, GS_SEARCH_R_N, GS_SEARCH_R_M, GS_SEARCH_R_TABLE, GS_SEARCH_R_LDS_TILES, GS_SEARCH_R_GLOBAL_TILES, GS_SEARCH_R_ENGINE) = range(7)
GS_SEARCH_R_PLAN = 8
GS_SEARCH_REPORT_WORDS = 20

# gs_debug_sort_route / gs_debug_set_hy_class / gs_debug_pass_flags / gs_debug_registry_* (test hooks)
GS_ROUTE_NONE = 0xFFFFFFFF
GS_PF_SKEW, GS_PF_SKIP, GS_PF_SRC_ALT, GS_PF_LAST, GS_PF_POS, GS_PF_HALF16 = 1, 2, 4, 8, 16, 32
(GS_KF_BIN, GS_KF_POS, GS_KF_PERSIST, GS_KF_SMALL, GS_KF_MID, GS_KF_SEG_WG, GS_KF_SEG_VB, GS_KF_TKR_TILE, GS_KF_TKR_VM, GS_KF_HIST,
 GS_KF_HY_HIST, GS_KF_HY_LOCAL, GS_KF_HY_LOCAL_PAIRS, GS_KF_COUNT) = range(14)
# gs_key_type behind the 64-bit ones: 2-byte keys, accepted by gs_topk_select_rows_keys / _pairs, gs_topk16_*, gs_sort16_*, gs_sort_rows16_* and gs_segsort16_*
KEY_UINT16, KEY_INT16, KEY_FLOAT16, KEY_BFLOAT16 = 6, 7, 8, 9

# every symbol include/gpusort.h declares: (name, restype, argtypes)
_u32, _vp, _int = C.c_uint32, C.c_void_p, C.c_int
_u32p, _u64p, _u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)

# gs_mgpu_transport (include/gpusort.h): the two functions a transport provides
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, _vp, _vp, _vp, C.c_size_t, _vp)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, _vp, _u32, C.POINTER(_vp), C.POINTER(_vp), _u32p, _u32p, _u32p, _u32p, _u32p, _vp)


class OneSweepOptions(C.Structure):
    """gs_onesweep_options (include/gpusort.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("shape_threads", C.c_uint32), ("shape_keys_per_thread", C.c_uint32),
                ("rank_mode", C.c_int32), ("small_path", C.c_int32), ("mid_path", C.c_int32), ("skip_passes", C.c_int32),
                ("position_chains", C.c_int32), ("position_chains_min_log2", C.c_uint32), ("key64_sweeps", C.c_int32),
                ("plan", C.c_int32), ("first_pass_big", C.c_int32), ("hist_blocks", C.c_uint32), ("debug_flags", C.c_uint32)]


class MgpuOptions(C.Structure):
    """gs_mgpu_options (include/gpusort.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("force_exchange", C.c_int32), ("overlap", C.c_int32), ("alltoallv", C.c_int32), ("by_bin", C.c_int32),
                ("sorter", OneSweepOptions)]


def onesweep_options_from_env(**overrides) -> "OneSweepOptions":
    """The library reads no environment variables; this harness does: GPUSORT_* names (tests, tools/, A/B runs) are
    translated into gs_onesweep_options here.  Keyword arguments win over the environment."""
    o = OneSweepOptions()
    load().gs_onesweep_options_default(C.byref(o))
    env = os.environ
    if "GPUSORT_SHAPE" in env:  # "512x16"
        try:
            t, k = env["GPUSORT_SHAPE"].lower().split("x")
            o.shape_threads, o.shape_keys_per_thread = int(t), int(k)
        except ValueError:
            pass
    for name, field in (("GPUSORT_RANK", "rank_mode"), ("GPUSORT_SMALL_PATH", "small_path"), ("GPUSORT_MID_PATH", "mid_path"),
                        ("GPUSORT_SKIP_PASSES", "skip_passes"), ("GPUSORT_POS", "position_chains"),
                        ("GPUSORT_POS_MIN_LOG2", "position_chains_min_log2"), ("GPUSORT_KEY64_SWEEPS", "key64_sweeps"),
                        ("GPUSORT_PLAN", "plan"), ("GPUSORT_FIRST_PASS_BIG", "first_pass_big"), ("GPUSORT_HIST_BLOCKS", "hist_blocks"),
                        ("GPUSORT_LS_EXP", "debug_flags")):
        if name in env:
            try:
                setattr(o, field, int(env[name], 0))
            except ValueError:
                pass
    _apply_overrides(o, overrides)
    return o


def _apply_overrides(o, overrides) -> None:
    """Keyword overrides of an options struct: a name the struct does not have is a TypeError (setattr on a ctypes.Structure
    would silently create a Python attribute and the option would be ignored)."""
    known = {f[0] for f in o._fields_}
    for k, v in overrides.items():
        if k not in known:
            raise TypeError(f"{type(o).__name__} has no option {k!r} (known: {sorted(known)})")
        if v is not None:
            setattr(o, k, int(v))


def mgpu_options_from_env(**overrides) -> "MgpuOptions":
    o = MgpuOptions()
    load().gs_mgpu_options_default(C.byref(o))
    o.sorter = onesweep_options_from_env()  # the context's local sorter follows the same GPUSORT_* switches
    for name, field in (("GPUSORT_MGPU_FORCE_EXCHANGE", "force_exchange"), ("GPUSORT_MGPU_OVERLAP", "overlap"),
                        ("GPUSORT_MGPU_ALLTOALLV", "alltoallv"), ("GPUSORT_MGPU_BY_BIN", "by_bin")):
        if name in os.environ:
            try:
                setattr(o, field, int(os.environ[name], 0))
            except ValueError:
                pass
    _apply_overrides(o, overrides)
    return o


class MgpuTransport(C.Structure):
    _fields_ = [("user", _vp), ("all_gather_u32", ALL_GATHER_FN), ("exchange", EXCHANGE_FN)]


_PROTOS = [
    ("gs_version", C.c_char_p, []),
    ("gs_status_string", C.c_char_p, [_int]),
    ("gs_last_hip_error", _int, []),
    ("gs_onesweep_create", _int, [C.POINTER(_vp), _u32, _int, _u32]),
    ("gs_onesweep_options_default", None, [_vp]),
    ("gs_onesweep_create_ex", _int, [C.POINTER(_vp), _u32, _int, _u32, _vp]),
    ("gs_onesweep_destroy", _int, [_vp]),
    ("gs_onesweep_temp_bytes", C.c_size_t, [_u32]),
    ("gs_onesweep_partition_size", _u32, [_int, _u32]),
    ("gs_onesweep_sort_keys", _int, [_vp, _vp, _vp, _u32, _int, _int, _vp]),
    ("gs_onesweep_sort_pairs", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _int, _int, _vp]),
    ("gs_onesweep_check", _int, [_vp, _vp]),
    ("gs_onesweep_set_shape", _int, [_vp, _u32, _u32]),
    ("gs_onesweep_get_partition_size", _u32, [_vp]),
    ("gs_onesweep_set_rank_mode", _int, [_vp, _int]),
    ("gs_onesweep_get_rank_mode", _int, [_vp]),
    ("gs_onesweep_set_small_path", _int, [_vp, _int]),
    ("gs_onesweep_set_skip_passes", _int, [_vp, _int]),
    ("gs_onesweep_set_mid_path", _int, [_vp, _int]),
    ("gs_onesweep_set_plan", _int, [_vp, _int]),
    ("gs_onesweep_last_plan", _int, [_vp, _u32p, _u32p, _vp]),
    ("gs_selftest_lds_atomic_order", _int, [_u32, _u32, C.POINTER(C.c_uint64), _vp]),
    ("gs_selftest_wave_primitives", _int, [_u32, _u32, _vp, _vp]),
    ("gs_debug_set_trace", _int, [_vp, _vp]),
    ("gs_debug_check_state", _int, [_vp, C.POINTER(C.c_uint64), _vp]),
    ("gs_debug_poke_status", _int, [_vp, _u32, _vp]),
    ("gs_debug_read_slab", _int, [_vp, _u32, _u32, _u32p, _vp]),
    ("gs_debug_sort_route", _int, [_vp, _u32, _int, _u32p]),
    ("gs_debug_set_hy_class", _int, [_vp, _int]),
    ("gs_debug_set_pos_grid", _int, [_vp, _u32]),
    ("gs_debug_pass_flags", _int, [_vp, _u32p, _vp]),
    ("gs_debug_hy_half_slot", _u32, [_u32, _u32, _u32, _u32, _u32]),
    ("gs_debug_registry_dims", _int, [_u32, C.POINTER(C.c_int32)]),
    ("gs_debug_registry_cell", _int, [_u32, C.POINTER(C.c_int32)]),
    ("gs_onesweep_global_histogram", _int, [_vp, _vp, _u32, _int, C.POINTER(_u32), _vp]),
    ("gs_onesweep_scan", _int, [_vp, _vp, _u32, _int, C.POINTER(_u32), _vp]),
    ("gs_onesweep_digit_pass", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_onesweep_msd_prepare", _int, [_vp, _vp, _u32, _int, C.POINTER(_u32), _vp]),
    ("gs_onesweep_msd_partition", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    ("gs_onesweep_set_profiling", _int, [_vp, _int]),
    ("gs_onesweep_get_profile", _int, [_vp, C.POINTER(C.c_float)]),
    ("gs_init_random", _int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp]),
    ("gs_validate", _int, [_vp, _vp, _u32, _u32, _int, _int, C.POINTER(_u32), _vp]),
    ("gs_msd_splitters", _int, [C.POINTER(C.c_uint64), _u32, C.POINTER(_u32)]),
    ("gs_msd_splitters_n", _int, [C.POINTER(C.c_uint64), _u32, _u32, C.POINTER(_u32)]),
    ("gs_onesweep_msd_fine_histogram", _int, [_vp, _vp, _u32, _int, C.POINTER(_u32), _vp]),
    ("gs_mgpu_get_unique_id", _int, [_u8p]),
    ("gs_mgpu_create", _int, [C.POINTER(_vp), _u8p, _u32, _u32, _u32, _u32, _int, _u32]),
    ("gs_mgpu_options_default", None, [_vp]),
    ("gs_mgpu_create_ex", _int, [C.POINTER(_vp), _u8p, _u32, _u32, _u32, _u32, _int, _u32, _vp]),
    ("gs_mgpu_set_alltoallv", _int, [_vp, _int]),
    ("gs_mgpu_create_with_transport_ex", _int, [C.POINTER(_vp), C.POINTER(MgpuTransport), _u32, _u32, _u32, _u32, _int, _u32, _vp]),
    ("gs_mgpu_destroy", _int, [_vp]),
    ("gs_onesweep_sort_sharded", _int, [_vp, _vp, _vp, _u32, _int, _vp, _vp, _u32p, _vp]),
    ("gs_mgpu_get_profile", _int, [_vp, C.POINTER(C.c_float), _u64p, _u64p, _u32p]),
    ("gs_mgpu_last_plan", _int, [_vp, _u32p, _u32]),
    ("gs_mgpu_check", _int, [_vp, _vp]),
    ("gs_mgpu_debug_fail", _int, [_vp, _int]),
    ("gs_mgpu_sorter", _vp, [_vp]),
    ("gs_mgpu_set_force_exchange", _int, [_vp, _int]),
    ("gs_mgpu_last_layout", _int, [_vp, _u32p]),
    ("gs_msd_exchange_round", _int, [_u32p, _u32, _u32, _u32p, _int, _u32, _u32p, _u32p, _u32p, _u32p, _u32p]),
    ("gs_last_rccl_error", _int, []),
    ("gs_mgpu_create_with_transport", _int, [C.POINTER(_vp), C.POINTER(MgpuTransport), _u32, _u32, _u32, _u32, _int, _u32]),
    ("gs_msd_plan", _int, [_u32p, _u32, _u32, _u32, _u32, _u32p]),
    ("gs_debug_msd_plan_device", _int, [_u32p, _u32, _u32, _u32, _u32, _u32p, _vp]),
    ("gs_segsort_create", _int, [C.POINTER(_vp), _u32, _u32, _int, _u32]),
    ("gs_segsort_destroy", _int, [_vp]),
    ("gs_segsort_temp_bytes", C.c_size_t, [_u32, _u32]),
    ("gs_segsort_class_of", _u32, [_u32, _int, _u32]),
    ("gs_segsort_max_lds_segment", _u32, [_int, _u32]),
    ("gs_segsort_sort_keys", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_segsort_sort_pairs", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_segsort_check", _int, [_vp, _vp]),
    ("gs_segsort_last_classes", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_segsort_engine", _vp, [_vp]),
    ("gs_segsort_set_long_route", _int, [_vp, _u32]),
    ("gs_segsort_get_long_route", _u32, [_vp]),
    ("gs_segsort_long_units", _u32, [_u32, _u32, _int, _u32]),
    ("gs_segsort_long_temp_bytes", C.c_size_t, [_u32, _u32, _int, _u32]),
    ("gs_segsort_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_topk_create", _int, [C.POINTER(_vp), _u32, _u32, _int, _u32]),
    ("gs_topk_destroy", _int, [_vp]),
    ("gs_topk_temp_bytes", C.c_size_t, [_u32, _u32, _u32]),
    ("gs_topk_select_keys", _int, [_vp, _vp, _u32, _u32, _vp, _int, _int, _vp]),
    ("gs_topk_select_pairs", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _int, _int, _vp]),
    ("gs_topk_check", _int, [_vp, _vp]),
    ("gs_topk_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_topk_engine", _vp, [_vp]),
    ("gs_topk_select_rows_keys", _int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _int, _int, _vp]),
    ("gs_topk_select_rows_pairs", _int, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _int, _int, _vp]),
    ("gs_topk_rows_max_k", _u32, [_int, _u32]),
    ("gs_topk_rows_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_sort16_create", _int, [C.POINTER(_vp), _u32, _int, _u32]),
    ("gs_sort16_destroy", _int, [_vp]),
    ("gs_sort16_temp_bytes", C.c_size_t, [_u32, _int, _u32]),
    ("gs_sort16_sort_keys", _int, [_vp, _vp, _u32, _int, _int, _vp]),
    ("gs_sort16_sort_pairs", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _int, _int, _vp]),
    ("gs_sort16_argsort", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _int, _int, _vp]),
    ("gs_sort16_check", _int, [_vp, _vp]),
    ("gs_sort16_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_sort16_plan", _int, [_u32, _int, _u32, _u32p]),
    ("gs_sort16_set_rank_mode", _int, [_vp, _int]),
    ("gs_sort16_get_rank_mode", _int, [_vp]),
    ("gs_topk16_create", _int, [C.POINTER(_vp), _u32, _u32, _int, _u32]),
    ("gs_topk16_destroy", _int, [_vp]),
    ("gs_topk16_temp_bytes", C.c_size_t, [_u32, _u32, _int, _u32]),
    ("gs_topk16_select_keys", _int, [_vp, _vp, _u32, _u32, _vp, _int, _int, _vp]),
    ("gs_topk16_select_pairs", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _int, _int, _vp]),
    ("gs_topk16_check", _int, [_vp, _vp]),
    ("gs_topk16_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_topk16_set_count_histogram", _int, [_vp, _u32]),
    ("gs_sort_rows_create", _int, [C.POINTER(_vp), _u32, _int, _u32]),
    ("gs_sort_rows_destroy", _int, [_vp]),
    ("gs_sort_rows_temp_bytes", C.c_size_t, [_u32, _int, _u32]),
    ("gs_sort_rows_plan", _int, [_u32, _u32, _int, _u32, _u32p]),
    ("gs_sort_rows_keys", _int, [_vp, _vp, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_sort_rows_pairs", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_sort_rows_check", _int, [_vp, _vp]),
    ("gs_sort_rows_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_sort_rows_set_rank_mode", _int, [_vp, _int]),
    ("gs_sort_rows_get_rank_mode", _int, [_vp]),
    ("gs_sort_rows16_create", _int, [C.POINTER(_vp), _u32, _int, _u32]),
    ("gs_sort_rows16_destroy", _int, [_vp]),
    ("gs_sort_rows16_temp_bytes", C.c_size_t, [_u32, _int, _u32]),
    ("gs_sort_rows16_plan", _int, [_u32, _u32, _int, _u32, _u32p]),
    ("gs_sort_rows16_keys", _int, [_vp, _vp, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_sort_rows16_pairs", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_sort_rows16_argsort", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_sort_rows16_check", _int, [_vp, _vp]),
    ("gs_sort_rows16_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_sort_rows16_set_rank_mode", _int, [_vp, _int]),
    ("gs_sort_rows16_get_rank_mode", _int, [_vp]),
    ("gs_segsort16_create", _int, [C.POINTER(_vp), _u32, _u32, _int, _u32]),
    ("gs_segsort16_destroy", _int, [_vp]),
    ("gs_segsort16_units", _u32, [_u32, _u32, _int, _u32]),
    ("gs_segsort16_temp_bytes", C.c_size_t, [_u32, _u32, _int, _u32]),
    ("gs_segsort16_sort_keys", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_segsort16_sort_pairs", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_segsort16_argsort", _int, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _int, _int, _vp]),
    ("gs_segsort16_check", _int, [_vp, _vp]),
    ("gs_segsort16_last_classes", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_segsort16_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_segsort16_set_rank_mode", _int, [_vp, _int]),
    ("gs_segsort16_get_rank_mode", _int, [_vp]),
    ("gs_segtopk_create", _int, [C.POINTER(_vp), _u32, _u32, _u32, _int, _u32]),
    ("gs_segtopk_destroy", _int, [_vp]),
    ("gs_segtopk_temp_bytes", C.c_size_t, [_u32]),
    ("gs_segtopk_select_keys", _int, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _int, _int, _vp]),
    ("gs_segtopk_select_pairs", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _int, _int, _vp]),
    ("gs_segtopk_check", _int, [_vp, _vp]),
    ("gs_segtopk_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_segtopk_set_rank_mode", _int, [_vp, _int]),
    ("gs_segtopk_get_rank_mode", _int, [_vp]),
    ("gs_segtopk16_create", _int, [C.POINTER(_vp), _u32, _u32, _u32, _int, _u32]),
    ("gs_segtopk16_destroy", _int, [_vp]),
    ("gs_segtopk16_temp_bytes", C.c_size_t, [_u32]),
    ("gs_segtopk16_select_keys", _int, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _int, _int, _vp]),
    ("gs_segtopk16_select_pairs", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _int, _int, _vp]),
    ("gs_segtopk16_check", _int, [_vp, _vp]),
    ("gs_segtopk16_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_segtopk16_set_rank_mode", _int, [_vp, _int]),
    ("gs_segtopk16_get_rank_mode", _int, [_vp]),
    ("gs_unique_create", _int, [C.POINTER(_vp), _u32, _int, _u32]),
    ("gs_unique_destroy", _int, [_vp]),
    ("gs_unique_temp_bytes", C.c_size_t, [_u32, _int, _u32]),
    ("gs_unique_keys", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_unique_positions", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_unique_consecutive", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gs_unique_plan", _int, [_u32, _u32p]),
    ("gs_unique_check", _int, [_vp, _vp]),
    ("gs_unique_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_unique16_create", _int, [C.POINTER(_vp), _u32]),
    ("gs_unique16_destroy", _int, [_vp]),
    ("gs_unique16_temp_bytes", C.c_size_t, [_u32]),
    ("gs_unique16_unique", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_unique16_consecutive", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gs_unique16_check", _int, [_vp, _vp]),
    ("gs_unique16_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_unique16_set_inverse_form", _int, [_vp, _u32]),
    ("gs_reduce_create", _int, [C.POINTER(_vp), _u32, _u32]),
    ("gs_reduce_destroy", _int, [_vp]),
    ("gs_reduce_temp_bytes", C.c_size_t, [_u32, _u32]),
    ("gs_reduce_by_key", _int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _vp]),
    ("gs_reduce_by_key_consecutive", _int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_reduce_check", _int, [_vp, _vp]),
    ("gs_reduce_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_unique64_create", _int, [C.POINTER(_vp), _u32, _int, _u32]),
    ("gs_unique64_destroy", _int, [_vp]),
    ("gs_unique64_temp_bytes", C.c_size_t, [_u32, _int, _u32]),
    ("gs_unique64_keys", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_unique64_positions", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_unique64_consecutive", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("gs_unique64_check", _int, [_vp, _vp]),
    ("gs_unique64_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_reduce64_create", _int, [C.POINTER(_vp), _u32, _u32]),
    ("gs_reduce64_destroy", _int, [_vp]),
    ("gs_reduce64_temp_bytes", C.c_size_t, [_u32, _u32]),
    ("gs_reduce64_by_key", _int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _vp]),
    ("gs_reduce64_by_key_consecutive", _int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    ("gs_reduce64_check", _int, [_vp, _vp]),
    ("gs_reduce64_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_search_create", _int, [C.POINTER(_vp), _u32, _u32, _u32, _int]),
    ("gs_search_destroy", _int, [_vp]),
    ("gs_search_temp_bytes", C.c_size_t, [_u32, _u32, _u32, _int]),
    ("gs_search_plan", _int, [_u32, _u32, _u32, _u32p]),
    ("gs_search_sorted", _int, [_vp, _vp, _u32, _vp, _u32, _vp, _int, _int, _int, _int, _vp]),
    ("gs_search_set_route", _int, [_vp, _u32]),
    ("gs_search_set_table", _int, [_vp, _u32]),
    ("gs_search_last", _int, [_vp, _u32p, _u32, _vp]),
    ("gs_merge_create", _int, [C.POINTER(_vp), _u32, _u32]),
    ("gs_merge_destroy", _int, [_vp]),
    ("gs_merge_temp_bytes", C.c_size_t, [_u32, _u32]),
    ("gs_merge_plan", _int, [_u32, _u32, _u32, _u32p]),
    ("gs_merge_keys", _int, [_vp, _vp, _u32, _vp, _u32, _vp, _int, _int, _vp]),
    ("gs_merge_pairs", _int, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _int, _int, _vp]),
    ("gs_merge_positions", _int, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _int, _int, _vp]),
    ("gs_merge_last", _int, [_vp, _u32p, _u32, _vp]),
]
EXPORTED_SYMBOLS = [p[0] for p in _PROTOS]

_lib = None


class GpuSortError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = load().gs_status_string(status).decode()
        if status == GS_ERR_HIP:
            msg += f" (hipError {load().gs_last_hip_error()})"
        if status == GS_ERR_COMM:
            msg += f" (ncclResult {load().gs_last_rccl_error()})"
        super().__init__(f"{where}: {msg} [gs_status {status}]")


def load() -> C.CDLL:
    """Load libgpusort.so and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make` (hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        for name, res, args in _PROTOS:
            try:
                fn = getattr(lib, name)
            except AttributeError:
                if "GPUSORT_LIB" in os.environ:  # A/B runs against an older build: later entry points are absent
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def load_tuning() -> C.CDLL:
    """libgpusort_tuning.so (-DGS_TUNING: calibration kernels and tuning tile shapes; tools/ and bench.py's box_floor block —
    never the product path)."""
    path = os.path.join(_HERE, "lib", "libgpusort_tuning.so")
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    lib.gs_debug_copy_floor.restype = _int
    lib.gs_debug_copy_floor.argtypes = [_vp, _vp, _u32, _u32, _u32, _vp]
    return lib


def check(status: int, where: str) -> None:
    if status != GS_OK:
        raise GpuSortError(status, where)
