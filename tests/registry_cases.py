"""The ledger of compiled kernel instantiations: one row per cell of the kernel registry (gpusorting_amd/csrc/kernel_registry.hpp) that
the product build compiles, and for every row the small GPU case that runs the cell and the evidence that proves the cell did the work.

A plain module (no conftest, no fixtures).  tests/test_registry_cpu.py holds ROWS against what libgpusort.so itself reports
(gs_debug_registry_dims / gs_debug_registry_cell): a cell the library builds without a row here, or a row for a cell it does not build,
fails on the CPU.  tests/test_gpu_registry.py runs every case of CASES on the GPU.

This file restates the registry's rules on purpose: it does not ask the library what is built.  A new instantiation therefore needs a
line here ("The registry's ledger").

A row:   (family, coord, case id | None, exemption | None)
           family     name of the launcher table, FAMILIES gives its GS_KF_* number
           coord      the cell, in the table's index order (include/gpusort.h documents it next to GS_KF_*)
           case id    key of CASES: the GPU case that reaches the cell (several rows may share one: the two LAST forms of g_pos run in
                      one sort, a workgroup class per rank mode in one handle ...)
           exemption  rows without a case: none today, and tests/test_registry_cpu.py accepts none (UNCOVERED is what such a row would say)
A case:  dict(kind=..., **what the runner of that kind in test_gpu_registry.py needs): handle kind, options and setters, the sizes
         and input kinds; "evidence" names what is asserted after the call.
"""

FAMILIES = {"g_bin": 0, "g_pos": 1, "g_persist": 2, "g_small": 3, "g_mid": 4, "g_seg_wg": 5, "g_seg_vb": 6, "g_tkr_tile": 7,
            "g_tkr_vm": 8, "g_hist": 9, "g_hy_hist": 10, "g_hy_local": 11, "g_hy_local_pairs": 12}
UNCOVERED = "uncovered"

VB = (0, 4, 8)                      # value bytes by vb index
VM = (0, 1, 4, 8)                   # row-wise top-k value mode by vm index: keys only, positions, 4- / 8-byte values
SHAPES = ((512, 32), (1024, 16), (512, 16))
SMALL_UPPER = (1024, 2048, 8192, 16384, 32768)   # single-tile / workgroup classes 0 .. 4: the longest input each takes
SMALL_LOWER = (0, 1024, 2048, 8192, 16384)       # ... and the longest the class below takes
KEY16 = (6, 7, 8, 9)                # uint16, int16, float16, bfloat16

# input kinds (test_gpu_registry.make_keys)
UNIFORM, SKEW90, AND4, LOW16, TOPBYTE = "uniform", "skew90", "and4", "low16const", "topbyte_const"


def small_holds(cls, vb):
    """What 160 KiB of LDS hold: classes 0 .. 2 every value width, class 3 keys only and 4-byte values, class 4 keys only."""
    return cls < 3 or (cls == 3 and vb != 8) or (cls == 4 and vb == 0)


ROWS = []
CASES = {}


def _row(family, coord, case=None, exempt=None):
    assert (case is None) != (exempt is None)
    ROWS.append((family, tuple(coord), case, exempt))


def _case(cid, **what):
    assert cid not in CASES, cid
    CASES[cid] = what
    return cid


# ---- g_small [class][rank][vb][kt]: the single-tile sort.  64-bit keys: classes 0 .. 2 --------------------------------------------
for cls in range(5):
    for v, vb in enumerate(VB):
        for kt in range(6):
            if not small_holds(cls, vb) or (cls >= 3 and kt >= 3):
                continue
            cid = _case(f"small-c{cls}-v{vb}-kt{kt}", kind="small", handle="onesweep", cls=cls, vb=vb, kt=kt, ranks=(0, 1),
                        options=dict(mid_path=0 if cls >= 3 else 1), sizes=(SMALL_UPPER[cls] - 1, SMALL_LOWER[cls] + 2),
                        inputs=(UNIFORM,), evidence="route.small == class; check_state keys_per_pass all zero")
            for r in (0, 1):
                _row("g_small", (cls, r, v, kt), cid)

# ---- g_bin [vr - 1][shape][rank][vb][kt]: digit_binning_kernel.  64-bit keys on 512 x 16 only; VR 2 (the two-round form of the
# 8-byte-value pass) on 512 x 32 with 32-bit keys: it runs beside VR 1 and the pass's PF_SKEW flag picks one of them --------------
for s, (threads, kpt) in enumerate(SHAPES):
    for v, vb in enumerate(VB):
        for kt in range(6 if s == 2 else 3):
            two_forms = s == 0 and vb == 8
            cid = _case(f"bin-s{s}-v{vb}-kt{kt}", kind="bin", handle="onesweep", shape=(threads, kpt), shape_index=s, vb=vb, kt=kt,
                        ranks=(0, 1), options=dict(small_path=0, mid_path=0, position_chains=0), sizes=(5 * threads * kpt + 37,),
                        inputs=(UNIFORM, SKEW90, AND4, LOW16), two_forms=two_forms,
                        evidence="route.shape; pass flags per input kind (PF_SKEW: which form of the 8-byte-value pass worked; PF_SKIP / "
                                 "PF_SRC_ALT: dropped passes); keys_per_pass; chains clean")
            for r in (0, 1):
                _row("g_bin", (0, s, r, v, kt), cid)
                if two_forms:
                    _row("g_bin", (1, s, r, v, kt), cid)

# ---- g_pos [vb][last][kt]: the position-chain forms (rank mode 1 only); both LAST forms run in one sort ---------------------------
for v, vb in enumerate(VB):
    for kt in range(3):
        cid = _case(f"pos-v{vb}-kt{kt}", kind="pos", handle="onesweep", vb=vb, kt=kt,
                    options=dict(position_chains=2, position_chains_min_log2=20, mid_path=0), sizes=((1 << 20) + 5,),
                    inputs=(UNIFORM,), evidence="route.pos; GS_PF_POS in every pass that ran; chains clean")
        for last in (0, 1):
            _row("g_pos", (v, last, kt), cid)

# ---- the two-level plan: g_hy_hist [kt], g_hy_local [class][kt], g_hy_local_pairs [8-byte values][class][kt], g_persist [8-byte
# values][kt].  The class of the bucket-local sort follows n (class 0 up to 2^27 keys): class 0 runs as every sort of this size does;
# classes 1 .. 3 are forced (gs_debug_set_hy_class) on the ladder input of tests/hy_bucket_inputs.py, whose largest buckets hold exactly
# the class's cap.  (8-byte values, class 3: not built — the 24 576-pair local sort does not fit LDS) ----
HY_CAP = (3072, 6144, 12288, 24576)   # keys the bucket-local sort's workgroup holds, by class
for kt in range(3):
    for v, vb in enumerate(VB):
        cid = _case(f"hy-v{vb}-kt{kt}", kind="hy", handle="onesweep", vb=vb, kt=kt, max_keys=1 << 22,
                    options=dict(plan=2, position_chains_min_log2=20, small_path=0, mid_path=0), sizes=((1 << 20) + 16385,),
                    inputs=(UNIFORM,), evidence="route.hy; last_plan two_level")
        if vb == 0:
            _row("g_hy_hist", (kt,), cid)
            _row("g_hy_local", (0, kt), cid)
        else:
            _row("g_persist", (v - 1, kt), cid)
            _row("g_hy_local_pairs", (v - 1, 0, kt), cid)
        for cls in (1, 2, 3):
            if vb == 8 and cls == 3:
                continue
            cid = _case(f"hycls-c{cls}-v{vb}-kt{kt}", kind="hy_class", handle="onesweep", hy_class=cls, cap=HY_CAP[cls], vb=vb, kt=kt,
                        max_keys=1 << 22, options=dict(plan=2, position_chains_min_log2=20, small_path=0, mid_path=0),
                        inputs=("ladder",), evidence="last_plan two_level; largest_bucket == cap of the class")
            if vb == 0:
                _row("g_hy_local", (cls, kt), cid)
            else:
                _row("g_hy_local_pairs", (v - 1, cls, kt), cid)

# ---- g_mid [class][rank][vb][kt]: the two-launch mid-size route, at the smallest n of each class ----------------------------------
MID_VB = {0: (0, 4, 8), 1: (0, 4), 2: (0,), 3: (0,), 4: (4,)}
MID_MIN_N = {0: 8193, 1: (1 << 20) + 1, 2: (1 << 21) + 1, 3: (1 << 22) + 1, 4: (1 << 21) + 1}
for cls in range(5):
    for vb in MID_VB[cls]:
        for kt in range(3):
            cid = _case(f"mid-c{cls}-v{vb}-kt{kt}", kind="mid", handle="onesweep", cls=cls, vb=vb, kt=kt, ranks=(0, 1), options={},
                        sizes=(MID_MIN_N[cls],), inputs=(UNIFORM, TOPBYTE), evidence="route.mid == class; no scan state left")
            for r in (0, 1):
                _row("g_mid", (cls, r, VB.index(vb), kt), cid)

# ---- g_seg_wg [class][rank][vb][kt]: one call holds every workgroup class the value width has; the engine's rank mode picks the rank ----
for v, vb in enumerate(VB):
    for kt in range(3):
        classes = tuple(c for c in range(5) if small_holds(c, vb))
        cid = _case(f"segwg-v{vb}-kt{kt}", kind="seg_wg", handle="segsort", vb=vb, kt=kt, ranks=(0, 1), classes=classes,
                    evidence="class_of before the call; last_classes; engine.rank_mode")
        for c in classes:
            for r in (0, 1):
                _row("g_seg_wg", (c, r, v, kt), cid)

# ---- g_seg_vb [vb]: packed, wave, head merge; the key type is a run-time argument: all three run ----------------------------------
for v, vb in enumerate(VB):
    _row("g_seg_vb", (v,), _case(f"segvb-v{vb}", kind="seg_vb", handle="segsort", vb=vb, kts=(0, 1, 2),
                                 evidence="last_classes: packed, wave and long segments counted"))

# ---- g_tkr_tile [2-byte keys][class][rank][vm], g_tkr_vm [2-byte keys][vm]: the key type within a width is a run-time argument ----
for k16 in (0, 1):
    for m, vm in enumerate(VM):
        vb = 0 if vm == 0 else 8 if vm == 8 else 4
        kts = KEY16 if k16 else (0, 1, 2)
        for cls in range(5):
            if not small_holds(cls, vb):
                continue
            cid = _case(f"tkrtile-k{16 if k16 else 32}-c{cls}-vm{vm}", kind="tkr_tile", handle="topk", key16=k16, cls=cls, vm=vm, vb=vb, kts=kts,
                        ranks=(0, 1), rows=8, row_lens=(SMALL_UPPER[cls], max(SMALL_LOWER[cls], 256) + 1), ks=(1, 7, "row_len"),
                        evidence="class of row_len before the call; rows_last route TILE; engine.rank_mode")
            for r in (0, 1):
                _row("g_tkr_tile", (k16, cls, r, m), cid)
        _row("g_tkr_vm", (k16, m), _case(f"tkrvm-k{16 if k16 else 32}-vm{vm}", kind="tkr_vm", handle="topk", key16=k16, vm=vm, vb=vb, kts=kts,
                                         wave_row_lens=(1, 65, 256), stream_extra=3, evidence="rows_last route WAVE / STREAM"))

# ---- g_hist [kt]: 32-bit key types through gs_onesweep_global_histogram against the oracle's histogram (and every sort above);
# 64-bit key types through the 512 x 16 binning cases, whose sorts start with that histogram -------------------------------------
for kt in range(3):
    _row("g_hist", (kt,), _case(f"hist-kt{kt}", kind="hist", handle="onesweep", kt=kt, sizes=(40997,), evidence="oracle.global_histogram"))
for kt in range(3, 6):
    _row("g_hist", (kt,), f"bin-s2-v0-kt{kt}")

# ---- 1-D top-k with the engine at rank 0: no registry table of its own (tk_scatter_kernel is instantiated by value mode in
# topk_host.hpp); the single-tile route and the select route's final sort of k run on the rank-0 single-tile kernels -------------
for vm in VM:
    _case(f"topk1d-vm{vm}", kind="topk1d", handle="topk", vm=vm, vb=0 if vm == 0 else 8 if vm == 8 else 4, ranks=(0, 1),
          single=(4097, 100), select=((1 << 16) + 1, 1000), evidence="gs_topk_last route; engine.rank_mode")


def rows_by_case():
    out = {}
    for family, coord, case, _ in ROWS:
        if case is not None:
            out.setdefault(case, []).append((family, coord))
    return out
