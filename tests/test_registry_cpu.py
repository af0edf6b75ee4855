"""CPU tests of the kernel registry's ledger (tests/registry_cases.py): the set of kernel instantiations libgpusort.so reports as built
(gs_debug_registry_dims / gs_debug_registry_cell, pure host functions) equals the ledger's rows, and every row has a GPU case — so a
new instantiation without a GPU case, or a case for a kernel that is gone, fails here, without a GPU."""
import ctypes as C
import itertools
import os

import registry_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gpusorting_amd import _lib
    return _lib, _lib.load()


def _dims(lib, family):
    d = (C.c_int32 * 5)(*([-7] * 5))
    r = lib.gs_debug_registry_dims(family, d)
    return r, list(d)


def _cell(lib, family, coord):
    c = (C.c_int32 * 5)(*(list(coord) + [0] * (5 - len(coord))))
    return lib.gs_debug_registry_cell(family, c)


def _built_cells(lib):
    built, unbuilt = set(), set()
    for name, family in rc.FAMILIES.items():
        r, d = _dims(lib, family)
        assert 1 <= r <= 5 and all(x >= 1 for x in d[:r]) and d[r:] == [1] * (5 - r), (name, r, d)
        for coord in itertools.product(*(range(x) for x in d[:r])):
            got = _cell(lib, family, coord)
            assert got in (0, 1), (name, coord, got)
            (built if got else unbuilt).add((name, coord))
    return built, unbuilt


def test_families_match_the_header():
    L, lib = _lib()
    assert len(rc.FAMILIES) == L.GS_KF_COUNT and sorted(rc.FAMILIES.values()) == list(range(L.GS_KF_COUNT))
    for name, family in rc.FAMILIES.items():
        assert getattr(L, "GS_KF_" + name[2:].upper()) == family, name
    text = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    for name, family in rc.FAMILIES.items():
        assert f"#define GS_KF_{name[2:].upper()} {family}u" in text, name
    for flag in ("SKEW", "SKIP", "SRC_ALT", "LAST", "POS"):
        assert f"#define GS_PF_{flag} {getattr(L, 'GS_PF_' + flag)}u" in text, flag


def test_ledger_equals_the_registry():
    """No built cell without a row, no row for a cell that is not built, no cell listed twice."""
    _, lib = _lib()
    built, unbuilt = _built_cells(lib)
    listed = [(family, coord) for family, coord, _, _ in rc.ROWS]
    assert len(listed) == len(set(listed)), sorted(x for x in set(listed) if listed.count(x) > 1)
    listed = set(listed)
    assert not (built - listed), f"built without a ledger row (add a case to tests/registry_cases.py): {sorted(built - listed)}"
    assert not (listed - built), f"ledger rows for cells this build does not compile: {sorted(listed - built)}"
    assert len(built) > 400 and unbuilt, (len(built), len(unbuilt))   # (the registry leaves cells out by design: 64-bit keys on big tiles ...)
    # the cells the issue that brought the ledger names: the rank-0 halves of the segmented sort and the row-wise top-k
    for name in ("g_seg_wg", "g_tkr_tile"):
        assert any(f == name and (c[1] if name == "g_seg_wg" else c[2]) == 0 and case for f, c, case, _ in rc.ROWS), name


def test_every_row_has_a_case():
    """No exemptions: the classes of the two-level plan's bucket-local sorts that n > 2^27 selects, once reached by full-size tests only
    (or not at all), run with their class forced (gs_debug_set_hy_class)."""
    used = set()
    for family, coord, case, exempt in rc.ROWS:
        assert family in rc.FAMILIES
        assert exempt is None and case in rc.CASES, (family, coord, case, exempt)
        used.add(case)
    extra = {c for c, what in rc.CASES.items() if what["kind"] == "topk1d"}   # (cases without a registry table of their own)
    assert used | extra == set(rc.CASES), sorted(set(rc.CASES) - used - extra)
    for cid, what in rc.CASES.items():
        assert what["evidence"], cid
    # the bucket-local sorts: 12 keys-only cells, 21 for pairs; classes 1 .. 3 by a case that forces the class and sorts a bucket of its cap
    local = [(f, c, case) for f, c, case, _ in rc.ROWS if f in ("g_hy_local", "g_hy_local_pairs")]
    assert sum(f == "g_hy_local" for f, _, _ in local) == 12 and sum(f == "g_hy_local_pairs" for f, _, _ in local) == 21
    for family, coord, case in local:
        cls, what = coord[-2], rc.CASES[case]
        if cls == 0:
            assert what["kind"] == "hy", (family, coord)
        else:
            assert what["kind"] == "hy_class" and what["hy_class"] == cls and what["cap"] == rc.HY_CAP[cls], (family, coord, what)
            assert what["kt"] == coord[-1] and what["vb"] == (0 if family == "g_hy_local" else (4, 8)[coord[0]]), (family, coord, what)
            assert what["evidence"] == "last_plan two_level; largest_bucket == cap of the class"


def test_uncovered_cells_are_the_ones_the_design_document_lists():
    """DESIGN.md carries the table of uncovered cells between its markers: the ledger has none, and the table is empty."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("<!-- uncovered-cells:begin -->")
    table = text[start:text.index("<!-- uncovered-cells:end -->")]
    listed = {ln.split("|")[1].strip() for ln in table.splitlines() if ln.startswith("| `g_")}
    want = {f"`{family}{list(coord)}`" for family, coord, _, exempt in rc.ROWS if exempt is not None}
    assert want == set() and listed == want, (sorted(listed - want), sorted(want - listed))


def test_registry_hooks_refuse_bad_families_and_coordinates():
    L, lib = _lib()
    d = (C.c_int32 * 5)()
    assert lib.gs_debug_registry_dims(L.GS_KF_COUNT, d) == -1 and lib.gs_debug_registry_dims(0xFFFFFFFF, d) == -1
    assert lib.gs_debug_registry_dims(L.GS_KF_BIN, None) == -1
    assert lib.gs_debug_registry_cell(L.GS_KF_BIN, None) == -1
    assert _cell(lib, L.GS_KF_COUNT, (0,)) == -1
    for name, family in rc.FAMILIES.items():
        r, dims = _dims(lib, family)
        for k in range(r):
            for bad in (-1, dims[k]):
                coord = [0] * r
                coord[k] = bad
                assert _cell(lib, family, coord) == -1, (name, coord)
        if r < 5:   # a coordinate behind the table's last index must be 0
            assert _cell(lib, family, [0] * r + [1]) == -1, name
    # the extents as the header documents them
    assert _dims(lib, L.GS_KF_BIN) == (5, [2, 3, 2, 3, 6]) and _dims(lib, L.GS_KF_SEG_WG) == (4, [5, 2, 3, 3, 1])
    assert _dims(lib, L.GS_KF_TKR_TILE) == (4, [2, 5, 2, 4, 1]) and _dims(lib, L.GS_KF_HIST) == (1, [6, 1, 1, 1, 1])


def test_route_and_flag_hooks_refuse_null_arguments():
    L, lib = _lib()
    buf = (C.c_uint32 * 8)()
    assert lib.gs_debug_sort_route(None, 1024, 0, buf) == L.GS_ERR_ARG
    assert lib.gs_debug_pass_flags(None, buf, None) == L.GS_ERR_ARG
    assert lib.gs_debug_set_hy_class(None, -1) == L.GS_ERR_ARG
    assert lib.gs_segsort_engine(None) is None and lib.gs_topk_engine(None) is None


def test_tuning_build_reports_its_own_registry():
    """The tuning build (u32 keys-only kernels, three more tile shapes) is outside the ledger; its registry hooks still answer, and
    say what that flavour is: more shapes, no segmented sort, no selection."""
    L, _ = _lib()
    path = os.path.join(os.path.dirname(L.LIB_PATH), "libgpusort_tuning.so")
    lib = C.CDLL(path)
    lib.gs_debug_registry_dims.argtypes = [C.c_uint32, C.POINTER(C.c_int32)]
    lib.gs_debug_registry_cell.argtypes = [C.c_uint32, C.POINTER(C.c_int32)]
    assert _dims(lib, L.GS_KF_BIN) == (5, [2, 6, 2, 3, 6])
    assert _cell(lib, L.GS_KF_BIN, (0, 5, 1, 0, 0)) == 1 and _cell(lib, L.GS_KF_BIN, (0, 0, 0, 1, 0)) == 0
    assert _cell(lib, L.GS_KF_SEG_VB, (0,)) == 0 and _cell(lib, L.GS_KF_TKR_VM, (0, 0)) == 0 and _cell(lib, L.GS_KF_HIST, (5,)) == 1
