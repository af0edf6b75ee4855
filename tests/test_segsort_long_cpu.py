"""CPU tests of the segmented sort's device route for long 32-bit segments (gs_segsort_set_long_route and its companions in
include/gpusort.h): the five entries and their constants are declared, exported and bound; the host-only entries
(gs_segsort_long_units, gs_segsort_long_temp_bytes) state the bound the header gives, that bound holds every exact unit count, and they
refuse what gs_segsort16_units refuses; the null handle is answered before anything touches a GPU.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS, PAIRS = 0, 1
MODES = ((KEYS, 0), (PAIRS, 4), (PAIRS, 8))
SYMBOLS = ("gs_segsort_set_long_route", "gs_segsort_get_long_route", "gs_segsort_long_units", "gs_segsort_long_temp_bytes", "gs_segsort_last")


def test_symbols_and_constants_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_segsort_[a-z0-9_]+)\s*\(", text))
    assert set(SYMBOLS) <= declared
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SEGSORT_(?:LONG|R|LF|REPORT)_?[A-Z0-9_]*)\s+(0x[0-9a-fA-F]+|\d+)u?\s*$", text, flags=re.M))
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value, 0), name
    assert {"GS_SEGSORT_LONG_HOST", "GS_SEGSORT_LONG_DEVICE", "GS_SEGSORT_LONG_PASSES", "GS_SEGSORT_REPORT_WORDS", "GS_SEGSORT_LF_UNITS",
            "GS_SEGSORT_LF_COUNT", "GS_SEGSORT_LF_SCAN", "GS_SEGSORT_LF_SCATTER", "GS_SEGSORT_LF_ALL"} \
        | {f"GS_SEGSORT_R_{w}" for w in ("ROUTE", "UNITS", "LONG", "UNIT_CAP", "FORMS", "STATUS", "RANK", "N")} == set(defines)
    assert (_lib.GS_SEGSORT_LONG_HOST, _lib.GS_SEGSORT_LONG_DEVICE, _lib.GS_SEGSORT_LONG_PASSES, _lib.GS_SEGSORT_REPORT_WORDS) == (0, 1, 4, 8)
    assert [getattr(_lib, f"GS_SEGSORT_R_{w}") for w in ("ROUTE", "UNITS", "LONG", "UNIT_CAP", "FORMS", "STATUS", "RANK", "N")] == list(range(8))
    # the part is whole tiles of the row-wise sort's pass route
    m = re.search(r"#define\s+GS_SEGSORT_LONG_PART\s+\((\d+)u \* GS_SORT_ROWS_TILE\)", text)
    assert m and _lib.GS_SEGSORT_LONG_PART == int(m.group(1)) * _lib.GS_SORT_ROWS_TILE and int(m.group(1)) in (4, 8, 16)
    # the forms: units, count, scan and one bit per (value width, rank mode) of the scatter
    bits = [_lib.GS_SEGSORT_LF_UNITS, _lib.GS_SEGSORT_LF_COUNT, _lib.GS_SEGSORT_LF_SCAN] + \
           [_lib.GS_SEGSORT_LF_SCATTER << (2 * v + r) for v in range(3) for r in range(2)]
    assert len(set(bits)) == 9 and sum(bits) == _lib.GS_SEGSORT_LF_ALL == 0x1FF
    import gpusorting_amd as g
    from gpusorting_amd import segsort
    assert g.segsort_long_units is segsort.segsort_long_units and segsort.LONG_ROUTES == {"host": 0, "device": 1}


def test_null_handle_and_refusals_that_need_no_device():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    p = (C.c_uint32 * 16)()
    for route in (_lib.GS_SEGSORT_LONG_HOST, _lib.GS_SEGSORT_LONG_DEVICE, 2, 0xFFFFFFFF):
        assert lib.gs_segsort_set_long_route(None, route) == A
    assert lib.gs_segsort_get_long_route(None) == 0xFFFFFFFF
    assert lib.gs_segsort_last(None, p, 8, None) == A
    # temp_bytes and units: 0 for what gs_segsort16_units refuses
    for f, f16 in ((lib.gs_segsort_long_temp_bytes, lib.gs_segsort16_temp_bytes), (lib.gs_segsort_long_units, lib.gs_segsort16_units)):
        for args in ((0, 16, KEYS, 0), (1 << 30, 16, KEYS, 0), (1024, 0, KEYS, 0), (1024, 1 << 30, KEYS, 0), (1024, 16, KEYS, 4),
                     (1024, 16, PAIRS, 2), (1024, 16, PAIRS, 0), (1024, 16, 7, 0)):
            assert f(*args) == 0 and f16(*args) == 0, args
    assert lib.gs_segsort_long_units(1024, 16, KEYS, 0) == 0 and lib.gs_segsort_long_temp_bytes(1024, 16, KEYS, 0) == 0   # nothing can be long


def test_units_is_the_bound_of_the_header_and_temp_bytes_is_sized_by_it():
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort import segsort_long_units
    lib = _lib.load()
    part = 4 * 4096   # the restatement: GS_SEGSORT_LONG_PART
    assert part == _lib.GS_SEGSORT_LONG_PART
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for mode, vb in MODES:
        lds = {0: 32768, 4: 16384, 8: 8192}[vb]
        assert lib.gs_segsort_max_lds_segment(mode, vb) == lds
        for n in (1, 1000, lds, lds + 1, part - 1, part, part + 1, 3 * part + 5, (1 << 20) + 3, 1 << 27, _lib.GS_MAX_KEYS):
            for segs in (1, 2, 3, 100, 4096, 1 << 20, _lib.GS_MAX_KEYS):
                longs = min(segs, n // (lds + 1))
                want = n // part + longs
                assert lib.gs_segsort_long_units(n, segs, mode, vb) == want == segsort_long_units(n, segs, mode, vb), (n, segs, mode, vb)
                assert lib.gs_segsort_long_temp_bytes(n, segs, mode, vb) == up(16 * want) + up(16 * longs) + 2 * up(1024 * want), (n, segs, mode, vb)


def test_units_is_never_below_the_exact_unit_count():
    """A segment of length L > the LDS limit is cut into ceil(L / PART) parts; the sum over any set of lengths that fits n stays within
    the bound."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    part = _lib.GS_SEGSORT_LONG_PART
    rng = np.random.default_rng(32)
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        worst = 0.0
        for trial in range(300):
            segs = int(rng.integers(1, 40))
            style = trial % 4
            if style == 0:      # just above the LDS limit: the most long segments per element
                lens = rng.integers(lds + 1, lds + 4, segs)
            elif style == 1:    # just above whole parts: the most parts per element
                lens = rng.integers(1, 5, segs) * part + rng.integers(1, 3, segs)
            elif style == 2:    # anything, short ones among them
                lens = rng.integers(0, 6 * part, segs)
            else:
                lens = np.where(rng.random(segs) < 0.5, rng.integers(0, 300, segs), rng.integers(lds + 1, 3 * part, segs))
            n = int(lens.sum()) + int(rng.integers(0, 3))
            if n == 0:
                continue
            exact = int(sum(-(-int(x) // part) for x in lens if x > lds))
            bound = lib.gs_segsort_long_units(n, segs, mode, vb)
            assert exact <= bound, (lens.tolist(), n, exact, bound)
            worst = max(worst, exact / max(bound, 1))
        assert worst > 0.9   # the sweep comes close to the bound: it is not vacuous
