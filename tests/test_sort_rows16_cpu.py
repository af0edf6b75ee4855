"""CPU tests of the row-wise sort of 16-bit keys (gs_sort_rows16_* in include/gpusort.h, gpusorting_amd/rowsort16.py): the symbols and
constants are declared, exported and bound; the host-only entries (gs_sort_rows16_plan, gs_sort_rows16_temp_bytes) are consistent with
gs_sort_rows_plan's cut; the host-side argument checks answer before anything touches a GPU; and sort_rows16_reference — the numpy
statement of the semantics the GPU tests compare with — is checked against hand-built rows and against the references the library
already has.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = 6, 7, 8, 9
KEY16 = (U16, I16, F16, BF16)
KEYS, PAIRS = 0, 1
MODES = ((KEYS, 0), (PAIRS, 4), (PAIRS, 8))
SYMBOLS = ("gs_sort_rows16_create", "gs_sort_rows16_destroy", "gs_sort_rows16_temp_bytes", "gs_sort_rows16_plan", "gs_sort_rows16_keys",
           "gs_sort_rows16_pairs", "gs_sort_rows16_argsort", "gs_sort_rows16_check", "gs_sort_rows16_last", "gs_sort_rows16_set_rank_mode",
           "gs_sort_rows16_get_rank_mode")


def test_symbols_and_constants_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_sort_rows16_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SORT_ROWS16_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", text))
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value, 0), name
    assert {"GS_SORT_ROWS16_PASSES", "GS_SORT_ROWS16_F_CLEAR", "GS_SORT_ROWS16_F_LDS_WAVE", "GS_SORT_ROWS16_F_LDS_TILE", "GS_SORT_ROWS16_F_COUNT",
            "GS_SORT_ROWS16_F_SCAN", "GS_SORT_ROWS16_F_SCATTER", "GS_SORT_ROWS16_F_ALL"} == set(defines)
    # the scatter's eight forms (keys only, positions, 4- and 8-byte values, each in both rank modes) lie behind the five plain ones
    assert _lib.GS_SORT_ROWS16_F_ALL == 31 | sum(_lib.GS_SORT_ROWS16_F_SCATTER << b for b in range(8))
    import gpusorting_amd as g
    from gpusorting_amd.rowsort16 import SORT_ROWS16_FORMS
    assert g.RowSort16 and g.sort_rows16_reference and g.sort_rows16_plan and g.sort_rows and g.sort_rows_ and g.argsort_rows
    assert g.SORT_ROWS16_FORMS is SORT_ROWS16_FORMS
    assert len(SORT_ROWS16_FORMS) == 13 and sum(SORT_ROWS16_FORMS.values()) == _lib.GS_SORT_ROWS16_F_ALL


def _plan(lib, rows, row_len, mode, vb, entry="gs_sort_rows16_plan"):
    from gpusorting_amd import _lib
    p = (C.c_uint32 * _lib.GS_SORT_ROWS_PLAN_WORDS)()
    assert getattr(lib, entry)(rows, row_len, mode, vb, p) == 0, (rows, row_len, mode, vb)
    return {"route": p[0], "parts": p[1], "per": p[2], "tile": p[3], "passes": p[4], "cap": p[5]}


def test_route_switches_exactly_behind_the_lds_limit():
    from gpusorting_amd import _lib
    from gpusorting_amd.rowsort16 import sort_rows16_plan
    lib = _lib.load()
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        for rows in (1, 2, 5, 1000):
            for row_len in (1, 2, 257, lds - 1, lds):
                p = _plan(lib, rows, row_len, mode, vb)
                assert p == {"route": _lib.GS_SORT_ROWS_ROUTE_LDS, "parts": 1, "per": row_len, "tile": 0, "passes": 0, "cap": max(rows, _lib.GS_SORT_ROWS_PCAP)}
            for row_len in (lds + 1, lds + 2, 2 * lds):
                p = _plan(lib, rows, row_len, mode, vb)
                assert (p["route"], p["tile"], p["passes"]) == (_lib.GS_SORT_ROWS_ROUTE_PASSES, _lib.GS_SORT_ROWS_TILE, 2) and _lib.GS_SORT_ROWS16_PASSES == 2
        assert sort_rows16_plan(3, lds, mode, vb)["route"] == 1 and sort_rows16_plan(3, lds + 1, mode, vb)["route"] == 2


def test_plan_is_the_cut_of_the_32_bit_plan_and_covers_the_row_in_whole_tiles():
    from gpusorting_amd import _lib
    from gpusorting_amd.rowsort16 import sort_rows16_plan
    lib = _lib.load()
    tile, pcap = _lib.GS_SORT_ROWS_TILE, _lib.GS_SORT_ROWS_PCAP
    shapes = [(1, 32769), (1, 8 * tile + 1), (1, 9 * tile), (1, 9 * tile - 1), (3, 40001), (1, 1 << 22), (4, 1 << 22), (32, 262144), (256, 131072),
              (64, 128256), (256, 32000), (8, 151936), (1, 262144), (1024, 32769), (1023, 40000), (1025, 40000), (pcap // 2, 10 * tile + 1),
              (20000, 32769), (1, _lib.GS_MAX_KEYS), (2, _lib.GS_MAX_KEYS // 2), (7, 100003), (5, 300), (9, 8193), (9, 16385)]
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        for rows, row_len in shapes:
            p, p32 = _plan(lib, rows, row_len, mode, vb), _plan(lib, rows, row_len, mode, vb, "gs_sort_rows_plan")
            # no constant was changed: the same route, parts, elements per part, tile and cap; only the number of passes differs
            assert {k: v for k, v in p.items() if k != "passes"} == {k: v for k, v in p32.items() if k != "passes"}, (rows, row_len, p, p32)
            if row_len <= lds:
                assert p["route"] == _lib.GS_SORT_ROWS_ROUTE_LDS and p["passes"] == 0
                continue
            assert p["route"] == _lib.GS_SORT_ROWS_ROUTE_PASSES and p["tile"] == tile and p["passes"] == 2 and p32["passes"] == 4
            tiles = -(-row_len // tile)
            assert p["per"] % tile == 0 and p["per"] >= tile
            assert 1 <= p["parts"] <= max(1, tiles // _lib.GS_SORT_ROWS_MIN_TILES)
            assert p["parts"] * p["per"] >= row_len > (p["parts"] - 1) * p["per"], (rows, row_len, p)
            assert p["cap"] == max(rows, pcap) and rows * p["parts"] <= p["cap"], (rows, row_len, p)
    assert sort_rows16_plan(3, 40001, PAIRS, 4) == {"route": 2, "parts": 5, "per_part": 2 * tile, "tile": tile, "passes": 2, "cap": pcap}
    assert sort_rows16_plan(3, 100)["route"] == 1


def test_temp_bytes_hold_every_plan_at_max_keys():
    from gpusorting_amd import _lib
    lib = _lib.load()
    tile, pcap = _lib.GS_SORT_ROWS_TILE, _lib.GS_SORT_ROWS_PCAP
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        for max_keys in (1, 1000, lds, lds + 1, 1 << 16, (1 << 20) + 3, 1 << 24, _lib.GS_MAX_KEYS):
            r = max_keys // (lds + 1)
            units = 0 if r == 0 else min(max(r, pcap), max_keys // tile + r)
            assert lib.gs_sort_rows16_temp_bytes(max_keys, mode, vb) == 256 + 2 * up(units * 1024), (max_keys, mode, vb)
            for rows in sorted({1, 2, 3, r, max(1, r // 2), min(r, pcap), min(r, pcap + 1)} - {0}):
                if rows > r:
                    continue
                for row_len in {lds + 1, max_keys // rows, min(max_keys // rows, lds + tile + 1)}:
                    assert rows * _plan(lib, rows, row_len, mode, vb)["parts"] <= units
    assert lib.gs_sort_rows16_temp_bytes(0, KEYS, 0) == 0 and lib.gs_sort_rows16_temp_bytes(1 << 30, KEYS, 0) == 0
    assert lib.gs_sort_rows16_temp_bytes(16, KEYS, 4) == 0 and lib.gs_sort_rows16_temp_bytes(16, PAIRS, 2) == 0 and lib.gs_sort_rows16_temp_bytes(16, 7, 0) == 0


def test_argument_errors_that_need_no_device():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    p = (C.c_uint32 * 8)()
    assert lib.gs_sort_rows16_plan(4, 16, KEYS, 0, None) == A
    assert lib.gs_sort_rows16_plan(0, 16, KEYS, 0, p) == S and lib.gs_sort_rows16_plan(4, 0, KEYS, 0, p) == S
    assert lib.gs_sort_rows16_plan(1 << 15, 1 << 15, KEYS, 0, p) == S and lib.gs_sort_rows16_plan(1 << 16, 1 << 16, KEYS, 0, p) == S
    assert lib.gs_sort_rows16_plan(1, _lib.GS_MAX_KEYS, KEYS, 0, p) == _lib.GS_OK
    for mode, vb in ((KEYS, 4), (PAIRS, 2), (PAIRS, 0), (7, 0)):
        assert lib.gs_sort_rows16_plan(4, 16, mode, vb, p) == M
    h = C.c_void_p()
    assert lib.gs_sort_rows16_create(None, 1024, KEYS, 0) == A
    assert lib.gs_sort_rows16_create(C.byref(h), 0, KEYS, 0) == S and lib.gs_sort_rows16_create(C.byref(h), 1 << 30, KEYS, 0) == S
    assert lib.gs_sort_rows16_create(C.byref(h), 1024, KEYS, 4) == M and lib.gs_sort_rows16_create(C.byref(h), 1024, PAIRS, 2) == M
    assert not h.value
    assert lib.gs_sort_rows16_destroy(None) == A
    # the null handle is looked at before anything else, in every entry
    assert lib.gs_sort_rows16_keys(None, None, None, 0, 0, 99, 0, None) == A
    assert lib.gs_sort_rows16_keys(None, 16, 32, 4, 4, U16, 0, None) == A
    assert lib.gs_sort_rows16_pairs(None, 16, 32, 48, 64, 4, 4, BF16, 0, None) == A
    assert lib.gs_sort_rows16_argsort(None, 16, 32, 48, 64, 4, 4, F16, 0, None) == A
    assert lib.gs_sort_rows16_check(None, None) == A
    assert lib.gs_sort_rows16_last(None, p, 8, None) == A
    assert lib.gs_sort_rows16_set_rank_mode(None, 0) == A
    assert lib.gs_sort_rows16_get_rank_mode(None) == -1


def _ref(keys, values=None, kt=U16, desc=False, dtype=np.uint16):
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    return sort_rows16_reference(np.asarray(keys, dtype=dtype), values, kt, desc)


def test_reference_on_hand_built_rows():
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    # ties: ascending keeps equal keys in rising position, descending is the exact reverse of the row; rows do not mix
    k, p = _ref([[5, 3, 5, 3, 9], [1, 1, 0, 1, 0]])
    assert k.dtype == np.uint16 and k.tolist() == [[3, 3, 5, 5, 9], [0, 0, 1, 1, 1]]
    assert p.dtype == np.uint32 and p.tolist() == [[1, 3, 0, 2, 4], [2, 4, 0, 1, 3]]
    k, p = _ref([[5, 3, 5, 3, 9], [1, 1, 0, 1, 0]], desc=True)
    assert k.tolist() == [[9, 5, 5, 3, 3], [1, 1, 1, 0, 0]] and p.tolist() == [[4, 2, 0, 3, 1], [3, 1, 0, 4, 2]]
    # rows = 1 and row_len = 1
    k, p = _ref([[7, 2, 7]])
    assert k.tolist() == [[2, 7, 7]] and p.tolist() == [[1, 0, 2]]
    k, p = _ref([[7], [2], [9]], desc=True)
    assert k.tolist() == [[7], [2], [9]] and p.tolist() == [[0], [0], [0]]
    # the same bits as uint16 and as int16
    bits = [[0x0001, 0xFFFF, 0x8000, 0x7FFF, 0]]
    assert _ref(bits, kt=U16)[0].tolist() == [[0, 1, 0x7FFF, 0x8000, 0xFFFF]]
    assert _ref(bits, kt=I16)[0].tolist() == [[0x8000, 0xFFFF, 0, 1, 0x7FFF]]
    assert _ref(np.array(bits, dtype=np.uint16).view(np.int16), kt=I16, dtype=np.int16)[0].tolist() == [[-32768, -1, 0, 1, 32767]]
    # float16 and bfloat16: -0 < +0, and equal zeros keep their positions
    for kt in (F16, BF16):
        k, p = _ref([[0x0000, 0x8000, 0x0000, 0x8000]], kt=kt)
        assert k.tolist() == [[0x8000, 0x8000, 0, 0]] and p.tolist() == [[1, 3, 0, 2]]
    # float16: +nan, +inf, -inf, -nan, 1, -1, +snan, -nan(all ones), +subnormal, -subnormal
    f16 = [[0x7E01, 0x7C00, 0xFC00, 0xFE01, 0x3C00, 0xBC00, 0x7C01, 0xFFFF, 0x0001, 0x8001]]
    assert _ref(f16, kt=F16)[0].tolist() == [[0xFFFF, 0xFE01, 0xFC00, 0xBC00, 0x8001, 0x0001, 0x3C00, 0x7C00, 0x7C01, 0x7E01]]
    assert _ref(f16, kt=F16, desc=True)[0].tolist() == [[0x7E01, 0x7C01, 0x7C00, 0x3C00, 0x0001, 0x8001, 0xBC00, 0xFC00, 0xFE01, 0xFFFF]]
    # bfloat16, the same list
    b16 = [[0x7FC1, 0x7F80, 0xFF80, 0xFFC1, 0x3F80, 0xBF80, 0x7F81, 0xFFFF, 0x0001, 0x8001]]
    assert _ref(b16, kt=BF16)[0].tolist() == [[0xFFFF, 0xFFC1, 0xFF80, 0xBF80, 0x8001, 0x0001, 0x3F80, 0x7F80, 0x7F81, 0x7FC1]]
    # float16 arrays are taken as they are
    k, p = _ref([[2.0, -1.0, 0.5], [0.0, -0.0, -3.0]], kt=F16, dtype=np.float16)
    assert k.dtype == np.float16 and k.tolist() == [[-1.0, 0.5, 2.0], [-3.0, -0.0, 0.0]] and p.tolist() == [[1, 2, 0], [2, 1, 0]]
    assert np.signbit(k[1, 1]) and not np.signbit(k[1, 2])
    # carried 8-byte values: bit-copied, dtype kept, each with its row
    vals = np.array([[1 << 40, 2, (1 << 63) + 5], [7, 8, 9]], dtype=np.uint64)
    k, v = _ref([[5, 3, 5], [2, 2, 1]], vals, desc=True)
    assert v.dtype == np.uint64 and v.tolist() == [[(1 << 63) + 5, 1 << 40, 2], [8, 7, 9]]
    with pytest.raises(ValueError):
        sort_rows16_reference(np.zeros(4, dtype=np.uint16))                         # 1-D
    with pytest.raises(ValueError):
        sort_rows16_reference(np.zeros((2, 2), dtype=np.uint32), None, U16)         # 4-byte elements
    with pytest.raises(ValueError):
        sort_rows16_reference(np.zeros((2, 2), dtype=np.uint16), None, 0)           # a 32-bit key type
    with pytest.raises(ValueError):
        sort_rows16_reference(np.zeros((2, 2), dtype=np.uint16), np.zeros((2, 3), dtype=np.uint32))


def test_the_32_bit_reference_keeps_refusing_2_byte_elements():
    from gpusorting_amd.rowsort import sort_rows_reference
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros((2, 2), dtype=np.uint16))
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros((2, 2), dtype=np.uint16), None, U16)
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros((2, 2), dtype=np.uint32), None, BF16)


def test_reference_agrees_with_the_references_the_library_has():
    from gpusorting_amd.rowsort import sort_rows_reference
    from gpusorting_amd.rowsort16 import sort_rows16_reference
    from gpusorting_amd.sort16 import sort16_reference
    rng = np.random.default_rng(7)
    for rows, row_len in ((1, 17), (5, 33), (7, 1), (3, 1000)):
        keys = (rng.integers(0, 64, (rows, row_len), dtype=np.uint16) << np.uint16(10)) | rng.integers(0, 2, (rows, row_len), dtype=np.uint16)
        vals = (np.arange(rows * row_len, dtype=np.uint64) * np.uint64(0x100000001)).reshape(rows, row_len)
        for kt in KEY16:
            for desc in (False, True):
                k, p = sort_rows16_reference(keys, None, kt, desc)
                k2, v = sort_rows16_reference(keys, vals, kt, desc)
                np.testing.assert_array_equal(k, k2)
                for r in range(rows):     # row r is what sort16_reference makes of that slice alone
                    sk, sp = sort16_reference(keys[r], None, kt, desc)
                    np.testing.assert_array_equal(k[r], sk)
                    np.testing.assert_array_equal(p[r], sp)
                    np.testing.assert_array_equal(v[r], sort16_reference(keys[r], vals[r], kt, desc)[1])
        # bfloat16 is the top half of a float32: the 32-bit reference on the shifted keys gives the same order
        for desc in (False, True):
            k, p = sort_rows16_reference(keys, None, BF16, desc)
            wk, wp = sort_rows_reference(keys.astype(np.uint32) << np.uint32(16), None, 2, desc)
            np.testing.assert_array_equal(k, (wk >> np.uint32(16)).astype(np.uint16))
            np.testing.assert_array_equal(p, wp)
