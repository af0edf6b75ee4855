"""CPU tests of the row-wise sort's boundary (gs_sort_rows_* in include/gpusort.h): the symbols and constants are declared, exported
and bound; the host-only entries (gs_sort_rows_plan, gs_sort_rows_temp_bytes) are consistent; the host-side argument checks answer
before anything touches a GPU; and sort_rows_reference — the numpy statement of the semantics the GPU tests compare with — is checked
against hand-built rows.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = 0, 1, 2
KEYS, PAIRS = 0, 1
MODES = ((KEYS, 0), (PAIRS, 4), (PAIRS, 8))
SYMBOLS = ("gs_sort_rows_create", "gs_sort_rows_destroy", "gs_sort_rows_temp_bytes", "gs_sort_rows_plan", "gs_sort_rows_keys", "gs_sort_rows_pairs",
           "gs_sort_rows_check", "gs_sort_rows_last", "gs_sort_rows_set_rank_mode", "gs_sort_rows_get_rank_mode")


def _header():
    return open(os.path.join(ROOT, "include", "gpusort.h")).read()


def test_symbols_and_constants_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(gs_sort_rows_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SORT_ROWS_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", text))
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value, 0), name
    assert {"GS_SORT_ROWS_ROUTE_LDS", "GS_SORT_ROWS_ROUTE_PASSES", "GS_SORT_ROWS_TILE", "GS_SORT_ROWS_PCAP", "GS_SORT_ROWS_PASSES",
            "GS_SORT_ROWS_PLAN_WORDS", "GS_SORT_ROWS_REPORT_WORDS", "GS_SORT_ROWS_R_FORMS", "GS_SORT_ROWS_F_SCATTER", "GS_SORT_ROWS_F_ALL"} <= set(defines)
    # the scatter's six forms lie behind the five plain ones and fill the mask
    assert _lib.GS_SORT_ROWS_F_ALL == 31 | sum(_lib.GS_SORT_ROWS_F_SCATTER << b for b in range(6))
    import gpusorting_amd as g
    from gpusorting_amd.rowsort import SORT_ROWS_FORMS
    assert g.RowSort and g.sort_rows_reference and g.sort_rows_plan
    assert len(SORT_ROWS_FORMS) == 11 and sum(SORT_ROWS_FORMS.values()) == _lib.GS_SORT_ROWS_F_ALL


def _plan(lib, rows, row_len, mode, vb):
    from gpusorting_amd import _lib
    p = (C.c_uint32 * _lib.GS_SORT_ROWS_PLAN_WORDS)()
    assert lib.gs_sort_rows_plan(rows, row_len, mode, vb, p) == 0, (rows, row_len, mode, vb)
    return {"route": p[0], "parts": p[1], "per": p[2], "tile": p[3], "passes": p[4], "cap": p[5]}


def test_route_switches_exactly_behind_the_lds_limit():
    from gpusorting_amd import _lib
    lib = _lib.load()
    assert [lib.gs_segsort_max_lds_segment(m, vb) for m, vb in MODES] == [32768, 16384, 8192]
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        for rows in (1, 2, 5, 1000):
            for row_len in (1, 2, 33, lds - 1, lds):
                p = _plan(lib, rows, row_len, mode, vb)
                assert p == {"route": _lib.GS_SORT_ROWS_ROUTE_LDS, "parts": 1, "per": row_len, "tile": 0, "passes": 0, "cap": max(rows, _lib.GS_SORT_ROWS_PCAP)}
            for row_len in (lds + 1, lds + 2, 2 * lds):
                p = _plan(lib, rows, row_len, mode, vb)
                assert (p["route"], p["tile"], p["passes"]) == (_lib.GS_SORT_ROWS_ROUTE_PASSES, _lib.GS_SORT_ROWS_TILE, 4)


def test_plan_covers_the_row_in_whole_tiles_and_stays_under_the_cap():
    from gpusorting_amd import _lib
    lib = _lib.load()
    tile, pcap = _lib.GS_SORT_ROWS_TILE, _lib.GS_SORT_ROWS_PCAP
    shapes = [(1, 32769), (1, 8 * tile + 1), (1, 9 * tile), (1, 9 * tile - 1), (3, 40001), (1, 1 << 22), (4, 1 << 22), (32, 262144), (256, 131072),
              (1024, 32769), (1023, 40000), (1025, 40000), (pcap // 2, 10 * tile + 1), (pcap // 3, 11 * tile), (20000, 32769), (1, _lib.GS_MAX_KEYS),
              (2, _lib.GS_MAX_KEYS // 2), (7, 100003)]
    for mode, vb in MODES:
        for rows, row_len in shapes:
            p = _plan(lib, rows, row_len, mode, vb)
            assert p["route"] == _lib.GS_SORT_ROWS_ROUTE_PASSES and p["tile"] == tile
            tiles = -(-row_len // tile)
            assert p["per"] % tile == 0 and p["per"] >= tile
            assert 1 <= p["parts"] <= max(1, tiles // _lib.GS_SORT_ROWS_MIN_TILES)
            assert p["parts"] * p["per"] >= row_len > (p["parts"] - 1) * p["per"], (rows, row_len, p)   # every part holds at least one element
            assert p["cap"] == max(rows, pcap) and rows * p["parts"] <= p["cap"], (rows, row_len, p)
            if rows >= pcap:
                assert p["parts"] == 1
            # the chip is filled where the rows are long enough for it: at least half the aim unless the tiles run out
            if rows < pcap and tiles >= _lib.GS_SORT_ROWS_MIN_TILES * (pcap // rows):
                assert rows * p["parts"] > pcap // 2, (rows, row_len, p)
        # the issue's examples
        assert _plan(lib, 256, 131072, mode, vb)["parts"] == 4 and _plan(lib, 32, 262144, mode, vb)["parts"] == 32
        assert _plan(lib, 4, 1 << 22, mode, vb)["parts"] == 256 and _plan(lib, 1, 40000, mode, vb)["parts"] == 5
        # an uneven last part: 10 tiles and a bit over 4 parts of 3 tiles
        p = _plan(lib, 256, 10 * tile + 5, mode, vb)
        assert (p["parts"], p["per"]) == (4, 3 * tile)
    from gpusorting_amd.rowsort import sort_rows_plan
    assert sort_rows_plan(3, 40001, PAIRS, 4) == {"route": 2, "parts": 5, "per_part": 2 * tile, "tile": tile, "passes": 4, "cap": pcap}
    # a row of fewer than twice the least tiles of a part is one part
    assert sort_rows_plan(1, 8193, PAIRS, 8)["parts"] == 1 and sort_rows_plan(1, 4 * tile, PAIRS, 8)["parts"] == 2
    assert sort_rows_plan(3, 100)["route"] == 1


def test_temp_bytes_hold_every_plan_at_max_keys():
    """The formula of the header, restated; and for every (rows, row_len) that fits max_keys the plan's rows x parts tables fit."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    tile, pcap = _lib.GS_SORT_ROWS_TILE, _lib.GS_SORT_ROWS_PCAP
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        for max_keys in (1, 1000, lds, lds + 1, 1 << 16, (1 << 20) + 3, 1 << 24, 1 << 28, _lib.GS_MAX_KEYS):
            r = max_keys // (lds + 1)
            units = 0 if r == 0 else min(max(r, pcap), max_keys // tile + r)
            want = 256 + up(4 * (64 + max_keys // 33 + 1)) + up(4 * (max_keys + 1)) + 2 * up(units * 1024)
            assert lib.gs_sort_rows_temp_bytes(max_keys, mode, vb) == want, (max_keys, mode, vb)
            if r == 0:
                continue
            tried = {1, 2, 3, r, max(1, r - 1), max(1, r // 2), min(r, pcap), min(r, pcap + 1), min(r, pcap // 2)}
            for rows in sorted(x for x in tried if x <= r):
                for row_len in {lds + 1, max_keys // rows, min(max_keys // rows, lds + tile + 1)}:
                    assert row_len > lds and rows * row_len <= max_keys
                    p = _plan(lib, rows, row_len, mode, vb)
                    assert rows * p["parts"] <= units, (max_keys, rows, row_len, p, units)
    assert lib.gs_sort_rows_temp_bytes(0, KEYS, 0) == 0 and lib.gs_sort_rows_temp_bytes(1 << 30, KEYS, 0) == 0
    assert lib.gs_sort_rows_temp_bytes(16, KEYS, 4) == 0 and lib.gs_sort_rows_temp_bytes(16, PAIRS, 2) == 0 and lib.gs_sort_rows_temp_bytes(16, 7, 0) == 0


def test_plan_argument_errors():
    from gpusorting_amd import _lib
    lib = _lib.load()
    p = (C.c_uint32 * 8)()
    assert lib.gs_sort_rows_plan(4, 16, KEYS, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_plan(0, 16, KEYS, 0, p) == _lib.GS_ERR_SIZE
    assert lib.gs_sort_rows_plan(4, 0, KEYS, 0, p) == _lib.GS_ERR_SIZE
    assert lib.gs_sort_rows_plan(1 << 15, 1 << 15, KEYS, 0, p) == _lib.GS_ERR_SIZE          # 2^30 elements
    assert lib.gs_sort_rows_plan(1 << 31, 1 << 31, KEYS, 0, p) == _lib.GS_ERR_SIZE          # the product does not wrap into range
    assert lib.gs_sort_rows_plan(1 << 16, 1 << 16, KEYS, 0, p) == _lib.GS_ERR_SIZE          # 2^32: wraps to 0 in 32 bits
    assert lib.gs_sort_rows_plan(1, _lib.GS_MAX_KEYS, KEYS, 0, p) == _lib.GS_OK
    for mode, vb in ((KEYS, 4), (PAIRS, 2), (PAIRS, 0), (7, 0)):
        assert lib.gs_sort_rows_plan(4, 16, mode, vb, p) == _lib.GS_ERR_MODE


def test_null_handle_and_null_pointer_returns():
    from gpusorting_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gs_sort_rows_create(None, 1024, KEYS, 0) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_create(C.byref(h), 0, KEYS, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_sort_rows_create(C.byref(h), 1 << 30, KEYS, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_sort_rows_create(C.byref(h), 1024, KEYS, 4) == _lib.GS_ERR_MODE
    assert lib.gs_sort_rows_create(C.byref(h), 1024, PAIRS, 2) == _lib.GS_ERR_MODE
    assert not h.value
    assert lib.gs_sort_rows_destroy(None) == _lib.GS_ERR_ARG
    # the null handle is looked at before anything else: arguments that would be refused as well do not change the answer
    assert lib.gs_sort_rows_keys(None, None, None, 0, 0, 99, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_keys(None, 16, 32, 4, 4, U32, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_pairs(None, 16, 32, 48, 64, 4, 4, F32, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_check(None, None) == _lib.GS_ERR_ARG
    r = (C.c_uint32 * 8)()
    assert lib.gs_sort_rows_last(None, r, 8, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_set_rank_mode(None, 0) == _lib.GS_ERR_ARG
    assert lib.gs_sort_rows_get_rank_mode(None) == -1


def _ref(keys, values=None, kt=U32, desc=False, dtype=np.uint32):
    from gpusorting_amd.rowsort import sort_rows_reference
    return sort_rows_reference(np.asarray(keys, dtype=dtype), values, kt, desc)


def test_reference_on_hand_built_rows():
    # ties: ascending keeps equal keys in rising position, descending is the exact reverse of the row (falling position); rows do not mix
    k, p = _ref([[5, 3, 5, 3, 9], [1, 1, 0, 1, 0]])
    assert k.tolist() == [[3, 3, 5, 5, 9], [0, 0, 1, 1, 1]] and p.tolist() == [[1, 3, 0, 2, 4], [2, 4, 0, 1, 3]] and p.dtype == np.uint32
    k, p = _ref([[5, 3, 5, 3, 9], [1, 1, 0, 1, 0]], desc=True)
    assert k.tolist() == [[9, 5, 5, 3, 3], [1, 1, 1, 0, 0]] and p.tolist() == [[4, 2, 0, 3, 1], [3, 1, 0, 4, 2]]
    # rows = 1 and row_len = 1
    k, p = _ref([[7, 2, 7]])
    assert k.tolist() == [[2, 7, 7]] and p.tolist() == [[1, 0, 2]]
    k, p = _ref([[7], [2], [9]], desc=True)
    assert k.tolist() == [[7], [2], [9]] and p.tolist() == [[0], [0], [0]]
    # the same bits as uint32 and as int32
    bits = [[0x00000001, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0]]
    assert _ref(bits, kt=U32)[0].tolist() == [[0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]]
    assert _ref(bits, kt=I32)[0].tolist() == [[0x80000000, 0xFFFFFFFF, 0, 1, 0x7FFFFFFF]]
    assert _ref(np.array(bits, dtype=np.uint32).view(np.int32), kt=I32, dtype=np.int32)[0].tolist() == [[-(1 << 31), -1, 0, 1, (1 << 31) - 1]]
    # floats: -0 < +0; negative NaNs in front of -inf, positive NaNs behind +inf, by bit pattern; payloads and subnormals kept
    f = [[0x00000000, 0x80000000, 0x00000000, 0x80000000]]
    k, p = _ref(f, kt=F32)
    assert k.tolist() == [[0x80000000, 0x80000000, 0, 0]] and p.tolist() == [[1, 3, 0, 2]]
    pats = [[0x7FC00001, 0x7F800000, 0xFF800000, 0xFFC00001, 0x3F800000, 0xBF800000, 0x7F800001, 0xFFFFFFFF, 0x00000001, 0x80000001]]
    #        +nan        +inf        -inf        -nan        1           -1          +snan       -nan(ones)  +subnormal  -subnormal
    k, _ = _ref(pats, kt=F32)
    assert k.tolist() == [[0xFFFFFFFF, 0xFFC00001, 0xFF800000, 0xBF800000, 0x80000001, 0x00000001, 0x3F800000, 0x7F800000, 0x7F800001, 0x7FC00001]]
    k, _ = _ref(pats, kt=F32, desc=True)
    assert k.tolist() == [[0x7FC00001, 0x7F800001, 0x7F800000, 0x3F800000, 0x00000001, 0x80000001, 0xBF800000, 0xFF800000, 0xFFC00001, 0xFFFFFFFF]]
    # float32 arrays are taken as they are
    k, p = _ref([[2.0, -1.0, 0.5], [0.0, -0.0, -3.0]], kt=F32, dtype=np.float32)
    assert k.dtype == np.float32 and k.tolist() == [[-1.0, 0.5, 2.0], [-3.0, -0.0, 0.0]] and p.tolist() == [[1, 2, 0], [2, 1, 0]]
    assert np.signbit(k[1, 1]) and not np.signbit(k[1, 2])
    # carried 8-byte values: bit-copied, dtype kept, each with its row
    vals = np.array([[1 << 40, 2, (1 << 63) + 5], [7, 8, 9]], dtype=np.uint64)
    k, v = _ref([[5, 3, 5], [2, 2, 1]], vals, desc=True)
    assert v.dtype == np.uint64 and v.tolist() == [[(1 << 63) + 5, 1 << 40, 2], [8, 7, 9]]
    from gpusorting_amd.rowsort import sort_rows_reference
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros(4, dtype=np.uint32))                       # 1-D
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros((2, 2), dtype=np.uint16))                  # 2-byte elements
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros((2, 2), dtype=np.uint32), None, 6)         # a 16-bit key type
    with pytest.raises(ValueError):
        sort_rows_reference(np.zeros((2, 2), dtype=np.uint32), np.zeros((2, 3), dtype=np.uint32))


def test_reference_agrees_with_the_segmented_reference_on_uniform_offsets():
    from gpusorting_amd.rowsort import sort_rows_reference
    from gpusorting_amd.segsort import segmented_sort_reference
    rng = np.random.default_rng(3)
    for rows, row_len in ((1, 17), (5, 33), (7, 1), (3, 1000)):
        keys = rng.integers(0, 16, (rows, row_len), dtype=np.uint32) << np.uint32(28)   # heavy ties, both float signs
        vals = np.arange(rows * row_len, dtype=np.uint32).reshape(rows, row_len)
        off = np.arange(rows + 1) * row_len
        for kt in (U32, I32, F32):
            for desc in (False, True):
                k, v = sort_rows_reference(keys, vals, kt, desc)
                sk, sv = segmented_sort_reference(keys.reshape(-1), off, vals.reshape(-1), kt, desc)
                np.testing.assert_array_equal(k.reshape(-1), sk)
                np.testing.assert_array_equal(v.reshape(-1), sv)
