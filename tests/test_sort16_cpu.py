"""CPU tests of the 16-bit sort's boundary (gs_sort16_* in include/gpusort.h): the symbols and constants are declared, exported and
bound; the host-only entries (gs_sort16_temp_bytes, gs_sort16_plan) are consistent; the host-side argument checks answer before
anything touches a GPU; and sort16_reference — the numpy statement of the semantics the GPU tests compare with — is checked against
hand-built lists and, on all 65 536 patterns, against the 32-bit sortable_bits.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = 6, 7, 8, 9
KEYS, PAIRS = 0, 1
SYMBOLS = ("gs_sort16_create", "gs_sort16_destroy", "gs_sort16_temp_bytes", "gs_sort16_sort_keys", "gs_sort16_sort_pairs", "gs_sort16_argsort",
           "gs_sort16_check", "gs_sort16_last", "gs_sort16_plan", "gs_sort16_set_rank_mode", "gs_sort16_get_rank_mode")


def _header():
    return open(os.path.join(ROOT, "include", "gpusort.h")).read()


def test_symbols_and_constants_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(gs_sort16_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SORT16_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", text))
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value, 0), name
    assert {"GS_SORT16_REPORT_WORDS", "GS_SORT16_ROUTE_KEYS", "GS_SORT16_ROUTE_PAIRS", "GS_SORT16_R_FORMS", "GS_SORT16_F_SCATTER",
            "GS_SORT16_F_ALL"} <= set(defines)
    # the scatter's six forms lie behind the five plain ones and fill the mask
    assert _lib.GS_SORT16_F_ALL == 31 | sum(_lib.GS_SORT16_F_SCATTER << b for b in range(6))
    import gpusorting_amd as g
    assert g.Sort16 and g.sort16_reference and g.sort16_plan
    # the header's note on the 16-bit key types names the new family
    note = re.search(r"/\* 16-bit keys: 2-byte elements.*?\*/", _header(), flags=re.S).group(0)
    assert "gs_sort16_" in note and "ONLY" not in note


def _plan(lib, n, mode, vb):
    p = (C.c_uint32 * 4)()
    assert lib.gs_sort16_plan(n, mode, vb, p) == 0, (n, mode, vb)
    return [int(x) for x in p]


def test_plan_and_temp_bytes_are_consistent():
    from gpusorting_amd import _lib
    lib = _lib.load()
    for mode, vb in ((KEYS, 0), (PAIRS, 4), (PAIRS, 8)):
        tile, cap = _plan(lib, 1, mode, vb)[2:]
        assert _plan(lib, 1, mode, vb)[:2] == [1, tile]          # n = 1: one range of one tile
        sizes = [1, 2, tile - 1, tile, tile + 1, 2 * tile + 3, (1 << 20) + 5, (cap - 1) * tile, (cap - 1) * tile + 1, cap * tile, cap * tile + 1,
                 (1 << 24) + 7, (1 << 28), _lib.GS_MAX_KEYS]
        for n in sizes:
            ranges, per, t, c = _plan(lib, n, mode, vb)
            assert (t, c) == (tile, cap)
            assert per % tile == 0 and per >= tile
            assert 1 <= ranges <= cap
            assert ranges * per >= n > (ranges - 1) * per, (n, ranges, per)
        assert _plan(lib, (cap - 1) * tile, mode, vb)[0] == cap - 1 and _plan(lib, (cap - 1) * tile + 1, mode, vb)[0] == cap
        assert _plan(lib, cap * tile + 1, mode, vb)[1] == 2 * tile
        b = lib.gs_sort16_temp_bytes(1 << 20, mode, vb)
        assert b == lib.gs_sort16_temp_bytes(_lib.GS_MAX_KEYS, mode, vb) and b % 256 == 0
        # keys only: control block, 65 536 counters, 65 537 prefix words; pairs: control block and two cap x 256 tables
        need = 256 + 65536 * 4 + 65537 * 4 if mode == KEYS else 256 + 2 * cap * 256 * 4
        assert need <= b <= need + 1024
    p = (C.c_uint32 * 4)()
    assert lib.gs_sort16_plan(16, KEYS, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_plan(0, KEYS, 0, p) == _lib.GS_ERR_SIZE
    assert lib.gs_sort16_plan(1 << 30, KEYS, 0, p) == _lib.GS_ERR_SIZE
    assert lib.gs_sort16_plan(16, KEYS, 4, p) == _lib.GS_ERR_MODE
    assert lib.gs_sort16_plan(16, PAIRS, 2, p) == _lib.GS_ERR_MODE
    assert lib.gs_sort16_plan(16, PAIRS, 0, p) == _lib.GS_ERR_MODE
    assert lib.gs_sort16_plan(16, 7, 0, p) == _lib.GS_ERR_MODE
    assert lib.gs_sort16_temp_bytes(0, KEYS, 0) == 0 and lib.gs_sort16_temp_bytes(1 << 30, KEYS, 0) == 0
    assert lib.gs_sort16_temp_bytes(16, KEYS, 4) == 0 and lib.gs_sort16_temp_bytes(16, PAIRS, 2) == 0
    from gpusorting_amd.sort16 import sort16_plan
    assert sort16_plan(1, PAIRS, 4) == {"ranges": 1, "per_range": 4096, "tile": 4096, "cap": 512}
    assert sort16_plan(1)["tile"] == 8192


def test_null_handle_and_null_pointer_returns():
    from gpusorting_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gs_sort16_create(None, 1024, KEYS, 0) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_create(C.byref(h), 0, KEYS, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_sort16_create(C.byref(h), 1 << 30, KEYS, 0) == _lib.GS_ERR_SIZE
    assert lib.gs_sort16_create(C.byref(h), 1024, KEYS, 4) == _lib.GS_ERR_MODE
    assert lib.gs_sort16_create(C.byref(h), 1024, PAIRS, 2) == _lib.GS_ERR_MODE
    assert not h.value
    assert lib.gs_sort16_destroy(None) == _lib.GS_ERR_ARG
    # the null handle is looked at before anything else: pointers that would be refused as well do not change the answer
    assert lib.gs_sort16_sort_keys(None, None, 0, 99, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_sort_keys(None, 16, 4, U16, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_sort_pairs(None, 16, 32, 48, 64, 4, U16, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_argsort(None, None, None, None, None, 4, F16, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_check(None, None) == _lib.GS_ERR_ARG
    r = (C.c_uint32 * 8)()
    assert lib.gs_sort16_last(None, r, 8, None) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_set_rank_mode(None, 0) == _lib.GS_ERR_ARG
    assert lib.gs_sort16_get_rank_mode(None) == -1


def _ref(keys, values=None, kt=U16, desc=False):
    from gpusorting_amd.sort16 import sort16_reference
    return sort16_reference(np.asarray(keys, dtype=np.uint16), values, kt, desc)


def test_reference_on_hand_built_lists():
    # ties: ascending keeps equal keys in rising position, descending is the exact reverse (falling position)
    k, p = _ref([5, 3, 5, 3, 9])
    assert k.tolist() == [3, 3, 5, 5, 9] and p.tolist() == [1, 3, 0, 2, 4] and p.dtype == np.uint32
    k, p = _ref([5, 3, 5, 3, 9], desc=True)
    assert k.tolist() == [9, 5, 5, 3, 3] and p.tolist() == [4, 2, 0, 3, 1]
    # -0 < +0, for both float formats (same sign / magnitude layout on the 16 bits)
    for kt in (F16, BF16):
        k, p = _ref([0x0000, 0x8000, 0x0000, 0x8000], kt=kt)
        assert k.tolist() == [0x8000, 0x8000, 0, 0] and p.tolist() == [1, 3, 0, 2]
    # NaNs by bit pattern: negative NaNs in front of -inf, positive NaNs behind +inf; payloads kept
    f16 = [0x7E01, 0x7C00, 0xFC00, 0xFE01, 0x3C00, 0xBC00, 0x7C01, 0xFFFF]    # +nan +inf -inf -nan 1 -1 +snan -nan(all ones)
    k, _ = _ref(f16, kt=F16)
    assert k.tolist() == [0xFFFF, 0xFE01, 0xFC00, 0xBC00, 0x3C00, 0x7C00, 0x7C01, 0x7E01]
    bf16 = [0x7FC1, 0x7F80, 0xFF80, 0xFFC1, 0x3F80, 0xBF80]                   # +nan +inf -inf -nan 1 -1
    k, _ = _ref(bf16, kt=BF16)
    assert k.tolist() == [0xFFC1, 0xFF80, 0xBF80, 0x3F80, 0x7F80, 0x7FC1]
    # the same bits as int16 and as uint16
    bits = [0x0001, 0xFFFF, 0x8000, 0x7FFF, 0x0000]
    assert _ref(bits, kt=U16)[0].tolist() == [0x0000, 0x0001, 0x7FFF, 0x8000, 0xFFFF]
    assert _ref(bits, kt=I16)[0].tolist() == [0x8000, 0xFFFF, 0x0000, 0x0001, 0x7FFF]
    assert _ref(np.array(bits, dtype=np.uint16).view(np.int16), kt=I16)[0].tolist() == [0x8000, 0xFFFF, 0x0000, 0x0001, 0x7FFF]
    # carried 8-byte values: bit-copied, dtype kept
    vals = np.array([1 << 40, 2, (1 << 63) + 5, 4, 5], dtype=np.uint64)
    k, v = _ref([5, 3, 5, 3, 9], vals, desc=True)
    assert v.dtype == np.uint64 and v.tolist() == [5, (1 << 63) + 5, 1 << 40, 4, 2]
    # float16 arrays are taken as they are (2-byte elements)
    from gpusorting_amd.sort16 import sort16_reference
    k, p = sort16_reference(np.array([2.0, -1.0, 0.5], dtype=np.float16), None, F16, False)
    assert k.dtype == np.float16 and k.tolist() == [-1.0, 0.5, 2.0] and p.tolist() == [1, 2, 0]
    with pytest.raises(ValueError):
        sort16_reference(np.zeros(4, dtype=np.uint32), None, U16)
    with pytest.raises(ValueError):
        sort16_reference(np.zeros(4, dtype=np.uint16), None, 2)


def test_reference_on_all_patterns_against_the_32_bit_sortable_bits():
    """A 16-bit key is the top half of a 32-bit key of the matching type (bfloat16 IS the top half of a float32; float16 shares the
    sign / magnitude layout): sorting all 65 536 patterns by the 16-bit rule and by the 32-bit rule on pattern << 16 is one order."""
    from gpusorting_amd.segsort import sortable_bits
    from gpusorting_amd.sort16 import sort16_reference
    rng = np.random.default_rng(16)
    pats = rng.permutation(65536).astype(np.uint16)
    for kt16, kt32 in ((U16, 0), (I16, 1), (F16, 2), (BF16, 2)):
        wide = sortable_bits(pats.astype(np.uint32) << np.uint32(16), kt32)
        for desc in (False, True):
            k, p = sort16_reference(pats, None, kt16, desc)
            order = np.argsort(wide, kind="stable")
            if desc:
                order = order[::-1]
            np.testing.assert_array_equal(k, pats[order])
            np.testing.assert_array_equal(p, order.astype(np.uint32))
            np.testing.assert_array_equal(np.sort(k), np.arange(65536, dtype=np.uint16))     # every pattern kept exactly once
        # bfloat16 against the float value order where that is defined (no NaNs, -0 < +0 aside)
    finite = pats[(pats & 0x7F80) != 0x7F80]
    k, _ = sort16_reference(finite, None, BF16, False)
    f = (k.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.all(np.diff(f) >= 0)
