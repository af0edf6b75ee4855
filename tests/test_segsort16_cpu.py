"""CPU tests of the segmented sort of 16-bit keys (gs_segsort16_* in include/gpusort.h, gpusorting_amd/segsort16.py): the symbols and
constants are declared, exported and bound; the host-only entries (gs_segsort16_units, gs_segsort16_temp_bytes) state the bound the
header gives and that bound holds every exact unit count; the host-side argument checks answer before anything touches a GPU; and
segmented_sort16_reference — the numpy statement of the semantics the GPU tests compare with — is checked against an independent loop
over the segments.  No compute is run."""
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
SYMBOLS = ("gs_segsort16_create", "gs_segsort16_destroy", "gs_segsort16_units", "gs_segsort16_temp_bytes", "gs_segsort16_sort_keys",
           "gs_segsort16_sort_pairs", "gs_segsort16_argsort", "gs_segsort16_check", "gs_segsort16_last_classes", "gs_segsort16_last",
           "gs_segsort16_set_rank_mode", "gs_segsort16_get_rank_mode")


def test_symbols_and_constants_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_segsort16_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SEGSORT16_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\s*$", text, flags=re.M))
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value, 0), name
    assert {"GS_SEGSORT16_PASSES", "GS_SEGSORT16_REPORT_WORDS", "GS_SEGSORT16_F_ALL", "GS_SEGSORT16_WG_ALL", "GS_SEGSORT16_F_CLASSIFY",
            "GS_SEGSORT16_F_FILL", "GS_SEGSORT16_F_PACKED", "GS_SEGSORT16_F_WAVE", "GS_SEGSORT16_F_UNITS", "GS_SEGSORT16_F_COUNT",
            "GS_SEGSORT16_F_SCAN", "GS_SEGSORT16_F_SCATTER"} | {f"GS_SEGSORT16_R_{w}" for w in
                                                               ("UNITS", "FORMS", "WG_FORMS", "STATUS", "RANK", "LONG", "UNIT_CAP", "N")} == set(defines)
    # the part is whole tiles of the row-wise sort's pass route
    m = re.search(r"#define\s+GS_SEGSORT16_PART\s+\((\d+)u \* GS_SORT_ROWS_TILE\)", text)
    assert m and _lib.GS_SEGSORT16_PART == int(m.group(1)) * _lib.GS_SORT_ROWS_TILE and int(m.group(1)) in (4, 8, 16)
    # the forms: 21 bits of the first word, and one bit per workgroup-class kernel in the second
    from gpusorting_amd.segsort16 import SEGSORT16_FORMS
    bits = list(SEGSORT16_FORMS.values())
    assert len(bits) == 53 and len(set(bits)) == 53 and all(b & (b - 1) == 0 for b in bits)
    assert sum(bits) == _lib.GS_SEGSORT16_F_ALL | (_lib.GS_SEGSORT16_WG_ALL << 32)
    wg = {_lib.GS_SEGSORT16_WG_FORM(c, v, r) for r in (0, 1) for c in (3, 4, 5, 6, 7) for v in range(4) if c <= 5 or (c == 6 and v != 3) or v == 0}
    assert len(wg) == 32 and sum(wg) == _lib.GS_SEGSORT16_WG_ALL
    import gpusorting_amd as g
    assert g.SegmentedSort16 and g.segmented_sort16_reference and g.segsort16_units and g.SEGSORT16_FORMS is SEGSORT16_FORMS


def test_argument_errors_that_need_no_device():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_segsort16_create(None, 1024, 16, KEYS, 0) == A
    assert lib.gs_segsort16_create(C.byref(h), 0, 16, KEYS, 0) == S and lib.gs_segsort16_create(C.byref(h), 1 << 30, 16, KEYS, 0) == S
    assert lib.gs_segsort16_create(C.byref(h), 1024, 0, KEYS, 0) == S and lib.gs_segsort16_create(C.byref(h), 1024, 1 << 30, KEYS, 0) == S
    assert lib.gs_segsort16_create(C.byref(h), 1024, 16, KEYS, 4) == M and lib.gs_segsort16_create(C.byref(h), 1024, 16, PAIRS, 2) == M
    assert not h.value
    assert lib.gs_segsort16_destroy(None) == A
    # the null handle is looked at before anything else, in every handle entry
    p = (C.c_uint32 * 16)()
    assert lib.gs_segsort16_sort_keys(None, None, None, 0, None, 0, 0, 99, 0, None) == A
    assert lib.gs_segsort16_sort_keys(None, 16, 32, 4, 64, 1, 0, U16, 0, None) == A
    assert lib.gs_segsort16_sort_pairs(None, 16, 32, 48, 64, 4, 80, 1, 0, BF16, 0, None) == A
    assert lib.gs_segsort16_argsort(None, 16, 32, 48, 64, 4, 80, 1, 0, F16, 0, None) == A
    assert lib.gs_segsort16_check(None, None) == A
    assert lib.gs_segsort16_last_classes(None, p, 10, None) == A
    assert lib.gs_segsort16_last(None, p, 8, None) == A
    assert lib.gs_segsort16_set_rank_mode(None, 0) == A
    assert lib.gs_segsort16_get_rank_mode(None) == -1
    # temp_bytes and units: 0 for what create refuses
    for f in (lib.gs_segsort16_temp_bytes, lib.gs_segsort16_units):
        assert f(0, 16, KEYS, 0) == 0 and f(1 << 30, 16, KEYS, 0) == 0 and f(1024, 0, KEYS, 0) == 0 and f(1024, 1 << 30, KEYS, 0) == 0
        assert f(1024, 16, KEYS, 4) == 0 and f(1024, 16, PAIRS, 2) == 0 and f(1024, 16, PAIRS, 0) == 0 and f(1024, 16, 7, 0) == 0
    assert lib.gs_segsort16_temp_bytes(1024, 16, KEYS, 0) > 0 and lib.gs_segsort16_units(1024, 16, KEYS, 0) == 0   # nothing can be long


def test_units_is_the_bound_of_the_header_and_temp_bytes_is_sized_by_it():
    from gpusorting_amd import _lib
    from gpusorting_amd.segsort16 import segsort16_units
    lib = _lib.load()
    part = _lib.GS_SEGSORT16_PART
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for mode, vb in MODES:
        lds = lib.gs_segsort_max_lds_segment(mode, vb)
        for n in (1, 1000, lds, lds + 1, part - 1, part, part + 1, 3 * part + 5, (1 << 20) + 3, 1 << 27, _lib.GS_MAX_KEYS):
            for segs in (1, 2, 3, 100, 4096, 1 << 20, _lib.GS_MAX_KEYS):
                longs = min(segs, n // (lds + 1))
                want = n // part + longs
                assert lib.gs_segsort16_units(n, segs, mode, vb) == want == segsort16_units(n, segs, mode, vb), (n, segs, mode, vb)
                assert lib.gs_segsort16_temp_bytes(n, segs, mode, vb) == up(4 * (64 + segs)) + up(16 * want) + up(16 * longs) + 2 * up(1024 * want)


def test_units_is_never_below_the_exact_unit_count():
    """A segment of length L > the LDS limit is cut into ceil(L / PART) parts; the sum over any set of lengths that fits n stays within
    the bound."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    part = _lib.GS_SEGSORT16_PART
    rng = np.random.default_rng(16)
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
            bound = lib.gs_segsort16_units(n, segs, mode, vb)
            assert exact <= bound, (lens.tolist(), n, exact, bound)
            worst = max(worst, exact / max(bound, 1))
        assert worst > 0.9   # the sweep comes close to the bound: it is not vacuous


def _loop_reference(keys, offsets, values, kt, desc):
    """An independent statement: a Python loop over the segments, stable numpy argsort on the sortable bits, reversed for descending."""
    from gpusorting_amd.segsort import sortable_bits
    out_k, out_v = keys.copy(), None if values is None else values.copy()
    perm = np.arange(keys.size, dtype=np.uint32)
    for a, b in zip(offsets[:-1], offsets[1:]):
        a, b = int(a), int(b)
        p = np.argsort(sortable_bits(keys[a:b], kt), kind="stable")
        if desc:
            p = p[::-1]
        out_k[a:b] = keys[a:b][p]
        perm[a:b] = a + p
        if values is not None:
            out_v[a:b] = values[a:b][p]
    return out_k, out_v, perm


_SPECIALS = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFFFF, 0x7FFF, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0],
                     dtype=np.uint16)


def test_reference_against_a_loop_over_the_segments():
    from gpusorting_amd.segsort import segmented_sort_reference
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    rng = np.random.default_rng(5)
    for trial in range(12):
        lens = rng.choice([0, 0, 1, 1, 2, 3, 17, 33, 64, 300, 1025], size=int(rng.integers(1, 30)))
        front, back = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        offsets = (front + np.concatenate(([0], np.cumsum(lens)))).astype(np.uint32)
        n = int(offsets[-1]) + back
        if n == 0:
            continue
        keys = (rng.integers(0, 16, n, dtype=np.uint16) << np.uint16(12)) | rng.integers(0, 3, n, dtype=np.uint16)   # heavy duplicates
        hit = rng.random(n) < 0.3
        keys[hit] = _SPECIALS[rng.integers(0, _SPECIALS.size, int(hit.sum()))]
        vals = np.arange(n, dtype=np.uint64) * np.uint64(0x100000001) + np.uint64(1 << 63)
        for kt in KEY16:
            for desc in (False, True):
                want_k, want_v, want_p = _loop_reference(keys, offsets, vals, kt, desc)
                got_k, got_p = segmented_sort16_reference(keys, offsets, None, kt, desc)
                np.testing.assert_array_equal(got_k, want_k)
                np.testing.assert_array_equal(got_p, want_p)
                assert got_p.dtype == np.uint32 and got_k.dtype == np.uint16
                k2, v2 = segmented_sort16_reference(keys, offsets, vals, kt, desc)
                np.testing.assert_array_equal(k2, want_k)
                np.testing.assert_array_equal(v2, want_v)
                assert v2.dtype == np.uint64
                np.testing.assert_array_equal(segmented_sort_reference(keys, offsets, None, kt, desc), want_k)   # the function it wraps
                # elements outside the segments: untouched keys and values, identity positions
                for sl in (slice(0, front), slice(int(offsets[-1]), n)):
                    np.testing.assert_array_equal(got_k[sl], keys[sl])
                    np.testing.assert_array_equal(v2[sl], vals[sl])
                    np.testing.assert_array_equal(got_p[sl], np.arange(n, dtype=np.uint32)[sl])
                # the argsort result gathers the keys into the sorted keys, and stays inside its segment
                np.testing.assert_array_equal(keys[got_p], got_k)
                seg = np.repeat(np.arange(lens.size), lens)
                np.testing.assert_array_equal(np.repeat(np.arange(lens.size), lens)[got_p[front:int(offsets[-1])].astype(np.int64) - front], seg)


def test_reference_on_hand_built_segments_and_its_refusals():
    from gpusorting_amd.segsort16 import segmented_sort16_reference
    keys = np.array([9, 5, 3, 5, 3, 7, 1, 1, 0, 8], dtype=np.uint16)
    off = np.array([1, 5, 5, 6, 9], dtype=np.uint32)        # [5 3 5 3] [] [7] [1 1 0]; 9 in front and 8 behind stay
    k, p = segmented_sort16_reference(keys, off)
    assert k.tolist() == [9, 3, 3, 5, 5, 7, 0, 1, 1, 8] and p.tolist() == [0, 2, 4, 1, 3, 5, 8, 6, 7, 9]
    k, p = segmented_sort16_reference(keys, off, descending=True)
    assert k.tolist() == [9, 5, 5, 3, 3, 7, 1, 1, 0, 8] and p.tolist() == [0, 3, 1, 4, 2, 5, 7, 6, 8, 9]
    # float16: -0 < +0; the same bits as int16
    z = np.array([0x0000, 0x8000, 0x0000, 0x8000], dtype=np.uint16)
    assert segmented_sort16_reference(z, [0, 4], None, F16)[0].tolist() == [0x8000, 0x8000, 0, 0]
    assert segmented_sort16_reference(z, [0, 4], None, BF16)[1].tolist() == [1, 3, 0, 2]
    assert segmented_sort16_reference(z.view(np.int16), [0, 4], None, I16)[0].tolist() == [-32768, -32768, 0, 0]
    with pytest.raises(ValueError):
        segmented_sort16_reference(np.zeros((2, 2), dtype=np.uint16), [0, 2])                      # 2-D
    with pytest.raises(ValueError):
        segmented_sort16_reference(np.zeros(4, dtype=np.uint32), [0, 2])                           # 4-byte elements
    with pytest.raises(ValueError):
        segmented_sort16_reference(np.zeros(4, dtype=np.uint16), [0, 2], None, 0)                  # a 32-bit key type
    with pytest.raises(ValueError):
        segmented_sort16_reference(np.zeros(4, dtype=np.uint16), [0, 2], np.zeros(5, dtype=np.uint32))
    with pytest.raises(ValueError):
        segmented_sort16_reference(np.zeros(4, dtype=np.uint16), [2, 1])                           # decreasing
    with pytest.raises(ValueError):
        segmented_sort16_reference(np.zeros(4, dtype=np.uint16), [0, 5])                           # beyond the keys
