"""CPU tests of the segmented top-k (gs_segtopk_* in include/gpusort.h, gpusorting_amd/segtopk.py): the symbols and constants are
declared, exported and bound; gs_segtopk_temp_bytes is the formula the header states; the null handle is answered before anything
touches a GPU; and segmented_topk_reference — the numpy statement of the semantics the GPU tests compare with — is checked against
an independent statement (per segment: stable argsort on the sortable bits, reversed for descending, head m_s).  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = 0, 1, 2
KEYS, PAIRS = 0, 1
SYMBOLS = ("gs_segtopk_create", "gs_segtopk_destroy", "gs_segtopk_temp_bytes", "gs_segtopk_select_keys", "gs_segtopk_select_pairs",
           "gs_segtopk_check", "gs_segtopk_last", "gs_segtopk_set_rank_mode", "gs_segtopk_get_rank_mode")


def test_symbols_and_constants_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_segtopk_[a-z0-9_]+)\s*\(", text))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SEGTOPK_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\s*$", text, flags=re.M))
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value, 0), name
    assert {"GS_SEGTOPK_REPORT_WORDS", "GS_SEGTOPK_F_PACKED", "GS_SEGTOPK_F_WAVE", "GS_SEGTOPK_F_STREAM", "GS_SEGTOPK_F_VM"} | {
        f"GS_SEGTOPK_R_{w}" for w in ("CLASSES", "LONGEST", "STATUS", "READS", "FORMS", "RANK", "K", "PACKED")} == set(defines)
    # the report holds a word per class in front of the scalars
    assert _lib.GS_SEGTOPK_R_CLASSES + _lib.GS_SEGSORT_CLASSES == _lib.GS_SEGTOPK_R_LONGEST and _lib.GS_SEGTOPK_R_PACKED < _lib.GS_SEGTOPK_REPORT_WORDS
    # the forms word: one bit per kernel form, none shared (the macro in the header is the function in _lib)
    m = re.search(r"#define\s+GS_SEGTOPK_F_TILE\(cls, rank\)\s+\((\d+)u << \(\(\(cls\) - 3u\) \+ (\d+)u \* \(rank\)\)\)", text)
    assert m and all(_lib.GS_SEGTOPK_F_TILE(c, r) == int(m.group(1)) << ((c - 3) + int(m.group(2)) * r) for c in range(3, 8) for r in (0, 1))
    bits = [_lib.GS_SEGTOPK_F_PACKED, _lib.GS_SEGTOPK_F_WAVE, _lib.GS_SEGTOPK_F_STREAM] + [_lib.GS_SEGTOPK_F_TILE(c, r) for r in (0, 1) for c in range(3, 8)] + [
        _lib.GS_SEGTOPK_F_VM << v for v in range(4)]
    assert len(set(bits)) == 17 and all(b & (b - 1) == 0 and b < 1 << 32 for b in bits)
    import gpusorting_amd as g
    from gpusorting_amd import functional
    assert g.SegmentedTopK and g.segmented_topk_reference and g.segmented_topk is functional.segmented_topk


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    lib = _lib.load()
    for segs in (1, 2, 63, 64, 65, 191, 192, 193, 1000, 4096, 65536, (1 << 20) + 7, 1 << 27, _lib.GS_MAX_KEYS):
        assert lib.gs_segtopk_temp_bytes(segs) == ((64 + segs) * 4 + 255) & ~255, segs


def test_the_null_handle_is_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_segtopk_create(None, 1024, 16, 8, KEYS, 0) == A
    assert lib.gs_segtopk_create(C.byref(h), 0, 16, 8, KEYS, 0) == S and lib.gs_segtopk_create(C.byref(h), 1 << 30, 16, 8, KEYS, 0) == S
    assert lib.gs_segtopk_create(C.byref(h), 1024, 0, 8, KEYS, 0) == S and lib.gs_segtopk_create(C.byref(h), 1024, 1 << 30, 8, KEYS, 0) == S
    assert lib.gs_segtopk_create(C.byref(h), 1024, 16, 0, KEYS, 0) == S and lib.gs_segtopk_create(C.byref(h), 1024, 16, 1 << 30, KEYS, 0) == S
    assert lib.gs_segtopk_create(C.byref(h), 1024, 16, 8, KEYS, 4) == M and lib.gs_segtopk_create(C.byref(h), 1024, 16, 8, PAIRS, 2) == M
    assert not h.value
    assert lib.gs_segtopk_destroy(None) == A
    p = (C.c_uint32 * 16)()
    assert lib.gs_segtopk_select_keys(None, None, 0, None, 0, 0, 0, None, 99, 0, None) == A
    assert lib.gs_segtopk_select_keys(None, 16, 4, 64, 1, 2, 0, 32, U32, 0, None) == A
    assert lib.gs_segtopk_select_pairs(None, 16, 32, 4, 64, 1, 2, 0, 48, 80, F32, 1, None) == A
    assert lib.gs_segtopk_select_pairs(None, 16, None, 4, 64, 1, 2, 0, 48, 80, I32, 0, None) == A
    assert lib.gs_segtopk_check(None, None) == A
    assert lib.gs_segtopk_last(None, p, 16, None) == A
    assert lib.gs_segtopk_set_rank_mode(None, 0) == A
    assert lib.gs_segtopk_get_rank_mode(None) == -1


def _bits(keys, kt):
    u = keys.view(np.uint32)
    if kt == I32:
        return u ^ np.uint32(0x80000000)
    if kt == F32:
        return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return u


def _independent(keys, offsets, k, values, descending, kt, fill_key, fill_value):
    """Per segment: stable argsort on the sortable bits, reversed for descending, head m_s."""
    segs = len(offsets) - 1
    out_k = np.full((segs, k), fill_key, dtype=keys.dtype)
    out_v = np.full((segs, k), fill_value, dtype=np.uint32 if values is None else values.dtype)
    counts = np.zeros(segs, dtype=np.int64)
    bits = _bits(keys, kt)
    for s in range(segs):
        a, b = int(offsets[s]), int(offsets[s + 1])
        order = sorted(range(a, b), key=lambda i: (int(bits[i]), i))
        if descending:
            order = order[::-1]
        order = order[:k]
        counts[s] = len(order)
        for o, i in enumerate(order):
            out_k[s, o] = keys[i]
            out_v[s, o] = i if values is None else values[i]
    return out_k, out_v, counts


def _ragged(rng, n_lo=0):
    """Seeded ragged offsets with empty and one-element segments, off[0] > 0 and off[S] < n."""
    lens = np.concatenate([rng.integers(0, 40, 30), [0, 0, 1, 1, 1, 2, 33, 64, 0, 300, 1]])
    rng.shuffle(lens)
    off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
    return off, int(off[-1]) + 5 + n_lo


def _keys(rng, n, kt, ties):
    if kt == F32:
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.5, -1.5, 1e-45, -1e-45], dtype=np.float32)
        k = rng.standard_normal(n).astype(np.float32)
        sel = rng.random(n) < (0.7 if ties else 0.3)
        k[sel] = pool[rng.integers(0, pool.size, int(sel.sum()))]
        nan2 = np.array([0x7FC00001, 0xFFC00002], dtype=np.uint32).view(np.float32)  # NaNs with other payloads
        k[rng.integers(0, n, 4)] = nan2[rng.integers(0, 2, 4)]
        return k
    if kt == I32:
        return (rng.integers(-4, 4, n) if ties else rng.integers(-(1 << 31), 1 << 31, n)).astype(np.int32)
    return (rng.integers(0, 5, n) if ties else rng.integers(0, 1 << 32, n)).astype(np.uint32)


@pytest.mark.parametrize("kt", (U32, I32, F32))
@pytest.mark.parametrize("ties", (False, True))
def test_reference_equals_the_independent_statement(kt, ties):
    from gpusorting_amd.segtopk import segmented_topk_reference
    rng = np.random.default_rng(100 + 10 * kt + ties)
    off, n = _ragged(rng)
    keys = _keys(rng, n, kt, ties)
    fill_k = np.array([0xDEADBEEF], dtype=np.uint32).view(keys.dtype)[0]
    for k in (1, 2, 33, 400):
        for desc in (False, True):
            for values in (None, rng.integers(0, 1 << 32, n).astype(np.uint32), rng.integers(0, 1 << 63, n).astype(np.uint64)):
                got = segmented_topk_reference(keys, off, k, values, desc, kt, fill_key=fill_k, fill_value=0xABCD)
                want = _independent(keys, off, k, values, desc, kt, fill_k, 0xABCD)
                # bit for bit: NaN payloads and the sign of zero count
                assert got[0].dtype == keys.dtype and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (k, desc)
                assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), (k, desc)
                assert np.array_equal(got[2], want[2])


def test_reference_positions_fill_and_counts():
    from gpusorting_amd.segtopk import segmented_topk_reference
    keys = np.array([9, 5, 3, 3, 9, 1, 7, 7, 2, 8], dtype=np.uint32)
    off = np.array([1, 1, 4, 5, 9])  # an empty segment, lengths 3, 1, 4; elements 0 and 9 belong to none
    k_out, v_out, counts = segmented_topk_reference(keys, off, 3, fill_key=111, fill_value=222)
    assert counts.tolist() == [0, 3, 1, 3] and np.array_equal(counts, np.minimum(np.diff(off), 3))
    # positions are those of the whole array: off[s] + the position in the segment; ties by rising position
    assert k_out.tolist() == [[111, 111, 111], [3, 3, 5], [9, 111, 111], [1, 2, 7]]
    assert v_out.tolist() == [[222, 222, 222], [2, 3, 1], [4, 222, 222], [5, 8, 6]] and v_out.dtype == np.uint32
    # descending: the exact reverse of the stable ascending order
    k_out, v_out, _ = segmented_topk_reference(keys, off, 2, descending=True, fill_key=111, fill_value=222)
    assert k_out.tolist() == [[111, 111], [5, 3], [9, 111], [7, 7]] and v_out.tolist() == [[222, 222], [1, 3], [4, 222], [7, 6]]
    # values are carried, and their dtype kept
    vals = (np.arange(10, dtype=np.uint64) + 1) << np.uint64(40)
    _, v_out, _ = segmented_topk_reference(keys, off, 2, vals)
    assert v_out.dtype == np.uint64 and v_out.tolist() == [[0, 0], [3 << 40, 4 << 40], [5 << 40, 0], [6 << 40, 9 << 40]]
    for bad in ([0, 5, 4], [0, 11], [3]):
        with pytest.raises(ValueError):
            segmented_topk_reference(keys, np.array(bad), 2)
    with pytest.raises(ValueError):
        segmented_topk_reference(keys, off, 0)
