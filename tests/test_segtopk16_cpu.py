"""CPU tests of the segmented top-k on 16-bit keys (gs_segtopk16_* in include/gpusort.h, gpusorting_amd/segtopk16.py): the symbols
are declared, exported and bound; gs_segtopk16_temp_bytes is the formula the header states; the null handle and the create arguments
are answered before anything touches a GPU; segmented_topk_reference on the four 16-bit key types — what the GPU tests compare with —
is checked against an independent statement (per segment: stable argsort on the sortable 16 bits, reversed for descending, head
m_s); and the argument errors of functional.segmented_topk16 that need no device.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = 6, 7, 8, 9
KEYS, PAIRS = 0, 1
SYMBOLS = ("gs_segtopk16_create", "gs_segtopk16_destroy", "gs_segtopk16_temp_bytes", "gs_segtopk16_select_keys", "gs_segtopk16_select_pairs",
           "gs_segtopk16_check", "gs_segtopk16_last", "gs_segtopk16_set_rank_mode", "gs_segtopk16_get_rank_mode")


def test_symbols_are_declared_exported_and_bound():
    from gpusorting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gs_segtopk16_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    # the report reuses the 32-bit call's macros: there is no second set
    assert not re.search(r"#define\s+GS_SEGTOPK16_", header)
    import gpusorting_amd as g
    from gpusorting_amd import functional
    assert g.SegmentedTopK16 and g.segmented_topk16 is functional.segmented_topk16
    assert issubclass(g.SegmentedTopK16, g.SegmentedTopK) and g.SegmentedTopK16._KEY_BYTES == 2


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    lib = _lib.load()
    for segs in (1, 2, 63, 64, 65, 191, 192, 193, 1000, 4096, 65536, (1 << 20) + 7, 1 << 27, _lib.GS_MAX_KEYS):
        assert lib.gs_segtopk16_temp_bytes(segs) == ((64 + segs) * 4 + 255) & ~255 == lib.gs_segtopk_temp_bytes(segs), segs


def test_the_null_handle_and_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_segtopk16_create(None, 1024, 16, 8, KEYS, 0) == A
    assert lib.gs_segtopk16_create(C.byref(h), 0, 16, 8, KEYS, 0) == S and lib.gs_segtopk16_create(C.byref(h), 1 << 30, 16, 8, KEYS, 0) == S
    assert lib.gs_segtopk16_create(C.byref(h), 1024, 0, 8, KEYS, 0) == S and lib.gs_segtopk16_create(C.byref(h), 1024, 1 << 30, 8, KEYS, 0) == S
    assert lib.gs_segtopk16_create(C.byref(h), 1024, 16, 0, KEYS, 0) == S and lib.gs_segtopk16_create(C.byref(h), 1024, 16, 1 << 30, KEYS, 0) == S
    assert lib.gs_segtopk16_create(C.byref(h), 1024, 16, 8, KEYS, 4) == M and lib.gs_segtopk16_create(C.byref(h), 1024, 16, 8, PAIRS, 2) == M
    assert not h.value
    assert lib.gs_segtopk16_destroy(None) == A
    p = (C.c_uint32 * 16)()
    assert lib.gs_segtopk16_select_keys(None, None, 0, None, 0, 0, 0, None, 99, 0, None) == A
    assert lib.gs_segtopk16_select_keys(None, 16, 4, 64, 1, 2, 0, 32, U16, 0, None) == A
    assert lib.gs_segtopk16_select_pairs(None, 16, 32, 4, 64, 1, 2, 0, 48, 80, BF16, 1, None) == A
    assert lib.gs_segtopk16_select_pairs(None, 16, None, 4, 64, 1, 2, 0, 48, 80, I16, 0, None) == A
    assert lib.gs_segtopk16_check(None, None) == A
    assert lib.gs_segtopk16_last(None, p, 16, None) == A
    assert lib.gs_segtopk16_set_rank_mode(None, 0) == A
    assert lib.gs_segtopk16_get_rank_mode(None) == -1


def _bits16(u, kt):
    """The 16-bit pattern whose unsigned order is the key order."""
    u = u.astype(np.uint32)
    if kt == U16:
        return u
    if kt == I16:
        return u ^ 0x8000
    return np.where(u & 0x8000, u ^ 0xFFFF, u ^ 0x8000)


def _independent(keys, offsets, k, values, descending, kt, fill_key, fill_value):
    segs = len(offsets) - 1
    out_k = np.full((segs, k), fill_key, dtype=np.uint16)
    out_v = np.full((segs, k), fill_value, dtype=np.uint32 if values is None else values.dtype)
    counts = np.zeros(segs, dtype=np.int64)
    bits = _bits16(keys, kt)
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


# +-0, +-inf, NaNs of both signs, denormals (float16 and bfloat16 patterns), INT16 min / max, 0 and 0xFFFF
SPECIAL = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7F80, 0xFF80, 0x7E00, 0xFE00, 0x7FC0, 0xFFC0, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF,
                    0x007F, 0x807F, 0x7FFF, 0x8000, 0x3C00, 0xBC00], dtype=np.uint16)


def special_keys(rng, n, share=0.4):
    keys = rng.integers(0, 1 << 16, n).astype(np.uint16)
    sel = rng.random(n) < share
    keys[sel] = SPECIAL[rng.integers(0, SPECIAL.size, int(sel.sum()))]
    return keys


@pytest.mark.parametrize("kt", (U16, I16, F16, BF16))
@pytest.mark.parametrize("descending", (False, True))
def test_reference_on_16_bit_keys_equals_the_independent_statement(kt, descending):
    from gpusorting_amd.segtopk import segmented_topk_reference
    rng = np.random.default_rng(160 + kt)
    lens = np.concatenate([rng.integers(0, 40, 30), [0, 0, 1, 1, 1, 2, 33, 64, 0, 300, 1]])
    rng.shuffle(lens)
    off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1]) + 5
    keys = special_keys(rng, n)
    for k in (1, 2, 33, 400):
        for values in (None, rng.integers(0, 1 << 32, n).astype(np.uint32), rng.integers(0, 1 << 63, n).astype(np.uint64)):
            got = segmented_topk_reference(keys, off, k, values, descending, kt, fill_key=0xDEAD, fill_value=0xABCD)
            want = _independent(keys, off, k, values, descending, kt, 0xDEAD, 0xABCD)
            assert got[0].dtype == np.uint16 and np.array_equal(got[0], want[0]), k
            assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), k
            assert np.array_equal(got[2], want[2])


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    off = torch.tensor([0, 4], dtype=torch.int32)
    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8):
        with pytest.raises(TypeError, match="segmented_topk"):
            functional.segmented_topk16(torch.zeros(4, dtype=dtype), off, 2)
    for dtype in (torch.float16, torch.bfloat16, torch.int16):
        with pytest.raises(ValueError):  # not on the device
            functional.segmented_topk16(torch.zeros(4, dtype=dtype), off, 2)
        with pytest.raises(ValueError):  # not 1-D
            functional.segmented_topk16(torch.zeros((2, 2), dtype=dtype), off, 2)
    # the 32-bit function keeps refusing 2-byte keys
    with pytest.raises((TypeError, ValueError)):
        functional.segmented_topk(torch.zeros(4, dtype=torch.int16), off, 2)
