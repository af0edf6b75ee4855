"""CPU tests of the 1-D top-k on 16-bit keys (gs_topk16_* in include/gpusort.h, gpusorting_amd/topk16.py): the symbols are declared,
exported and bound; every handle entry answers a null handle with GS_ERR_ARG; gs_topk16_temp_bytes has no term that grows with
max_keys and is the formula the header states; topk_reference on the four 16-bit key types — what the GPU tests compare with — is the
head of sort16_reference; and the argument errors of functional.topk16 that need no device.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = 6, 7, 8, 9
KEYS, PAIRS = 0, 1
SYMBOLS = ("gs_topk16_create", "gs_topk16_destroy", "gs_topk16_temp_bytes", "gs_topk16_select_keys", "gs_topk16_select_pairs", "gs_topk16_check",
           "gs_topk16_last", "gs_topk16_set_count_histogram")


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gs_topk16_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_TOPK16_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert len(defines) == 18
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    import gpusorting_amd as g
    import importlib
    from gpusorting_amd import functional
    topk16 = importlib.import_module("gpusorting_amd.topk16")  # (the package attribute of that name is the function)
    assert g.TopK16 is topk16.TopK16 and g.topk16 is functional.topk16
    assert (topk16.ROUTE_NONE, topk16.ROUTE_TILE, topk16.ROUTE_COUNT, topk16.ROUTE_SELECT) == (0, 1, 2, 3)
    assert len(topk16._REPORT) == _lib.GS_TOPK16_REPORT_WORDS


def test_every_handle_entry_answers_a_null_handle_with_an_argument_error():
    """Every other argument is plausible: aligned, distinct addresses, a 16-bit key type, valid sizes."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    buf = (C.c_uint32 * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    assert lib.gs_topk16_destroy(None) == A
    for kt in (U16, I16, F16, BF16):
        for order in (0, 1):
            assert lib.gs_topk16_select_keys(None, p, 1024, 8, p + 4096, kt, order, None) == A
            assert lib.gs_topk16_select_pairs(None, p, p + 8192, 1024, 8, p + 4096, p + 4352, kt, order, None) == A
            assert lib.gs_topk16_select_pairs(None, p, None, 1024, 8, p + 4096, p + 4352, kt, order, None) == A
    assert lib.gs_topk16_check(None, None) == A
    assert lib.gs_topk16_last(None, rep, 4096, None) == A
    for which in (0, 1, 2):
        assert lib.gs_topk16_set_count_histogram(None, which) == A


def test_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_topk16_create(None, 1024, 8, KEYS, 0) == A
    assert lib.gs_topk16_create(C.byref(h), 0, 8, KEYS, 0) == S and lib.gs_topk16_create(C.byref(h), 1 << 30, 8, KEYS, 0) == S
    assert lib.gs_topk16_create(C.byref(h), 1024, 0, KEYS, 0) == S and lib.gs_topk16_create(C.byref(h), 1024, 1025, KEYS, 0) == S
    assert lib.gs_topk16_create(C.byref(h), 1024, 8, KEYS, 4) == M and lib.gs_topk16_create(C.byref(h), 1024, 8, PAIRS, 2) == M
    assert lib.gs_topk16_create(C.byref(h), 1024, 8, PAIRS, 0) == M and lib.gs_topk16_create(C.byref(h), 1024, 8, 2, 4) == M
    assert not h.value


def _up(x):
    return (x + 255) & ~255


def _formula(max_k, mode, vb, sorter):
    """The header's statement of gs_topk16_temp_bytes."""
    total = 256 + 2 * 262144 + 256 * 131088
    if mode == KEYS:
        return total + _up(262148)
    return total + 2048 + _up(max_k * 2) + _up(max_k * vb) + sorter


def test_temp_bytes_has_no_term_in_max_keys_and_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    lib = _lib.load()
    for mode, vb in ((KEYS, 0), (PAIRS, 4), (PAIRS, 8)):
        for max_k in (1, 127, 128, 129, 4096, 65536, (1 << 20) - 3):
            small, large = lib.gs_topk16_temp_bytes(1 << 20, max_k, mode, vb), lib.gs_topk16_temp_bytes((1 << 30) - 1, max_k, mode, vb)
            assert small == large > 0, (mode, vb, max_k)
            sorter = lib.gs_sort16_temp_bytes(max_k, mode, vb) if mode == PAIRS else 0
            assert small == _formula(max_k, mode, vb, sorter), (mode, vb, max_k)
    # a handle for 2^30 - 1 keys and k = 2^16 with positions stays below 40 MiB: nothing is n-sized
    assert lib.gs_topk16_temp_bytes((1 << 30) - 1, 1 << 16, PAIRS, 4) < 40 << 20
    # invalid mode, value width or sizes
    for args in ((1024, 8, KEYS, 4), (1024, 8, PAIRS, 0), (1024, 8, PAIRS, 2), (1024, 8, 2, 0), (1024, 8, 7, 4), (0, 8, KEYS, 0), (1 << 30, 8, KEYS, 0),
                 (1024, 0, KEYS, 0), (1024, 1025, KEYS, 0)):
        assert lib.gs_topk16_temp_bytes(*args) == 0, args


# +-0, +-inf, NaNs of both signs, denormals (float16 and bfloat16 patterns), INT16 min / max, 0 and 0xFFFF
SPECIAL = np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7F80, 0xFF80, 0x7E00, 0xFE00, 0x7FC0, 0xFFC0, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF,
                    0x007F, 0x807F, 0x3C00, 0xBC00], dtype=np.uint16)


@pytest.mark.parametrize("kt", (U16, I16, F16, BF16))
@pytest.mark.parametrize("descending", (False, True))
def test_reference_on_16_bit_keys_is_the_head_of_the_16_bit_sort(kt, descending):
    from gpusorting_amd.sort16 import sort16_reference
    from gpusorting_amd.topk import topk_reference
    rng = np.random.default_rng(1600 + kt)
    n = 3001
    patterns = {"random": rng.integers(0, 1 << 16, n).astype(np.uint16),
                "ties": rng.integers(0, 7, n).astype(np.uint16) * 0x1111,
                "special": SPECIAL[rng.integers(0, SPECIAL.size, n)],
                "equal": np.full(n, 0x8000, dtype=np.uint16)}
    v4, v8 = rng.integers(0, 1 << 32, n).astype(np.uint32), rng.integers(0, 1 << 63, n).astype(np.uint64)
    for name, keys in patterns.items():
        for values in (None, v4, v8):
            sk, sv = sort16_reference(keys, values, kt, descending)
            for k in (1, 2, 64, 1000, n - 1, n):
                gk, gv = topk_reference(keys, k, values, kt, descending)
                assert gk.dtype == np.uint16 and np.array_equal(gk, sk[:k]), (name, k)
                assert gv.dtype == sv.dtype and np.array_equal(gv, sv[:k]), (name, k)
    # the tie rule, spelled out: ascending the lowest positions rising, descending the highest falling
    eq = patterns["equal"]
    assert np.array_equal(topk_reference(eq, 5, None, kt, False)[1], np.arange(5))
    assert np.array_equal(topk_reference(eq, 5, None, kt, True)[1], n - 1 - np.arange(5))


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8):
        with pytest.raises(TypeError, match="topk"):
            functional.topk16(torch.zeros(4, dtype=dtype), 2)
    for dtype in (torch.float16, torch.bfloat16, torch.int16):
        with pytest.raises(ValueError):  # not on the device
            functional.topk16(torch.zeros(4, dtype=dtype), 2)
        with pytest.raises(ValueError):  # not 1-D or 2-D
            functional.topk16(torch.zeros((2, 2, 2), dtype=dtype), 2)
    # the 32-bit function keeps refusing 1-D 2-byte keys, and names both ways out
    with pytest.raises((TypeError, ValueError)):
        functional.topk(torch.zeros(4, dtype=torch.int16), 2)
