"""CPU tests of unique / run-length encode (gs_unique_* in include/gpusort.h, gpusorting_amd/unique.py): the symbols are declared,
exported and bound; every handle entry answers a null handle with GS_ERR_ARG; the create arguments are answered before a device is
looked for; gs_unique_temp_bytes is the formula the header states; gs_unique_plan's properties; unique_reference — what the GPU tests
compare with — against numpy.unique on integers, against a hand-written expectation on float specials and against a plain loop for
the consecutive mode; and the argument errors of functional.unique that need no device.  No compute is run."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = 0, 1, 2
KEYS, PAIRS = 0, 1
SYMBOLS = ("gs_unique_create", "gs_unique_destroy", "gs_unique_temp_bytes", "gs_unique_keys", "gs_unique_positions", "gs_unique_consecutive",
           "gs_unique_plan", "gs_unique_check", "gs_unique_last")


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gs_unique_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_UNIQUE_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert len(defines) == 13
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    import gpusorting_amd as g
    from gpusorting_amd import functional
    unique = importlib.import_module("gpusorting_amd.unique")  # (the package attribute of that name is the function)
    assert g.Unique is unique.Unique and g.unique is functional.unique and g.unique_consecutive is functional.unique_consecutive
    assert g.unique_reference is unique.unique_reference and g.unique_plan is unique.unique_plan
    assert (unique.ROUTE_NONE, unique.ROUTE_KEYS, unique.ROUTE_POSITIONS, unique.ROUTE_CONSECUTIVE) == (0, 1, 2, 3)
    assert len(unique._REPORT) == _lib.GS_UNIQUE_REPORT_WORDS


def test_every_handle_entry_answers_a_null_handle_with_an_argument_error():
    """Every other argument is plausible: aligned, distinct addresses, a 32-bit key type, valid sizes."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    buf = (C.c_uint32 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    n, step = 1024, 4096
    assert lib.gs_unique_destroy(None) == A
    for kt in (U32, I32, F32):
        for order in (0, 1):
            assert lib.gs_unique_keys(None, p, n, p + step, p + 2 * step, p + 5 * step, kt, order, None) == A
            assert lib.gs_unique_positions(None, p, n, p + step, p + 2 * step, p + 3 * step, p + 4 * step, p + 5 * step, kt, order, None) == A
            assert lib.gs_unique_positions(None, p, n, p + step, None, None, None, None, kt, order, None) == A
    assert lib.gs_unique_consecutive(None, p, n, p + step, p + 2 * step, p + 4 * step, p + 5 * step, None) == A
    assert lib.gs_unique_check(None, None) == A
    assert lib.gs_unique_last(None, rep, 8192, None) == A


def test_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_unique_create(None, 1024, KEYS, 0) == A
    assert lib.gs_unique_create(C.byref(h), 0, KEYS, 0) == S and lib.gs_unique_create(C.byref(h), 1 << 30, KEYS, 0) == S
    assert lib.gs_unique_create(C.byref(h), 0, PAIRS, 8) == S  # the size is looked at first
    assert lib.gs_unique_create(C.byref(h), 1024, PAIRS, 8) == M and lib.gs_unique_create(C.byref(h), 1024, PAIRS, 2) == M
    assert lib.gs_unique_create(C.byref(h), 1024, KEYS, 4) == M and lib.gs_unique_create(C.byref(h), 1024, PAIRS, 0) == M
    assert lib.gs_unique_create(C.byref(h), 1024, 2, 4) == M
    assert not h.value


def _up(x):
    return (x + 255) & ~255


def _formula(max_keys, mode, engine):
    """The header's statement of gs_unique_temp_bytes."""
    return _up(64 * 4) + 4 * _up(1024 * 4) + (4 if mode == PAIRS else 2) * _up(4 * max_keys) + engine


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    from gpusorting_amd.unique import temp_bytes
    lib = _lib.load()
    for mode, vb in ((KEYS, 0), (PAIRS, 4)):
        for max_keys in (1, 63, 64, 65, 4096, 4097, 65536, (1 << 20) - 3, (1 << 20) + 1, 1 << 24, (1 << 30) - 1):
            got = lib.gs_unique_temp_bytes(max_keys, mode, vb)
            assert got == _formula(max_keys, mode, lib.gs_onesweep_temp_bytes(max_keys)) > 0, (mode, max_keys)
            assert temp_bytes(max_keys, mode, vb) == got
    for args in ((1024, KEYS, 4), (1024, PAIRS, 0), (1024, PAIRS, 2), (1024, PAIRS, 8), (1024, 2, 0), (1024, 7, 4), (0, KEYS, 0), (1 << 30, KEYS, 0)):
        assert lib.gs_unique_temp_bytes(*args) == 0, args


def test_plan_properties_and_refusals():
    from gpusorting_amd import _lib
    from gpusorting_amd.unique import unique_plan
    lib = _lib.load()
    plan = (C.c_uint32 * 3)()
    assert lib.gs_unique_plan(1024, None) == _lib.GS_ERR_ARG
    assert lib.gs_unique_plan(0, plan) == _lib.GS_ERR_SIZE and lib.gs_unique_plan(1 << 30, plan) == _lib.GS_ERR_SIZE
    rng = np.random.default_rng(21)
    sizes = [1, 2, 4095, 4096, 4097, 8192, 8193, 1 << 20, (1 << 20) + 1, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 1 << 28, (1 << 30) - 1]
    sizes += [int(x) for x in rng.integers(1, 1 << 30, 200)]
    for n in sizes:
        ranges, per, tile = unique_plan(n)
        assert tile == 4096 and per % tile == 0 and per >= tile, n
        assert 1 <= ranges <= 1024 and ranges * per >= n > (ranges - 1) * per, n  # enough room, and no empty range
        assert per == -(-(-(-n // 1024)) // tile) * tile, n                       # the header's formula
    assert unique_plan(4096) == (1, 4096, 4096) and unique_plan(4097) == (2, 4096, 4096)
    assert unique_plan((1 << 22) + 1) == (513, 8192, 4096)


def _np_expect(values, descending):
    """numpy.unique's four results, reversed for descending."""
    uk, first, inverse, counts = np.unique(values, return_index=True, return_inverse=True, return_counts=True)
    if descending:
        uk, first, counts, inverse = uk[::-1], first[::-1], counts[::-1], uk.size - 1 - inverse
    return uk, counts, first, inverse


@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("kt", (U32, I32))
def test_reference_against_numpy_unique_on_integers(kt, descending):
    from gpusorting_amd.unique import unique_reference
    rng = np.random.default_rng(300 + kt)
    dtype = np.uint32 if kt == U32 else np.int32
    info = np.iinfo(dtype)
    for n, distinct in ((1, 1), (2, 1), (2, 2), (1000, 7), (5000, 37), (5000, 1 << 31), (4097, 3)):
        pool = rng.integers(info.min, int(info.max) + 1, min(distinct, 1 << 16)).astype(dtype) if distinct < (1 << 31) else None
        values = pool[rng.integers(0, pool.size, n)] if pool is not None else rng.integers(info.min, int(info.max) + 1, n).astype(dtype)
        if n >= 1000:
            values[:3] = (info.min, info.max, 0)
        gk, gc, gf, gi = unique_reference(values, kt, descending)
        ek, ec, ef, ei = _np_expect(values, descending)
        assert all(a.dtype == np.uint32 for a in (gk, gc, gf, gi))
        assert np.array_equal(gk.view(dtype), ek) and np.array_equal(gc, ec) and np.array_equal(gf, ef) and np.array_equal(gi, ei), (n, distinct)
        assert gc.sum() == n and np.array_equal(gk[gi], values.view(np.uint32)) and np.array_equal(values[gf].view(np.uint32), gk)


# float32 patterns in the library's ascending order: negative NaNs (largest pattern first), -inf, -1, negative subnormals, -0, +0,
# positive subnormals, 1, +inf, positive NaNs
F32_ASCENDING = np.array([0xFFC00001, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000002, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x00000002,
                          0x3F800000, 0x7F800000, 0x7FC00000, 0x7FC00001], dtype=np.uint32)


def float_special_case(rng, copies=(3, 1, 2, 5, 1, 4, 2, 6, 1, 2, 3, 1, 2, 4)):
    """A shuffled array holding pattern j of F32_ASCENDING copies[j] times, and where each lies."""
    values = np.repeat(F32_ASCENDING, copies)
    rng.shuffle(values)
    return values, np.array(copies, dtype=np.uint32)


@pytest.mark.parametrize("descending", (False, True))
def test_reference_on_float_specials_is_the_hand_written_order_and_multiplicity(descending):
    from gpusorting_amd.unique import unique_reference
    values, copies = float_special_case(np.random.default_rng(5))
    gk, gc, gf, gi = unique_reference(values, F32, descending)
    order = F32_ASCENDING[::-1] if descending else F32_ASCENDING
    assert np.array_equal(gk, order)  # -0 and +0 apart, four NaN patterns apart
    assert np.array_equal(gc, copies[::-1] if descending else copies)
    for j, pattern in enumerate(order):
        where = np.flatnonzero(values == pattern)
        assert gf[j] == where[0] and np.all(gi[where] == j)
    # the same bits as float32 storage
    assert all(np.array_equal(a, b) for a, b in zip(unique_reference(values.view(np.float32), F32, descending), (gk, gc, gf, gi)))
    # numpy compares values: it merges the zeros (one key fewer at the least)
    assert np.unique(values.view(np.float32)).size < gk.size


def test_reference_consecutive_against_a_plain_loop():
    from gpusorting_amd.unique import unique_reference
    rng = np.random.default_rng(8)
    cases = [rng.integers(0, 3, 500).astype(np.uint32), np.zeros(17, np.uint32), np.arange(33, dtype=np.uint32), np.array([5], np.uint32),
             np.tile(np.array([1, 2], np.uint32), 40), float_special_case(rng)[0], np.array([0x80000000, 0, 0, 0x80000000], np.uint32)]
    for values in cases:
        keys, counts, first, inverse = [], [], [], []
        for i, v in enumerate(values.tolist()):
            if i == 0 or v != keys[-1]:
                keys.append(v)
                counts.append(0)
                first.append(i)
            counts[-1] += 1
            inverse.append(len(keys) - 1)
        for kt, descending in ((U32, False), (F32, True)):  # neither is looked at
            gk, gc, gf, gi = unique_reference(values, kt, descending, consecutive=True)
            assert gk.tolist() == keys and gc.tolist() == counts and gf.tolist() == first and gi.tolist() == inverse
    assert all(a.size == 0 and a.dtype == np.uint32 for a in unique_reference(np.zeros(0, np.uint32)))
    with pytest.raises(ValueError):
        unique_reference(np.zeros(4, np.uint16))
    with pytest.raises(ValueError):
        unique_reference(np.zeros(4, np.uint32), key_type=3)


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    for f in (functional.unique, functional.unique_consecutive):
        with pytest.raises(ValueError):  # 2-D
            f(torch.zeros((2, 2), dtype=torch.int32))
        for dtype in (torch.int64, torch.float16, torch.int16, torch.float64, torch.uint8):
            with pytest.raises(TypeError, match="unique"):
                f(torch.zeros(4, dtype=dtype))
        with pytest.raises(ValueError):  # not on the device
            f(torch.zeros(4, dtype=torch.float32))
