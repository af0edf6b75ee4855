"""CPU tests of unique / run-length encode on 16-bit keys (gs_unique16_* in include/gpusort.h, gpusorting_amd/unique16.py): the symbols
are declared, exported and bound; every handle entry answers a null handle with GS_ERR_ARG; the create arguments are answered before a
device is looked for; gs_unique16_temp_bytes is the formula the header states and has no term in max_keys; unique16_reference — what
the GPU tests compare with — against numpy.unique on int16 and uint16, against a hand-written table on float16 and bfloat16 specials
and against a plain loop for the consecutive mode; and the argument errors of functional.unique16 that need no device.  No compute is
run."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = 6, 7, 8, 9
SYMBOLS = ("gs_unique16_create", "gs_unique16_destroy", "gs_unique16_temp_bytes", "gs_unique16_unique", "gs_unique16_consecutive",
           "gs_unique16_check", "gs_unique16_last", "gs_unique16_set_inverse_form")


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gs_unique16_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_UNIQUE16_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert len(defines) == 20
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    assert re.search(r"#define\s+GS_UNIQUE16_INVERSE_LDS_MIN\s+\(1u << (\d+)\)", text).group(1) == str(_lib.GS_UNIQUE16_INVERSE_LDS_MIN.bit_length() - 1)
    import gpusorting_amd as g
    from gpusorting_amd import functional
    unique16 = importlib.import_module("gpusorting_amd.unique16")  # (the package attribute of that name is the function)
    assert g.Unique16 is unique16.Unique16 and g.unique16 is functional.unique16 and g.unique_consecutive16 is functional.unique_consecutive16
    assert g.unique16_reference is unique16.unique16_reference
    assert (unique16.ROUTE_NONE, unique16.ROUTE_HISTOGRAM, unique16.ROUTE_CONSECUTIVE) == (0, 1, 2)
    assert (unique16.RAN_FIRST, unique16.RAN_INVERSE_LDS, unique16.RAN_INVERSE_GATHER) == (1, 2, 4)
    assert len(unique16._REPORT) == _lib.GS_UNIQUE16_REPORT_WORDS
    # the 32-bit family's comment points here instead of saying "not built"
    assert "not built" not in header[header.index("---- unique / run-length encode:"):header.index("typedef struct gs_unique gs_unique;")]


def test_every_handle_entry_answers_a_null_handle_with_an_argument_error():
    """Every other argument is plausible: aligned, distinct addresses, a 16-bit key type, valid sizes."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    buf = (C.c_uint32 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    n, step = 1024, 4096
    assert lib.gs_unique16_destroy(None) == A
    for kt in (U16, I16, F16, BF16):
        for order in (0, 1):
            assert lib.gs_unique16_unique(None, p, n, p + step, p + 2 * step, p + 3 * step, p + 4 * step, p + 6 * step, kt, order, None) == A
            assert lib.gs_unique16_unique(None, p, n, p + step, None, None, None, None, kt, order, None) == A
    assert lib.gs_unique16_consecutive(None, p, n, p + step, p + 2 * step, p + 4 * step, p + 6 * step, None) == A
    assert lib.gs_unique16_check(None, None) == A
    assert lib.gs_unique16_last(None, rep, 8192, None) == A
    for which in (0, 1, 2):
        assert lib.gs_unique16_set_inverse_form(None, which) == A


def test_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gs_unique16_create(None, 1024) == _lib.GS_ERR_ARG
    assert lib.gs_unique16_create(None, 0) == _lib.GS_ERR_ARG  # the null pointer first
    assert lib.gs_unique16_create(C.byref(h), 0) == _lib.GS_ERR_SIZE and lib.gs_unique16_create(C.byref(h), 1 << 30) == _lib.GS_ERR_SIZE
    assert not h.value


def _up(x):
    return (x + 255) & ~255


def test_temp_bytes_is_the_formula_of_the_header_and_has_no_term_in_max_keys():
    from gpusorting_amd import _lib
    from gpusorting_amd.unique16 import temp_bytes
    lib = _lib.load()
    formula = _up(64 * 4) + _up(65536 * 4) + _up(65536 * 4) + _up(65536 * 2) + 4 * _up(1024 * 4)
    assert formula == 672000  # the figure the header gives
    for max_keys in (1, 63, 65536, (1 << 20) + 1, 1 << 28, _lib.GS_MAX_KEYS):
        assert lib.gs_unique16_temp_bytes(max_keys) == formula == temp_bytes(max_keys), max_keys
    assert lib.gs_unique16_temp_bytes(0) == 0 and lib.gs_unique16_temp_bytes(_lib.GS_MAX_KEYS + 1) == 0


def _np_expect(values, descending):
    """numpy.unique's four results, reversed for descending (the lowest index is kept)."""
    uk, first, inverse, counts = np.unique(values, return_index=True, return_inverse=True, return_counts=True)
    if descending:
        uk, first, counts, inverse = uk[::-1], first[::-1], counts[::-1], uk.size - 1 - inverse
    return uk, counts, first, inverse


@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("kt", (U16, I16))
def test_reference_against_numpy_unique_on_integers(kt, descending):
    from gpusorting_amd.unique16 import unique16_reference
    rng = np.random.default_rng(300 + kt)
    dtype = np.uint16 if kt == U16 else np.int16
    info = np.iinfo(dtype)
    for n, distinct in ((1, 1), (2, 1), (2, 2), (1000, 7), (5000, 37), (5000, 0), (4097, 3), (200000, 0)):
        if distinct:
            pool = rng.integers(info.min, int(info.max) + 1, distinct).astype(dtype)
            values = pool[rng.integers(0, pool.size, n)]
        else:
            values = rng.integers(info.min, int(info.max) + 1, n).astype(dtype)
        if n >= 1000:
            values[:3] = (info.min, info.max, 0)
        gk, gc, gf, gi = unique16_reference(values, kt, descending)
        ek, ec, ef, ei = _np_expect(values, descending)
        assert gk.dtype == np.uint16 and all(a.dtype == np.uint32 for a in (gc, gf, gi))
        assert np.array_equal(gk.view(dtype), ek) and np.array_equal(gc, ec) and np.array_equal(gf, ef) and np.array_equal(gi, ei), (n, distinct)
        assert gc.sum() == n and np.array_equal(gk[gi], values.view(np.uint16)) and np.array_equal(values[gf].view(np.uint16), gk)


# bit patterns in the library's ascending order: two negative NaNs (largest pattern first), -inf, the largest finite value negated, -1,
# the smallest denormal negated, -0, +0, the smallest denormal, 1, the largest finite value, +inf, two positive NaNs
F16_ASCENDING = np.array([0xFE01, 0xFE00, 0xFC00, 0xFBFF, 0xBC00, 0x8001, 0x8000, 0x0000, 0x0001, 0x3C00, 0x7BFF, 0x7C00, 0x7E00, 0x7E01], dtype=np.uint16)
BF16_ASCENDING = np.array([0xFFC1, 0xFFC0, 0xFF80, 0xFF7F, 0xBF80, 0x8001, 0x8000, 0x0000, 0x0001, 0x3F80, 0x7F7F, 0x7F80, 0x7FC0, 0x7FC1], dtype=np.uint16)
SPECIALS = {F16: F16_ASCENDING, BF16: BF16_ASCENDING}


def special_case(kt, rng, copies=(3, 1, 2, 5, 1, 4, 2, 6, 1, 2, 3, 1, 2, 4)):
    """A shuffled array holding pattern j of the key type's table copies[j] times, and the copies."""
    values = np.repeat(SPECIALS[kt], copies)
    rng.shuffle(values)
    return values, np.array(copies, dtype=np.uint32)


def test_the_special_tables_say_what_their_comment_says():
    f = F16_ASCENDING.view(np.float16)
    assert np.isnan(f[[0, 1, 12, 13]]).all() and f[2] == -np.inf and f[11] == np.inf and f[3] == -65504.0 and f[10] == 65504.0
    assert f[4] == -1 and f[9] == 1 and f[8] == np.float16(2.0 ** -24) and np.signbit(f[6]) and f[6] == 0 and not np.signbit(f[7]) and f[7] == 0
    b = (BF16_ASCENDING.astype(np.uint32) << 16).view(np.float32)  # a bfloat16 is the top half of a float32
    assert np.isnan(b[[0, 1, 12, 13]]).all() and b[2] == -np.inf and b[11] == np.inf and b[10] == np.float32(2.0 ** 127 * (2 - 2.0 ** -7))
    assert b[3] == -b[10] and b[4] == -1 and b[9] == 1 and b[8] == np.float32(2.0 ** -133) and np.signbit(b[6]) and b[6] == 0 and b[7] == 0


@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("kt", (F16, BF16))
def test_reference_on_float_specials_is_the_hand_written_order_and_multiplicity(kt, descending):
    from gpusorting_amd.unique16 import unique16_reference
    values, copies = special_case(kt, np.random.default_rng(5))
    gk, gc, gf, gi = unique16_reference(values, kt, descending)
    order = SPECIALS[kt][::-1] if descending else SPECIALS[kt]
    assert np.array_equal(gk, order)  # -0 and +0 apart, four NaN patterns apart
    assert np.array_equal(gc, copies[::-1] if descending else copies)
    for j, pattern in enumerate(order):
        where = np.flatnonzero(values == pattern)
        assert gf[j] == where[0] and np.all(gi[where] == j)
    if kt == F16:  # the same bits as float16 storage; numpy compares values: it merges the zeros
        assert all(np.array_equal(a, b) for a, b in zip(unique16_reference(values.view(np.float16), kt, descending), (gk, gc, gf, gi)))
        assert np.unique(values.view(np.float16)).size < gk.size


def test_reference_consecutive_against_a_plain_loop_and_empty_input():
    from gpusorting_amd.unique16 import unique16_reference
    rng = np.random.default_rng(8)
    cases = [rng.integers(0, 3, 500).astype(np.uint16), np.zeros(17, np.uint16), np.arange(33, dtype=np.uint16), np.array([5], np.uint16),
             np.tile(np.array([1, 2], np.uint16), 40), special_case(F16, rng)[0], np.array([0x8000, 0, 0, 0x8000], np.uint16)]
    for values in cases:
        keys, counts, first, inverse = [], [], [], []
        for i, v in enumerate(values.tolist()):
            if i == 0 or v != keys[-1]:
                keys.append(v)
                counts.append(0)
                first.append(i)
            counts[-1] += 1
            inverse.append(len(keys) - 1)
        for kt, descending in ((U16, False), (BF16, True)):  # neither is looked at
            gk, gc, gf, gi = unique16_reference(values, kt, descending, consecutive=True)
            assert gk.tolist() == keys and gc.tolist() == counts and gf.tolist() == first and gi.tolist() == inverse
    for consecutive in (False, True):
        gk, gc, gf, gi = unique16_reference(np.zeros(0, np.uint16), consecutive=consecutive)
        assert gk.size == 0 and gk.dtype == np.uint16 and all(a.size == 0 and a.dtype == np.uint32 for a in (gc, gf, gi))
    with pytest.raises(ValueError):
        unique16_reference(np.zeros(4, np.uint32))
    with pytest.raises(ValueError):
        unique16_reference(np.zeros((2, 2), np.uint16))
    with pytest.raises(ValueError):
        unique16_reference(np.zeros(4, np.uint16), key_type=2)


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    for f in (functional.unique16, functional.unique_consecutive16):
        with pytest.raises(ValueError):  # 2-D
            f(torch.zeros((2, 2), dtype=torch.int16))
        for dtype in (torch.int64, torch.float32, torch.int32, torch.float64, torch.uint8):
            with pytest.raises(TypeError, match="unique"):
                f(torch.zeros(4, dtype=dtype))
        with pytest.raises(ValueError):  # not on the device
            f(torch.zeros(4, dtype=torch.float16))
