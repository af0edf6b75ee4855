"""CPU tests of unique / run-length encode on 64-bit keys (gs_unique64_* in include/gpusort.h, gpusorting_amd/unique64.py): the symbols
are declared, exported and bound; every handle entry answers a null handle with GS_ERR_ARG; the create arguments are answered before a
device is looked for; gs_unique64_temp_bytes is the formula the header states; unique64_reference — what the GPU tests compare with —
against numpy.unique on uint64 / int64 / float64 in both orders, by hand, and on float64 specials by pattern; and the argument errors of
functional.unique64 that need no device.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, I64, F64 = 3, 4, 5
SYMBOLS = ("gs_unique64_create", "gs_unique64_destroy", "gs_unique64_temp_bytes", "gs_unique64_keys", "gs_unique64_positions",
           "gs_unique64_consecutive", "gs_unique64_check", "gs_unique64_last")
PROTOTYPES = {  # (result, arguments) as the header declares them: p pointer, u uint32_t, i an enum, z size_t
    "gs_unique64_create": ("i", "puiu"), "gs_unique64_destroy": ("i", "p"), "gs_unique64_temp_bytes": ("z", "uiu"),
    "gs_unique64_keys": ("i", "ppupppiip"), "gs_unique64_positions": ("i", "ppupppppiip"), "gs_unique64_consecutive": ("i", "ppuppppp"),
    "gs_unique64_check": ("i", "pp"), "gs_unique64_last": ("i", "ppup")}

# float64 patterns in the library's ascending order: -NaN (larger payload first), -inf, -1, negative denormals, -0.0, +0.0, ..., +NaN
F64_ASCENDING = np.array([0xFFF8000000000001, 0xFFF8000000000000, 0xFFF0000000000000, 0xBFF0000000000000, 0x8000000000000002, 0x8000000000000001,
                          0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x0000000000000002, 0x3FF0000000000000, 0x7FF0000000000000,
                          0x7FF8000000000000, 0x7FF8000000000001], dtype=np.uint64)


def draws64(n, seed, distinct):
    """n draws from `distinct` random 64-bit patterns (both words random, both sides of the sign bit); distinct == 0: all different."""
    rng = np.random.default_rng(seed)
    if distinct == 0:
        return rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # (an odd multiplier modulo 2^64: a bijection)
    pool = rng.integers(0, 1 << 64, distinct, dtype=np.uint64)
    return pool[rng.integers(0, distinct, n)]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)


def declared(text, name):
    """(result, arguments) of the header's declaration of `name`, in the letters of PROTOTYPES."""
    m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"

    def letter(t):
        t = t.strip()
        if "*" in t or "[" in t:
            return "p"
        return {"uint32_t": "u", "size_t": "z"}.get(t.split()[0], "i")

    return letter(m.group(1)), "".join(letter(a) for a in m.group(2).split(","))


def bound(proto):
    """The same letters from a ctypes prototype of _lib._PROTOS."""
    def letter(t):
        if t is C.c_uint32:
            return "u"
        if t is C.c_size_t:
            return "z"
        return "i" if t is C.c_int else "p"

    return letter(proto[1]), "".join(letter(a) for a in proto[2])


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = header_text()
    assert set(re.findall(r"\b(gs_unique64_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    protos = {p[0]: p for p in _lib._PROTOS}
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
        assert declared(text, name) == PROTOTYPES[name] == bound(protos[name]), name
    defines = dict(re.findall(r"#define\s+(GS_UNIQUE64_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert len(defines) == 13
    for name, value in defines.items():  # the 32-bit family's words under their own names
        assert getattr(_lib, name) == int(value) == getattr(_lib, name.replace("UNIQUE64", "UNIQUE")), name
    import gpusorting_amd as g
    import importlib
    from gpusorting_amd import functional
    unique64 = importlib.import_module("gpusorting_amd.unique64")  # (the package attribute of that name is the function)
    assert g.Unique64 is unique64.Unique64 and g.unique64_reference is unique64.unique64_reference
    assert g.unique64 is functional.unique64 and g.unique_consecutive64 is functional.unique_consecutive64
    assert issubclass(g.Unique64, g.Unique) and g.Unique64._PREFIX == "gs_unique64_" and g.Unique._PREFIX == "gs_unique_"
    assert unique64.KEY64_TYPES == (g.KEY_UINT64, g.KEY_INT64, g.KEY_FLOAT64) == (U64, I64, F64)


def test_every_handle_entry_answers_a_null_handle_with_an_argument_error():
    """Every other argument is plausible: aligned, distinct addresses, valid types and sizes."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    buf = (C.c_uint32 * 32768)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    n, step = 1024, 16384
    assert lib.gs_unique64_destroy(None) == A
    for kt in (U64, I64, F64):
        for order in (0, 1):
            assert lib.gs_unique64_keys(None, p, n, p + step, p + 2 * step, p + 3 * step, kt, order, None) == A
            assert lib.gs_unique64_positions(None, p, n, p + step, p + 2 * step, p + 3 * step, p + 4 * step, p + 5 * step, kt, order, None) == A
    assert lib.gs_unique64_consecutive(None, p, n, p + step, p + 2 * step, p + 3 * step, p + 4 * step, None) == A
    assert lib.gs_unique64_check(None, None) == A
    assert lib.gs_unique64_last(None, rep, 32768, None) == A


def test_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_unique64_create(None, 1024, 0, 0) == A
    assert lib.gs_unique64_create(C.byref(h), 0, 0, 0) == S and lib.gs_unique64_create(C.byref(h), 1 << 30, 1, 4) == S
    assert lib.gs_unique64_create(C.byref(h), 0, 0, 8) == S  # the size is looked at first
    for mode, vb in ((0, 4), (0, 8), (1, 0), (1, 8), (1, 2), (2, 0), (-1, 4)):
        assert lib.gs_unique64_create(C.byref(h), 1024, mode, vb) == M, (mode, vb)
    assert not h.value


def _up(x):
    return (x + 255) & ~255


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    from gpusorting_amd.unique64 import temp_bytes
    lib = _lib.load()
    for mode, vb in ((0, 0), (1, 4)):
        for max_keys in (1, 63, 64, 65, 4096, 4097, 65536, (1 << 20) - 3, (1 << 20) + 1, 1 << 24, (1 << 30) - 1):
            want = _up(64 * 4) + 4 * _up(1024 * 4) + 2 * _up(8 * max_keys) + (2 * _up(4 * max_keys) if mode else 0) + lib.gs_onesweep_temp_bytes(max_keys)
            got = lib.gs_unique64_temp_bytes(max_keys, mode, vb)
            assert got == want > 0, (mode, max_keys)
            assert temp_bytes(max_keys, mode, vb) == got
            assert got - lib.gs_unique_temp_bytes(max_keys, mode, vb) == 2 * (_up(8 * max_keys) - _up(4 * max_keys))  # the keys alone are wider
    for args in ((1024, 0, 4), (1024, 1, 0), (1024, 1, 8), (0, 0, 0), (1 << 30, 1, 4)):
        assert lib.gs_unique64_temp_bytes(*args) == 0, args


def test_reference_hand_worked_cases():
    from gpusorting_amd.unique64 import unique64_reference as ref
    b = 1 << 32
    keys = np.array([3 * b, 1, 3 * b, 2 * b + 5, 1, 3 * b], np.uint64)  # keys that a 32-bit view would order and merge differently
    for got, want in ((ref(keys), ([1, 2 * b + 5, 3 * b], [2, 1, 3], [1, 3, 0], [2, 0, 2, 1, 0, 2])),
                      (ref(keys, descending=True), ([3 * b, 2 * b + 5, 1], [3, 1, 2], [0, 3, 1], [0, 2, 0, 1, 2, 0])),
                      (ref(keys, consecutive=True), (keys.tolist(), [1] * 6, list(range(6)), list(range(6))))):
        assert [g.tolist() for g in got] == [list(w) for w in want]
        assert got[0].dtype == np.uint64 and all(g.dtype == np.uint32 for g in got[1:])
    # the low word alone is equal, and the high word alone is equal: four keys
    split = np.array([b + 7, 7, b + 8, b + 7, 2 * b + 7], np.uint64)
    assert ref(split)[0].tolist() == [7, b + 7, b + 8, 2 * b + 7] and ref(split)[1].tolist() == [1, 2, 1, 1]
    # signed keys: -1 sorts first as int64, last as uint64
    sk = np.array([-1, 0, -1, 5], np.int64)
    assert ref(sk, I64)[0].view(np.int64).tolist() == [-1, 0, 5] and ref(sk, U64)[0].view(np.int64).tolist() == [0, 5, -1]
    e = ref(np.zeros(0, np.int64), I64)
    assert e[0].dtype == np.uint64 and all(a.size == 0 for a in e)
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint32))
    with pytest.raises(ValueError):
        ref(np.zeros((2, 2), np.uint64))
    for kt in (0, 1, 2, 6, 9):
        with pytest.raises(ValueError):
            ref(np.zeros(4, np.uint64), kt)


@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("kt", (U64, I64, F64))
def test_reference_against_numpy_unique(kt, descending):
    from gpusorting_amd.unique64 import unique64_reference as ref
    dtype = {U64: np.uint64, I64: np.int64, F64: np.float64}[kt]
    for n, distinct in ((1, 1), (2, 1), (2, 2), (1000, 7), (5000, 37), (4097, 3), (3000, 0)):
        bits = draws64(n, 11 * n + kt, distinct)
        if kt == F64:  # finite, nonzero values: there numpy's equality of values is the equality of bits
            bits = (bits & np.uint64(0x800FFFFFFFFFFFFF)) | (np.uint64(0x3FF) + (bits >> np.uint64(60))) << np.uint64(52)
        keys = bits.view(dtype)
        uk, index, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
        if descending:
            uk, index, counts, inverse = uk[::-1], index[::-1], counts[::-1], uk.size - 1 - inverse
        gk, gc, gf, gi = ref(keys, kt, descending)
        assert np.array_equal(gk, uk.view(np.uint64)) and np.array_equal(gc, counts) and np.array_equal(gf, index) and np.array_equal(gi, inverse.reshape(-1))
        runs = np.sort(keys)
        gk, gc, gf, gi = ref(runs, consecutive=True)
        uk, index, inverse, counts = np.unique(runs, return_index=True, return_inverse=True, return_counts=True)
        assert np.array_equal(gk, uk.view(np.uint64)) and np.array_equal(gc, counts) and np.array_equal(gf, index) and np.array_equal(gi, inverse.reshape(-1))


def test_reference_float64_specials_by_pattern():
    """-0.0 and +0.0 are two keys, NaN patterns are placed by their bits: the list above is the ascending order, whatever the input's."""
    from gpusorting_amd.unique64 import sortable_bits64, unique64_reference as ref
    sb = sortable_bits64(F64_ASCENDING, F64)
    assert np.all(sb[1:] > sb[:-1])
    rng = np.random.default_rng(5)
    keys = np.repeat(F64_ASCENDING, np.arange(1, 15))
    rng.shuffle(keys)
    gk, gc, gf, gi = ref(keys, F64)
    assert gk.tolist() == F64_ASCENDING.tolist() and gc.tolist() == list(range(1, 15))
    assert np.array_equal(gk[gi], keys) and all(f == np.flatnonzero(keys == k)[0] for k, f in zip(gk, gf))
    dk, dc, df, di = ref(keys, F64, True)
    assert dk.tolist() == F64_ASCENDING[::-1].tolist() and np.array_equal(df, gf[::-1]) and np.array_equal(dc, gc[::-1])
    assert np.unique(keys.view(np.float64)).size < 14  # numpy merges the zeros (and NaNs): the statement here is another one
    # as uint64 and int64 the same patterns order differently
    assert ref(keys, U64)[0].tolist() == sorted(F64_ASCENDING.tolist())
    assert ref(keys, I64)[0].view(np.int64).tolist() == sorted(F64_ASCENDING.view(np.int64).tolist())


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    for f in (functional.unique64, functional.unique_consecutive64):
        with pytest.raises(ValueError):  # 2-D
            f(torch.zeros((2, 2), dtype=torch.int64))
        for dtype in (torch.int32, torch.float32, torch.float16, torch.int16, torch.uint8, torch.bool):
            with pytest.raises(TypeError, match=f.__name__):
                f(torch.zeros(4, dtype=dtype))
        with pytest.raises(ValueError):  # not on the device
            f(torch.zeros(4, dtype=torch.int64))
        with pytest.raises(ValueError):
            f(torch.zeros(4, dtype=torch.float64))
    # the 32-bit functions keep refusing 64-bit keys
    for f in (functional.unique, functional.unique_consecutive):
        with pytest.raises(TypeError):
            f(torch.zeros(4, dtype=torch.int64))
