"""CPU tests of reduce by key on 64-bit keys (gs_reduce64_* in include/gpusort.h, gpusorting_amd/reduce64.py): the symbols are declared,
exported and bound with the header's prototypes; every handle entry answers a null handle with GS_ERR_ARG; the create arguments are
answered before a device is looked for; gs_reduce64_temp_bytes is the formula the header states; reduce_by_key64_reference — what the
GPU tests compare with — by hand, against numpy.unique + np.add.at / np.minimum.at / np.maximum.at on uint64 / int64 / float64 keys in
both orders, and on float64 key specials by pattern; and the argument errors of functional.reduce_by_key64 that need no device.  No
compute is run."""
import ctypes as C

import numpy as np
import pytest

from test_unique64_cpu import F64_ASCENDING, bound, declared, draws64, header_text

U64, I64, F64 = 3, 4, 5
VI32, VU32, VF32, VI64, VU64, VF64 = range(6)
SUM, MIN, MAX = range(3)
NP = {VI32: np.int32, VU32: np.uint32, VF32: np.float32, VI64: np.int64, VU64: np.uint64, VF64: np.float64}
SYMBOLS = ("gs_reduce64_create", "gs_reduce64_destroy", "gs_reduce64_temp_bytes", "gs_reduce64_by_key", "gs_reduce64_by_key_consecutive",
           "gs_reduce64_check", "gs_reduce64_last")
PROTOTYPES = {"gs_reduce64_create": ("i", "puu"), "gs_reduce64_destroy": ("i", "p"), "gs_reduce64_temp_bytes": ("z", "uu"),
              "gs_reduce64_by_key": ("i", "pppuppppiiiip"), "gs_reduce64_by_key_consecutive": ("i", "pppuppppiip"),
              "gs_reduce64_check": ("i", "pp"), "gs_reduce64_last": ("i", "ppup")}


def test_symbols_constants_and_exports():
    import re
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = header_text()
    assert set(re.findall(r"\b(gs_reduce64_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    protos = {p[0]: p for p in _lib._PROTOS}
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
        assert declared(text, name) == PROTOTYPES[name] == bound(protos[name]), name
    defines = dict(re.findall(r"#define\s+(GS_REDUCE64_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert len(defines) == 14
    for name, value in defines.items():  # the 32-bit family's words under their own names
        assert getattr(_lib, name) == int(value) == getattr(_lib, name.replace("REDUCE64", "REDUCE")), name
    import gpusorting_amd as g
    from gpusorting_amd import functional, reduce64
    assert g.ReduceByKey64 is reduce64.ReduceByKey64 and g.reduce_by_key64_reference is reduce64.reduce_by_key64_reference
    assert g.reduce_by_key64 is functional.reduce_by_key64 and g.reduce_by_key_consecutive64 is functional.reduce_by_key_consecutive64
    assert issubclass(g.ReduceByKey64, g.ReduceByKey) and g.ReduceByKey64._PREFIX == "gs_reduce64_" and g.ReduceByKey._PREFIX == "gs_reduce_"
    assert "torch.amin" in reduce64.__doc__ and "fmin" in reduce64.__doc__


def test_every_handle_entry_answers_a_null_handle_with_an_argument_error():
    """Every other argument is plausible: aligned, distinct addresses, valid types and sizes."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    buf = (C.c_uint32 * 32768)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    n, step = 1024, 16384
    assert lib.gs_reduce64_destroy(None) == A
    for vt in range(6):
        for op in range(3):
            assert lib.gs_reduce64_by_key(None, p, p + step, n, p + 2 * step, p + 3 * step, p + 4 * step, p + 5 * step, U64, 0, vt, op, None) == A
            assert lib.gs_reduce64_by_key_consecutive(None, p, p + step, n, p + 2 * step, p + 3 * step, None, None, vt, op, None) == A
    assert lib.gs_reduce64_check(None, None) == A
    assert lib.gs_reduce64_last(None, rep, 32768, None) == A


def test_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_reduce64_create(None, 1024, 4) == A
    assert lib.gs_reduce64_create(C.byref(h), 0, 4) == S and lib.gs_reduce64_create(C.byref(h), 1 << 30, 8) == S
    assert lib.gs_reduce64_create(C.byref(h), 0, 3) == S  # the size is looked at first
    for vb in (0, 1, 2, 3, 5, 16):
        assert lib.gs_reduce64_create(C.byref(h), 1024, vb) == M, vb
    assert not h.value


def _up(x):
    return (x + 255) & ~255


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    from gpusorting_amd.reduce64 import temp_bytes
    lib = _lib.load()
    for vb in (4, 8):
        for max_keys in (1, 63, 64, 65, 4096, 4097, 65536, (1 << 20) - 3, (1 << 20) + 1, 1 << 24, (1 << 30) - 1):
            want = (_up(64 * 4) + 4 * _up(1024 * 4) + 2 * _up(1024 * 8) + 2 * _up(8 * max_keys) + 2 * _up(vb * max_keys) +
                    lib.gs_onesweep_temp_bytes(max_keys))
            got = lib.gs_reduce64_temp_bytes(max_keys, vb)
            assert got == want > 0, (vb, max_keys)
            assert temp_bytes(max_keys, vb) == got
            assert got - lib.gs_reduce_temp_bytes(max_keys, vb) == 2 * (_up(8 * max_keys) - _up(4 * max_keys))  # the keys alone are wider
    for args in ((1024, 0), (1024, 2), (1024, 16), (0, 4), (1 << 30, 8)):
        assert lib.gs_reduce64_temp_bytes(*args) == 0, args


def test_reference_hand_worked_cases():
    from gpusorting_amd.reduce64 import reduce_by_key64_reference as ref
    b = 1 << 32
    keys = np.array([3 * b, 1, 3 * b, 2 * b + 5, 1, 3 * b], np.uint64)
    vals = np.array([1, -2, 3, 4, 5, -6], np.int32)
    for got, want in ((ref(keys, vals, U64, False, VI32, SUM), ([1, 2 * b + 5, 3 * b], [3, 4, -2], [2, 1, 3])),
                      (ref(keys, vals, U64, True, VI32, SUM), ([3 * b, 2 * b + 5, 1], [-2, 4, 3], [3, 1, 2])),
                      (ref(keys, vals, U64, False, VI32, MIN), ([1, 2 * b + 5, 3 * b], [-2, 4, -6], [2, 1, 3])),
                      (ref(keys, vals, U64, False, VI32, MAX), ([1, 2 * b + 5, 3 * b], [5, 4, 3], [2, 1, 3])),
                      (ref(keys, vals, U64, False, VU32, MAX), ([1, 2 * b + 5, 3 * b], [-2, 4, -6], [2, 1, 3])),  # as uint32, -2 and -6 are large
                      (ref(keys, vals, U64, False, VI32, SUM, consecutive=True), (keys.tolist(), vals.tolist(), [1] * 6))):
        assert got[0].tolist() == want[0] and got[1].view(np.int32).tolist() == want[1] and got[2].tolist() == want[2]
        assert got[0].dtype == np.uint64 and got[2].dtype == np.uint32
    # one word alone is equal: no merge
    split = np.array([b + 7, 7, b + 8, b + 7, 2 * b + 7], np.uint64)
    got = ref(split, np.array([1, 10, 100, 1000, 10000], np.int64), U64, False, VI64, SUM)
    assert got[0].tolist() == [7, b + 7, b + 8, 2 * b + 7] and got[1].tolist() == [10, 1001, 100, 10000]
    # signed keys: -1 sorts first as int64, last as uint64
    sk = np.array([-1, 0, -1, 5], np.int64)
    assert ref(sk, vals[:4], I64, False, VI32, SUM)[0].view(np.int64).tolist() == [-1, 0, 5]
    assert ref(sk, vals[:4], U64, False, VI32, SUM)[0].view(np.int64).tolist() == [0, 5, -1]
    # modular sums; float sums come in float64 and a run of -0.0 stays -0.0
    big64 = np.array([0xFFFFFFFFFFFFFFFF, 2], np.uint64)
    assert ref(np.zeros(2, np.uint64), big64, U64, False, VU64, SUM)[1].tolist() == [1]
    f = np.array([-0.0, -0.0, 0.5, -0.0, 0.0], np.float32)
    out = ref(np.array([7, 7, 8, 9, 9], np.uint64), f, U64, False, VF32, SUM)[1]
    assert out.dtype == np.float64 and out.tolist() == [0.0, 0.5, 0.0] and np.signbit(out).tolist() == [True, False, False]
    e = ref(np.zeros(0, np.uint64), np.zeros(0, np.int64), U64, False, VI64, MIN)
    assert all(a.size == 0 for a in e) and e[0].dtype == np.uint64 and e[1].dtype == np.int64
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint32), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint64), np.zeros(4, np.int64), value_type=VI32)
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint64), np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint64), np.zeros(4, np.int32), op=3)
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint64), np.zeros(4, np.int32), key_type=0)


@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("kt", (U64, I64, F64))
@pytest.mark.parametrize("vt", (VI32, VU64))
def test_reference_against_numpy_scatter_on_integers(vt, kt, descending):
    from gpusorting_amd.reduce64 import reduce_by_key64_reference as ref
    rng = np.random.default_rng(40 + vt)
    dtype = NP[vt]
    info = np.iinfo(dtype)
    kdtype = {U64: np.uint64, I64: np.int64, F64: np.float64}[kt]
    for n, distinct in ((1, 1), (2, 1), (2, 2), (1000, 7), (5000, 37), (4097, 3)):
        bits = draws64(n, 13 * n + kt, distinct)
        if kt == F64:  # finite, nonzero values: there numpy's equality of values is the equality of bits
            bits = (bits & np.uint64(0x800FFFFFFFFFFFFF)) | (np.uint64(0x3FF) + (bits >> np.uint64(60))) << np.uint64(52)
        keys = bits.view(kdtype)
        vals = rng.integers(info.min, int(info.max) + 1, n, dtype=dtype)
        uk, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
        if descending:
            uk, counts, inverse = uk[::-1], counts[::-1], uk.size - 1 - inverse
        with np.errstate(over="ignore"):
            s = np.zeros(uk.size, dtype)
            np.add.at(s, inverse, vals)
            lo = np.full(uk.size, info.max, dtype)
            np.minimum.at(lo, inverse, vals)
            hi = np.full(uk.size, info.min, dtype)
            np.maximum.at(hi, inverse, vals)
        for op, want in ((SUM, s), (MIN, lo), (MAX, hi)):
            gk, gv, gc = ref(keys, vals, kt, descending, vt, op)
            assert gv.dtype == dtype and np.array_equal(gk, uk.view(np.uint64)) and np.array_equal(gv, want) and np.array_equal(gc, counts), (n, op)


def test_reference_float64_key_specials_by_pattern():
    """-0.0 and +0.0 are two keys, NaN patterns are keys of their own, placed by their bits."""
    from gpusorting_amd.reduce64 import reduce_by_key64_reference as ref
    keys = np.repeat(F64_ASCENDING, np.arange(1, 15))
    vals = np.ones(keys.size, np.int32)
    perm = np.random.default_rng(8).permutation(keys.size)
    gk, gv, gc = ref(keys[perm], vals, F64, False, VI32, SUM)
    assert gk.tolist() == F64_ASCENDING.tolist() and gv.tolist() == list(range(1, 15)) == gc.tolist()
    gk, gv, gc = ref(keys[perm], vals, F64, True, VI32, SUM)
    assert gk.tolist() == F64_ASCENDING[::-1].tolist() and gv.tolist() == list(range(14, 0, -1))


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    k, v = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float32)
    for f in (functional.reduce_by_key64, functional.reduce_by_key_consecutive64):
        with pytest.raises(ValueError):  # 2-D
            f(torch.zeros((2, 2), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32))
        with pytest.raises(ValueError):  # lengths
            f(k, torch.zeros(3, dtype=torch.float32))
        for dtype in (torch.int32, torch.float32, torch.float16, torch.int16, torch.uint8):
            with pytest.raises(TypeError, match=f.__name__):
                f(torch.zeros(4, dtype=dtype), v)
        for dtype in (torch.float16, torch.int16, torch.uint8, torch.bool):
            with pytest.raises(TypeError, match=f.__name__):
                f(k, torch.zeros(4, dtype=dtype))
        with pytest.raises(ValueError):
            f(k, v, op="prod")
        with pytest.raises(ValueError):  # not on the device
            f(k, v)
    # the 32-bit functions keep refusing 64-bit keys
    for f in (functional.reduce_by_key, functional.reduce_by_key_consecutive):
        with pytest.raises(TypeError):
            f(k, v)
