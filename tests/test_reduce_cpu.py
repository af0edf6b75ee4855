"""CPU tests of reduce by key (gs_reduce_* in include/gpusort.h, gpusorting_amd/reduce.py): the symbols are declared, exported and
bound; every handle entry answers a null handle with GS_ERR_ARG; the create arguments are answered before a device is looked for;
gs_reduce_temp_bytes is the formula the header states; reduce_by_key_reference — what the GPU tests compare with — against hand-worked
cases, against np.add.at / np.minimum.at / np.maximum.at on integers, and on float NaNs and signed zeros for MIN / MAX; and the argument
errors of functional.reduce_by_key that need no device.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = 0, 1, 2
VI32, VU32, VF32, VI64, VU64, VF64 = range(6)
SUM, MIN, MAX = range(3)
NP = {VI32: np.int32, VU32: np.uint32, VF32: np.float32, VI64: np.int64, VU64: np.uint64, VF64: np.float64}
SYMBOLS = ("gs_reduce_create", "gs_reduce_destroy", "gs_reduce_temp_bytes", "gs_reduce_by_key", "gs_reduce_by_key_consecutive", "gs_reduce_check",
           "gs_reduce_last")


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(gs_reduce_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_REDUCE_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert len(defines) == 14
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    enums = dict(re.findall(r"\b(GS_VALUE_[A-Z0-9]+|GS_REDUCE_(?:SUM|MIN|MAX))\s*=\s*(\d+)", text))
    assert len(enums) == 9
    for name, value in enums.items():
        assert getattr(_lib, name) == int(value), name
    import gpusorting_amd as g
    from gpusorting_amd import functional, reduce
    assert g.ReduceByKey is reduce.ReduceByKey and g.reduce_by_key is functional.reduce_by_key
    assert g.reduce_by_key_consecutive is functional.reduce_by_key_consecutive and g.reduce_by_key_reference is reduce.reduce_by_key_reference
    assert (reduce.VALUE_INT32, reduce.VALUE_UINT32, reduce.VALUE_FLOAT32, reduce.VALUE_INT64, reduce.VALUE_UINT64, reduce.VALUE_FLOAT64) == tuple(range(6))
    assert (reduce.OP_SUM, reduce.OP_MIN, reduce.OP_MAX) == (0, 1, 2) and (reduce.ROUTE_NONE, reduce.ROUTE_SORTED, reduce.ROUTE_CONSECUTIVE) == (0, 1, 2)
    assert len(reduce._REPORT) == _lib.GS_REDUCE_REPORT_WORDS
    assert "torch.amin" in reduce.__doc__ and "fmin" in reduce.__doc__ and "torch.amin" in header and "fmin" in header


def test_every_handle_entry_answers_a_null_handle_with_an_argument_error():
    """Every other argument is plausible: aligned, distinct addresses, valid types and sizes."""
    from gpusorting_amd import _lib
    lib = _lib.load()
    A = _lib.GS_ERR_ARG
    buf = (C.c_uint32 * 16384)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    n, step = 1024, 8192
    assert lib.gs_reduce_destroy(None) == A
    for vt in range(6):
        for op in range(3):
            assert lib.gs_reduce_by_key(None, p, p + step, n, p + 2 * step, p + 3 * step, p + 4 * step, p + 5 * step, U32, 0, vt, op, None) == A
            assert lib.gs_reduce_by_key_consecutive(None, p, p + step, n, p + 2 * step, p + 3 * step, None, None, vt, op, None) == A
    assert lib.gs_reduce_check(None, None) == A
    assert lib.gs_reduce_last(None, rep, 16384, None) == A


def test_create_arguments_are_answered_before_anything_touches_a_gpu():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S, M = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE, _lib.GS_ERR_MODE
    h = C.c_void_p()
    assert lib.gs_reduce_create(None, 1024, 4) == A
    assert lib.gs_reduce_create(C.byref(h), 0, 4) == S and lib.gs_reduce_create(C.byref(h), 1 << 30, 8) == S
    assert lib.gs_reduce_create(C.byref(h), 0, 3) == S  # the size is looked at first
    for vb in (0, 1, 2, 3, 5, 16):
        assert lib.gs_reduce_create(C.byref(h), 1024, vb) == M, vb
    assert not h.value


def _up(x):
    return (x + 255) & ~255


def _formula(max_keys, vb, engine):
    """The header's statement of gs_reduce_temp_bytes."""
    return _up(64 * 4) + 4 * _up(1024 * 4) + 2 * _up(1024 * 8) + 2 * _up(4 * max_keys) + 2 * _up(vb * max_keys) + engine


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    from gpusorting_amd.reduce import temp_bytes
    lib = _lib.load()
    for vb in (4, 8):
        for max_keys in (1, 63, 64, 65, 4096, 4097, 65536, (1 << 20) - 3, (1 << 20) + 1, 1 << 24, (1 << 30) - 1):
            got = lib.gs_reduce_temp_bytes(max_keys, vb)
            assert got == _formula(max_keys, vb, lib.gs_onesweep_temp_bytes(max_keys)) > 0, (vb, max_keys)
            assert temp_bytes(max_keys, vb) == got
    for args in ((1024, 0), (1024, 2), (1024, 16), (0, 4), (1 << 30, 8)):
        assert lib.gs_reduce_temp_bytes(*args) == 0, args


def test_reference_hand_worked_cases():
    from gpusorting_amd.reduce import reduce_by_key_reference as ref
    keys = np.array([3, 1, 3, 2, 1, 3], np.uint32)
    vals = np.array([1, -2, 3, 4, 5, -6], np.int32)
    for got, want in ((ref(keys, vals, U32, False, VI32, SUM), ([1, 2, 3], [3, 4, -2], [2, 1, 3])),
                      (ref(keys, vals, U32, True, VI32, SUM), ([3, 2, 1], [-2, 4, 3], [3, 1, 2])),
                      (ref(keys, vals, U32, False, VI32, MIN), ([1, 2, 3], [-2, 4, -6], [2, 1, 3])),
                      (ref(keys, vals, U32, False, VI32, MAX), ([1, 2, 3], [5, 4, 3], [2, 1, 3])),
                      (ref(keys, vals, U32, False, VU32, MAX), ([1, 2, 3], [-2, 4, -6], [2, 1, 3])),  # as uint32, -2 and -6 are large
                      (ref(keys, vals, U32, False, VI32, SUM, consecutive=True), ([3, 1, 3, 2, 1, 3], vals.tolist(), [1] * 6))):
        assert got[0].tolist() == want[0] and got[1].view(np.int32).tolist() == want[1] and got[2].tolist() == want[2]
        assert got[0].dtype == np.uint32 and got[2].dtype == np.uint32
    # signed keys: -1 sorts first as int32, last as uint32
    sk = np.array([-1, 0, -1, 5], np.int32)
    assert ref(sk, vals[:4], I32, False, VI32, SUM)[0].view(np.int32).tolist() == [-1, 0, 5]
    assert ref(sk, vals[:4], U32, False, VI32, SUM)[0].view(np.int32).tolist() == [0, 5, -1]
    # modular sums
    big = np.array([0xFFFFFFFF, 2, 0x80000000, 0x80000000], np.uint32)
    assert ref(np.zeros(4, np.uint32), big, U32, False, VU32, SUM)[1].tolist() == [1]
    big64 = np.array([0xFFFFFFFFFFFFFFFF, 2], np.uint64)
    assert ref(np.zeros(2, np.uint32), big64, U32, False, VU64, SUM)[1].tolist() == [1]
    assert ref(np.zeros(2, np.uint32), big64.view(np.int64), U32, False, VI64, SUM)[1].tolist() == [1]
    # float sums come in float64; a run of -0.0 stays -0.0, and a run of length 1 is itself
    f = np.array([-0.0, -0.0, 0.5, -0.0, 0.0], np.float32)
    out = ref(np.array([7, 7, 8, 9, 9], np.uint32), f, U32, False, VF32, SUM)[1]
    assert out.dtype == np.float64 and out.tolist() == [0.0, 0.5, 0.0] and np.signbit(out).tolist() == [True, False, False]
    # empty, and refusals
    e = ref(np.zeros(0, np.uint32), np.zeros(0, np.int64), U32, False, VI64, MIN)
    assert all(a.size == 0 for a in e) and e[1].dtype == np.int64
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint16), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint32), np.zeros(4, np.int64), value_type=VI32)
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint32), np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint32), np.zeros(4, np.int32), op=3)
    with pytest.raises(ValueError):
        ref(np.zeros(4, np.uint32), np.zeros(4, np.int32), key_type=3)


@pytest.mark.parametrize("descending", (False, True))
@pytest.mark.parametrize("vt", (VI32, VU32, VI64, VU64))
def test_reference_against_numpy_scatter_on_integers(vt, descending):
    from gpusorting_amd.reduce import reduce_by_key_reference as ref
    rng = np.random.default_rng(40 + vt)
    dtype = NP[vt]
    info = np.iinfo(dtype)
    for kt, kdtype in ((U32, np.uint32), (I32, np.int32)):
        for n, distinct in ((1, 1), (2, 1), (2, 2), (1000, 7), (5000, 37), (4097, 3)):
            kinfo = np.iinfo(kdtype)
            pool = rng.integers(kinfo.min, int(kinfo.max) + 1, distinct).astype(kdtype)
            keys = pool[rng.integers(0, distinct, n)]
            vals = rng.integers(info.min, int(info.max) + 1, n, dtype=dtype)
            uk, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
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
                assert gv.dtype == dtype and np.array_equal(gk.view(kdtype), uk) and np.array_equal(gv, want) and np.array_equal(gc, counts), (n, op)


# float32 patterns in the library's ascending order (tests/test_unique_cpu.py states the same list for the keys)
F32_ASCENDING = np.array([0xFFC00001, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000002, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x00000002,
                          0x3F800000, 0x7F800000, 0x7FC00000, 0x7FC00001], dtype=np.uint32)


def f64_ascending():
    """The same fourteen values as float64 patterns, in the same order."""
    return np.array([0xFFF8000000000001, 0xFFF8000000000000, 0xFFF0000000000000, 0xBFF0000000000000, 0x8000000000000002, 0x8000000000000001,
                     0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x0000000000000002, 0x3FF0000000000000, 0x7FF0000000000000,
                     0x7FF8000000000000, 0x7FF8000000000001], dtype=np.uint64)


@pytest.mark.parametrize("vt", (VF32, VF64))
def test_reference_min_max_place_nans_and_signed_zeros_by_the_total_order(vt):
    """Every pair and a few larger subsets of the ascending list: MIN is the one that stands first in it, MAX the one that stands last,
    bit for bit, in whatever order the run holds them."""
    from gpusorting_amd.reduce import reduce_by_key_reference as ref, value_from_order_bits, value_order_bits
    asc = F32_ASCENDING if vt == VF32 else f64_ascending()
    ob = value_order_bits(asc.view(NP[vt]), vt)
    assert np.all(ob[1:] > ob[:-1]) and np.array_equal(value_from_order_bits(ob, vt).view(asc.dtype), asc)
    rng = np.random.default_rng(3)
    subsets = [(a, b) for a in range(asc.size) for b in range(asc.size)] + [tuple(rng.choice(asc.size, 5, replace=False)) for _ in range(50)]
    keys = np.concatenate([np.full(len(s), j, np.uint32) for j, s in enumerate(subsets)])
    vals = np.concatenate([asc[list(s)] for s in subsets])
    lo = ref(keys, vals, U32, False, vt, MIN, consecutive=True)[1].view(asc.dtype)
    hi = ref(keys, vals, U32, False, vt, MAX, consecutive=True)[1].view(asc.dtype)
    assert np.array_equal(lo, np.array([asc[min(s)] for s in subsets])) and np.array_equal(hi, np.array([asc[max(s)] for s in subsets]))
    # unlike numpy / torch: a NaN does not poison the minimum, -0.0 lies below +0.0
    pair = np.array([0x7FC00000, 0x3F800000], np.uint32)
    assert ref(np.zeros(2, np.uint32), pair, U32, False, VF32, MIN)[1].view(np.uint32).tolist() == [0x3F800000]
    assert np.isnan(np.minimum.reduce(pair.view(np.float32)))
    zeros = np.array([0x00000000, 0x80000000], np.uint32)
    assert ref(np.zeros(2, np.uint32), zeros, U32, False, VF32, MIN)[1].view(np.uint32).tolist() == [0x80000000]
    assert ref(np.zeros(2, np.uint32), zeros, U32, False, VF32, MAX)[1].view(np.uint32).tolist() == [0]


def test_functional_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd import functional
    k, v = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float32)
    for f in (functional.reduce_by_key, functional.reduce_by_key_consecutive):
        with pytest.raises(ValueError):  # 2-D
            f(torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32))
        with pytest.raises(ValueError):  # lengths
            f(k, torch.zeros(3, dtype=torch.float32))
        for dtype in (torch.int64, torch.float16, torch.int16, torch.float64, torch.uint8):
            with pytest.raises(TypeError, match="reduce_by_key"):
                f(torch.zeros(4, dtype=dtype), v)
        for dtype in (torch.float16, torch.int16, torch.uint8, torch.bool):
            with pytest.raises(TypeError, match="reduce_by_key"):
                f(k, torch.zeros(4, dtype=dtype))
        with pytest.raises(ValueError):
            f(k, v, op="prod")
        with pytest.raises(ValueError):  # not on the device
            f(k, v)
