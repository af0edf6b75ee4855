"""CPU tests of the merge (gs_merge_* in include/gpusort.h, gpusorting_amd/_merge.py): the symbols are declared, exported and bound;
merge_reference — what the GPU tests compare with — against a brute-force statement that shares no code with the package (Python's
sorted over (word, side, index) tuples, the flip restated here) for all six key types and both orders, on draws with NaNs of both signs,
+-inf, +-0.0, the integers' extremes and many duplicates; hand-worked float cases; gs_merge_plan against its Python statement;
gs_merge_temp_bytes against the header's formula; every refusal that is answered before a device is looked for, in the header's order;
the tensor functions' argument errors that need no device; and that the package gained one privately named module and no other.  No
compute is run."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32, U64, I64, F64 = range(6)
KEY_TYPES = (U32, I32, F32, U64, I64, F64)
SYMBOLS = ("gs_merge_create", "gs_merge_destroy", "gs_merge_temp_bytes", "gs_merge_plan", "gs_merge_keys", "gs_merge_pairs",
           "gs_merge_positions", "gs_merge_last")
MAX_KEYS = (1 << 30) - 1

F32_SPECIALS = np.array([0xFFC00001, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000002, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
                         0x00000002, 0x3F800000, 0x7F800000, 0x7FC00000, 0x7FC00001], dtype=np.uint32)
F64_SPECIALS = np.array([0xFFF8000000000001, 0xFFF8000000000000, 0xFFF0000000000000, 0xBFF0000000000000, 0x8000000000000002,
                         0x8000000000000001, 0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x0000000000000002,
                         0x3FF0000000000000, 0x7FF0000000000000, 0x7FF8000000000000, 0x7FF8000000000001], dtype=np.uint64)
INT_EDGES = {U32: [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], I32: [0x80000000, 0x80000001, 0xFFFFFFFF, 0, 1, 0x7FFFFFFF],
             U64: [0, 1, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF, 0x00000001FFFFFFFF, 0x0000000200000000],
             I64: [0x8000000000000000, 0x8000000000000001, 0xFFFFFFFFFFFFFFFF, 0, 1, 0x7FFFFFFFFFFFFFFF, 0x00000001FFFFFFFF, 0x0000000200000000]}


def word_dtype(kt):
    return np.uint64 if kt >= U64 else np.uint32


def specials(kt):
    """The bit patterns every draw of key type kt contains."""
    if kt == F32:
        return F32_SPECIALS
    if kt == F64:
        return F64_SPECIALS
    return np.array(INT_EDGES[kt], dtype=word_dtype(kt))


def draws(kt, count, seed, distinct=0):
    """`count` bit patterns of key type kt: the specials, and random patterns over the whole word (distinct > 0: drawn from that many)."""
    rng = np.random.default_rng(seed)
    dt = word_dtype(kt)
    pool = rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), distinct or count, dtype=dt)
    body = pool[rng.integers(0, pool.size, count)] if distinct else pool
    sp = specials(kt)
    body[rng.choice(count, min(sp.size, count), replace=False)] = sp[:count]
    return body


def flipped(bits, kt, descending):
    """The words of `bits` as Python integers: a restatement of the flip that shares no code with the package."""
    width = 8 * bits.dtype.itemsize
    top, full = 1 << (width - 1), (1 << width) - 1
    out = []
    for x in bits.astype(object):
        if kt in (I32, I64):
            x ^= top
        elif kt in (F32, F64):
            x ^= full if x & top else top
        out.append(full - x if descending else x)
    return out


def sort_as_library(bits, kt, descending):
    """`bits` in the order the library's sort leaves them, by the restated flip."""
    w = flipped(bits, kt, descending)
    return bits[np.array(sorted(range(bits.size), key=lambda i: w[i]), dtype=np.int64)].copy() if bits.size else bits.copy()


def brute_force(a, b, kt, descending):
    """(keys, src): Python's sorted over (word, side, index): A's elements first among equal words, each side in its input order."""
    wa, wb = flipped(a, kt, descending), flipped(b, kt, descending)
    order = sorted([(w, 0, i) for i, w in enumerate(wa)] + [(w, 1, j) for j, w in enumerate(wb)])
    src = np.array([i if side == 0 else a.size + i for _, side, i in order], dtype=np.uint32)
    return np.concatenate([a, b])[src.astype(np.int64)], src


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib, _merge
    lib = _lib.load()
    text = header_text()
    assert set(re.findall(r"\b(gs_merge_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_MERGE_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert {"GS_MERGE_FORM_POSITIONS", "GS_MERGE_P_LDS_BYTES", "GS_MERGE_R_PLAN", "GS_MERGE_R_COPY_TILES"} <= set(defines)
    for name, value in defines.items():
        assert getattr(_merge, name) == int(value), name  # the constants live in the new module, not in _lib
        assert not hasattr(_lib, name), name
    assert _merge.GS_MERGE_R_PLAN + _merge.GS_MERGE_PLAN_WORDS <= _merge.GS_MERGE_REPORT_WORDS
    assert len(_merge._PLAN) <= _merge.GS_MERGE_PLAN_WORDS and len(_merge._REPORT) <= _merge.GS_MERGE_R_PLAN


@pytest.mark.parametrize("descending", (False, True), ids=("asc", "desc"))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_reference_against_a_brute_force_merge(kt, descending):
    from gpusorting_amd._merge import merge_reference
    a = sort_as_library(draws(kt, 150, 10 + kt, distinct=40), kt, descending)  # duplicates inside and across the sides, every special
    b = sort_as_library(np.concatenate([draws(kt, 90, 20 + kt, distinct=40), a[::5], specials(kt)]), kt, descending)
    va, vb = np.arange(a.size, dtype=np.uint32) * 3 + 1, np.arange(b.size, dtype=np.uint32) * 5 + 2
    for x, y, vx, vy in ((a, b, va, vb), (b, a, vb, va), (a, a[:0], va, va[:0]), (a[:0], b, vb[:0], vb)):
        keys, src = merge_reference(x, y, kt, descending)
        want_keys, want_src = brute_force(x, y, kt, descending)
        assert src.dtype == np.uint32 and keys.dtype == x.dtype
        np.testing.assert_array_equal(src, want_src)
        np.testing.assert_array_equal(keys, want_keys)
        k2, s2, vals = merge_reference(x, y, kt, descending, vx, vy)
        np.testing.assert_array_equal(k2, want_keys)
        np.testing.assert_array_equal(s2, want_src)
        np.testing.assert_array_equal(vals, np.concatenate([vx, vy])[want_src.astype(np.int64)])
    one = specials(kt)[3]  # both sides all equal: every A in front of every B
    same = np.full(33, one, dtype=word_dtype(kt))
    keys, src = merge_reference(same, same[:7], kt, descending)
    np.testing.assert_array_equal(src, np.arange(40))
    np.testing.assert_array_equal(keys, np.full(40, one, dtype=word_dtype(kt)))


def test_reference_hand_worked_cases():
    from gpusorting_amd._merge import merge_reference as ref
    f = lambda *v: np.array(v, dtype=np.float32)  # noqa: E731
    bits = lambda x: np.asarray(x).view(np.uint32).tolist()  # noqa: E731
    # -0.0 and +0.0 are two keys: across the sides -0.0 comes first wherever it lies
    keys, src = ref(f(-1.0, 0.0, 2.0), f(-0.0, 0.0, 3.0), F32)
    assert src.tolist() == [0, 3, 1, 4, 2, 5] and bits(keys) == bits(f(-1.0, -0.0, 0.0, 0.0, 2.0, 3.0))
    keys, src = ref(f(-0.0, 1.0), f(-0.0, 0.0), F32)
    assert src.tolist() == [0, 2, 3, 1] and bits(keys) == bits(f(-0.0, -0.0, 0.0, 1.0))
    # equal NaNs: A's first; -NaN in front of everything, +NaN behind +inf
    keys, src = ref(f(-np.nan, 1.0, np.inf, np.nan), f(-np.nan, np.inf, np.nan, np.nan), F32)
    assert src.tolist() == [0, 4, 1, 2, 5, 3, 6, 7]
    assert bits(keys) == bits(f(-np.nan, -np.nan, 1.0, np.inf, np.inf, np.nan, np.nan, np.nan))
    # descending: the same rule on the inverted words
    keys, src = ref(f(np.nan, 2.0, 0.0, -0.0), f(np.nan, 0.0, -0.0, -np.inf), F32, descending=True)
    assert src.tolist() == [0, 4, 1, 2, 5, 3, 6, 7]
    ints = np.array([-5, -5, 0, 3, 3, 9], dtype=np.int32)
    more = np.array([-6, -5, 3, 4, 10], dtype=np.int32)
    keys, src, vals = ref(ints, more, I32, a_values=np.arange(6, dtype=np.int64), b_values=np.arange(100, 105, dtype=np.int64))
    assert keys.tolist() == [-6, -5, -5, -5, 0, 3, 3, 3, 4, 9, 10] and src.tolist() == [6, 0, 1, 7, 2, 3, 4, 8, 9, 5, 10]
    assert vals.tolist() == [100, 0, 1, 101, 2, 3, 4, 102, 103, 5, 104]
    assert ref(ints, ints[:0], I32)[1].tolist() == list(range(6)) and ref(ints[:0], ints, I32)[0].tolist() == ints.tolist()
    with pytest.raises(ValueError):
        ref(ints, more, U64)
    with pytest.raises(ValueError):
        ref(ints.astype(np.int16), more.astype(np.int16), 7)  # KEY_INT16
    with pytest.raises(ValueError):
        ref(ints, more.astype(np.uint32), I32)
    with pytest.raises(ValueError):
        ref(ints, more, I32, a_values=np.arange(6))


def test_plan_against_its_python_statement():
    from gpusorting_amd import _lib
    from gpusorting_amd._merge import GS_MERGE_PLAN_WORDS, merge_plan, merge_plan_reference
    lib = _lib.load()
    count = 0
    for kb in (4, 8):
        T = merge_plan(1, 0, kb)["tile"]
        sizes = {1, 2, MAX_KEYS - 1, MAX_KEYS}
        for mult in (1, 2, 3, 5, 1000):
            sizes |= {mult * T - 1, mult * T, mult * T + 1}
        for n in sorted(sizes):
            for na in sorted({0, 1, n // 2, n // 65, n - 1, n}):
                got, want = merge_plan(na, n - na, kb), merge_plan_reference(na, n - na, kb)
                assert got == want, (na, n - na, kb)
                assert got["grid"] == -(-n // T) and got["tile"] == got["vt"] * got["threads"] and got["threads"] == 512
                assert got["lds_bytes"] <= 160 * 1024 // 2 and got["vt"] % 4 == 0
                count += 1
    assert count > 150
    plan = (C.c_uint32 * GS_MERGE_PLAN_WORDS)()
    A, S = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE
    assert lib.gs_merge_plan(1024, 1024, 4, None) == A
    for kb in (0, 2, 3, 16):
        assert lib.gs_merge_plan(1024, 1024, kb, plan) == A, kb
    for na, nb in ((0, 0), (1 << 30, 0), (0, 1 << 30), (1 << 29, 1 << 29), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 0x80000000)):
        assert lib.gs_merge_plan(na, nb, 4, plan) == S, (na, nb)   # the last three: the sum overflows 32 bits
        assert lib.gs_merge_plan(na, nb, 2, plan) == S, (na, nb)   # the sizes are looked at first, as gs_merge_create does
    assert lib.gs_merge_plan(MAX_KEYS, 0, 8, plan) == 0 and lib.gs_merge_plan(0, MAX_KEYS, 4, plan) == 0
    for bad in ((0, 0), (MAX_KEYS, 1), (-1, 2)):
        with pytest.raises(ValueError):
            merge_plan_reference(*bad)


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    from gpusorting_amd._merge import temp_bytes
    lib = _lib.load()
    for kb in (4, 8):
        for mk in (1, 4097, 1 << 20, MAX_KEYS):
            assert lib.gs_merge_temp_bytes(mk, kb) == 32 * 128 == temp_bytes(mk, kb)  # the control block: nothing grows with max_keys
    for args in ((0, 4), (1 << 30, 4), (1024, 2), (1024, 0), (1024, 16)):
        assert lib.gs_merge_temp_bytes(*args) == 0, args


def test_refusals_answered_before_a_device_is_looked_for():
    from gpusorting_amd import _lib
    from gpusorting_amd._merge import GS_MERGE_REPORT_WORDS
    lib = _lib.load()
    A, S = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE
    h = C.c_void_p()
    assert lib.gs_merge_create(None, 1024, 4) == A
    for mk in (0, 1 << 30, 0xFFFFFFFF):
        assert lib.gs_merge_create(C.byref(h), mk, 4) == S, mk
    assert lib.gs_merge_create(C.byref(h), 0, 2) == S  # the sizes are looked at first
    for kb in (2, 0, 1, 3, 16):  # 2: the 16-bit key types are a follow-up
        assert lib.gs_merge_create(C.byref(h), 1024, kb) == A, kb
    assert not h.value
    # every handle entry answers a null handle first, whatever else it is given: plausible arguments, 16-bit key types, sizes whose sum
    # overflows 32 bits, value widths nobody has
    buf = (C.c_uint32 * 32768)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    assert lib.gs_merge_destroy(None) == A
    for kt in range(10):
        for order in (0, 1, 2):
            for na, nb in ((512, 512), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF)):
                assert lib.gs_merge_keys(None, p, na, p + 4096, nb, p + 8192, kt, order, None) == A
                assert lib.gs_merge_positions(None, p, na, p + 4096, nb, p + 8192, p + 16384, kt, order, None) == A
                for vb in (4, 8, 2, 0):
                    assert lib.gs_merge_pairs(None, p, p + 32768, na, p + 4096, p + 36864, nb, p + 8192, p + 16384, vb, kt, order, None) == A
    assert lib.gs_merge_last(None, rep, GS_MERGE_REPORT_WORDS, None) == A


def test_tensor_functions_argument_errors_that_need_no_device():
    import torch
    from gpusorting_amd._merge import argmerge, merge, merge_by_key
    a = torch.arange(8, dtype=torch.int32)
    for fn in (merge, argmerge):
        with pytest.raises(TypeError, match="follow-up"):
            fn(a.to(torch.int16), a.to(torch.int16))  # 16-bit keys
        with pytest.raises(TypeError, match="follow-up"):
            fn(a.to(torch.bfloat16), a.to(torch.bfloat16))
        with pytest.raises(TypeError):
            fn(a, a.to(torch.int64))
        with pytest.raises(TypeError):
            fn(a.to(torch.uint8), a.to(torch.uint8))
        with pytest.raises(TypeError):
            fn(a, a.numpy())
        with pytest.raises(ValueError):
            fn(a.reshape(2, 4), a)
        with pytest.raises(ValueError):
            fn(a, a)  # not on a GPU
    v = torch.arange(8, dtype=torch.float32)
    with pytest.raises(TypeError, match="follow-up"):
        merge_by_key(a.to(torch.float16), v, a.to(torch.float16), v)
    with pytest.raises(TypeError):
        merge_by_key(a, v, a, v.to(torch.float64))  # one value dtype for both sides
    with pytest.raises(TypeError):
        merge_by_key(a, v.to(torch.float16), a, v.to(torch.float16))  # 2-byte values
    with pytest.raises(TypeError):
        merge_by_key(a, None, a, v)
    with pytest.raises(ValueError):
        merge_by_key(a, v[:5], a, v)  # one value per key
    with pytest.raises(ValueError):
        merge_by_key(a, v, a, v)  # not on a GPU


def test_the_package_gained_one_private_module_and_no_public_name():
    """Why the module is called _merge: the fixture of tests/test_python_api_cpu.py pins every module's public names and lets a new
    module in only under a private name."""
    spec = importlib.util.spec_from_file_location("dump_python_api", os.path.join(ROOT, "tools", "dump_python_api.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got = tool.dump()["modules"]
    with open(os.path.join(ROOT, "tests", "golden", "python_api.json")) as f:
        want = json.load(f)["modules"]
    assert "gpusorting_amd._merge" in got
    assert sorted(set(got) - set(want)) == ["gpusorting_amd._handle", "gpusorting_amd._merge"]  # (_handle: the wrappers' base, there before)
    for name in ("merge", "merge_by_key", "argmerge", "Merge", "merge_reference", "merge_plan", "merge_plan_reference"):
        assert name in got["gpusorting_amd._merge"], name
        for module in ("gpusorting_amd", "gpusorting_amd.functional", "gpusorting_amd._lib"):
            assert name not in got[module], (module, name)
    assert not [n for n in got["gpusorting_amd._lib"] if n.startswith("GS_MERGE")]
