"""CPU tests of the sorted search (gs_search_* in include/gpusort.h, gpusorting_amd/search.py): the symbols are declared, exported and
bound; searchsorted_reference — what the GPU tests compare with — against a brute-force count over the flipped order for all six key
types, both orders and both sides, on inputs with +-0.0, +-inf, NaNs of both signs, the integers' minimum and maximum and all-equal
arrays; gs_search_plan against its Python statement over a grid that brackets every point where S changes and where m crosses T;
gs_search_temp_bytes against the header's formula; and every refusal that is answered before a device is looked for.  A handle cannot
be created without a device, so the refusals that need one (a key type of the wrong width or of 16 bits, route SORT on a handle without
the engine) are in tests/test_gpu_search.py.  No compute is run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32, U64, I64, F64 = range(6)
KEY_TYPES = (U32, I32, F32, U64, I64, F64)
SYMBOLS = ("gs_search_create", "gs_search_destroy", "gs_search_temp_bytes", "gs_search_plan", "gs_search_sorted", "gs_search_set_route",
           "gs_search_set_table", "gs_search_last")

# float patterns the library's order treats unlike a comparison of values: NaNs of both signs with two payloads, infinities, denormals, zeros
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
    top = 1 << (8 * np.dtype(dt).itemsize)
    pool = rng.integers(0, top, distinct or count, dtype=dt)
    body = pool[rng.integers(0, pool.size, count)] if distinct else pool
    sp = specials(kt)
    body[rng.choice(count, min(sp.size, count), replace=False)] = sp[:count]
    return body


def sort_as_library(bits, kt, descending):
    """`bits` in the order the library's sort leaves them (the numpy statement of it: the sortable bits, ascending, then reversed)."""
    from gpusorting_amd.search import _words
    return bits[np.argsort(_words(bits, kt, False), kind="stable")][::-1 if descending else 1].copy()


def brute_force(hay, queries, kt, descending, right):
    """The table of the header, counted: keys strictly below / below or equal (ascending), strictly above / above or equal (descending),
    with below and above taken in the flipped domain by a restatement of the flip that shares no code with the package."""
    def flip(bits):
        b = bits.astype(object)  # python integers: no overflow, no numpy promotion
        width = 8 * bits.dtype.itemsize
        top, full = 1 << (width - 1), (1 << width) - 1
        if kt in (I32, I64):
            return [x ^ top for x in b]
        if kt in (F32, F64):
            return [x ^ (full if x & top else top) for x in b]
        return list(b)

    h, q = flip(hay), flip(queries)
    out = []
    for x in q:
        if descending:
            out.append(sum(1 for y in h if (y >= x if right else y > x)))
        else:
            out.append(sum(1 for y in h if (y <= x if right else y < x)))
    return np.array(out, dtype=np.uint32)


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpusort.h")).read(), flags=re.S)


def test_symbols_constants_and_exports():
    from gpusorting_amd import _lib
    lib = _lib.load()
    text = header_text()
    assert set(re.findall(r"\b(gs_search_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libgpusort.so does not export {name}"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound"
    defines = dict(re.findall(r"#define\s+(GS_SEARCH_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert {"GS_SEARCH_ROUTE_TILE", "GS_SEARCH_P_WINDOW", "GS_SEARCH_R_PLAN", "GS_SEARCH_SORT_MIN_KEYS"} <= set(defines)
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    assert (_lib.GS_SEARCH_LEFT, _lib.GS_SEARCH_RIGHT) == (0, 1)
    assert _lib.GS_SEARCH_R_PLAN + _lib.GS_SEARCH_PLAN_WORDS <= _lib.GS_SEARCH_REPORT_WORDS
    import gpusorting_amd as g
    from gpusorting_amd import functional, search
    assert g.SortedSearch is search.SortedSearch and g.searchsorted_reference is search.searchsorted_reference
    assert g.search_plan is search.search_plan and g.searchsorted is functional.searchsorted and g.bucketize is functional.bucketize
    assert (search.ROUTE_TILE, search.ROUTE_SORT, search.ROUTE_BINARY) == (_lib.GS_SEARCH_ROUTE_TILE, _lib.GS_SEARCH_ROUTE_SORT, _lib.GS_SEARCH_ROUTE_BINARY)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("descending", (False, True), ids=("asc", "desc"))
@pytest.mark.parametrize("kt", KEY_TYPES)
def test_reference_against_a_brute_force_count(kt, descending, right):
    from gpusorting_amd import searchsorted_reference
    hay = sort_as_library(draws(kt, 150, 10 + kt, distinct=40), kt, descending)      # duplicates, every special
    queries = np.concatenate([draws(kt, 60, 20 + kt), hay[::7], specials(kt)])       # in no order: hits, misses, every special
    got = searchsorted_reference(hay, queries, kt, descending, right)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, brute_force(hay, queries, kt, descending, right))
    # all equal: LEFT and RIGHT of the key differ by the length; of a key in front of it both are 0, behind it both n
    one = specials(kt)[3]
    same = np.full(33, one, dtype=word_dtype(kt))
    np.testing.assert_array_equal(searchsorted_reference(same, same[:2], kt, descending, right), [33 if right else 0] * 2)
    np.testing.assert_array_equal(searchsorted_reference(same, queries, kt, descending, right), brute_force(same, queries, kt, descending, right))


def test_reference_hand_worked_cases():
    from gpusorting_amd import searchsorted_reference as ref
    f = lambda *v: np.array(v, dtype=np.float32)  # noqa: E731
    hay = f(-np.inf, -1.0, -0.0, 0.0, 0.0, 2.0, np.inf, np.nan)  # ascending in the library's order (+NaN last)
    np.testing.assert_array_equal(ref(hay, f(-0.0, 0.0, 1.0, np.nan, -np.nan), F32), [2, 3, 5, 7, 0])
    np.testing.assert_array_equal(ref(hay, f(-0.0, 0.0, 1.0, np.nan, -np.nan), F32, right=True), [3, 5, 5, 8, 0])
    np.testing.assert_array_equal(ref(hay[::-1].copy(), f(-0.0, 0.0, 1.0, np.nan, -np.nan), F32, descending=True), [5, 3, 3, 0, 8])
    np.testing.assert_array_equal(ref(hay[::-1].copy(), f(-0.0, 0.0, 1.0), F32, descending=True, right=True), [6, 5, 3])
    ints = np.array([-5, -5, 0, 3, 3, 3, 9], dtype=np.int32)
    q = np.array([-6, -5, 3, 4, 9, 10], dtype=np.int32)
    for right in (False, True):
        np.testing.assert_array_equal(ref(ints, q, I32, right=right), np.searchsorted(ints, q, "right" if right else "left"))
    assert ref(ints, q[:0], I32).size == 0 and ref(ints[:0], q, I32).tolist() == [0] * 6
    with pytest.raises(ValueError):
        ref(ints, q, U64)
    with pytest.raises(ValueError):
        ref(ints.astype(np.int16), q.astype(np.int16), 7)  # KEY_INT16


def plan_grid():
    """(n, m, key_bytes): n one below, at and one above every point where S changes (ceil(n / S) crosses the table's capacity), m
    around T and on either side of the AUTO rule's constants."""
    from gpusorting_amd import _lib
    tm, sm, sk = _lib.GS_SEARCH_TABLE_MIN_QUERIES, _lib.GS_SEARCH_SORT_MIN_QUERIES, _lib.GS_SEARCH_SORT_MIN_KEYS
    for kb in (4, 8):
        cap = 65536 // kb
        ns = {1, 2, 63, 64, 65, sk - 1, sk, (1 << 30) - 1}
        s = 1
        while cap * s < (1 << 30):
            ns |= {cap * s - 1, cap * s, cap * s + 1}
            s *= 2
        for n in sorted(x for x in ns if 0 < x < (1 << 30)):
            for m in (1, 2047, 2048, 2049, 2 * 2048 + 3, tm - 1, tm, sm - 1, sm, (1 << 30) - 1):
                yield n, m, kb


def test_plan_against_its_python_statement():
    from gpusorting_amd import _lib, search_plan, search_plan_reference
    lib = _lib.load()
    count = 0
    for n, m, kb in plan_grid():
        got, want = search_plan(n, m, kb), search_plan_reference(n, m, kb)
        assert got == want, (n, m, kb)
        cap = 65536 // kb
        s, ns = got["stride"], got["samples"]
        assert s & (s - 1) == 0 and -(-n // s) <= cap and (s == 1 or -(-n // (s // 2)) > cap), (n, kb)  # the smallest power of two that fits
        assert ns == n // s <= cap and got["window"] == 32768 // kb and got["tile_grid"] == -(-m // got["tile"])
        count += 1
    assert count > 500
    # S changes exactly behind a full table
    assert [search_plan(n, 1, 4)["stride"] for n in (16384, 16385, 32768, 32769)] == [1, 2, 2, 4]
    assert [search_plan(n, 1, 8)["stride"] for n in (8192, 8193, 16384, 16385)] == [1, 2, 2, 4]
    plan = (C.c_uint32 * _lib.GS_SEARCH_PLAN_WORDS)()
    A, S = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE
    assert lib.gs_search_plan(1024, 1024, 4, None) == A
    for kb in (0, 2, 3, 16):
        assert lib.gs_search_plan(1024, 1024, kb, plan) == A, kb
    for n, m in ((0, 1), (1, 0), (1 << 30, 1), (1, 1 << 30)):
        assert lib.gs_search_plan(n, m, 4, plan) == S, (n, m)
        assert lib.gs_search_plan(n, m, 2, plan) == S, (n, m)  # the sizes are looked at first, as gs_search_create does
    with pytest.raises(ValueError):
        search_plan_reference(0, 1)


def _up(x):
    return (x + 255) & ~255


def test_temp_bytes_is_the_formula_of_the_header():
    from gpusorting_amd import _lib
    from gpusorting_amd.search import temp_bytes
    lib = _lib.load()
    for kb in (4, 8):
        for mq in (1, 63, 64, 65, 4097, 65536, (1 << 20) + 1, (1 << 30) - 1):
            for mk in (1, 1 << 20, (1 << 30) - 1):
                small = _up(64 * 4) + _up(65536)
                assert lib.gs_search_temp_bytes(mk, mq, kb, 0) == small == temp_bytes(mk, mq, kb, False)  # only the control block and the table
                want = small + 2 * _up(kb * mq) + 2 * _up(4 * mq) + lib.gs_onesweep_temp_bytes(mq)
                assert lib.gs_search_temp_bytes(mk, mq, kb, 1) == want == temp_bytes(mk, mq, kb, True), (kb, mq)
    for args in ((0, 1, 4, 0), (1, 0, 4, 0), (1 << 30, 1, 4, 0), (1, 1 << 30, 8, 1), (1024, 1024, 2, 0), (1024, 1024, 0, 0), (1024, 1024, 4, 2),
                 (1024, 1024, 4, -1)):
        assert lib.gs_search_temp_bytes(*args) == 0, args


def test_refusals_answered_before_a_device_is_looked_for():
    from gpusorting_amd import _lib
    lib = _lib.load()
    A, S = _lib.GS_ERR_ARG, _lib.GS_ERR_SIZE
    h = C.c_void_p()
    assert lib.gs_search_create(None, 1024, 1024, 4, 0) == A
    for mk, mq in ((0, 1024), (1024, 0), (1 << 30, 1024), (1024, 1 << 30)):
        assert lib.gs_search_create(C.byref(h), mk, mq, 4, 1) == S, (mk, mq)
    assert lib.gs_search_create(C.byref(h), 0, 1024, 2, 0) == S  # the sizes are looked at first
    for kb in (2, 0, 1, 3, 16):  # 2: the 16-bit key types are a follow-up
        assert lib.gs_search_create(C.byref(h), 1024, 1024, kb, 0) == A, kb
    for sq in (2, -1):
        assert lib.gs_search_create(C.byref(h), 1024, 1024, 4, sq) == A, sq
    assert not h.value
    # every handle entry answers a null handle first, whatever else it is given: plausible arguments, 16-bit key types, route SORT
    buf = (C.c_uint32 * 32768)()
    p = (C.addressof(buf) + 15) & ~15
    rep = C.cast(buf, C.POINTER(C.c_uint32))
    assert lib.gs_search_destroy(None) == A
    for kt in range(10):
        for order in (0, 1):
            for side in (0, 1):
                assert lib.gs_search_sorted(None, p, 1024, p + 16384, 1024, p + 32768, kt, order, side, 0, None) == A
    for route in range(5):
        assert lib.gs_search_set_route(None, route) == A and lib.gs_search_set_table(None, route) == A
    assert lib.gs_search_last(None, rep, 32768, None) == A


def test_functional_argument_errors_that_need_no_device():
    import torch
    import gpusorting_amd as g
    hay = torch.arange(8, dtype=torch.int32)
    with pytest.raises(TypeError):
        g.searchsorted(hay.to(torch.int16), hay.to(torch.int16))  # 16-bit keys: a follow-up
    with pytest.raises(TypeError):
        g.searchsorted(hay, hay.to(torch.int64))
    with pytest.raises(ValueError):
        g.searchsorted(hay.reshape(2, 4), hay)
    with pytest.raises(ValueError):
        g.searchsorted(hay, hay)  # not on a GPU
    with pytest.raises(ValueError):
        g.bucketize(hay, hay)
