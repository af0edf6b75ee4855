"""GPU tests (-m gpu) of every size class of the two-level plan's bucket-local sorts (hy_local_sort_kernel, hy_local_sort_pairs_kernel;
gpusorting_amd/csrc/hybrid_kernels.hpp) on FULL buckets.  The class of a sort follows n — class 1 starts above 2^27 keys — so at test
sizes only class 0 ever ran, on buckets of a few hundred keys.  gs_debug_set_hy_class (OneSweep.set_hy_class) unties the class from n;
tests/hy_bucket_inputs.py builds 2^21 + 777 keys whose 16-bit-prefix buckets hold exactly the counts at which the kernels change
behaviour: every keys-per-thread value at both edges, cap - 1, cap (the first and the last prefix among them), for every low-bit
pattern that loads one LDS counter or makes a pass an identity.

Reference: oracle.std_sort (std::stable_sort by the keys' radix-sortable bits, descending = its exact reverse), values = input index.
Every comparison is bit-exact, on uint32 views: the float inputs hold NaN patterns of both signs, which the library and the oracle
order by their bits.  The 8-byte values are index | index << 40, derived from the oracle's permutation of the 4-byte index.

The proof that the FORCED class ran — not the one n implies — is test_capacity_boundary_of_every_class: a bucket of exactly the
class's cap runs the plan (largest_bucket == cap), one key more and the same launches fall back."""
import numpy as np
import pytest

import hy_bucket_inputs as hb

pytestmark = pytest.mark.gpu

MAXK = 1 << 22
OPTIONS = dict(small_path=0, mid_path=0, plan=2, position_chains_min_log2=20)
N = hb.N


def built(cls, vb):
    """The registry's rule (kernel_registry.hpp, hy_pairs_built): no 24 576-pair bucket sort with 8-byte values — it does not fit LDS."""
    return not (cls == 3 and vb == 8)


@pytest.fixture(scope="module")
def sorters(gpu):
    made = {}

    def get(vb, kt, order):
        if vb not in made:
            made[vb] = gpu.OneSweep(MAXK, 0, 0, gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb, **OPTIONS)
        s = made[vb]
        s.key_type, s.order = kt, order
        return s
    yield get
    for s in made.values():
        s.close()


# ---- inputs and references, computed once and shared: the cases are ordered so that neighbours use the same ones -------------------
_bits, _refs = {}, {}


def _input(builder, tag, cls, kt, *what):
    """Keys of key type kt; built once per class in the space of the bits (the same for every key type)."""
    if _bits.get("owner") != (tag, cls):
        _bits.clear()
        _bits["owner"] = (tag, cls)
    if what not in _bits:
        _bits[what] = builder(cls, 0, *what)
    return hb.from_bits(_bits[what], kt)


def _reference(oracle, tag, cls, kt, order, keys, *what):
    """(sorted keys, permutation) of the oracle's stable sort, once per class x key type."""
    if _refs.get("owner") != (tag, cls, kt):
        _refs.clear()
        _refs["owner"] = (tag, cls, kt)
    if (order,) + what not in _refs:
        _refs[(order,) + what] = oracle.std_sort(keys, kt, order, hb.index_values(keys.size, 4))
    return _refs[(order,) + what]


def _sort_exact(s, keys, vb, want_keys, perm, what):
    import torch
    dk = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    dv = None
    if vb:
        dv = torch.from_numpy(hb.index_values(keys.size, vb).view(np.int32 if vb == 4 else np.int64)).cuda()
    s.sort(dk, dv)
    s.check()
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), want_keys, err_msg=f"keys {what}")
    if vb == 4:
        np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), perm, err_msg=f"values {what}")
    elif vb == 8:
        p = perm.astype(np.uint64)
        np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint64), p | (p << np.uint64(40)), err_msg=f"values {what}")


def _assert_ran_two_level(s, cap, n, what):
    lp = s.last_plan()
    assert lp["two_level"] and lp["largest_bucket"] == cap, (what, lp, cap)
    r = s.check_state()
    assert (r["rows_not_inclusive"], r["rows_not_monotone"], r["chains_short_of_tickets"], r["hist_words_nonzero"]) == (0, 0, 0, 0), (what, r)
    assert r["keys_per_pass"][:2] == [n, n] and sum(r["keys_per_pass"]) == 2 * n, (what, r)   # pass A, pass B; no LSD pass behind them


def _ladder_case(oracle, s, cls, vb, kt, order, kinds=hb.KINDS, layouts=hb.LAYOUTS):
    s.set_hy_class(cls)
    offered = s.sort_route(N)["hy"]
    assert offered == built(cls, vb), (cls, vb, s.sort_route(N))
    for kind in kinds:
        for layout in layouts:
            what = (cls, vb, kt, order, kind, layout)
            keys = _input(hb.ladder_input, "ladder", cls, kt, kind, layout)
            want_keys, perm = _reference(oracle, "ladder", cls, kt, order, keys, kind, layout)
            _sort_exact(s, keys, vb, want_keys, perm, what)
            if offered:
                _assert_ran_two_level(s, hb.cap(cls), N, what)
            else:
                assert not s.last_plan()["two_level"], what


LADDER_CASES = [(cls, kt, order, vb) for cls in range(4) for kt in range(3) for order in (0, 1) for vb in (0, 4, 8)]


@pytest.mark.parametrize("cls,kt,order,vb", [c for c in LADDER_CASES if built(c[0], c[3])])
def test_every_class_sorts_the_ladder(gpu, oracle, sorters, cls, kt, order, vb):
    """Every compiled bucket-local sort — class x value width x key type, both orders — on the ladder of bucket counts, every low-bit
    kind, permuted and sorted by bits: bit-exact, on the two-level plan, with a largest bucket of exactly the class's cap."""
    _ladder_case(oracle, sorters(vb, kt, order), cls, vb, kt, order)


@pytest.mark.parametrize("cls,kt,order,vb", [c for c in LADDER_CASES if not built(c[0], c[3])])
def test_a_class_without_a_kernel_is_not_offered_the_plan(gpu, oracle, sorters, cls, kt, order, vb):
    """8-byte values, class 3: no kernel.  Forcing the class must not fail the sort: it is not offered the plan and is exact (on the LSD
    passes, which have their own tests: two low-bit kinds — random, and heavy ties for the values' order — suffice here)."""
    _ladder_case(oracle, sorters(vb, kt, order), cls, vb, kt, order, kinds=("uniform", "two_values"))


@pytest.mark.parametrize("cls,vb", [(cls, vb) for cls in range(4) for vb in (0, 4, 8)])
def test_capacity_boundary_of_every_class(gpu, oracle, sorters, cls, vb):
    """One prefix holds exactly cap keys, every other one <= cap / 2: the plan runs.  One key more: the same launches fall back.  Which
    class's cap the device used is thereby pinned from both sides — for the histogram kernel's own verdict (sorted layout: the heavy
    bucket lies inside one workgroup's range) and the scan kernel's (permuted layout)."""
    kt = 0 if cls % 2 == 0 else 2
    cap = hb.cap(cls)
    for order in (0, 1):
        s = sorters(vb, kt, order)
        s.set_hy_class(cls)
        assert s.sort_route(N)["hy"] == built(cls, vb)
        for layout in hb.LAYOUTS:
            for heavy in (cap, cap + 1):
                what = (cls, vb, order, layout, heavy)
                keys = _input(hb.boundary_input, "boundary", cls, kt, heavy, layout)
                want_keys, perm = _reference(oracle, "boundary", cls, kt, order, keys, heavy, layout)
                _sort_exact(s, keys, vb, want_keys, perm, what)
                if heavy == cap and built(cls, vb):
                    _assert_ran_two_level(s, cap, N, what)
                else:
                    assert not s.last_plan()["two_level"], (what, s.last_plan())
                    assert s.check_state()["hist_words_nonzero"] == 0


def test_forced_class_survives_reuse_and_reset(gpu, oracle):
    """One handle, in a row: class 3, class 0, back to "by n" (class 0 at this size), a void sort of class 2, class 2.  The tables,
    slices and slab regions are reused; every sort starts clean and follows the class in force."""
    vb, kt, order = 4, 0, 0
    s = gpu.OneSweep(MAXK, order, kt, gpu.MODE_PAIRS, vb, **OPTIONS)

    def ladder(cls, forced, two_level=True):
        keys = hb.ladder_input(cls, kt)
        want_keys, perm = oracle.std_sort(keys, kt, order, hb.index_values(N, 4))
        _sort_exact(s, keys, vb, want_keys, perm, ("ladder", cls, forced))
        if two_level:
            _assert_ran_two_level(s, hb.cap(cls), N, ("ladder", cls, forced))
        else:
            assert not s.last_plan()["two_level"]
        assert s.check_state()["hist_words_nonzero"] == 0

    s.set_hy_class(3)
    ladder(3, 3)
    s.set_hy_class(0)
    ladder(0, 0)
    s.set_hy_class(-1)
    ladder(0, -1)
    s.set_hy_class(2)
    keys = hb.boundary_input(2, kt, hb.cap(2) + 1)
    want_keys, perm = oracle.std_sort(keys, kt, order, hb.index_values(N, 4))
    _sort_exact(s, keys, vb, want_keys, perm, "class 2, cap + 1")
    assert not s.last_plan()["two_level"] and s.check_state()["hist_words_nonzero"] == 0
    ladder(2, 2)
    s.close()


def test_hook_arguments(gpu, oracle):
    from gpusorting_amd import _lib
    lib = _lib.load()
    assert lib.gs_debug_set_hy_class(None, 0) == _lib.GS_ERR_ARG
    s = gpu.OneSweep(MAXK, **OPTIONS)
    by_n = [s.sort_route(n) for n in ((1 << 20) + 1, N, MAXK)]
    for bad in (-2, 4, 1 << 20):
        assert lib.gs_debug_set_hy_class(s._h, bad) == _lib.GS_ERR_ARG
    for cls in (3, 2, 1, 0, -1):
        assert lib.gs_debug_set_hy_class(s._h, cls) == _lib.GS_OK
        assert [s.sort_route(n) for n in ((1 << 20) + 1, N, MAXK)] == by_n     # keys only: every class has its kernel
    s.close()
    # a handle without the plan's tables (default plan, below the plan's size): forcing a class changes nothing
    p = gpu.OneSweep(MAXK, small_path=0, mid_path=0, position_chains_min_log2=20)
    route = p.sort_route(N)
    p.set_hy_class(2)
    assert p.sort_route(N) == route and not route["hy"]
    keys = hb.ladder_input(2, 0)
    _sort_exact(p, keys, 0, oracle.std_sort(keys, 0, 0), None, "no tables")
    assert not p.last_plan()["two_level"]
    p.close()
