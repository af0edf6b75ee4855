"""The builder of tests/few_valued_inputs.py at small n, without a GPU: counts, expectation, border offsets, and that its torch form
(on the CPU here) and its numpy twin agree."""
import numpy as np
import pytest

import few_valued_inputs as fv

N_SMALL = (1 << 16, (1 << 16) + 12_345)  # 5000 keys off n / 2 needs n > 10 000


def _check(keys, expected, counts, n, v):
    assert keys.dtype == np.uint32 and expected.dtype == np.uint32 and keys.shape == expected.shape == (n,)
    assert len(counts) == v and sum(counts) == n
    vals, got = np.unique(keys, return_counts=True)
    present = [c for c in counts if c]
    assert got.tolist() == present  # the counts are exact (values ascend, so np.unique lists them in the builder's order)
    assert np.all(expected[1:] >= expected[:-1])  # sorted ...
    ve, ge = np.unique(expected, return_counts=True)
    assert ve.tolist() == vals.tolist() and ge.tolist() == got.tolist()  # ... and a permutation of the input


def test_pools_have_31_bits_and_no_shared_byte_between_neighbours():
    for v in (2, 3, 16):
        p = fv.pool(v)
        assert p.dtype == np.uint32 and p.shape == (v,) and int(p.max()) < 1 << 31
        assert np.all(p[1:] > p[:-1])
        for a, b in zip(p[:-1].tolist(), p[1:].tolist()):
            assert all(((a >> s) & 255) != ((b >> s) & 255) for s in (0, 8, 16, 24)), (hex(a), hex(b))
    assert fv.pool(2).tolist() == [0x277B4B58, 0x3E121E97]


def test_seglog_is_the_scan_kernels():
    for n, want in ((1 << 28, 24), (1 << 27, 23), (1 << 22, 18), ((1 << 22) + 12_345, 19), (1 << 20, 16), (17, 1), (16, 1), (33, 2)):
        assert fv.seglog(n) == want, n
        assert (16 << fv.seglog(n)) >= n


@pytest.mark.parametrize("n", N_SMALL)
@pytest.mark.parametrize("layout", fv.LAYOUTS)
def test_numpy_form(layout, n):
    v, fixed = fv.layout_counts(layout, n)
    keys, expected, counts = fv.build_numpy(layout, n, seed=3)
    _check(keys, expected, counts, n, v)
    if fixed is not None:
        assert counts == fixed
    else:  # every key drawn uniformly: each count within six standard deviations of n / v
        sd = (n * (1 / v) * (1 - 1 / v)) ** 0.5
        assert all(abs(c - n / v) <= 6 * sd for c in counts), counts
    if layout == "presorted":
        assert np.array_equal(keys, expected)
    else:
        assert not np.array_equal(keys, expected)
    again = fv.build_numpy(layout, n, seed=3)
    assert np.array_equal(again[0], keys) and again[2] == counts  # seeded
    if fixed is None:
        assert not np.array_equal(fv.build_numpy(layout, n, seed=4)[0], keys)


def test_border_offsets_are_the_requested_ones():
    n = 1 << 20  # n / 2 = 8 << seglog, n / 16 = 1 << seglog, and half a segment is more than 5000 keys
    assert fv.seglog(n) == 16
    for d in fv.EXACT_OFFSETS:
        _, _, counts = fv.build_numpy(f"two_exact({d})", n)
        assert counts == [n // 2 + d, n // 2 - d]
        assert fv.border_offsets(counts, n) == [d]
    _, _, counts = fv.build_numpy("sixteen_exact", n)
    assert counts == [n // 16] * 16 and fv.border_offsets(counts, n) == [0] * 15
    _, _, counts = fv.build_numpy("presorted", n)
    assert fv.border_offsets(counts, n) == [0] * 15
    # the control: shares 1/2, 1/3, 1/6 put the second border a third of a segment away from every segment border — but the first one,
    # at n / 2, ON one: the layout separates "a border near a segment border" from "every border near one", not from "none"
    _, _, counts = fv.build_numpy("three_values", n)
    assert counts == [n // 2, n // 3, n - n // 2 - n // 3]
    offs = fv.border_offsets(counts, n)
    assert offs[0] == 0 and abs(offs[1]) > (1 << 16) // 4  # (the first border, n / 2, is a segment border; the second is not)
    # the random layouts: within six standard deviations of a segment border, i.e. about sqrt(n)
    for layout, v in (("two_random", 2), ("sixteen_random", 16)):
        _, _, counts = fv.build_numpy(layout, n, seed=1)
        assert all(abs(o) <= 6 * (n * 0.25) ** 0.5 for o in fv.border_offsets(counts, n)), layout


@pytest.mark.parametrize("layout", fv.LAYOUTS)
def test_torch_and_numpy_forms_agree(layout):
    torch = pytest.importorskip("torch")
    n = N_SMALL[1]
    tk, te, tc = fv.build_torch(layout, n, torch.device("cpu"), seed=5)
    assert tk.dtype == torch.int32 and te.dtype == torch.int32 and tk.shape == te.shape == (n,)
    tk, te = tk.numpy().view(np.uint32), te.numpy().view(np.uint32)
    v, fixed = fv.layout_counts(layout, n)
    _check(tk, te, tc, n, v)
    nk, ne, nc = fv.build_numpy(layout, n, seed=5)
    if fixed is not None:  # counts fixed by n: the same counts, the same expectation, inputs that are permutations of each other
        assert tc == nc == fixed and np.array_equal(te, ne)
        assert np.array_equal(np.sort(tk), np.sort(nk))
        if layout == "presorted":
            assert np.array_equal(tk, nk)
    else:  # drawn: each form states its own counts; both use the same values
        assert np.unique(tk).tolist() == np.unique(nk).tolist() == fv.pool(v).tolist()
    t2 = fv.build_torch(layout, n, torch.device("cpu"), seed=5)
    assert torch.equal(t2[0].view(torch.int32), torch.from_numpy(tk.view(np.int32))) and t2[2] == tc  # seeded


def test_values_can_be_replaced_in_the_callers_order():
    vals = [0x80000000, 0x00000000]  # -0.0 in front of +0.0: the float order, not the unsigned one
    keys, expected, counts = fv.build_numpy("two_exact(0)", 1 << 12, values=vals)
    assert expected[:counts[0]].tolist() == [0x80000000] * counts[0] and expected[-1] == 0
    assert sorted(np.unique(keys).tolist()) == [0, 0x80000000]
    with pytest.raises(AssertionError):
        fv.build_numpy("two_exact(0)", 64, values=[7, 7])
