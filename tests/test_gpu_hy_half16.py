"""GPU tests (-m gpu) of the 16-bit hand-over of the keys-only two-level plan (gpusorting_amd/csrc/hybrid_kernels.hpp, hy_half_slot):
pass B writes only the low 16 bits of every key, as a uint16 into the first half of its bucket's own bytes (PF_HALF16, set by
hy_scan_kernel for keys-only sorts), and hy_local_sort_kernel reads two halfwords per dword and puts the prefix back from its bucket's
number.  Pairs, void plans (the LSD passes) and every other route keep whole keys.

Set-up as tests/test_gpu_hy_classes.py: N = 2^21 + 777 keys (odd), plan 2, the class of the bucket-local sort forced where a bucket has
to reach the class's capacity.  Everything is built in the space of the keys' radix-sortable bits and mapped to the key type at the end,
so prefixes, halves and bucket sizes are exact for uint32, int32 and float32 alike.  Reference: oracle.std_sort; every comparison is
bit-exact on uint32 views (the float inputs hold NaNs of both signs)."""
import numpy as np
import pytest

import hy_bucket_inputs as hb
from guard_arena import Arena

pytestmark = pytest.mark.gpu

MAXK = 1 << 22
OPTIONS = dict(small_path=0, mid_path=0, plan=2, position_chains_min_log2=20)
N = hb.N
CLS = 0
CAP = hb.cap(CLS)
# float32 patterns a sort can get wrong: +-0, +-inf, NaNs of both signs (quiet, signalling, all mantissa bits, low half == high half)
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
                     0xFFFFFFFF, 0x7FFF7FFF, 0xFFFEFFFE], dtype=np.uint32)
HALF_KINDS = ("all_0000", "all_ffff", "own_high_half", "alternating_00ff_ff00")


def _half16(gpu):
    from gpusorting_amd import _lib
    return _lib.GS_PF_HALF16


def _sort(s, keys, vals=None):
    import torch
    dk = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    dv = None if vals is None else torch.from_numpy(vals.view(np.int32).copy()).cuda()
    s.sort(dk, dv)
    s.check()
    return dk.cpu().numpy().view(np.uint32), (None if dv is None else dv.cpu().numpy().view(np.uint32))


def _assert_two_level(s, largest, what):
    """As _assert_ran_two_level of tests/test_gpu_hy_classes.py, for any largest bucket."""
    lp = s.last_plan()
    assert lp["two_level"] and (largest is None or lp["largest_bucket"] == largest), (what, lp, largest)
    r = s.check_state()
    assert (r["rows_not_inclusive"], r["rows_not_monotone"], r["chains_short_of_tickets"], r["hist_words_nonzero"]) == (0, 0, 0, 0), (what, r)
    assert r["keys_per_pass"][:2] == [N, N] and sum(r["keys_per_pass"]) == 2 * N, (what, r)


# ---- inputs (built once per module, never modified) -----------------------------------------------------------------------------------
_cache = {}


def half_kind_bits(kind):
    """Random prefixes (about 32 keys per bucket), low halves of `kind`; the first keys are the float specials' bits, three times each."""
    if ("half", kind) not in _cache:
        rng = np.random.default_rng(77)
        prefix = rng.integers(0, 1 << 16, N, dtype=np.uint32)
        if kind == "all_0000":
            low = np.zeros(N, dtype=np.uint32)
        elif kind == "all_ffff":
            low = np.full(N, 0xFFFF, dtype=np.uint32)
        elif kind == "own_high_half":
            low = prefix.copy()
        else:
            low = np.where(np.arange(N) & 1, 0xFF00, 0x00FF).astype(np.uint32)
        bits = (prefix << np.uint32(16)) | low
        bits[:3 * SPECIALS.size] = hb.to_bits(np.tile(SPECIALS, 3), 2)
        _cache[("half", kind)] = bits
    return _cache[("half", kind)]


FIRST_COUNTS = (1, 0, 3, 2, CAP - 1, 0)   # prefixes 0x0000 .. 0x0005: an empty bucket between two odd ones, an odd one at the first prefix
LAST_COUNTS = (0, 2, 3, 0, 1, CAP - 1)    # prefixes 0xFFFA .. 0xFFFF: ... and the largest, odd, at the last prefix


def edge_bits():
    """Neighbouring prefixes of 0, 1, 2, 3 and cap - 1 keys at the first and at the last prefix, the rest uniform over the prefixes
    between them; one seeded permutation."""
    if "edge" not in _cache:
        rng = np.random.default_rng(78)
        special = [(p, c) for p, c in zip(range(0, 6), FIRST_COUNTS)] + [(p, c) for p, c in zip(range(0xFFFA, 0x10000), LAST_COUNTS)]
        pre = np.concatenate([np.full(c, p, dtype=np.uint32) for p, c in special])
        rest = rng.integers(6, 0xFFFA, N - pre.size, dtype=np.uint32)
        prefix = np.concatenate([pre, rest])
        bits = (prefix << np.uint32(16)) | rng.integers(0, 1 << 16, N, dtype=np.uint32)
        bits = bits[rng.permutation(N)]
        hist = np.bincount(bits >> np.uint32(16), minlength=1 << 16)
        assert tuple(hist[:6]) == FIRST_COUNTS and tuple(hist[-6:]) == LAST_COUNTS and hist.max() == CAP - 1 and N % 2 == 1
        _cache["edge"] = bits
    return _cache["edge"]


@pytest.fixture(scope="module")
def sorter(gpu):
    s = gpu.OneSweep(MAXK, 0, 0, gpu.MODE_KEYS_ONLY, 0, **OPTIONS)
    s.set_hy_class(CLS)
    yield s
    s.close()


# ---- it ran, and only where it should -------------------------------------------------------------------------------------------------
def test_flag_is_set_on_pass_b_of_a_keys_only_two_level_sort_only(gpu, oracle, sorter):
    H = _half16(gpu)
    s = sorter
    s.key_type, s.order = 0, 0
    keys = hb.from_bits(edge_bits(), 0)
    got, _ = _sort(s, keys)
    np.testing.assert_array_equal(got, oracle.std_sort(keys, 0, 0))
    _assert_two_level(s, CAP - 1, "keys only")
    flags = s.pass_flags()
    assert flags[1] & H and not flags[0] & H and not (flags[2] | flags[3]) & H, flags
    # a void plan on the same handle: the LSD passes write whole keys, no word carries the flag, the result is exact
    void = hb.boundary_input(CLS, 0, CAP + 1)
    got, _ = _sort(s, void)
    np.testing.assert_array_equal(got, oracle.std_sort(void, 0, 0))
    assert not s.last_plan()["two_level"]
    assert not any(f & H for f in s.pass_flags()), s.pass_flags()
    # (u32, u32) pairs on the two-level plan: whole keys
    p = gpu.OneSweep(MAXK, 0, 0, gpu.MODE_PAIRS, 4, **OPTIONS)
    try:
        p.set_hy_class(CLS)
        vals = hb.index_values(N, 4)
        gk, gv = _sort(p, keys, vals)
        wk, wv = oracle.std_sort(keys, 0, 0, vals)
        np.testing.assert_array_equal(gk, wk)
        np.testing.assert_array_equal(gv, wv)
        _assert_two_level(p, CAP - 1, "pairs")
        assert not any(f & H for f in p.pass_flags()), p.pass_flags()
    finally:
        p.close()


# ---- halves that can go wrong ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt,order", [(kt, order) for kt in range(3) for order in (0, 1)])
def test_low_halves_that_can_go_wrong(gpu, oracle, sorter, kt, order):
    s = sorter
    s.key_type, s.order = kt, order
    for kind in HALF_KINDS:
        keys = hb.from_bits(half_kind_bits(kind), kt)
        got, _ = _sort(s, keys)
        np.testing.assert_array_equal(got, oracle.std_sort(keys, kt, order), err_msg=f"{kind} kt={kt} order={order}")
        _assert_two_level(s, None, (kind, kt, order))
        assert s.pass_flags()[1] & _half16(gpu)


# ---- bucket sizes at the layout's edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt,order", [(kt, order) for kt in range(3) for order in (0, 1)])
def test_bucket_sizes_at_the_edges_of_the_layout(gpu, oracle, sorter, kt, order):
    """Odd counts leave a stale upper half in the bucket's last dword; an empty bucket sits between two odd ones; the first and the
    last prefix hold 1 and cap - 1 keys (descending mirrors them to the other end of the buffer)."""
    s = sorter
    s.key_type, s.order = kt, order
    keys = hb.from_bits(edge_bits(), kt)
    got, _ = _sort(s, keys)
    np.testing.assert_array_equal(got, oracle.std_sort(keys, kt, order))
    _assert_two_level(s, CAP - 1, (kt, order))


# ---- buffer contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,fill", [(0, 0x00), (0, 0xFF), (1, 0x00), (1, 0xFF)])
def test_nothing_outside_the_buffers_is_touched(gpu, oracle, sorter, order, fill):
    """Key and alternate buffer 16 bytes off a 32-byte boundary inside guard bands, n odd: the halfwords of the last bucket (ascending:
    cap - 1 keys under 0xFFFF; descending: one key under 0x0000) end in the dword nearest the end of the buffer."""
    s = sorter
    kt = 1 + order
    s.key_type, s.order = kt, order
    keys = hb.from_bits(edge_bits(), kt)
    count = N + 3
    arena = Arena.for_views([(count, np.uint32)] * 2, "cuda", fill)
    dk = arena.carve(count, np.uint32, 1 + 2 * order, "keys")
    da = arena.carve(count, np.uint32, 7 + 2 * order, "alt_keys")
    arena.write(dk, keys)
    arena.live(dk, N)
    arena.live(da, N)
    s.sort(dk, n=N, alt_keys=da)
    s.check()
    _assert_two_level(s, CAP - 1, (order, fill))
    np.testing.assert_array_equal(arena.read(dk, np.uint32, N), oracle.std_sort(keys, kt, order))
    arena.verify()


# ---- reuse ----------------------------------------------------------------------------------------------------------------------------
def test_one_handle_two_level_void_descending_ascending(gpu, oracle):
    s = gpu.OneSweep(MAXK, 0, 2, gpu.MODE_KEYS_ONLY, 0, **OPTIONS)
    try:
        s.set_hy_class(CLS)
        kt = 2
        edge = hb.from_bits(edge_bits(), kt)
        void = hb.boundary_input(CLS, kt, CAP + 1)
        for step, (keys, order, two_level) in enumerate(((edge, 0, True), (void, 0, False), (edge, 1, True), (edge, 0, True))):
            s.order = order
            got, _ = _sort(s, keys)
            np.testing.assert_array_equal(got, oracle.std_sort(keys, kt, order), err_msg=f"step {step}")
            if two_level:
                _assert_two_level(s, CAP - 1, step)
                assert s.pass_flags()[1] & _half16(gpu)
            else:
                assert not s.last_plan()["two_level"] and s.check_state()["hist_words_nonzero"] == 0, step
                assert not any(f & _half16(gpu) for f in s.pass_flags()), step
    finally:
        s.close()
