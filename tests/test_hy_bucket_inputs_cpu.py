"""CPU tests of tests/hy_bucket_inputs.py: the builder of exact bucket sizes is held to its own promises where there is no GPU —
the GPU tests that sort its inputs (tests/test_gpu_hy_classes.py, the ledger's class cases) rely on "exactly cap keys under one
prefix" to prove which size class of the bucket-local sort ran."""
import numpy as np
import pytest

import hy_bucket_inputs as hb


def test_classes_restate_the_registry():
    """g_hy_class of kernel_registry.hpp, restated on purpose (as tests/registry_cases.py restates the registry's rules)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "gpusorting_amd", "csrc", "kernel_registry.hpp")).read()
    line = next(ln for ln in text.splitlines() if "constexpr HyLocalClass g_hy_class[4]" in ln)
    shapes = tuple((int(t), int(k)) for t, k in re.findall(r"\{[^{},]+,\s*(\d+),\s*(\d+)\}", line))
    assert shapes == hb.CLASSES
    assert [hb.cap(c) for c in range(4)] == [3072, 6144, 12288, 24576]


@pytest.mark.parametrize("cls", range(4))
def test_ladder_hits_every_keys_per_thread_value_at_both_edges(cls):
    threads, kpt = hb.CLASSES[cls]
    lad = hb.ladder(cls)
    assert lad == sorted(set(lad)) and lad[:5] == [1, 2, 63, 64, 65] and lad[-2:] == [hb.cap(cls) - 1, hb.cap(cls)]
    for m in range(1, kpt + 1):
        assert m * threads in lad and m * threads - 1 in lad                      # upper edge of kpt m, one short of it
        assert (m * threads + 1 in lad) == (m < kpt)                              # one past = lower edge of kpt m + 1; nothing above cap
        assert {-(-c // threads) for c in lad} == set(range(1, kpt + 1))          # the kernel's uniform kpt = ceil(count / threads)
    # what the ladder weighs: about 60 k, 120 k, 240 k, 922 k keys
    assert sum(lad) == 195 + 3 * threads * kpt * (kpt + 1) // 2 - (hb.cap(cls) + 1)


@pytest.mark.parametrize("kt", range(3))
@pytest.mark.parametrize("cls", range(4))
def test_ladder_input_holds_exactly_the_requested_buckets(cls, kt):
    buckets = hb.ladder_buckets(cls)
    want = np.zeros(1 << 16, dtype=np.int64)
    for p, c in buckets:
        assert want[p] == 0
        want[p] = c
    cap = hb.cap(cls)
    assert want[0x0000] == cap and want[0xFFFF] == cap
    filler = [c for p, c in buckets if p % 16 == 8]
    assert len(filler) == hb.FILLER_PREFIXES and max(filler) <= cap // 2 and max(filler) - min(filler) <= 1   # explicit counts, none random
    assert {p >> 8 for p, c in buckets if p % 16 == 8} == set(range(256))            # every chain of the plan's second pass carries keys
    ladder_part = [(p, c) for p, c in buckets if p % 16 == 3]
    assert [c for _, c in ladder_part] == hb.ladder(cls)
    assert {p >> 15 for p, _ in ladder_part} == {0, 1}                               # both halves of the sign bit
    for kind in ("uniform", "descending_run"):
        for layout in hb.LAYOUTS:
            k = hb.ladder_input(cls, kt, kind, layout)
            assert k.dtype == np.uint32 and k.size == hb.N == (1 << 21) + 777
            h = hb.prefix_histogram(k, kt)
            np.testing.assert_array_equal(h, want)
            assert h.max() == cap and h.sum() == hb.N
            assert set(hb.ladder(cls)) <= set(h.tolist())
            if layout == "sorted":
                b = hb.to_bits(k, kt)
                assert np.all(b[1:] >= b[:-1])


def test_low_bit_kinds_are_what_they_say():
    cls = 1
    buckets = hb.ladder_buckets(cls)
    by_kind = {kind: hb.to_bits(hb.ladder_input(cls, 2, kind, "permuted"), 2) for kind in hb.KINDS}
    same_prefixes = by_kind["uniform"] >> np.uint32(16)
    for kind, b in by_kind.items():
        np.testing.assert_array_equal(b >> np.uint32(16), same_prefixes)             # one seed, one permutation: only the low bits differ
    low = {kind: b & np.uint32(0xFFFF) for kind, b in by_kind.items()}
    assert len(np.unique(low["equal"])) == 1
    assert np.all(low["byte0_const"] & 0xFF == 0x5A) and len(np.unique(low["byte0_const"] >> 8)) == 256
    assert np.all(low["byte1_const"] >> 8 == 0x3C) and len(np.unique(low["byte1_const"] & 0xFF)) == 256
    assert sorted(np.unique(low["two_values"]).tolist()) == [0x1233, 0x1234]
    full = by_kind["descending_run"][same_prefixes == 0xFFFF] & np.uint32(0xFFFF)
    assert sorted(full.tolist()) == list(range(hb.cap(cls)))                         # distinct: every slot of a full bucket is told apart
    two = low["two_values"][same_prefixes == 0x0000]
    assert abs(int((two == 0x1234).sum()) - int((two == 0x1233).sum())) <= 1
    assert len(np.unique(low["uniform"])) > 60000
    assert len(buckets) == 2 + len(hb.ladder(cls)) + hb.FILLER_PREFIXES


def test_transforms_round_trip_and_agree_with_the_oracle(oracle):
    edge = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    sample = np.concatenate([edge, np.random.default_rng(7).integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32),
                             np.array([0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00001, 0x00800000, 0x80000001], dtype=np.uint32)])
    for kt in range(3):
        np.testing.assert_array_equal(hb.from_bits(hb.to_bits(sample, kt), kt), sample)
        np.testing.assert_array_equal(hb.to_bits(hb.from_bits(sample, kt), kt), sample)
        want_bits = np.array([oracle.lib.gso_key_to_bits(int(x), kt) for x in sample], dtype=np.uint32)
        want_keys = np.array([oracle.lib.gso_bits_to_key(int(x), kt) for x in sample], dtype=np.uint32)
        np.testing.assert_array_equal(hb.to_bits(sample, kt), want_bits)
        np.testing.assert_array_equal(hb.from_bits(sample, kt), want_keys)
    # the order the bits give is the key type's own order (finite floats, integers)
    ints = np.array([-(1 << 31), -5, -1, 0, 1, (1 << 31) - 1], dtype=np.int32)
    assert np.all(np.diff(hb.to_bits(ints.view(np.uint32), 1).astype(np.int64)) > 0)
    floats = np.array([-np.inf, -1.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], dtype=np.float32)
    assert np.all(np.diff(hb.to_bits(floats.view(np.uint32), 2).astype(np.int64)) > 0)


@pytest.mark.parametrize("cls", range(4))
def test_boundary_inputs_hold_cap_and_cap_plus_one(cls):
    cap = hb.cap(cls)
    kt = 0 if cls % 2 == 0 else 2
    for heavy in (cap, cap + 1):
        for layout in hb.LAYOUTS:
            k = hb.boundary_input(cls, kt, heavy, layout)
            h = hb.prefix_histogram(k, kt)
            assert k.size == hb.N and h.sum() == hb.N and h[hb.HEAVY_PREFIX] == heavy == h.max()
            others = np.delete(h, hb.HEAVY_PREFIX)
            assert others.max() <= cap // 2 and np.count_nonzero(others) == hb.FILLER_PREFIXES


def test_index_values_show_a_truncated_value():
    assert hb.index_values(5, 0) is None
    v4, v8 = hb.index_values(hb.N, 4), hb.index_values(hb.N, 8)
    assert v4.dtype == np.uint32 and v8.dtype == np.uint64
    np.testing.assert_array_equal(v8 & np.uint64(0xFFFFFFFF), v4.astype(np.uint64))
    np.testing.assert_array_equal(v8 >> np.uint64(40), v4.astype(np.uint64))
