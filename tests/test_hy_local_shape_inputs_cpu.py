"""CPU tests of tests/hy_local_shape_inputs.py: the builder of the 256 x 24 ladder is held to its promises where there is no GPU —
tests/test_gpu_hy_local_shape.py relies on "exactly c keys under one prefix" for every count at which the kernel changes behaviour."""
import os
import re

import numpy as np
import pytest

import hy_bucket_inputs as hb
import hy_local_shape_inputs as hs


def test_shape_restates_the_registry():
    """g_hy_keys_shape of kernel_registry.hpp, restated on purpose: class 1 sorts 256 x 24, every class holds its g_hy_class cap."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "gpusorting_amd", "csrc", "kernel_registry.hpp")).read()
    line = next(ln for ln in text.splitlines() if "constexpr HyKeysShape g_hy_keys_shape[4]" in ln)
    shapes = [(int(t), int(k)) for t, k in re.findall(r"\{(\d+),\s*(\d+),\s*(?:true|false)\}", line)]
    assert len(shapes) == 4 and shapes[hs.CLS] == (hs.THREADS, hs.KPT)
    assert [t * k for t, k in shapes] == [hb.cap(c) for c in range(4)]
    assert hs.CAP == hb.cap(hs.CLS) == 6144 and hs.N == (1 << 21) + 777


def test_ladder_hits_every_keys_per_thread_value_at_both_edges():
    lad = hs.ladder()
    assert lad == sorted(set(lad)) and lad[:5] == [1, 2, 63, 64, 65] and lad[-2:] == [6143, 6144]
    for m in range(1, hs.KPT + 1):
        assert m * 256 in lad and m * 256 - 1 in lad
        assert (m * 256 + 1 in lad) == (m < hs.KPT)
    assert {-(-c // hs.THREADS) for c in lad} == set(range(1, hs.KPT + 1))       # the kernel's uniform kpt, odd and even values
    assert {c & 1 for c in lad} == {0, 1} and len(lad) == 5 + 3 * hs.KPT - 1
    assert sum(lad) == 195 + 3 * 256 * hs.KPT * (hs.KPT + 1) // 2 - (hs.CAP + 1)


@pytest.mark.parametrize("kt", range(3))
def test_input_holds_exactly_the_requested_buckets(kt):
    buckets = hs.buckets()
    want = np.zeros(1 << 16, dtype=np.int64)
    for p, c in buckets:
        assert want[p] == 0
        want[p] = c
    assert want[0x0000] == hs.CAP and want[0xFFFF] == hs.CAP and want.sum() == hs.N and want.max() == hs.CAP
    filler = [c for p, c in buckets if p % 16 == 8]
    assert len(filler) == hb.FILLER_PREFIXES and max(filler) <= hs.CAP // 2 and max(filler) - min(filler) <= 1
    assert {p >> 8 for p, c in buckets if p % 16 == 8} == set(range(256))        # every chain of the plan's second pass carries keys
    assert [c for p, c in buckets if p % 16 == 3] == hs.ladder()
    for kind in hs.KINDS:
        k = hs.keys(kt, kind)
        assert k.dtype == np.uint32 and k.size == hs.N
        np.testing.assert_array_equal(hb.prefix_histogram(k, kt), want)


def test_low_bit_kinds_are_what_they_say():
    bits = {kind: hb.to_bits(hs.keys(2, kind), 2) for kind in hs.KINDS}
    full = {kind: b[(b >> np.uint32(16)) == 0xFFFF] & np.uint32(0xFFFF) for kind, b in bits.items()}
    assert all(f.size == hs.CAP for f in full.values())
    assert len(np.unique(full["uniform"])) > 5000
    assert len(np.unique(full["equal"])) == 1
    assert len(np.unique(full["byte0_const"] & 0xFF)) == 1 and len(np.unique(full["byte0_const"] >> 8)) == 256
