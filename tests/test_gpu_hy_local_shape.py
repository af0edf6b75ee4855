"""GPU tests (-m gpu) of the keys-only bucket-local sort of size class 1 on its own workgroup shape: 256 threads x 24 keys on 16-bit
halves (hy_local_sort_kernel with HALF, g_hy_keys_shape in kernel_registry.hpp).  The class's cap stays 6144, so the ladder of
tests/hy_bucket_inputs.py — cut for 512 x 12 — still passes through the kernel but no longer meets its edges: on 256 threads the
uniform keys-per-thread value changes at every multiple of 256 and takes odd values.  tests/hy_local_shape_inputs.py builds
2^21 + 777 keys whose buckets hold exactly those counts, a full bucket under prefix 0x0000 and one under 0xFFFF.

Set-up as tests/test_gpu_hy_classes.py: plan 2, the class forced (at this size n alone would pick class 0).  Reference: torch.sort of
the keys' radix-sortable bits, computed once per low-bit kind (the bits are the same for every key type; descending is its reverse).
Every comparison is bit-exact on uint32 views: the float inputs hold NaN patterns of both signs."""
import numpy as np
import pytest

import hy_bucket_inputs as hb
import hy_local_shape_inputs as hs

pytestmark = pytest.mark.gpu

MAXK = 1 << 22
OPTIONS = dict(small_path=0, mid_path=0, plan=2, position_chains_min_log2=20)
_sorted_bits = {}


def _want(kt, order, kind, seed=3):
    """The sorted keys of hs.keys(kt, kind, seed=seed) in key type kt: torch.sort on the bit patterns, once per (kind, seed)."""
    import torch
    if (kind, seed) not in _sorted_bits:
        bits = hb.to_bits(hs.keys(0, kind, seed=seed), 0).astype(np.int64)
        _sorted_bits[(kind, seed)] = torch.sort(torch.from_numpy(bits).cuda()).values.cpu().numpy().astype(np.uint32)
    b = _sorted_bits[(kind, seed)]
    return hb.from_bits(b[::-1] if order else b, kt)


@pytest.fixture(scope="module")
def sorter(gpu):
    s = gpu.OneSweep(MAXK, **OPTIONS)
    s.set_hy_class(hs.CLS)
    yield s
    s.close()


def _sort_exact(s, kt, order, kind):
    import torch
    s.key_type, s.order = kt, order
    dk = torch.from_numpy(hs.keys(kt, kind).view(np.int32).copy()).cuda()
    s.sort(dk)
    s.check()
    lp = s.last_plan()
    assert lp["two_level"] and lp["largest_bucket"] == hs.CAP == 6144, (kt, order, kind, lp)
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), _want(kt, order, kind), err_msg=f"{(kt, order, kind)}")


@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("kt", range(3))
def test_every_bucket_count_of_256_x_24(gpu, sorter, kt, order):
    """uint32, int32, float32, ascending and descending: buckets of 1, 2, 63, 64, 65 keys, of 256 m - 1, 256 m and 256 m + 1 keys for
    every keys-per-thread value m = 1 .. 24, and of 6143 and 6144 keys, random low halves."""
    _sort_exact(sorter, kt, order, "uniform")


@pytest.mark.parametrize("order", (0, 1))
def test_buckets_whose_low_halves_are_all_equal(gpu, sorter, order):
    """One counter of each LDS pass takes a whole bucket; both passes are identity passes."""
    _sort_exact(sorter, 2, order, "equal")


@pytest.mark.parametrize("order", (0, 1))
def test_buckets_whose_low_bytes_are_all_equal(gpu, sorter, order):
    """One pass-1 counter takes 6144 adds, and pass 2 alone orders the bucket: its stability on the slot map shows."""
    _sort_exact(sorter, 1, order, "byte0_const")


def test_in_a_captured_hip_graph(gpu):
    """Captured once with the class forced, replayed on two inputs of the ladder (different low halves and permutation)."""
    import torch
    s = gpu.OneSweep(MAXK, **OPTIONS)
    s.set_hy_class(hs.CLS)
    dk = torch.from_numpy(hs.keys(0, "uniform").view(np.int32).copy()).cuda()
    alt = torch.empty_like(dk)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.sort(dk, alt_keys=alt)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.sort(dk, alt_keys=alt)
    for seed in (3, 4):
        dk.copy_(torch.from_numpy(hs.keys(0, "uniform", seed=seed).view(np.int32).copy()))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), _want(0, 0, "uniform", seed), err_msg=f"seed {seed}")
        lp = s.last_plan()
        assert lp["two_level"] and lp["largest_bucket"] == hs.CAP, (seed, lp)
    s.check()
    s.close()
