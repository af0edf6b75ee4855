"""CPU tests of the hand-over layout between pass B and the bucket-local sort of the keys-only two-level plan (hy_half_slot,
gpusorting_amd/csrc/hybrid_kernels.hpp, through the host entry gs_debug_hy_half_slot): pass B writes the low 16 bits of every key as a
uint16 into the first half of its bucket's own bytes.

The rule, restated here independently: bucket p has count = base[p + 1] - base[p] keys; its final range starts at key index
at = base[p] (ascending) or n - base[p + 1] (descending); with the key buffer viewed as uint16[2 n], the key pass B ranks r inside the
bucket goes to halfword 2 at + r.  What must hold for any table of bucket sizes: the slots of a bucket are distinct, lie in
[2 at, 2 at + count) — inside the bucket's own bytes, 2 at + count <= 2 (at + count) — and no two buckets share a halfword."""
import numpy as np
import pytest

BINS = 1 << 16


@pytest.fixture(scope="module")
def half_slot():
    from gpusorting_amd import _lib
    fn = _lib.load().gs_debug_hy_half_slot

    def call(base_p, base_p1, n, descending, rank):
        return int(fn(int(base_p), int(base_p1), int(n), int(descending), int(rank)))
    return call


def _tables():
    """Random bucket tables: 65 536 counts, zeros included, of a few shapes."""
    rng = np.random.default_rng(16)
    # most prefixes empty, the others small: odd and even counts, runs of empty buckets between them
    sparse = np.zeros(BINS, dtype=np.int64)
    hit = rng.choice(BINS, 3000, replace=False)
    sparse[hit] = rng.integers(1, 40, hit.size)
    sparse[[0, BINS - 1]] = (7, 5)   # the first and the last prefix are taken
    yield "sparse", sparse
    # every count 0 .. 3: about a quarter of the buckets empty
    yield "tiny", rng.integers(0, 4, BINS).astype(np.int64)
    # a few large buckets (a workgroup's capacity) among ones, the first and the last prefix empty
    large = (rng.random(BINS) < 0.3).astype(np.int64)
    large[rng.choice(BINS, 4, replace=False)] = (24576, 24575, 3071, 3072)
    large[[0, BINS - 1]] = 0
    yield "large", large


@pytest.mark.parametrize("descending", (0, 1))
def test_slots_of_every_bucket_are_distinct_and_inside_its_own_bytes(half_slot, descending):
    for name, counts in _tables():
        assert counts.size == BINS and (counts == 0).any()
        n = int(counts.sum())
        base = np.concatenate([[0], np.cumsum(counts)])
        taken = np.zeros(2 * n, dtype=np.uint8)
        for p in np.flatnonzero(counts):
            b0, b1, count = int(base[p]), int(base[p + 1]), int(counts[p])
            at = n - b1 if descending else b0
            slots = [half_slot(b0, b1, n, descending, r) for r in range(count)]
            assert len(set(slots)) == count, (name, p)
            assert min(slots) >= 2 * at and max(slots) < 2 * at + count, (name, p, at, count)
            assert 2 * at + count <= 2 * (at + count) <= 2 * n, (name, p)
            assert slots == [2 * at + r for r in range(count)], (name, p)   # the rule as stated
            assert not taken[slots].any(), (name, p)                          # no other bucket's halfword
            taken[slots] = 1
        assert int(taken.sum()) == n


def test_nothing_overflows_32_bits_at_the_largest_sort(half_slot):
    n = (1 << 30) - 1
    for b0, b1 in ((0, 1), (0, 24576), (n - 24575, n), (n - 1, n), (n // 2, n // 2 + 3), (12345, 12345 + 24576)):
        count = b1 - b0
        for descending in (0, 1):
            at = n - b1 if descending else b0
            for r in (0, count // 2, count - 1):
                got = half_slot(b0, b1, n, descending, r)
                assert got == 2 * at + r < 2 * n < 1 << 32, (b0, b1, descending, r, got)
