"""The histogram sweep in front of the LSD and position-chain plans (global_histogram_kernel) with few workgroups
(``hist_blocks``): the digit-0 replicas' cadence fold, their folds at a change of position segment, and the guarded tail.  Digit 0 is
counted on 16-bit lane-private replicas that are folded into the 32-bit table when the workgroup's position segment changes, every
HIST_FOLD_CHUNKS chunks inside a segment, and at the end; on the default grid a workgroup never stays long enough in one segment for
a missing cadence fold to show below 2^29 keys.  One workgroup makes it reachable at 39 M keys."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH = 16                  # position segments of a sort's first pass
CHUNK = 4096              # keys per histogram chunk: four of each of 1024 threads
REPLICAS = 32             # lane-private replicas of a digit-0 counter
TILE = 16384              # position segments are whole tiles: at most this many keys longer than n / NCH
HY_MIN_KEYS = 3 << 24     # the two-level plan (another sweep kernel) starts here
LOW_BYTE = 0x5A


def _byte_counts(keys):
    return np.stack([np.bincount((keys >> np.uint32(8 * q)) & np.uint32(255), minlength=256) for q in range(4)]).astype(np.uint32)


def _upload(gpu, keys):
    import torch
    return torch.from_numpy(keys.view(np.int32)).to(torch.device("cuda", torch.cuda.current_device()))


CADENCE_N = NCH * 600 * CHUNK + 3 * CHUNK + 77


@pytest.fixture(scope="module")
def cadence_words():
    """Three random words per key, drawn once for both key sets of the cadence test."""
    rng = np.random.default_rng(20261021)
    return [rng.integers(0, 1 << 32, CADENCE_N, dtype=np.uint32) for _ in range(3)]


@pytest.mark.parametrize("upper", ["uniform", "and3"])
def test_cadence_fold(gpu, cadence_words, upper):
    """ONE workgroup, 39 333 965 keys with the constant low byte 0x5A: every lane of every chunk adds to its replica of digit 0x5A.
    uniform: random upper bytes; and3: the AND of three random words up there (each bit set with probability 1 / 8: bin 0 of every
    joint table dominates, the sticky path).  The histogram is exact, the sort on the same handle is, and the histogram after it is
    the histogram before."""
    n = CADENCE_N
    assert n == 39_333_965 and n < HY_MIN_KEYS  # below the two-level plan: the sort runs global_histogram_kernel
    per_replica = CHUNK // REPLICAS  # keys a replica of a constant digit receives per chunk
    # segments are n / NCH keys rounded up to whole tiles: the first NCH - 1 hold at least `least` chunks, at most `most`; the last the rest
    least = n // NCH // CHUNK
    most = -(-(n // NCH + TILE) // CHUNK)
    last = -(-n // CHUNK) - (NCH - 1) * most
    assert least == 600 and least * per_replica == 76_800 > 0xFFFF   # a replica that is never folded inside a segment wraps ...
    assert last * per_replica > 0xFFFF                               # ... in the last, shorter segment as well
    w = cadence_words
    keys = ((w[0] if upper == "uniform" else w[0] & w[1] & w[2]) & np.uint32(0xFFFFFF00)) | np.uint32(LOW_BYTE)
    exp = _byte_counts(keys)
    assert exp[0, LOW_BYTE] == n
    dk = _upload(gpu, keys)
    s = gpu.OneSweep(n, hist_blocks=1)
    before = s.global_histogram(dk)
    np.testing.assert_array_equal(before, exp)
    s.sort(dk)
    s.check()
    assert not s.last_plan()["two_level"]
    assert gpu.validate(dk) == 0
    np.testing.assert_array_equal(s.global_histogram(dk), before)
    s.close()


@pytest.mark.parametrize("hist_blocks", [1, 3])
@pytest.mark.parametrize("n", [16 * 5 * 4096 + 1234, 3 * 4096 + 5])
@pytest.mark.parametrize("kind", ["random", "equal"])
def test_segment_folds_and_tail(gpu, hist_blocks, n, kind):
    """Few workgroups crossing position segments (a fold at each change; with three workgroups a segment is shared) and ending in a
    partial chunk (the guarded tail adds to the 32-bit table directly): the histogram is np.bincount's, the sorted keys np.sort's.
    mid_path = 0 keeps the larger size's sort on the sweep as well."""
    rng = np.random.default_rng(n + hist_blocks)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint32) if kind == "random" else np.full(n, 0xC3A55A3C, dtype=np.uint32)
    dk = _upload(gpu, keys)
    s = gpu.OneSweep(n, hist_blocks=hist_blocks, mid_path=0)
    np.testing.assert_array_equal(s.global_histogram(dk), _byte_counts(keys))
    s.sort(dk)
    s.check()
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), np.sort(keys))
    s.close()
