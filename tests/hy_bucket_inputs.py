"""Inputs whose 16-bit-prefix buckets have EXACT sizes, for the bucket-local sorts of the two-level plan (hy_local_sort_kernel and
hy_local_sort_pairs_kernel, gpusorting_amd/csrc/hybrid_kernels.hpp): one workgroup sorts one bucket in LDS, in one of four size classes
(g_hy_class in kernel_registry.hpp; gs_debug_set_hy_class forces one).  What those kernels could get wrong shows at a bucket count near
a multiple of the workgroup's threads, at a bucket of exactly the workgroup's capacity, or with one digit holding a whole bucket — a
bucket is at most 24 576 keys, so none of that needs a large sort.

A plain module (no conftest, no fixtures).  Everything is built in the space of the keys' radix-sortable BITS (what the kernels count
prefixes of) and mapped back to the key type at the end (from_bits), so the bucket sizes are exact for uint32, int32 and float32 alike.
Float keys built this way include NaN patterns of both signs: compare uint32 views, never float values — the library and the oracle
order keys by their bits (oracle/gs_oracle.cpp: gso_key_to_bits inside gso_std_sort).

tests/test_hy_bucket_inputs_cpu.py holds this module to its promises without a GPU; tests/test_gpu_hy_classes.py and the ledger's
class cases (tests/test_gpu_registry.py) sort what it builds."""
import numpy as np

# (threads, keys per thread) of the four size classes; cap = threads x keys per thread
CLASSES = ((256, 12), (512, 12), (1024, 12), (1024, 24))
N = (1 << 21) + 777                 # keys of every input built here
FILLER_PREFIXES = 4096              # ... at stride 16: sixteen under every top byte, so all 256 chains of the plan's second pass carry keys
KINDS = ("uniform", "equal", "byte0_const", "byte1_const", "two_values", "descending_run")
LAYOUTS = ("permuted", "sorted")
HEAVY_PREFIX = 0x9A31               # the boundary inputs' one heavy prefix (upper half of the sign bit; no filler prefix)


def cap(cls):
    threads, kpt = CLASSES[cls]
    return threads * kpt


def to_bits(keys, kt):
    """uint32 patterns of key type kt (0 uint32, 1 int32, 2 float32) -> radix-sortable bits."""
    k = np.asarray(keys, dtype=np.uint32)
    if kt == 0:
        return k.copy()
    if kt == 1:
        return k ^ np.uint32(0x80000000)
    return np.where(k >> np.uint32(31), ~k, k ^ np.uint32(0x80000000)).astype(np.uint32)


def from_bits(bits, kt):
    """The inverse: int32 bits ^ 0x80000000; float32 bits ^ 0x80000000 where bit 31 is set, ~bits otherwise."""
    b = np.asarray(bits, dtype=np.uint32)
    if kt == 0:
        return b.copy()
    if kt == 1:
        return b ^ np.uint32(0x80000000)
    return np.where(b >> np.uint32(31), b ^ np.uint32(0x80000000), ~b).astype(np.uint32)


def ladder(cls):
    """Bucket counts of one class: 1, 2 and the wave's edges, then every keys-per-thread value 1 .. K of the kernel's uniform
    kpt = ceil(count / T) at its upper edge (m T), one short of it (m T - 1) and one past it (m T + 1 = the lower edge of m + 1);
    nothing above cap, so the last two entries are cap - 1 and cap."""
    threads, kpt = CLASSES[cls]
    counts = {1, 2, 63, 64, 65}
    for m in range(1, kpt + 1):
        counts |= {m * threads - 1, m * threads, m * threads + 1}
    return sorted(c for c in counts if c <= cap(cls))


def _ladder_prefixes(count):
    """Prefixes of the ladder's buckets: alternately in the lower and the upper half of the sign bit, none of them a filler prefix
    (those are 8 mod 16), 0x0000 or 0xFFFF."""
    p = [((i & 1) << 15) + 16 * (7 + 53 * (i >> 1)) + 3 for i in range(count)]
    assert len(set(p)) == count and max(p) < 0xFFFF
    return p


def _filler_prefixes():
    return [16 * j + 8 for j in range(FILLER_PREFIXES)]


def _spread(total, buckets, limit):
    """total keys over `buckets` buckets in explicit counts: as equal as they get, every one of them in 1 .. limit."""
    base, extra = divmod(total, buckets)
    counts = [base + 1] * extra + [base] * (buckets - extra)
    assert base >= 1 and max(counts) <= limit, (total, buckets, limit)
    return counts


def ladder_buckets(cls):
    """[(prefix, count)] of the ladder input of class cls: cap keys under prefix 0x0000 (the bucket that starts at 0; its descending
    mirror n - start - count lies at the array's end) and under 0xFFFF (the bucket whose end is the last word of the table of bucket
    starts), one bucket per ladder count, and the filler: N in all."""
    c = cap(cls)
    counts = ladder(cls)
    buckets = [(0x0000, c), (0xFFFF, c)] + list(zip(_ladder_prefixes(len(counts)), counts))
    rest = N - sum(n for _, n in buckets)
    buckets += list(zip(_filler_prefixes(), _spread(rest, FILLER_PREFIXES, c // 2)))
    return buckets


def boundary_buckets(cls, heavy):
    """[(prefix, count)]: `heavy` keys under HEAVY_PREFIX, the rest of N spread over the filler prefixes (each <= cap / 2)."""
    return [(HEAVY_PREFIX, heavy)] + list(zip(_filler_prefixes(), _spread(N - heavy, FILLER_PREFIXES, cap(cls) // 2)))


def _low16(kind, counts, rng):
    """The low 16 bits of every key, bucket by bucket (the keys of a bucket are consecutive here)."""
    total = int(sum(counts))
    if kind == "uniform":
        return rng.integers(0, 1 << 16, total, dtype=np.uint32)
    if kind == "equal":            # one value: one counter of each LDS pass takes the whole bucket
        return np.full(total, 0xA5C3, dtype=np.uint32)
    if kind == "byte0_const":      # the first LDS pass is an identity pass
        return (rng.integers(0, 256, total, dtype=np.uint32) << np.uint32(8)) | np.uint32(0x5A)
    if kind == "byte1_const":      # ... the second
        return np.uint32(0x3C00) | rng.integers(0, 256, total, dtype=np.uint32)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.arange(total, dtype=np.int64) - np.repeat(starts, counts)   # position inside the bucket
    if kind == "two_values":       # alternating: half a bucket of ties on either value — stability shows in the values
        return np.where(rank & 1, 0x1233, 0x1234).astype(np.uint32)
    if kind == "descending_run":   # count - 1 .. 0: distinct in every bucket (cap < 65 536), the reverse of the sorted order
        return (np.repeat(np.asarray(counts, dtype=np.int64), counts) - 1 - rank).astype(np.uint32)
    raise ValueError(kind)


def build(buckets, kt, kind="uniform", layout="permuted", seed=1):
    """The keys (uint32 patterns of key type kt) of [(prefix, count)]: np.repeat over the buckets, the low 16 bits of `kind` attached,
    then one seeded permutation (layout "permuted") or the whole array sorted by its bits (layout "sorted": every bucket is one
    contiguous run, so a single histogram workgroup sees all of it)."""
    prefixes = np.array([p for p, _ in buckets], dtype=np.uint32)
    counts = np.array([c for _, c in buckets], dtype=np.int64)
    assert len(set(prefixes.tolist())) == len(prefixes) and prefixes.max() <= 0xFFFF and counts.min() >= 1
    bits = (np.repeat(prefixes, counts) << np.uint32(16)) | _low16(kind, counts, np.random.default_rng(seed))
    if layout == "permuted":   # (a generator of its own: the same permutation for every kind)
        bits = bits[np.random.default_rng([seed, 1]).permutation(bits.size)]
    elif layout == "sorted":
        bits = np.sort(bits)
    else:
        raise ValueError(layout)
    return from_bits(bits, kt)


def ladder_input(cls, kt, kind="uniform", layout="permuted", seed=1):
    return build(ladder_buckets(cls), kt, kind, layout, seed)


def boundary_input(cls, kt, heavy, layout="permuted", seed=2):
    return build(boundary_buckets(cls, heavy), kt, "uniform", layout, seed)


def prefix_histogram(keys, kt):
    """Keys per 16-bit prefix of the radix-sortable bits: 65 536 counts."""
    return np.bincount(to_bits(keys, kt) >> np.uint32(16), minlength=1 << 16)


def index_values(n, vb):
    """Values = the input index; 8-byte values carry it in both words (index | index << 40): a value moved in halves, or truncated, shows."""
    if vb == 4:
        return np.arange(n, dtype=np.uint32)
    if vb == 8:
        i = np.arange(n, dtype=np.uint64)
        return i | (i << np.uint64(40))
    return None
