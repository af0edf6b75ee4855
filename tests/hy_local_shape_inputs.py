"""Inputs for the keys-only bucket-local sort of size class 1 on its OWN workgroup shape (g_hy_keys_shape in kernel_registry.hpp:
256 threads x 24 keys, the class's cap of 6144 unchanged), built with the machinery of tests/hy_bucket_inputs.py.  That module's
ladder is cut for the class's 512 x 12: its edges are multiples of 512.  The kernel's uniform keys-per-thread value is
ceil(count / threads), so on 256 threads it changes at every multiple of 256 and takes 24 values, odd ones among them (an odd value
makes the last loaded dword of every thread half empty).

A plain module (no conftest, no fixtures).  tests/test_hy_local_shape_inputs_cpu.py holds it to its promises without a GPU;
tests/test_gpu_hy_local_shape.py sorts what it builds."""
import hy_bucket_inputs as hb

CLS = 1
THREADS, KPT = 256, 24     # the keys-only kernel's shape for class 1, restated on purpose
CAP = THREADS * KPT        # 6144 = hb.cap(CLS)
N = hb.N
KINDS = ("uniform", "equal", "byte0_const")   # random low halves; all low halves equal; all low bytes equal (one pass-1 counter takes the bucket)


def ladder():
    """Bucket counts: 1, 2 and the wave's edges, then every keys-per-thread value m = 1 .. 24 at its upper edge (256 m), one short of
    it and one past it (the lower edge of m + 1); nothing above the cap, so the last two are 6143 and 6144."""
    counts = {1, 2, 63, 64, 65, CAP - 1, CAP}
    for m in range(1, KPT + 1):
        counts |= {m * THREADS - 1, m * THREADS, m * THREADS + 1}
    return sorted(c for c in counts if c <= CAP)


def buckets():
    """[(prefix, count)]: a full bucket under prefix 0x0000 and one under 0xFFFF (the first and the last entry of the table of bucket
    starts; descending, their mirrored ranges lie at the array's other end), one bucket per ladder count, the rest of N as filler spread
    over 4096 other prefixes, each far below the cap."""
    counts = ladder()
    b = [(0x0000, CAP), (0xFFFF, CAP)] + list(zip(hb._ladder_prefixes(len(counts)), counts))
    rest = N - sum(c for _, c in b)
    return b + list(zip(hb._filler_prefixes(), hb._spread(rest, hb.FILLER_PREFIXES, CAP // 2)))


def keys(kt, kind="uniform", layout="permuted", seed=3):
    """uint32 patterns of key type kt (0 uint32, 1 int32, 2 float32) whose radix-sortable bits hold exactly buckets()."""
    return hb.build(buckets(), kt, kind, layout, seed)
