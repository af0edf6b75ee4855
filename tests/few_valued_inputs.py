"""Few-valued keys with known counts, and what sorting them must give: the input the keys-only position-chain plan got wrong.

A keys-only sort of 2 or 16 distinct values left a few keys out of order at 2^27 and 2^28 keys.  After the first pass
such an array consists of runs of ONE key, every tile of the later passes holds one digit and one next digit, and the run borders lie
near the position-segment borders `x << seglog` of the later passes.  This module builds such inputs together with the expected sorted
array, which comes from the COUNTS alone — the values in their order, each repeated by its count: a counting sort by construction, no
`torch.sort`, no oracle.

Two forms: `build_torch` (on a device, for the GPU tests) and `build_numpy` (its twin, for the CPU test).  Both are seeded.  The layouts
whose counts are fixed by n (`two_exact*`, `sixteen_exact`, `three_values`, `presorted`) give the SAME counts and the same expectation in
both forms; `two_random` and `sixteen_random` draw every key with the form's own generator, so their counts differ by the draw and are
stated by the builder.

Values: 31-bit patterns (so that int32, uint32 and positive-float orders agree on them) whose four bytes ALL differ between neighbouring
values — no pass is an identity pass.  Two values: the pair tests/test_gpu_unique.py uses.  `values=` replaces the pool by the caller's
bit patterns, given in the order the expectation lists them (the key order of another key type, or its reverse for a descending sort).
"""
import numpy as np

LO, HI = 0x277B4B58, 0x3E121E97  # test_two_values_among_2_27_keys's two values
NCH = 16  # chains (position segments) of a pass
EXACT_OFFSETS = (-1, 0, 1, -5000, 5000)

LAYOUTS = ("two_random", "sixteen_random") + tuple(f"two_exact({d})" for d in EXACT_OFFSETS) + ("sixteen_exact", "three_values", "presorted")


def pool(v):
    """v ascending 31-bit values; all four bytes differ between neighbours (odd byte steps), the top byte ascends."""
    if v == 2:
        return np.array([LO, HI], dtype=np.uint32)
    i = np.arange(v, dtype=np.uint32)
    b3, b2, b1, b0 = 0x08 + 7 * i, (0x7B + 37 * i) & 255, (0x4B + 91 * i) & 255, (0x58 + 63 * i) & 255
    vals = (b3 << 24) | (b2 << 16) | (b1 << 8) | b0
    assert int(b3.max()) < 0x80
    return vals.astype(np.uint32)


def seglog(n):
    """log2 of the position segments of the passes behind the first one, as the Scan kernel takes it: the smallest power of two that
    covers ceil(n / 16) keys (at least 2)."""
    return int((((n + NCH - 1) // NCH - 1) | 1)).bit_length()


def layout_counts(layout, n):
    """(number of values, counts or None).  None: the counts come from the draw."""
    if layout == "two_random":
        return 2, None
    if layout == "sixteen_random":
        return 16, None
    if layout.startswith("two_exact("):
        d = int(layout[len("two_exact("):-1])
        c0 = n // 2 + d
        assert 0 < c0 < n
        return 2, [c0, n - c0]
    if layout in ("sixteen_exact", "presorted"):
        q, r = divmod(n, 16)
        return 16, [q + (1 if j < r else 0) for j in range(16)]
    if layout == "three_values":
        return 3, [n // 2, n // 3, n - n // 2 - n // 3]
    raise ValueError(layout)


def border_offsets(counts, n):
    """For every border between two runs of the sorted array: its signed distance to the nearest position-segment border x << seglog."""
    sl = seglog(n)
    seg = 1 << sl
    out, at = [], 0
    for c in list(counts)[:-1]:
        at += int(c)
        near = ((at + seg // 2) >> sl) << sl
        out.append(at - near)
    return out


def _values(v, values):
    vals = pool(v) if values is None else np.asarray(values, dtype=np.uint32)
    assert vals.shape == (v,) and len(set(vals.tolist())) == v
    return vals


def build_numpy(layout, n, seed=0, values=None):
    """(keys, expected, counts): uint32 arrays of n keys and the list of counts, in the order of the values."""
    v, counts = layout_counts(layout, n)
    vals = _values(v, values)
    rng = np.random.default_rng(seed)
    if counts is None:
        idx = rng.integers(0, v, n, dtype=np.int64)
        counts = np.bincount(idx, minlength=v).tolist()
        keys = vals[idx]
        expected = np.repeat(vals, counts)
    else:
        expected = np.repeat(vals, counts)
        keys = expected.copy() if layout == "presorted" else expected[rng.permutation(n)]
    return keys, expected, [int(c) for c in counts]


def build_torch(layout, n, device, seed=0, values=None):
    """The same on `device`: (keys, expected, counts) — int32 tensors holding the 32-bit patterns, and the list of counts.  Positions are
    shuffled with torch.randperm; the random layouts draw with torch.randint.  Nothing but the two results stays allocated."""
    import torch
    v, counts = layout_counts(layout, n)
    vals = torch.from_numpy(_values(v, values).view(np.int32).copy()).to(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    if counts is None:
        idx = torch.randint(0, v, (n,), device=device, generator=gen, dtype=torch.int64)
        counts = torch.bincount(idx, minlength=v).tolist()
        keys = vals[idx]
        del idx
        expected = torch.repeat_interleave(vals, torch.tensor(counts, device=device))
    else:
        expected = torch.repeat_interleave(vals, torch.tensor(counts, device=device))
        if layout == "presorted":
            keys = expected.clone()
        else:
            perm = torch.randperm(n, device=device, generator=gen)
            keys = expected[perm]
            del perm
    return keys, expected, [int(c) for c in counts]
