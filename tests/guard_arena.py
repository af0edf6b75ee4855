"""A guard arena for the buffer contract of include/gpusort.h — TEST INFRASTRUCTURE ONLY (a helper module: no fixtures, no hooks).

The header promises three things about caller memory: buffers need 16 bytes of alignment and no more; nothing outside [0, n) of a
buffer is written and no element outside it influences a result; inputs declared const are not written.  A fresh torch allocation
can show none of that: its base is 512-byte aligned and the slack behind n belongs to the allocator.  Here every buffer of a call
is a view into ONE uint8 tensor the test owns:

    arena = Arena.for_views([(count, np.uint32), (count, np.uint32)], "cuda", fill=0xFF)
    keys = arena.carve(count, np.uint32, skew=1)     # data_ptr() = 16 * skew (mod 256), skew odd: 16-byte and NOT 32-byte aligned
    alt = arena.carve(count, np.uint32, skew=3)      # another skew: misaligned relative to `keys` as well
    arena.write(keys, host_keys)                     # the host copy follows, so a read-only input is compared too
    arena.live(keys, n); arena.live(alt, n)          # [0, n) of each is the ONLY writable region; a view never declared is read-only
    ... the call ...
    arena.verify()                                   # one copy back; every byte outside the live regions must be what it was

Every view has GUARD_BYTES (one tile of the widest shape: 16 384 elements x 8 bytes) of its own in front and behind, views never
share a band, and [n, count) of a view is guard like the bands around it.  Fills: 0x00 (as a key word the smallest uint32), 0xFF (the
largest) and "hash" (byte = f(offset): a shifted copy of guard content is seen as well).  Scratch is carved and left as it is: its
[0, n) holds the fill, and garbage in scratch must not influence a result.  Works on CPU tensors too (tests/test_guard_arena_cpu.py).
"""
import numpy as np

GUARD_BYTES = 16384 * 8  # one full tile of the widest shape, 8-byte elements
FILLS = (0x00, 0xFF, "hash")
_ALIGN = 256


def hash_bytes(nbytes, first=0):
    """byte = f(offset): no period a kernel's strides could hide in (a multiplicative hash of the offset, top byte)."""
    o = np.arange(first, first + nbytes, dtype=np.uint64)
    return ((((o + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(56)) & np.uint64(0xFF)).astype(np.uint8)


def _torch_dtype(np_dtype):
    import torch
    return {1: torch.uint8, 4: torch.int32, 8: torch.int64}[np.dtype(np_dtype).itemsize]


class _View:
    def __init__(self, name, start, count, itemsize):
        self.name, self.start, self.count, self.itemsize = name, start, count, itemsize
        self.live = (0, 0)  # element range that may be written; empty = read-only

    @property
    def nbytes(self):
        return self.count * self.itemsize


class Arena:
    def __init__(self, nbytes, device="cuda", fill=0x00):
        import torch
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}")
        self.fill = fill
        self.nbytes = int(nbytes)
        self.host = hash_bytes(self.nbytes) if fill == "hash" else np.full(self.nbytes, fill, dtype=np.uint8)
        self.buf = torch.from_numpy(self.host.copy()).to(device)
        self.base = self.buf.data_ptr()
        self._cursor = 0   # first byte no view's back guard covers
        self._views = {}   # data_ptr -> _View, in carving order

    @classmethod
    def for_views(cls, specs, device="cuda", fill=0x00):
        """An arena with room for the given (count, dtype) views, whatever skews they are carved with."""
        need = sum(c * np.dtype(d).itemsize + 2 * GUARD_BYTES + 2 * _ALIGN for c, d in specs) + _ALIGN
        return cls(need, device, fill)

    # -- carving -----------------------------------------------------------------------------------------------------------
    def carve(self, count, dtype, skew, name=None):
        """A 1-D contiguous view of `count` elements whose address is 16 * skew (mod 256), skew odd, with a guard band of its own on
        each side."""
        if not (0 <= skew < 16 and skew % 2 == 1):
            raise ValueError("skew must be odd, 1 .. 15")
        if any(v.skew == skew for v in self._views.values()):
            raise ValueError(f"skew {skew} is taken: every buffer of one call gets a different one")
        itemsize = np.dtype(dtype).itemsize
        start = self._cursor + GUARD_BYTES
        start += (16 * skew - (self.base + start)) % _ALIGN
        end = start + count * itemsize
        if end + GUARD_BYTES > self.nbytes:
            raise ValueError("the arena is too small for this view and its guard bands")
        view = self.buf[start:end].view(_torch_dtype(dtype))
        assert view.is_contiguous() and view.dim() == 1 and view.numel() == count
        assert view.data_ptr() % _ALIGN == 16 * skew and view.data_ptr() % 16 == 0 and view.data_ptr() % 32 == 16, hex(view.data_ptr())
        v = _View(name or f"view{len(self._views)}", start, count, itemsize)
        v.skew = skew
        self._views[view.data_ptr()] = v
        self._cursor = end + GUARD_BYTES  # the next view's front guard starts here: no band is shared
        return view

    def _record(self, view):
        try:
            return self._views[view.data_ptr()]
        except KeyError:
            raise ValueError("not a view carved from this arena") from None

    def write(self, view, array, first=0):
        """Copies a host array into view[first : first + len] and into the host copy: what a read-only view is compared with."""
        v = self._record(view)
        a = np.ascontiguousarray(array)
        if a.dtype.itemsize != v.itemsize or first + a.size > v.count:
            raise ValueError("the array does not fit the view")
        lo = v.start + first * v.itemsize
        self.host[lo:lo + a.nbytes] = a.view(np.uint8).reshape(-1)
        import torch
        view[first:first + a.size].copy_(torch.from_numpy(a.view({4: np.int32, 8: np.int64, 1: np.uint8}[v.itemsize]).copy()))

    def live(self, view, n, first=0):
        """Declares [first, n) of the view (first = 0: [0, n)) the only region a call may write."""
        v = self._record(view)
        if not 0 <= first <= n <= v.count:
            raise ValueError("the live region must lie inside the view")
        v.live = (int(first), int(n))

    def read_only(self, view):
        self.live(view, 0)

    def read(self, view, dtype, n=None):
        """view[:n] on the host, as `dtype`."""
        t = view if n is None else view[:n]
        return t.cpu().numpy().view(dtype).copy()

    # -- checking ----------------------------------------------------------------------------------------------------------
    def damage(self):
        """[(view name, first damaged byte relative to the view, last, count)]: negative offsets = the front guard."""
        now = self.buf.cpu().numpy()
        bad = now != self.host
        views = list(self._views.values())
        for v in views:
            lo, hi = v.live
            bad[v.start + lo * v.itemsize: v.start + hi * v.itemsize] = False
        if not bad.any():
            return []
        out = []
        for i, v in enumerate(views):  # a view answers for everything from the end of its predecessor's back guard to the end of its own
            lo = 0 if i == 0 else views[i - 1].start + views[i - 1].nbytes + GUARD_BYTES
            hi = self.nbytes if i + 1 == len(views) else v.start + v.nbytes + GUARD_BYTES
            idx = np.flatnonzero(bad[lo:hi])
            if idx.size:
                out.append((v.name, int(idx[0]) + lo - v.start, int(idx[-1]) + lo - v.start, int(idx.size)))
        if not views:
            idx = np.flatnonzero(bad)
            out.append(("arena", int(idx[0]), int(idx[-1]), int(idx.size)))
        return out

    def verify(self):
        d = self.damage()
        if d:
            lines = []
            for name, first, last, count in d:
                v = next(x for x in self._views.values() if x.name == name)
                lines.append(f"{name} ({v.count} x {v.itemsize} bytes, live elements [{v.live[0]}, {v.live[1]}), skew {v.skew}): {count} damaged "
                             f"byte(s), first at byte {first}, last at byte {last} relative to the view (negative = front guard)")
            raise AssertionError("written outside the declared regions (fill %r):\n  " % (self.fill,) + "\n  ".join(lines))
