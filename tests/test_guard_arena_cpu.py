"""A test of the test: tests/guard_arena.py on CPU tensors.  Every kind of stray write the GPU cases rely on verify() to see is
planted here by hand, and verify() must name the view and the damaged byte offsets; writes inside the live region must pass."""
import numpy as np
import pytest

from guard_arena import GUARD_BYTES, Arena, hash_bytes

COUNT, N = 1000, 777


def _arena(fill, dtype=np.uint32):
    arena = Arena.for_views([(COUNT, dtype)] * 3, "cpu", fill)
    keys = arena.carve(COUNT, dtype, 1, "keys")
    alt = arena.carve(COUNT, dtype, 3, "alt")
    src = arena.carve(COUNT, dtype, 5, "input")
    arena.write(keys, np.arange(N, dtype=dtype) * 3 + 1)
    arena.write(src, np.arange(N, dtype=dtype) + 7)
    arena.live(keys, N)
    arena.live(alt, N)
    arena.read_only(src)
    return arena, keys, alt, src


def _poke(arena, view, byte_offset):
    """Flips one byte at `byte_offset` relative to the view's first byte."""
    at = view.data_ptr() - arena.base + byte_offset
    arena.buf[at] = int(arena.buf[at]) ^ 0x5A


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_planted_writes_are_named(fill, dtype):
    size = np.dtype(dtype).itemsize
    planted = {
        "last byte of the front guard": ("alt", -1),
        "first byte behind n": ("alt", N * size),
        "last byte of the back guard": ("alt", COUNT * size + GUARD_BYTES - 1),
        "inside a read-only view": ("input", 5 * size + 1),
        "inside [n, count)": ("keys", (N + 100) * size + size - 1),
        "first byte of the front guard": ("keys", -GUARD_BYTES),
    }
    for what, (name, offset) in planted.items():
        arena, keys, alt, src = _arena(fill, dtype)
        arena.verify()
        _poke(arena, {"keys": keys, "alt": alt, "input": src}[name], offset)
        assert arena.damage() == [(name, offset, offset, 1)], what
        with pytest.raises(AssertionError) as e:
            arena.verify()
        msg = str(e.value)
        assert msg.count("damaged") == 1 and f"\n  {name} (" in msg, (what, msg)
        assert f"1 damaged byte(s), first at byte {offset}, last at byte {offset} " in msg, (what, msg)


def test_several_writes_report_first_last_and_count():
    arena, keys, alt, src = _arena(0x00)
    for offset in (-3, 4 * N, 4 * N + 9):
        _poke(arena, alt, offset)
    _poke(arena, src, 0)
    assert arena.damage() == [("alt", -3, 4 * N + 9, 3), ("input", 0, 0, 1)]
    with pytest.raises(AssertionError) as e:
        arena.verify()
    assert "alt (" in str(e.value) and "input (" in str(e.value) and "keys (" not in str(e.value)


@pytest.mark.parametrize("fill", [0x00, 0xFF, "hash"])
def test_writes_inside_the_live_region_pass(fill):
    arena, keys, alt, src = _arena(fill)
    keys[:N] = 0x12345678
    alt[:N] = -1
    _poke(arena, keys, 0)
    _poke(arena, keys, 4 * N - 1)
    arena.verify()
    arena.live(keys, N, first=10)  # (segmented sort: the elements in front of offsets[0] are not to be touched either)
    with pytest.raises(AssertionError, match="first at byte 0, last at byte 39 "):
        arena.verify()


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_alignment_for_all_eight_odd_skews(dtype):
    arena = Arena.for_views([(100 + s, dtype) for s in range(8)], "cpu", 0xFF)
    views = [arena.carve(100 + i, dtype, skew) for i, skew in enumerate((1, 3, 5, 7, 9, 11, 13, 15))]
    starts = []
    for i, (v, skew) in enumerate(zip(views, (1, 3, 5, 7, 9, 11, 13, 15))):
        assert v.data_ptr() % 256 == 16 * skew and v.data_ptr() % 16 == 0 and v.data_ptr() % 32 != 0
        assert v.numel() == 100 + i and v.element_size() == np.dtype(dtype).itemsize and v.is_contiguous()
        starts.append((v.data_ptr() - arena.base, v.numel() * v.element_size()))
    assert starts[0][0] >= GUARD_BYTES and arena.nbytes - sum(starts[-1]) >= GUARD_BYTES
    for (a, na), (b, _) in zip(starts, starts[1:]):
        assert b - (a + na) >= 2 * GUARD_BYTES, "two views never share a guard band"
    with pytest.raises(ValueError):
        arena.carve(10, dtype, 2)   # even: 32-byte aligned
    with pytest.raises(ValueError):
        arena.carve(10, dtype, 3)   # taken


def test_hash_fill_sees_a_shifted_copy():
    arena, keys, alt, src = _arena("hash")
    at = alt.data_ptr() - arena.base + 4 * COUNT
    arena.buf[at:at + 64] = arena.buf[at + 4:at + 68].clone()  # guard content moved by one element
    assert arena.damage() and arena.damage()[0][0] == "alt"
    h = hash_bytes(1 << 16)
    assert np.unique(h).size == 256 and not np.array_equal(h[:-4], h[4:]) and np.array_equal(hash_bytes(100, 50), h[50:150])


def _sort_one_too_many(arena, keys, alt, n, descending):
    """A "sort" with the classic defect: it works on n + 1 elements (numpy on the views' memory)."""
    k = keys.numpy().view(np.uint32)
    a = alt.numpy().view(np.uint32)
    a[:n + 1] = k[:n + 1]
    k[:n + 1] = np.sort(a[:n + 1])[::-1] if descending else np.sort(a[:n + 1])


@pytest.mark.parametrize("fill,descending", [(0x00, False), (0x00, True), (0xFF, False), (0xFF, True)])
def test_a_sort_of_n_plus_one_elements_is_caught(fill, descending):
    """Whichever way the guard word sorts, it either moves into [0, n) — the result differs from the reference — or stays put while
    the scratch copy of it lands behind n: verify() sees that under both constant fills."""
    rng = np.random.default_rng(1)
    arena, keys, alt, src = _arena(fill)
    data = rng.integers(1, 0xFFFFFFFF, size=N, dtype=np.uint64).astype(np.uint32)
    arena.write(keys, data)
    _sort_one_too_many(arena, keys, alt, N, descending)
    ref = np.sort(data)[::-1] if descending else np.sort(data)
    wrong_result = not np.array_equal(arena.read(keys, np.uint32, N), ref)
    moved = (fill == 0x00) != descending  # the guard word is the smallest key ascending-first / the largest descending-first
    assert wrong_result == moved
    if moved:
        with pytest.raises(AssertionError, match=r"keys \(.*first at byte %d, " % (4 * N)):
            arena.verify()   # the largest / smallest real key now sits in the guard behind n
    else:
        # keys[n] got its own value back and alt[n] a copy of the fill: only a fill that differs from the copy can show it
        arena.verify()
        arena2, keys2, alt2, _ = _arena("hash")
        arena2.write(keys2, data)
        _sort_one_too_many(arena2, keys2, alt2, N, descending)
        with pytest.raises(AssertionError, match="first at byte %d, " % (4 * N)):
            arena2.verify()
