"""GPU test of what the eight handles share (gpusorting_amd/csrc/handle_core.hpp): the workspace, the create/destroy frame, the control
block's read-back and the rank-mode pair.  Every handle at its smallest sizes (max_keys 64, one segment, max_k 1), keys only and pairs
with 4-byte values:

  * create; `check` answers GS_OK before any call (the workspace zeroes the control block) and `last` reports a zeroed route, forms
    and status;
  * the rank mode reads back what was set; 2 is refused with GS_ERR_ARG and leaves the mode as it was (gs_segsort and gs_topk have no
    rank-mode entries of their own: theirs is their engine's);
  * one sort or selection of 64 keys equals the numpy reference the package ships;
  * destroy, then create and destroy once more (release and re-allocation).

Only refused arguments: nothing here provokes a fault."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
KEYS, PAIRS = 0, 1
RNG = np.random.default_rng(64)
KEYS32 = RNG.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
KEYS32[::7] = KEYS32[3]                                 # duplicates: the order of their values shows the sort is stable
KEYS16 = (KEYS32 >> np.uint32(16)).astype(np.uint16)
VALS = (np.arange(N, dtype=np.uint32) * np.uint32(3) + np.uint32(1))
OFFSETS = np.array([0, N], dtype=np.uint32)


def _dev(a):
    import torch
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}[a.dtype]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _flat_sort16(g, h, pairs):
    k, v = _dev(KEYS16), _dev(VALS) if pairs else None
    h.sort(k, v)
    want_k, want_v = g.sort16_reference(KEYS16, VALS if pairs else None, g.KEY_UINT16)
    return [(_host(k, np.uint16), want_k)] + ([(_host(v, np.uint32), want_v)] if pairs else [])


def _rows(ref, keys, dtype):
    def run(g, h, pairs):
        k, v = _dev(keys.reshape(2, N // 2)), _dev(VALS.reshape(2, N // 2)) if pairs else None
        h.sort(k, v)
        want_k, want_v = getattr(g, ref)(keys.reshape(2, N // 2), VALS.reshape(2, N // 2) if pairs else None)
        return [(_host(k, dtype), want_k)] + ([(_host(v, np.uint32), want_v)] if pairs else [])
    return run


def _segments(ref, keys, dtype):
    def run(g, h, pairs):
        k, v = _dev(keys), _dev(VALS) if pairs else None
        h.sort(k, _dev(OFFSETS), v)
        want = getattr(g, ref)(keys, OFFSETS, VALS if pairs else None)
        if not pairs:
            return [(_host(k, dtype), want[0] if isinstance(want, tuple) else want)]
        return [(_host(k, dtype), want[0]), (_host(v, np.uint32), want[1])]
    return run


def _select(g, h, pairs):
    import torch
    ok, ov = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda") if pairs else None
    h.select(_dev(KEYS32), 1, ok, _dev(VALS) if pairs else None, ov)
    want_k, want_v = g.topk_reference(KEYS32, 1, VALS if pairs else None)
    return [(_host(ok, np.uint32), want_k)] + ([(_host(ov, np.uint32), want_v)] if pairs else [])


def _seg_select(keys, dtype):
    def run(g, h, pairs):
        import torch
        ok = torch.zeros(1, dtype=torch.int16 if dtype == np.uint16 else torch.int32, device="cuda")
        ov = torch.zeros(1, dtype=torch.int32, device="cuda") if pairs else None
        h.select(_dev(keys), _dev(OFFSETS), 1, ok, _dev(VALS) if pairs else None, ov)
        want_k, want_v, counts = g.segmented_topk_reference(keys, OFFSETS, 1, VALS if pairs else None, key_type=h.key_type)
        assert counts.tolist() == [1]
        return [(_host(ok, dtype), want_k.reshape(-1))] + ([(_host(ov, np.uint32), want_v.reshape(-1))] if pairs else [])
    return run


# name -> (class, the sizes behind max_keys, whether the handle has rank-mode entries of its own, the call and its reference)
HANDLES = {
    "gs_sort16": ("Sort16", (), True, _flat_sort16),
    "gs_sort_rows": ("RowSort", (), True, _rows("sort_rows_reference", KEYS32, np.uint32)),
    "gs_sort_rows16": ("RowSort16", (), True, _rows("sort_rows16_reference", KEYS16, np.uint16)),
    "gs_segsort": ("SegmentedSort", (1,), False, _segments("segmented_sort_reference", KEYS32, np.uint32)),
    "gs_segsort16": ("SegmentedSort16", (1,), True, _segments("segmented_sort16_reference", KEYS16, np.uint16)),
    "gs_topk": ("TopK", (1,), False, _select),
    "gs_segtopk": ("SegmentedTopK", (1, 1), True, _seg_select(KEYS32, np.uint32)),
    "gs_segtopk16": ("SegmentedTopK16", (1, 1), True, _seg_select(KEYS16, np.uint16)),
}


@pytest.mark.parametrize("pairs", [False, True], ids=["keys", "pairs4"])
@pytest.mark.parametrize("name", list(HANDLES))
def test_create_check_rank_mode_one_call_destroy(gpu, name, pairs):
    g = gpu
    from gpusorting_amd import _lib
    cls, sizes, has_rank, run = HANDLES[name]
    key16 = name.endswith("16")
    make = lambda: getattr(g, cls)(N, *sizes, key_type=g.KEY_UINT16 if key16 else g.KEY_UINT32,  # noqa: E731
                                   mode=PAIRS if pairs else KEYS, value_bytes=4 if pairs else 0)
    h = make()
    # before any call: the control block was zeroed at create
    assert h.status() == _lib.GS_OK
    first = h.last()
    assert first["route" if "route" in first else "forms"] == 0 and first.get("forms", 0) == 0 and first.get("status", 0) == 0, first
    if has_rank:
        probed = h.rank_mode
        assert probed in (0, 1)
        for mode in (1 - probed, probed):
            h.set_rank_mode(mode)
            assert h.rank_mode == mode
        with pytest.raises(g.GpuSortError) as refused:
            h.set_rank_mode(2)
        assert refused.value.status == _lib.GS_ERR_ARG and h.rank_mode == probed
    for got, want in run(g, h, pairs):
        np.testing.assert_array_equal(got, want)
    h.check()
    h.close()
    # release and re-allocation
    again = make()
    assert again.status() == _lib.GS_OK
    again.close()
