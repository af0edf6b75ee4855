"""The top-k selection (gs_topk_*, gpusorting_amd/csrc/topk_kernels.hpp) on the GPU: every case compares keys AND values bit for bit
with gpusorting_amd.topk_reference (itself checked against the oracle in tests/test_topk_cpu.py) and calls check().  Keys come
from init_random with seeds and entropy presets, or are built against the structure of the selection.  No counterpart in the
reference project."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VALUE_DTYPE = {4: np.uint32, 8: np.uint64}
SINGLE_TILE = {0: 32768, 4: 16384, 8: 8192}  # n up to here takes the single-tile route
SELECT, SINGLE = 1, 3
KS = (1, 2, 63, 64, 65, 1000, 1 << 16)
# value modes: keys only, 4-byte values, 8-byte values, positions
MODES = ("keys", "v4", "v8", "pos")


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).cuda()


def _keys(gpu, n, seed, preset):
    torch = _torch()
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.init_random(dk, seed, preset)
    torch.cuda.synchronize()
    return dk.cpu().numpy().view(np.uint32).copy()


def _vb(mode):
    return {"keys": 0, "v4": 4, "v8": 8, "pos": 4}[mode]


def _values(n, mode):
    """Values that differ from the position, so that a position written for a value shows."""
    if mode == "v4":
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x5A5A5A5A)
    if mode == "v8":
        return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x1F)
    return None


def _handle(gpu, n, k, mode, key_type=0, descending=False):
    vb = _vb(mode)
    return gpu.TopK(n, k, gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, key_type, gpu.MODE_PAIRS if vb else gpu.MODE_KEYS_ONLY, vb)


_ref_cache = {}


def _reference(gpu, keys, k, vals, key_type, descending):
    """topk_reference(keys, k, ...): by its definition the head of topk_reference(keys, n, ...), which is kept for the array last seen."""
    tag = (id(keys), keys.size, int(keys[0]), int(keys[-1]), None if vals is None else vals.dtype.itemsize, key_type, descending)
    if _ref_cache.get("tag") != tag:
        _ref_cache["tag"], _ref_cache["full"] = tag, gpu.topk_reference(keys, keys.size, vals, key_type, descending)
    rk, rv = _ref_cache["full"]
    return rk[:k], rv[:k]


def _run(gpu, keys, k, mode="keys", key_type=0, descending=False, handle=None, pad=5, dkeys=None):
    """Selects on the GPU into outputs over-allocated by `pad`, compares with the reference, checks that the inputs and the padding
    are untouched, returns last()."""
    torch = _torch()
    n, vb = keys.size, _vb(mode)
    vals = _values(n, mode)
    h = handle or _handle(gpu, n, k, mode, key_type, descending)
    dk = _dev(keys) if dkeys is None else dkeys
    dv = _dev(vals) if vals is not None else None
    ok = torch.full((k + pad,), 0x5EEDBEEF, dtype=torch.int32, device="cuda")
    ov = None
    if vb:
        ov = torch.full((k + pad,), 0x5EEDBEEF, dtype=torch.int32 if vb == 4 else torch.int64, device="cuda")
    h.select(dk, k, ok, dv, ov, n=n)
    h.check()
    rep = h.last()
    if handle is None:
        h.close()
    rk, rv = _reference(gpu, keys, k, vals, key_type, descending)
    hk = ok.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(hk[:k], rk)
    assert np.all(hk[k:] == 0x5EEDBEEF), "nothing behind the k-th output key is written"
    if vb:
        hv = ov.cpu().numpy().view(VALUE_DTYPE[vb])
        np.testing.assert_array_equal(hv[:k], rv.astype(VALUE_DTYPE[vb]))
        assert np.all(hv[k:] == 0x5EEDBEEF), "nothing behind the k-th output value is written"
        if dv is not None:
            np.testing.assert_array_equal(dv.cpu().numpy().view(VALUE_DTYPE[vb]), vals)
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32)[:n], keys)
    return rep


def _check_report(gpu, rep, keys, k, key_type, descending, vb):
    """Route by size; on the select route the counts bracket k and T is the reference's k-th key."""
    from gpusorting_amd.segsort import sortable_bits
    if keys.size <= SINGLE_TILE[vb]:
        assert rep["route"] == SINGLE
        return
    assert rep["route"] == SELECT and rep["level2"] == 1
    bits = sortable_bits(keys, key_type)
    kth = sortable_bits(_reference(gpu, keys, k, None, key_type, descending)[0][-1:], key_type)[0]
    assert rep["threshold"] == int(kth)
    in_front = int(np.count_nonzero(bits > kth if descending else bits < kth))
    equal = int(np.count_nonzero(bits == kth))
    assert rep["in_front"] == in_front and rep["equal"] == equal and rep["taken"] == k - in_front
    assert rep["in_front"] < k <= rep["in_front"] + rep["equal"]
    assert rep["candidates"] == int(np.count_nonzero((bits >> 16) == (kth >> 16)))


def _ks(n):
    return sorted({k for k in KS + (n // 2, n - 1, n) if 1 <= k <= n})


@pytest.mark.parametrize("key_type", [0, 1, 2])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_types_orders_modes(gpu, key_type, descending, mode):
    for n, preset in ((100_003, gpu.ENTROPY_PRESET_1), (300_001, gpu.ENTROPY_PRESET_3), (20_000, gpu.ENTROPY_PRESET_5)):
        keys = _keys(gpu, n, 40 + key_type, preset)
        if key_type == 2:
            keys[::97] = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001], dtype=np.uint32)[np.arange(keys[::97].size) % 6]
        for k in (1, 65, 1000, n // 3, n):
            rep = _run(gpu, keys, k, mode, key_type, descending)
            _check_report(gpu, rep, keys, k, key_type, descending, _vb(mode))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, (1 << 16) + 1, (1 << 20) - 1])
@pytest.mark.parametrize("mode", MODES)
def test_sizes_and_ks(gpu, n, mode):
    for i, preset in enumerate((gpu.ENTROPY_PRESET_1, gpu.ENTROPY_PRESET_2, gpu.ENTROPY_PRESET_3, gpu.ENTROPY_PRESET_4, gpu.ENTROPY_PRESET_5)):
        keys = _keys(gpu, n, 7 * n + i, preset)
        descending = bool(i & 1)
        h = _handle(gpu, n, n, mode, 0, descending)
        for k in _ks(n):
            rep = _run(gpu, keys, k, mode, 0, descending, handle=h)
            _check_report(gpu, rep, keys, k, 0, descending, _vb(mode))
        h.close()


@pytest.mark.parametrize("descending", [False, True])
def test_sixteen_million_and_three(gpu, descending):
    n = (1 << 24) + 3
    for i, preset in enumerate((gpu.ENTROPY_PRESET_1, gpu.ENTROPY_PRESET_5)):
        keys = _keys(gpu, n, 900 + i, preset)
        h = _handle(gpu, n, n, "pos", 0, descending)
        dk = _dev(keys)
        for k in _ks(n):
            rep = _run(gpu, keys, k, "pos", 0, descending, handle=h, dkeys=dk)
            assert rep["route"] == SELECT
            if k <= 1 << 16:
                _check_report(gpu, rep, keys, k, 0, descending, 4)
        h.close()


def _structured(name, n, rng):
    if name == "all-equal":
        return np.full(n, 0xC0FFEE00, dtype=np.uint32)
    if name == "half-one-key":  # every second element the same key, the others random: k falls inside the run
        keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        keys[rng.permutation(n)[: n // 2]] = 0x80000000
        return keys
    if name == "shared-top-16":
        return (rng.integers(0, 1 << 16, size=n, dtype=np.uint64).astype(np.uint32)) | np.uint32(0xABCD0000)
    if name == "lowest-byte":
        return (rng.integers(0, 256, size=n, dtype=np.uint64).astype(np.uint32)) | np.uint32(0x12345600)
    if name == "sorted":
        return np.sort(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    if name == "reverse-sorted":
        return np.sort(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))[::-1].copy()
    if name == "heavy-prefix":  # one 16-bit prefix holds 3/4 of the keys, scattered
        keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        heavy = rng.permutation(n)[: n // 4 * 3]
        keys[heavy] = (keys[heavy] & np.uint32(0xFFFF)) | np.uint32(0x7FFF0000)
        return keys
    if name == "two-heavy-prefixes":  # two such prefixes, 2/5 of the keys each
        keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        pick = rng.permutation(n)
        a, b = pick[: n * 2 // 5], pick[n * 2 // 5: n * 4 // 5]
        keys[a] = (keys[a] & np.uint32(0xFF)) | np.uint32(0x00010000)
        keys[b] = (keys[b] & np.uint32(0xFF)) | np.uint32(0xFFFE0000)
        return keys
    raise AssertionError(name)


STRUCTURES = ("all-equal", "half-one-key", "shared-top-16", "lowest-byte", "sorted", "reverse-sorted", "heavy-prefix", "two-heavy-prefixes")


@pytest.mark.parametrize("name", STRUCTURES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("mode", ["pos", "v8", "keys"])
def test_inputs_against_the_structure(gpu, name, descending, mode):
    n = (1 << 22) + 77
    keys = _structured(name, n, np.random.default_rng(sum(map(ord, name))))
    h = _handle(gpu, n, n // 2 + 9, mode, 0, descending)
    dk = _dev(keys)
    for k in (1, 1000, n // 4 + 3, n // 2 + 9):
        rep = _run(gpu, keys, k, mode, 0, descending, handle=h, dkeys=dk)
        _check_report(gpu, rep, keys, k, 0, descending, _vb(mode))
        if name in ("all-equal", "shared-top-16", "lowest-byte"):
            assert rep["candidates"] == n and rep["level2"] == 1, "level 2 runs on all n candidates"
        if name == "half-one-key" and k == n // 2 + 9:
            assert rep["threshold"] == 0x80000000 and 0 < rep["taken"] < rep["equal"], "k falls inside the run: the tie rule decides"
    h.close()


@pytest.mark.parametrize("descending", [False, True])
def test_packed_counter_overflow(gpu, descending):
    """2^26 keys in 256 ranges of 262 144: two 16-bit prefixes hold 2/5 of every range each, 104 857 keys — the range's register-counted
    bin takes one of them at most, the other one wraps its packed 16-bit counter and the range recounts itself."""
    n = (1 << 26) + 5
    keys = _structured("two-heavy-prefixes", n, np.random.default_rng(8))
    h = _handle(gpu, n, n // 2 + 9, "pos", 0, descending)
    dk = _dev(keys)
    for k in (1000, n // 2 + 9):
        rep = _run(gpu, keys, k, "pos", 0, descending, handle=h, dkeys=dk)
        _check_report(gpu, rep, keys, k, 0, descending, 4)
    h.close()


@pytest.mark.parametrize("key_type", [1, 2])
def test_ties_inside_a_run_signed_and_float(gpu, key_type):
    n = 500_000
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[rng.permutation(n)[: n // 2]] = 0x80000000 if key_type == 2 else 0  # -0.0 / 0
    keys[rng.permutation(n)[: n // 8]] = 0x00000000 if key_type == 2 else 1  # +0.0 / 1
    for descending in (False, True):
        for k in (n // 3, n // 2, n * 3 // 4):
            for mode in ("pos", "v4"):
                rep = _run(gpu, keys, k, mode, key_type, descending)
                _check_report(gpu, rep, keys, k, key_type, descending, 4)


@pytest.mark.parametrize("descending", [False, True])
def test_full_size_positions(gpu, descending):
    torch = _torch()
    n, k = 1 << 28, 1024
    dk = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu.init_random(dk, 4242, gpu.ENTROPY_PRESET_1)
    torch.cuda.synchronize()
    keys = dk.cpu().numpy().view(np.uint32).copy()
    rep = _run(gpu, keys, k, "pos", 0, descending, dkeys=dk)
    assert rep["route"] == SELECT and rep["in_front"] < k <= rep["in_front"] + rep["equal"]
    assert rep["candidates"] < n >> 10, "spread keys: level 2 sees a sliver"


def test_small_k_on_spread_keys_takes_the_select_route(gpu):
    n = 1 << 22
    keys = _keys(gpu, n, 11, gpu.ENTROPY_PRESET_1)
    for k in (1, 64, 1024):
        for descending in (False, True):
            rep = _run(gpu, keys, k, "pos", 0, descending)
            _check_report(gpu, rep, keys, k, 0, descending, 4)
            assert rep["route"] == SELECT and rep["candidates"] < 1024, "a silent full sort cannot pass as a select"


def test_handle_reuse_and_two_streams(gpu):
    torch = _torch()
    h = _handle(gpu, 1 << 21, 1 << 20, "pos")
    for n, k in (((1 << 21), 1000), (5, 5), (70_001, 70_000), ((1 << 20) + 1, 1), (40_000, 1 << 10), ((1 << 21) - 3, 1 << 20)):
        _run(gpu, _keys(gpu, n, n + k, gpu.ENTROPY_PRESET_2), k, "pos", handle=h)
    h.close()
    n, k = (1 << 20) + 17, 5000
    ka, kb = _keys(gpu, n, 1, gpu.ENTROPY_PRESET_1), _keys(gpu, n, 2, gpu.ENTROPY_PRESET_4)
    ha, hb = _handle(gpu, n, k, "pos"), _handle(gpu, n, k, "pos", descending=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = _dev(ka), _dev(kb)
    outs = [(torch.empty(k, dtype=torch.int32, device="cuda"), torch.empty(k, dtype=torch.int32, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        ha.select(da, k, outs[0][0], None, outs[0][1], stream=sa)
        hb.select(db, k, outs[1][0], None, outs[1][1], stream=sb)
    ha.check(sa)
    hb.check(sb)
    for keys, (ok, ov), desc in ((ka, outs[0], False), (kb, outs[1], True)):
        rk, rv = gpu.topk_reference(keys, k, None, 0, desc)
        np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), rv)
    ha.close()
    hb.close()


def test_captured_graph_replayed_on_new_data(gpu):
    torch = _torch()
    n, k = (1 << 21) + 5, 777
    h = _handle(gpu, n, k, "pos", 2, True)
    first = _keys(gpu, n, 31, gpu.ENTROPY_PRESET_1)
    dk = _dev(first)
    ok = torch.empty(k, dtype=torch.int32, device="cuda")
    ov = torch.empty(k, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        h.select(dk, k, ok, None, ov)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h.select(dk, k, ok, None, ov)
    for seed, preset in ((32, gpu.ENTROPY_PRESET_1), (33, gpu.ENTROPY_PRESET_5), (34, gpu.ENTROPY_PRESET_3)):
        keys = _keys(gpu, n, seed, preset)
        dk.copy_(_dev(keys))
        ok.zero_()
        ov.zero_()
        graph.replay()
        torch.cuda.synchronize()
        h.check()
        rk, rv = gpu.topk_reference(keys, k, None, 2, True)
        np.testing.assert_array_equal(ok.cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(ov.cpu().numpy().view(np.uint32), rv)
    h.close()


def test_functional_topk(gpu):
    torch = _torch()
    n = 300_000
    keys = _keys(gpu, n, 5, gpu.ENTROPY_PRESET_1)
    x = torch.from_numpy(keys.view(np.float32).copy()).cuda()
    for largest in (True, False):
        v, i = gpu.topk(x, 50, largest=largest)
        rk, rv = gpu.topk_reference(keys, 50, None, 2, largest)
        assert i.dtype == torch.int32 and v.dtype == torch.float32
        np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), rk)
        np.testing.assert_array_equal(i.cpu().numpy().view(np.uint32), rv)
    xi = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    vals = torch.arange(n, dtype=torch.int64, device="cuda") * 3
    v, w = gpu.topk(xi, 1234, largest=False, values=vals, unsigned=True)
    rk, rv = gpu.topk_reference(keys, 1234, np.arange(n, dtype=np.uint64) * 3, 0, False)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint32), rk)
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint64), rv)


def test_error_returns(gpu):
    from gpusorting_amd import _lib
    torch = _torch()
    lib = _lib.load()
    n = 100_000
    dk = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    outv = torch.zeros(n, dtype=torch.int64, device="cuda")
    hk = gpu.TopK(n, 1000)
    hp = gpu.TopK(n, 1000, mode=gpu.MODE_PAIRS, value_bytes=4)
    h8 = gpu.TopK(n, 1000, mode=gpu.MODE_PAIRS, value_bytes=8)
    p = lambda t: t.data_ptr()  # noqa: E731
    assert lib.gs_topk_select_keys(hk._h, p(dk), 10, 11, p(out), 0, 0, None) == _lib.GS_ERR_SIZE      # k > n
    assert lib.gs_topk_select_keys(hk._h, p(dk), n, 1001, p(out), 0, 0, None) == _lib.GS_ERR_SIZE     # k > max_k
    assert lib.gs_topk_select_keys(hk._h, p(dk), n, 0, p(out), 0, 0, None) == _lib.GS_ERR_SIZE        # k == 0
    for kt in (3, 4, 5):                                                                              # 64-bit key types
        assert lib.gs_topk_select_keys(hk._h, p(dk), n, 10, p(out), kt, 0, None) == _lib.GS_ERR_ARG
    assert lib.gs_topk_select_keys(hk._h, p(dk) + 4, 100, 10, p(out), 0, 0, None) == _lib.GS_ERR_ARG  # misaligned
    assert lib.gs_topk_select_keys(hk._h, p(dk), n, 10, p(dk), 0, 0, None) == _lib.GS_ERR_ARG         # output overlaps the input
    assert lib.gs_topk_select_pairs(hk._h, p(dk), p(dk), n, 10, p(out), p(outv), 0, 0, None) == _lib.GS_ERR_MODE
    assert lib.gs_topk_select_keys(hp._h, p(dk), n, 10, p(out), 0, 0, None) == _lib.GS_ERR_MODE
    assert lib.gs_topk_select_pairs(h8._h, p(dk), None, n, 10, p(out), p(outv), 0, 0, None) == _lib.GS_ERR_ARG  # positions are 4 bytes
    assert lib.gs_topk_select_pairs(hp._h, p(dk), None, n, 10, p(out), None, 0, 0, None) == _lib.GS_ERR_ARG
    for h in (hk, hp, h8):
        assert h.status() == _lib.GS_OK and h.last()["route"] == 0
        h.close()
