"""Characterisation of the C-ABI's host side on the GPU: what the structural entry points (GlobalHistogram, Scan, the two
multi-GPU histograms) answer to bad arguments — and in which order their checks fire —, that a refused call leaves the
handle usable, and what the profile of the two one-launch routes looks like.  The expected statuses are the ones the
library returned before its host side was split into one file per handle; they are written out, not derived."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 20000  # above the 8192-key single-tile limit, with a partial tile: the two-launch mid-size route
ARG, SIZE = 1, 2  # GS_ERR_ARG, GS_ERR_SIZE (include/gpusort.h)
ENTRIES = ("gs_onesweep_global_histogram", "gs_onesweep_scan", "gs_onesweep_msd_prepare", "gs_onesweep_msd_fine_histogram")
# (key type, keys pointer offset in bytes, output given, n - None: max_keys + 1) -> status.  The last case fails two checks:
# the argument check fires first.
REFUSALS = (("kt = 3", 3, 0, True, N, ARG),
            ("keys + 4 bytes", 0, 4, True, N, ARG),
            ("null output", 0, 0, False, N, ARG),
            ("n = 0", 0, 0, True, 0, SIZE),
            ("n = max_keys + 1", 0, 0, True, N + 1, SIZE),
            ("kt = 3 and n = 0", 3, 0, True, 0, ARG))


@pytest.fixture(scope="module")
def keys(oracle):
    return oracle.init_random(N, 7)


def _dev(a):
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def test_refused_structural_calls_keep_their_statuses_and_leave_the_handle_usable(gpu, oracle, keys):
    from gpusorting_amd import _lib
    from gpusorting_amd.onesweep import _stream_ptr
    lib = _lib.load()
    assert (_lib.GS_ERR_ARG, _lib.GS_ERR_SIZE) == (ARG, SIZE)
    plain = gpu.OneSweep(N)
    pairs = gpu.OneSweep(N, mode=gpu.MODE_PAIRS, value_bytes=4)
    dk = _dev(keys)
    out = (C.c_uint32 * 4096)()
    plain.scan_rows(dk)  # a tiled call first: gs_debug_check_state has a scan state (and HIST) to look at afterwards
    pairs.scan_rows(dk)
    for s in (plain, pairs):
        for entry in ENTRIES:
            for what, kt, off, with_out, n, want in REFUSALS:
                got = getattr(lib, entry)(s._h, dk.data_ptr() + off, n, kt, out if with_out else None, _stream_ptr())
                print(f"{entry} [{what}] -> {got}")
                assert got == want, (entry, what)
        assert s.check_state()["hist_words_nonzero"] == 0
    hist = plain.global_histogram(dk)
    for q in range(4):
        np.testing.assert_array_equal(hist[q], np.bincount((keys >> (8 * q)) & 0xFF, minlength=256))
    plain.sort(dk)
    plain.check()
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), oracle.std_sort(keys))
    vals = np.arange(N, dtype=np.uint32)
    dk, dv = _dev(keys), _dev(vals)
    pairs.sort(dk, dv)
    pairs.check()
    rk, rv = oracle.std_sort(keys, vals=vals)
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), rk)
    np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), rv)


# slots 1-6 of a one-launch route are pairs of events with nothing between them.  The largest value measured before the
# host side was split: PARENT_EMPTY_SLOT_MS; the bound is ten times that, and never below 0.02 ms.
PARENT_EMPTY_SLOT_MS = 0.00564  # slot 6 of the mid-size route; the others read 0.0045-0.0047
EMPTY_SLOT_BOUND_MS = max(0.02, 10 * PARENT_EMPTY_SLOT_MS)


def test_profile_of_the_one_launch_routes(gpu, keys):
    from gpusorting_amd import _lib
    s = gpu.OneSweep(N)
    s.set_profiling(True)
    for n in (1000, N):  # the single-tile route; the mid-size route (two launches)
        dk = _dev(keys[:n])
        s.sort(dk)
        s.check()
        p = list(s.get_profile().values())
        print(f"n = {n}: profile slots (ms) {p}")
        assert max(p[1:7]) <= EMPTY_SLOT_BOUND_MS, (n, p)
        assert p[7] >= p[0] > 0, (n, p)
    s.set_profiling(False)
    s.sort(_dev(keys))
    s.check()
    with pytest.raises(_lib.GpuSortError) as e:
        s.get_profile()
    assert e.value.status == _lib.GS_ERR_ARG
