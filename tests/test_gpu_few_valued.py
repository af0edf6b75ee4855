"""Keys-only sorts of few-valued input at the sizes where the position-chain plan left keys out of order: 2 or 16
distinct values among 2^27 / 2^28 keys, and the same layouts at 2^22 keys on 16 / 48 persistent workgroups, where a workgroup sees as
many one-digit tiles per pass as it does at full size.  Through gpu.OneSweep (the C-ABI), compared element for element on the device
with the expectation tests/few_valued_inputs.py builds from the counts alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import few_valued_inputs as fv

pytestmark = pytest.mark.gpu

TILE = 16384  # keys per tile of the keys-only position-chain passes


def _header_word(name):
    """A #define of include/gpusort.h (the status-block words of gs_debug_set_pos_grid)."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpusort.h")).read()
    return int(re.search(rf"#define {name} (\d+)u", text).group(1))


def _set_pos_grid(gpu, s, workgroups):
    gpu._lib.check(gpu._lib.load().gs_debug_set_pos_grid(s._h, workgroups), "gs_debug_set_pos_grid")


def _pos_evidence(gpu, s):
    """What the counting position-chain workgroups of the last sort left in its status block (synchronises)."""
    buf = (C.c_uint32 * 8)()
    gpu._lib.check(gpu._lib.load().gs_debug_read_slab(s._h, _header_word("GS_SLAB_STATUS_WORD"), 8, buf, None), "gs_debug_read_slab")
    return {"guard_handovers": int(buf[_header_word("GS_ST_GUARD_HANDOVERS")]), "stolen_tiles": int(buf[_header_word("GS_ST_STOLEN_TILES")])}


def _torch():
    import torch
    return torch


def _describe(out, exp, vals, n):
    """What a wrong result looks like: descents (in the order of `vals`), and the first five wrong positions with their neighbours."""
    torch = _torch()
    rank = torch.full((n,), -1, dtype=torch.int8, device=out.device)
    for j, v in enumerate(vals.tolist()):
        rank[out == v] = j
    foreign = int((rank < 0).sum().item())
    descents = int((rank[1:] < rank[:-1]).sum().item())
    wrong = torch.nonzero(out != exp)[:, 0]
    sl = fv.seglog(n)
    lines = [f"{int(wrong.numel())} wrong positions, {descents} descents, {foreign} keys that are none of the values"]
    for p in wrong[:5].tolist():
        a, b = max(p - 2, 0), min(p + 3, n)
        lines.append(f"  at {p} (mod tile {p % TILE}, mod 1 << {sl}: {p % (1 << sl)}; segment {p >> sl}): got "
                     + " ".join(f"{x & 0xFFFFFFFF:08x}" for x in out[a:b].tolist()) + f", expected {exp[p].item() & 0xFFFFFFFF:08x}")
    return "\n".join(lines)


def _values_for(gpu, v, key_type, descending, specials=()):
    """Bit patterns of v values in the library's key order for key_type (descending: reversed).  Signed and float types get values of
    both signs; `specials` replace the first values (the float zeros)."""
    from gpusorting_amd.segsort import sortable_bits  # the key-word mapping the project's numpy references use
    vals = fv.pool(v).copy()
    if key_type != gpu.KEY_UINT32:
        vals[0::2] |= np.uint32(0x80000000)
    for i, s in enumerate(specials):
        vals[i] = s
    assert len(set(vals.tolist())) == v
    vals = vals[np.argsort(sortable_bits(vals, key_type), kind="stable")]
    return vals[::-1].copy() if descending else vals


def _sort_and_compare(gpu, layout, n, reps, *, options=None, key_type=None, descending=False, values=None, pos_grid=0, want_pos=True,
                      want_two_level=False, evidence=None, seed=0):
    """Build the layout once, sort a fresh clone `reps` times on one handle, compare every result.  Returns nothing; fails with every
    wrong repetition described."""
    torch = _torch()
    key_type = gpu.KEY_UINT32 if key_type is None else key_type
    dev = torch.device("cuda", torch.cuda.current_device())
    keys, exp, counts = fv.build_torch(layout, n, dev, seed=seed, values=values)
    v, _ = fv.layout_counts(layout, n)
    vals = torch.from_numpy((fv.pool(v) if values is None else np.asarray(values, dtype=np.uint32)).view(np.int32).copy()).to(dev)
    s = gpu.OneSweep(n, key_type=key_type, order=gpu.ORDER_DESCENDING if descending else gpu.ORDER_ASCENDING, **(options or {}))
    if pos_grid:
        _set_pos_grid(gpu, s, pos_grid)
    failures = []
    for rep in range(reps):
        work = keys.clone()
        s.sort(work)
        if rep == 0 and evidence is not None:
            evidence.update(_pos_evidence(gpu, s))
        if not torch.equal(work, exp):
            failures.append(f"{layout}, n = {n}, repetition {rep}: " + _describe(work, exp, vals, n))
        del work
    plan, flags = s.last_plan(), s.pass_flags()[:4]
    s.check()
    s.close()
    assert not failures, (f"{len(failures)} of {reps} repetitions wrong (counts {counts}, border offsets {fv.border_offsets(counts, n)}, "
                          f"pass flags {flags})\n" + "\n".join(failures))
    ran = [f for f in flags if not f & gpu._lib.GS_PF_SKIP]
    assert plan["two_level"] == want_two_level, plan
    assert ran and all(bool(f & gpu._lib.GS_PF_POS) == want_pos for f in ran), (flags, want_pos)


@pytest.mark.parametrize("layout", fv.LAYOUTS)
def test_defaults_2pow28(gpu, layout):
    """Default options, 2^28 keys, twelve repetitions per layout, each exact; the position-chain plan ran (every pass that ran carries
    PF_POS, the two-level plan did not run).  Twelve is derived, not tuned: the defect showed in 9 - 10 of 12 runs, so twelve clean runs
    of a sort that still has it have probability below (3 / 12)^12 < 10^-7."""
    _sort_and_compare(gpu, layout, 1 << 28, 12)


@pytest.mark.parametrize("layout", fv.LAYOUTS)
def test_defaults_2pow27(gpu, layout):
    """The same at 2^27 keys, eight repetitions.  At the rate the defect showed here (1 run of 8) this size decides nothing — eight
    clean runs of a broken sort have probability (7 / 8)^8 = 0.34; it is kept because 2^27 is the other size class of the default routing
    (the bucket-local sort's class 0, the two-level plan offered and refused).  2^28 is the deciding size."""
    _sort_and_compare(gpu, layout, 1 << 27, 8)


@pytest.mark.parametrize("name,options,want_pos", [
    ("position_chains=2", {"position_chains": 2}, True),   # showed the defect
    ("plan=1", {"plan": 1}, True),                          # showed the defect
    ("position_chains=0", {"position_chains": 0}, False),  # control
    ("rank_mode=0", {"rank_mode": 0}, False),              # control (the position-chain forms need the LDS-atomic ranking)
])
def test_settings_2pow28(gpu, name, options, want_pos):
    """`two_random` at 2^28 keys, twelve repetitions per setting: the two settings that showed the defect and two that did not."""
    _sort_and_compare(gpu, "two_random", 1 << 28, 12, options=options, want_pos=want_pos)


@pytest.mark.parametrize("layout", ["two_exact(0)", "sixteen_exact"])
@pytest.mark.parametrize("kind", ["int32", "float32", "uint32-descending"])
def test_types_and_order_2pow28(gpu, layout, kind):
    """Signed keys with negative values, float keys with -0.0 (two values) and -0.0 / +0.0 (sixteen) among them, and the descending
    order: the expectation lists the values in the library's key order (gpusorting_amd.segsort.sortable_bits).  Four repetitions."""
    v, _ = fv.layout_counts(layout, 1 << 28)
    if kind == "int32":
        kt, desc, specials = gpu.KEY_INT32, False, ()
    elif kind == "float32":
        kt, desc, specials = gpu.KEY_FLOAT32, False, ((0x80000000,) if v == 2 else (0x80000000, 0x00000000))
    else:
        kt, desc, specials = gpu.KEY_UINT32, True, ()
    _sort_and_compare(gpu, layout, 1 << 28, 4, key_type=kt, descending=desc, values=_values_for(gpu, v, kt, desc, specials))


SMALL_OPTIONS = {"position_chains": 2, "position_chains_min_log2": 20, "mid_path": 0}


@pytest.mark.parametrize("n", [1 << 22, (1 << 22) + 12_345])
@pytest.mark.parametrize("grid", [16, 48])
def test_few_workgroups_small(gpu, grid, n):
    """The state a position-chain workgroup keeps across its tiles, at 2^22 keys: with gs_debug_set_pos_grid the passes run on 16 or 48
    persistent workgroups, so a workgroup runs 16 (5 - 6) tiles per pass, as it does at 2^28 on the default grid.  Every layout, four
    repetitions, exact.  That the paths ran is read from the sort's status block (first repetition):
    * the guard of the packed table, on 16 workgroups: one workgroup per chain runs the 16 tiles of its chain in the first pass, and
      its counter of a value it does not leave out receives up to 16 x 8192 keys of a two-valued layout (16 x 5461 or more of the
      three-valued one) for one or two output segments: counters must have gone over early (sixteen values put 16 x 1024 keys on a
      counter, below the guard's 0xC000: nothing to assert; nor on 48 workgroups, which see five or six tiles each);
    * tiles of other chains, at the ragged size on either grid: 2^22 + 12 345 keys are eight segments of 2^19 and one of 12 345 keys
      in the passes behind the first, so the workgroups of chains 9 .. 15 own nothing and every tile they run is taken from another
      chain.  (At 2^22 keys all chains hold 16 tiles and the workgroups run in step: whether a tile changes hands there is up to the
      timing, so it is printed, not asserted.)"""
    seen = {}
    for layout in fv.LAYOUTS:
        ev = {}
        _sort_and_compare(gpu, layout, n, 4, options=SMALL_OPTIONS, pos_grid=grid, evidence=ev)
        seen[layout] = ev
        if grid == 16 and (layout.startswith("two_") or layout == "three_values"):
            assert ev["guard_handovers"] > 0, (layout, ev)
        if n != 1 << 22:
            assert ev["stolen_tiles"] > 0, (layout, ev)
    print(f"grid {grid}, n {n}: {seen}")


def test_pos_grid_control(gpu):
    """gs_debug_set_pos_grid: 0 and anything from 16 up is taken, 1 .. 15 and a null handle are refused; a default-grid sort of the
    forced position-chain plan at 2^22 keys sees one tile per workgroup and hands nothing over early."""
    lib = gpu._lib.load()
    s = gpu.OneSweep(1 << 22, **SMALL_OPTIONS)
    assert lib.gs_debug_set_pos_grid(None, 0) == gpu._lib.GS_ERR_ARG
    for bad in (1, 15, 65536):
        assert lib.gs_debug_set_pos_grid(s._h, bad) == gpu._lib.GS_ERR_ARG
    for ok in (16, 17, 48, 65535, 0):
        assert lib.gs_debug_set_pos_grid(s._h, ok) == gpu._lib.GS_OK
    s.close()
    ev = {}
    _sort_and_compare(gpu, "two_random", 1 << 22, 1, options=SMALL_OPTIONS, evidence=ev)
    assert ev["guard_handovers"] == 0, ev


@pytest.mark.parametrize("layout", ["two_exact(5000)", "sixteen_random"])
def test_unique_keys_only_engine_at_defaults(gpu, layout):
    """gs_unique's keys-only engine is created with the library's defaults again (it used to switch the position-chain plan off to stay
    clear of the defect these tests are about): 2^28 keys of a layout the plan got wrong in 12 of 12 (5 of 12) runs, four calls, the
    distinct keys and their counts exact.  A misplaced key would be a run of its own: u would not be the number of values."""
    torch = _torch()
    n = 1 << 28
    dev = torch.device("cuda", torch.cuda.current_device())
    keys, exp, counts = fv.build_torch(layout, n, dev)
    del exp
    v, _ = fv.layout_counts(layout, n)
    h = gpu.Unique(n)
    for _ in range(4):
        ok, oc, num = h.unique(keys)
        assert int(num.item()) == v
        assert (ok[:v].cpu().numpy().view(np.uint32).tolist(), oc[:v].cpu().numpy().view(np.uint32).tolist()) == (fv.pool(v).tolist(), counts)
    h.check()
    h.close()
