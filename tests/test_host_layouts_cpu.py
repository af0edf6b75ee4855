"""CPU test of every host-only sizing entry of the C-ABI: the *_temp_bytes, *_units and *_plan functions, over a small grid of sizes,
segment counts, mode / value-width pairs and refused arguments.  The expected values are not computed here: tests/golden/
host_layouts.json holds what the library of the commit *before* the handle core (handle_core.hpp: one layout arena for all the
layout functions) returned for the same grid, so a change of a layout, a rounding, a plan or a refusal shows as a difference.

The file was recorded by running this module as a script against that older build:

    GPUSORT_LIB=<the older libgpusort.so> python tests/test_host_layouts_cpu.py tests/golden/host_layouts.json

gs_segsort_temp_bytes and gs_topk_temp_bytes add gs_onesweep_temp_bytes of their engine, which depends on the device's compute units;
the grid records them with that term subtracted (the engine's sizing is not the subject here).  No compute is run."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_layouts.json")
KEYS, PAIRS = 0, 1
MODES = ((KEYS, 0), (PAIRS, 4), (PAIRS, 8))
BAD_MODES = ((KEYS, 4), (PAIRS, 0), (PAIRS, 2), (7, 0))
MAX = (1 << 30) - 1                                        # GS_MAX_KEYS
SIZES = (1, 63, 65, 4095, 4097, 1000003, (1 << 27) + 1, MAX)   # 63, 4095: just below a multiple of 64; 65, 4097: just above
SEGMENTS = (1, 63, 64, 1 << 20)
BAD_SIZES = (0, MAX + 1)
PLAN_WORDS = 8                                             # GS_SORT_ROWS_PLAN_WORDS; gs_sort16_plan writes 4


def _plan(fn, *args):
    plan = (C.c_uint32 * PLAN_WORDS)(*([0xdeadbeef] * PLAN_WORDS))   # words the entry does not write stay as they are
    return [fn(*args, plan), list(plan)]


def _topk_sort_cap(max_keys, max_k):
    """The capacity of gs_topk's engine (include/gpusort.h, gs_topk_create): max_k, or the single-tile route's 32 768 keys if larger."""
    return max(max_k, min(max_keys, 32768))


def grid(lib):
    """Every call of the grid as (entry, args, result), in a fixed order."""
    out = []

    def add(entry, args, result):
        out.append([entry, [int(a) for a in args], result])

    # (max_keys, mode, value_bytes): the flat 16-bit sort and the two row-wise sorts
    for name in ("gs_sort16_temp_bytes", "gs_sort_rows_temp_bytes", "gs_sort_rows16_temp_bytes"):
        fn = getattr(lib, name)
        for mode, vb in MODES:
            for n in SIZES + BAD_SIZES:
                add(name, (n, mode, vb), fn(n, mode, vb))
        for mode, vb in BAD_MODES:
            add(name, (4097, mode, vb), fn(4097, mode, vb))
    # (max_keys, max_segments, mode, value_bytes): the long routes of the two segmented sorts
    for name in ("gs_segsort_long_temp_bytes", "gs_segsort_long_units", "gs_segsort16_temp_bytes", "gs_segsort16_units"):
        fn = getattr(lib, name)
        for mode, vb in MODES:
            for n in SIZES + BAD_SIZES:
                for segs in SEGMENTS:
                    add(name, (n, segs, mode, vb), fn(n, segs, mode, vb))
            for segs in BAD_SIZES:
                add(name, (4097, segs, mode, vb), fn(4097, segs, mode, vb))
        for mode, vb in BAD_MODES:
            add(name, (4097, 64, mode, vb), fn(4097, 64, mode, vb))
    # (max_keys, max_segments): the 32-bit segmented sort's control block and class lists, its engine's term subtracted
    for n in SIZES:
        for segs in SEGMENTS:
            add("gs_segsort_temp_bytes - gs_onesweep_temp_bytes", (n, segs), lib.gs_segsort_temp_bytes(n, segs) - lib.gs_onesweep_temp_bytes(n))
    # (max_segments): the two segmented selections
    for name in ("gs_segtopk_temp_bytes", "gs_segtopk16_temp_bytes"):
        for segs in SEGMENTS + (2, 65, MAX):
            add(name, (segs,), getattr(lib, name)(segs))
    # (max_keys, max_k, value_bytes): the selection, its engine's term subtracted
    for vb in (0, 4, 8):
        for n in SIZES:
            for k in sorted({1, min(n, 64), min(n, 40000), n}):
                add("gs_topk_temp_bytes - gs_onesweep_temp_bytes", (n, k, vb),
                    lib.gs_topk_temp_bytes(n, k, vb) - lib.gs_onesweep_temp_bytes(_topk_sort_cap(n, k)))
    # the plans.  (n, mode, value_bytes) and (rows, row_len, mode, value_bytes); products above GS_MAX_KEYS and zeros are refused
    for mode, vb in MODES + BAD_MODES:
        for n in (SIZES + BAD_SIZES if (mode, vb) in MODES else (4097, 0)):
            add("gs_sort16_plan", (n, mode, vb), _plan(lib.gs_sort16_plan, n, mode, vb))
    add("gs_sort16_plan(null)", (4097, KEYS, 0), lib.gs_sort16_plan(4097, KEYS, 0, None))
    for name in ("gs_sort_rows_plan", "gs_sort_rows16_plan"):
        fn = getattr(lib, name)
        for mode, vb in MODES:
            for rows in (0, 1, 63, 65, 1 << 20):
                for row_len in (0, 1, 63, 65, 1023, 4097, 32768, 32769, 1000003, MAX):
                    add(name, (rows, row_len, mode, vb), _plan(fn, rows, row_len, mode, vb))
        for mode, vb in BAD_MODES:
            add(name, (65, 4097, mode, vb), _plan(fn, 65, 4097, mode, vb))
        add(name + "(null)", (65, 4097, KEYS, 0), fn(65, 4097, KEYS, 0, None))
    return out


def test_every_sizing_entry_returns_what_the_parent_library_returned():
    from gpusorting_amd import _lib
    assert _lib.GS_MAX_KEYS == MAX and _lib.GS_SORT_ROWS_PLAN_WORDS == PLAN_WORDS
    golden = json.load(open(GOLDEN))["cases"]
    got = grid(_lib.load())
    assert [c[:2] for c in got] == [c[:2] for c in golden], "the grid of this test and of the recorded file differ"
    wrong = [(g[0], g[1], g[2], w[2]) for g, w in zip(got, golden) if g[2] != w[2]]
    assert not wrong, f"{len(wrong)} of {len(got)} differ; (entry, args, got, recorded): {wrong[:8]}"


def test_the_grid_covers_every_entry_and_is_not_vacuous():
    cases = json.load(open(GOLDEN))["cases"]
    entries = {c[0].split(" ")[0].split("(")[0] for c in cases}
    assert entries == {"gs_sort16_temp_bytes", "gs_sort_rows_temp_bytes", "gs_sort_rows16_temp_bytes", "gs_segsort_temp_bytes",
                       "gs_segsort_long_temp_bytes", "gs_segsort16_temp_bytes", "gs_segtopk_temp_bytes", "gs_segtopk16_temp_bytes",
                       "gs_topk_temp_bytes", "gs_segsort_long_units", "gs_segsort16_units", "gs_sort16_plan", "gs_sort_rows_plan",
                       "gs_sort_rows16_plan"}
    for entry in entries:
        results = [json.dumps(c[2]) for c in cases if c[0].split(" ")[0].split("(")[0] == entry]
        assert len(set(results)) >= 3, entry                  # the arguments change the answer (gs_sort16's: keys, pairs, refused)
    # refusals are in it: 0 bytes / units, and each status a plan entry can give without a device (OK, ARG, SIZE, MODE)
    assert any(c[2] == 0 for c in cases if c[0] == "gs_sort_rows_temp_bytes") and any(c[2] == 0 for c in cases if c[0] == "gs_segsort16_units")
    assert {c[2][0] for c in cases if c[0] == "gs_sort_rows16_plan"} == {0, 2, 5} and {c[2] for c in cases if c[0].endswith("(null)")} == {1}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from gpusorting_amd import _lib
    with open(sys.argv[1], "w") as f:
        json.dump({"recorded_from": "the library of the commit before handle_core.hpp, by tests/test_host_layouts_cpu.py run as a script",
                   "cases": grid(_lib.load())}, f, separators=(",", ":"))
        f.write("\n")
