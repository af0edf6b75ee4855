#!/usr/bin/env python3
"""The segmented sort's two routes for long 32-bit segments against each other, on one GPU; prints one JSON line.

--n uint32 keys under a list of offset sets (--shapes):
  mix        the heavy-tailed mix of tools/segsort16_perf.py: about two million segments, a few hundred of them long;
  RxL        R long segments of L elements (256x131072, 2048x65536, 32x4194304, 3x33554432);
  above      segments of one element more than the LDS limit of the mode, as many as n holds, 16 000 at the most.
Each as a keys-only sort, with 4-byte and with 8-byte values (--modes).  Per shape and mode, on ONE handle:
  device     gs_segsort_set_long_route(h, GS_SEGSORT_LONG_DEVICE): four passes over all long segments at once, no host wait;
  host       GS_SEGSORT_LONG_HOST, the default: one host wait for the list of long segments, one per long segment, the engine sorts each.
Both with max_segment_len = 0.  The two alternate in one process, both warmed, --reps timed repetitions each (device events around every
single call, fresh input copied in before it, outside the events; the host route's waits lie inside, as a caller pays them); median,
extremes and spread (max - min over min) per side.  The result of EVERY repetition, warm-up ones included, is compared bit for bit (keys
and values) with the other route's result on the same input, behind the timed span.  The JSON names the part size the library was built
with (read from gs_segsort_long_units) and, where GPUSORT_LIB picked another build, that library's file name."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from segsort16_perf import lengths as lengths16  # noqa: E402
from sort_rows_perf import stats  # noqa: E402

SHAPES = ("mix", "256x131072", "2048x65536", "above", "32x4194304", "3x33554432")
MODES = ("keys", "pairs4", "pairs8")


def lengths(shape: str, n: int, lds: int) -> np.ndarray:
    if shape == "above":
        return np.full(min(16000, n // (lds + 1)), lds + 1, dtype=np.int64)
    return lengths16(shape, n, lds)


def part_of(lib) -> int:
    """GS_SEGSORT_LONG_PART of the loaded library: gs_segsort_long_units(n, 1, keys only) = n / part + 1 for n above the LDS limit."""
    n = 1 << 24
    return n // (int(lib.gs_segsort_long_units(n, 1, g.MODE_KEYS_ONLY, 0)) - 1)


def timed_checked(fn, reset, reps, warm, result, want):
    """`reps` timed repetitions behind `warm` untimed ones, device events around every call; behind each one's span its result() must
    equal `want` (None: nothing to compare with yet).  Returns the times and whether every comparison held."""
    times, same = [], True
    for i in range(warm + reps):
        reset()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if i >= warm:
            times.append(s.elapsed_time(e))
        if want is not None:
            same = same and all(torch.equal(a, b) for a, b in zip(result(), want))
    return times, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    total = args.n
    src = torch.empty(total, dtype=torch.int32, device=dev)
    g.init_random(src, 12345, g.ENTROPY_PRESET_1)
    keys = torch.empty(total, dtype=torch.int32, device=dev)
    index = {4: torch.arange(total, dtype=torch.int32, device=dev), 8: torch.arange(total, dtype=torch.int64, device=dev)}
    vals = {vb: torch.empty_like(t) for vb, t in index.items()}
    lib = g._lib.load()
    out_rows = []
    for shape in args.shapes.split(","):
        for what in args.modes.split(","):
            vb = {"keys": 0, "pairs4": 4, "pairs8": 8}[what]
            mode = g.MODE_PAIRS if vb else g.MODE_KEYS_ONLY
            lds = int(lib.gs_segsort_max_lds_segment(mode, vb))
            lens = lengths(shape, total, lds)
            offsets = np.concatenate(([0], np.cumsum(lens)))
            n, segs = int(offsets[-1]), int(lens.size)
            d_off = torch.from_numpy(offsets.astype(np.int32)).to(dev)
            s = g.SegmentedSort(n, segs, key_type=g.KEY_UINT32, mode=mode, value_bytes=vb, long_route="device")

            def reset():
                keys[:n].copy_(src[:n])
                if vb:
                    vals[vb][:n].copy_(index[vb][:n])

            def run():
                s.sort(keys, d_off, vals[vb] if vb else None, n=n)

            def result():
                return (keys[:n], vals[vb][:n]) if vb else (keys[:n],)

            # what each route gives on this input, once, untimed: every repetition of the OTHER route is compared with it
            kept = {}
            for route in ("device", "host"):
                s.set_long_route(route)
                reset()
                run()
                s.check()
                kept[route] = tuple(t.clone() for t in result())
                if route == "device":
                    last, cls = s.last(), s.last_classes()
            times = {"device": [], "host": []}
            same = all(torch.equal(a, b) for a, b in zip(kept["device"], kept["host"]))
            for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the two: half the repetitions each, twice
                for route, other in (("device", "host"), ("host", "device")):
                    s.set_long_route(route)
                    t, ok = timed_checked(run, reset, max(half, 1), 2, result, kept[other])
                    times[route] += t
                    same = same and ok
                    s.check()
            same = bool(same)
            kept.clear()
            a, b = stats(times["device"]), stats(times["host"])
            row = {"shape": shape, "mode": what, "n": n, "segments": segs, "longest": cls["longest"], "long_segments": last["long"],
                   "units": last["units"], "unit_cap": last["unit_cap"], "device_route": a, "host_route": b, "host_over_device": b["median_ms"] / a["median_ms"],
                   # the criterion of DESIGN.md 3.8: the new side's slowest run against the old side's fastest
                   "device_slowest_beats_host_fastest": bool(a["max_ms"] < b["min_ms"]), "device_gkeys_per_s": n / a["median_ms"] / 1e6,
                   "routes_agree": same}
            out_rows.append(row)
            print(f"# {shape:12s} {what:7s} segs {segs:8d} long {last['long']:5d} units {last['units']:5d}  device {a['median_ms']:9.3f} ms "
                  f"[{a['min_ms']:.3f}, {a['max_ms']:.3f}]  host {b['median_ms']:9.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]  "
                  f"x{row['host_over_device']:.2f}  agree {same}", file=sys.stderr, flush=True)
            s.close()
    out = {"tool": "segsort_long_perf", "n": args.n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "key_type": "uint32",
           "part": part_of(lib), "part_tiles": part_of(lib) // g._lib.GS_SORT_ROWS_TILE,
           "library": os.path.basename(os.environ["GPUSORT_LIB"]) if "GPUSORT_LIB" in os.environ else "libgpusort.so",
           "baseline": "the host route on the same handle (GS_SEGSORT_LONG_HOST, the default), max_segment_len = 0, its host waits inside the timed span",
           "rows": out_rows}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
