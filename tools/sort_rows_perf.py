#!/usr/bin/env python3
"""Row-wise sort against what the library had before it, on one GPU; prints one JSON line.

Shapes [rows, row_len] of 2^24 .. 2^25 uniform-random uint32 elements (--shapes), each as a keys-only sort and as an argsort (4-byte
values = the position within the row).  Per shape and mode:
  rowsort   gs_sort_rows_* (RowSort): the LDS route up to gs_segsort_max_lds_segment, the pass route above (13 launches, no host wait);
  baseline  the only way to sort rows before: gs_segsort_sort_* (SegmentedSort) on uniform CSR offsets over the same data — with
            max_segment_len = row_len where the row fits LDS (its asynchronous path), and max_segment_len = 0 above, where every row is
            a class-8 segment sorted one by one by the embedded 1-D engine behind a host wait;
  torch     torch.sort(x, dim=-1, stable=True), which always returns values and indices: recorded for information.
rowsort and baseline alternate in one process, both warmed, --reps timed repetitions each (device events around every single call —
the baseline's host waits lie inside them — with fresh input copied in before it, outside the events); median and spread (max - min
over min) per side; GB/s = 2 x element bytes x n over the median.  --check compares the two results bit for bit."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd.rowsort import ROUTE_PASSES, sort_rows_plan  # noqa: E402

SHAPES = ((4096, 4096), (1024, 32768), (256, 131072), (32, 262144), (4, 1 << 22), (1 << 16, 256))


def timed(fn, reset, reps, warm=3):
    times = []
    for i in range(warm + reps):
        reset()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if i >= warm:
            times.append(s.elapsed_time(e))
    return times


def stats(times):
    t = np.asarray(times)
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "spread": float((t.max() - t.min()) / t.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(f"{r}x{n}" for r, n in SHAPES), help="rows x row_len, comma separated")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--check", action="store_true", help="compare every rowsort result with the baseline's")
    ap.add_argument("--no-torch", action="store_true", help="leave torch.sort out")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.lower().split("x")) for s in args.shapes.split(",")]
    total = max(r * n for r, n in shapes)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    src = torch.empty(total, dtype=torch.int32, device=dev)
    g.init_random(src, 12345, g.ENTROPY_PRESET_1)
    keys, vals, kept = (torch.empty(total, dtype=torch.int32, device=dev) for _ in range(3))
    out_rows = []
    for rows, row_len in shapes:
        n = rows * row_len
        pos = torch.arange(row_len, dtype=torch.int32, device=dev).repeat(rows)
        d_off = (torch.arange(rows + 1, dtype=torch.int64, device=dev) * row_len).to(torch.int32)
        for vb in (0, 4):
            mode = g.MODE_PAIRS if vb else g.MODE_KEYS_ONLY
            plan = sort_rows_plan(rows, row_len, mode, vb)
            passes = plan["route"] == ROUTE_PASSES
            rs = g.RowSort(n, mode=mode, value_bytes=vb)
            seg = g.SegmentedSort(n, rows, mode=mode, value_bytes=vb)
            k2, v2 = keys[:n].view(rows, row_len), vals[:n].view(rows, row_len)

            def reset():
                keys[:n].copy_(src[:n])
                if vb:
                    vals[:n].copy_(pos)

            run_rows = lambda: rs.sort(k2, v2 if vb else None)  # noqa: E731
            run_base = lambda: seg.sort(keys, d_off, vals if vb else None, n=n, max_segment_len=0 if passes else row_len)  # noqa: E731
            t_rows, t_base = [], []
            for _ in range(2):  # alternate the two: half the repetitions each, twice
                t_rows += timed(run_rows, reset, args.reps // 2)
                t_base += timed(run_base, reset, args.reps // 2)
            rs.check()
            seg.check()
            ok = None
            if args.check:
                reset()
                run_base()
                kept[:n].copy_(keys[:n])
                kept_v = vals[:n].clone() if vb else None
                reset()
                run_rows()
                ok = bool(torch.equal(keys[:n], kept[:n]) and (not vb or torch.equal(vals[:n], kept_v)))
            t_torch = None
            if not args.no_torch:
                x = src[:n].view(rows, row_len)
                t_torch = stats(timed(lambda: torch.sort(x, dim=-1, stable=True), lambda: None, max(args.reps // 4, 3)))
            s_rows, s_base = stats(t_rows), stats(t_base)
            byts = 2 * (4 + vb) * n
            last = rs.last()
            row = {"rows": rows, "row_len": row_len, "mode": "argsort" if vb else "keys", "n": n, "route": "passes" if passes else "lds",
                   "parts": last["parts"], "per_part": last["per_part"], "launches": 1 + 3 * plan["passes"] if passes else None,
                   "rowsort": s_rows, "baseline_segsort": s_base, "baseline_max_segment_len": 0 if passes else row_len,
                   "speedup": s_base["median_ms"] / s_rows["median_ms"], "rowsort_wins_beyond_spread": bool(s_rows["max_ms"] < s_base["min_ms"]),
                   "baseline_wins_beyond_spread": bool(s_base["max_ms"] < s_rows["min_ms"]), "rowsort_gbps": byts / s_rows["median_ms"] / 1e6,
                   "rowsort_gkeys_per_s": n / s_rows["median_ms"] / 1e6, "torch_sort": t_torch, "matches_baseline": ok}
            out_rows.append(row)
            print(f"# {rows:6d} x {row_len:8d} {row['mode']:8s} {row['route']:6s} rowsort {s_rows['median_ms']:8.3f} ms (spread {s_rows['spread']:.3f})  "
                  f"baseline {s_base['median_ms']:8.3f} ms (spread {s_base['spread']:.3f})  x{row['speedup']:.2f}"
                  + (f"  torch {t_torch['median_ms']:8.3f} ms" if t_torch else "") + (f"  match {ok}" if ok is not None else ""), file=sys.stderr, flush=True)
            rs.close()
            seg.close()
    out = {"tool": "sort_rows_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "baseline": "gs_segsort_sort_* on uniform offsets, same library (the segmented sort is unchanged); rows above the LDS limit are its class 8",
           "rows": out_rows}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
