#!/usr/bin/env python3
"""Row-wise sort of 16-bit keys against what the library had before it, on one GPU; prints one JSON line.

Shapes [rows, row_len] of bfloat16 keys (normal deviates rounded to bfloat16: heavy ties, as logits have them), each as a keys-only sort
and as an argsort.  Per shape and mode:
  rowsort16  gs_sort_rows16_* (RowSort16): the LDS route up to gs_segsort_max_lds_segment (one launch), the pass route above (two
             passes, 7 launches, no host wait);
  baseline   the only way before: widen to float32 (``.float()``), gs_sort_rows_* (RowSort) on the widened keys, narrow back
             (``.bfloat16()``) — the argsort also copies the in-row positions in, which the 32-bit route reads as values.  Widening,
             the copy of the positions and narrowing lie inside the timed span, as a caller pays them;
  torch      torch.sort(x, dim=-1, stable=True), which always returns values and indices: recorded for information.
rowsort16 and baseline alternate in one process, both warmed, --reps timed repetitions each (device events around every single call,
fresh input copied in before it, outside the events); median and spread (max - min over min) per side.  --check compares the two
results bit for bit (keys, and positions for the argsort)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd.rowsort16 import ROUTE_PASSES, sort_rows16_plan  # noqa: E402
from sort_rows_perf import SHAPES as SHAPES32, stats, timed  # noqa: E402

SHAPES = SHAPES32 + ((64, 128256), (256, 32000), (8, 151936), (1, 262144))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(f"{r}x{n}" for r, n in SHAPES), help="rows x row_len, comma separated")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--check", action="store_true", help="compare every rowsort16 result with the baseline's")
    ap.add_argument("--no-torch", action="store_true", help="leave torch.sort out")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.lower().split("x")) for s in args.shapes.split(",")]
    total = max(r * n for r, n in shapes)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(12345)
    src = torch.randn(total, dtype=torch.float32, device=dev).to(torch.bfloat16)
    keys = torch.empty(total, dtype=torch.bfloat16, device=dev)
    pos16 = torch.empty(total, dtype=torch.int32, device=dev)
    vals32 = torch.empty(total, dtype=torch.int32, device=dev)
    out_rows = []
    for rows, row_len in shapes:
        n = rows * row_len
        pos = torch.arange(row_len, dtype=torch.int32, device=dev).repeat(rows)
        for argsort in (False, True):
            vb = 4 if argsort else 0
            mode = g.MODE_PAIRS if vb else g.MODE_KEYS_ONLY
            plan = sort_rows16_plan(rows, row_len, mode, vb)
            passes = plan["route"] == ROUTE_PASSES
            rs16 = g.RowSort16(n, key_type=g.KEY_BFLOAT16, mode=mode, value_bytes=vb)
            rs32 = g.RowSort(n, key_type=g.KEY_FLOAT32, mode=mode, value_bytes=vb)
            k2, p2, v2 = keys[:n].view(rows, row_len), pos16[:n].view(rows, row_len), vals32[:n].view(rows, row_len)
            res = {}

            def reset():
                keys[:n].copy_(src[:n])

            def run_rows():
                if argsort:
                    rs16.argsort(k2, p2)
                else:
                    rs16.sort(k2)

            def run_base():
                wide = k2.float()
                if argsort:
                    vals32[:n].copy_(pos)
                    rs32.sort(wide.view(torch.int32), v2)
                else:
                    rs32.sort(wide.view(torch.int32))
                res["keys"] = wide.to(torch.bfloat16)

            t_rows, t_base = [], []
            for _ in range(2):  # alternate the two: half the repetitions each, twice
                t_rows += timed(run_rows, reset, args.reps // 2)
                t_base += timed(run_base, reset, args.reps // 2)
            rs16.check()
            rs32.check()
            ok = None
            if args.check:
                reset()
                run_base()
                reset_keys = res["keys"].view(torch.int16).clone()
                reset()
                run_rows()
                ok = bool(torch.equal(k2.view(torch.int16), reset_keys) and (not argsort or torch.equal(p2, v2)))
            res.clear()
            t_torch = None
            if not args.no_torch:
                x = src[:n].view(rows, row_len)
                t_torch = stats(timed(lambda: torch.sort(x, dim=-1, stable=True), lambda: None, max(args.reps // 4, 3)))
            s_rows, s_base = stats(t_rows), stats(t_base)
            last = rs16.last()
            row = {"rows": rows, "row_len": row_len, "mode": "argsort" if argsort else "keys", "n": n, "route": "passes" if passes else "lds",
                   "parts": last["parts"], "per_part": last["per_part"], "launches": 1 + 3 * plan["passes"] if passes else 2,
                   "rowsort16": s_rows, "baseline_widen_rowsort_narrow": s_base, "speedup": s_base["median_ms"] / s_rows["median_ms"],
                   "rowsort16_wins_beyond_spread": bool(s_rows["max_ms"] < s_base["min_ms"]),
                   "baseline_wins_beyond_spread": bool(s_base["max_ms"] < s_rows["min_ms"]),
                   "rowsort16_gkeys_per_s": n / s_rows["median_ms"] / 1e6, "torch_sort": t_torch, "matches_baseline": ok}
            out_rows.append(row)
            print(f"# {rows:6d} x {row_len:8d} {row['mode']:8s} {row['route']:6s} rowsort16 {s_rows['median_ms']:8.3f} ms (spread {s_rows['spread']:.3f})  "
                  f"baseline {s_base['median_ms']:8.3f} ms (spread {s_base['spread']:.3f})  x{row['speedup']:.2f}"
                  + (f"  torch {t_torch['median_ms']:8.3f} ms" if t_torch else "") + (f"  match {ok}" if ok is not None else ""), file=sys.stderr, flush=True)
            rs16.close()
            rs32.close()
    out = {"tool": "sort_rows16_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "key_type": "bfloat16",
           "baseline": "widen to float32, gs_sort_rows_* (the 32-bit row-wise sort, unchanged), narrow to bfloat16; all inside the timed span",
           "rows": out_rows}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
