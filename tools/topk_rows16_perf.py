#!/usr/bin/env python3
"""Row-wise top-k on bfloat16 keys (gs_topk_select_rows_pairs with GS_KEY_BFLOAT16) against what a caller did before the 16-bit key
types existed, on one GPU; prints one JSON line.

bfloat16 keys with positions, largest first, the row-wise shapes of the README (rows x row_len, k).  Keys: the 16-bit words of the
init_random output (preset 1), with the NaN / infinity exponent taken out so that the widening cast changes no bit.  Per shape:
  rows16     gs_topk_select_rows_pairs on the bfloat16 matrix itself (d_vals = NULL: positions within the row);
  yardstick  x.float() followed by the 32-bit gs_topk_select_rows_pairs on the result, timed together: the route a caller had;
  torch      torch.topk(dim=-1) on the bfloat16 tensor, an outside comparator only.
The candidates alternate in one process, all warmed, --reps timed repetitions each (device events around every single call); median
and spread (max - min over min).  not_slower: the 16-bit call's median is not above the yardstick's by more than the yardstick's own
max - min.  --check compares positions with the yardstick's, and the keys with its keys narrowed.  Numbers of one box carry the
pool's +-3 % band."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from topk_perf import stats, timed  # noqa: E402

SHAPES = [(1 << 20, 64, 8), (1 << 16, 256, 8), (4096, 4096, 64), (1024, 32768, 64), (256, 131072, 50), (256, 131072, 1024),
          (32, 262144, 1024)]
ROUTE = {0: "none", 1: "wave", 2: "tile", 3: "stream", 4: "loop"}


def markdown(rows):
    """The table of DESIGN.md 3.11."""
    def cell(t):
        return f"{t['median_ms']:.3f} ({t['spread']:.3f})"
    lines = ["| rows × row_len | k | route 16-bit (reads) | route 32-bit (reads) | 16-bit call ms (spread) | x.float() + 32-bit call ms (spread) | "
             "yardstick / 16-bit | not slower | torch.topk bf16 ms |", "|" + "---|" * 9]
    for r in rows:
        lines.append(f"| {r['rows']} × {r['row_len']} | {r['k']} | {r['route']} ({r['reads_of_a_row'] or 1}) | {r['route32']} ({r['reads32'] or 1}) | "
                     f"{cell(r['rows16'])} | {cell(r['yardstick'])} | {r['yardstick']['median_ms'] / r['rows16']['median_ms']:.2f} | "
                     f"{'yes' if r['not_slower'] else 'NO'} | {'—' if r['torch_topk_bf16'] is None else format(r['torch_topk_bf16']['median_ms'], '.3f')} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", type=int, nargs="+", default=list(range(len(SHAPES))), help="indices into the shape list")
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("ROWS", "ROW_LEN", "K"), help="measure this shape instead (repeatable)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out_rows = []
    for rows, row_len, k in (args.shape or [SHAPES[si] for si in args.shapes]):
        n = rows * row_len
        words = torch.empty(n // 2, dtype=torch.int32, device=dev)
        g.init_random(words, 12345, g.ENTROPY_PRESET_1, n=n // 2)
        w = words.view(torch.int16)
        w = torch.where((w & 0x7F80) == 0x7F80, w & ~0x4000, w)  # no NaN, no infinity
        x = w.view(torch.bfloat16).view(rows, row_len)
        del words, w
        out_k = torch.empty(rows * k, dtype=torch.bfloat16, device=dev)
        out_k32 = torch.empty(rows * k, dtype=torch.float32, device=dev)
        out_v, out_v32 = (torch.empty(rows * k, dtype=torch.int32, device=dev) for _ in range(2))
        h16 = g.TopK(n, k, g.ORDER_DESCENDING, g.KEY_BFLOAT16, g.MODE_PAIRS, 4)
        h32 = g.TopK(n, k, g.ORDER_DESCENDING, g.KEY_FLOAT32, g.MODE_PAIRS, 4)

        def run16():
            h16.select_rows(x, rows, row_len, row_len, k, out_k, None, out_v)

        def run_yardstick():
            h32.select_rows(x.float(), rows, row_len, row_len, k, out_k32, None, out_v32)

        t16, t32, tt = [], [], []
        for _ in range(2):  # alternate: half the repetitions each, twice
            t16 += timed(run16, args.reps // 2)
            t32 += timed(run_yardstick, args.reps // 2)
            if not args.no_torch:
                tt += timed(lambda: torch.topk(x, k, dim=-1), max(args.reps // 4, 3), warm=1)
        h16.check()
        h32.check()
        rep, rep32 = h16.rows_last(), h32.rows_last()
        ok = None
        if args.check:
            ok = bool(torch.equal(out_v, out_v32) and torch.equal(out_k.view(torch.int16), (out_k32.view(torch.int32) >> 16).to(torch.int16)))
        s16, s32 = stats(t16), stats(t32)
        row = {"rows": rows, "row_len": row_len, "k": k, "key_type": "bfloat16", "mode": "positions", "order": "descending",
               "route": ROUTE[rep["route"]], "reads_of_a_row": rep["reads"], "route32": ROUTE[rep32["route"]], "reads32": rep32["reads"],
               "rows16": s16, "yardstick": s32, "torch_topk_bf16": stats(tt) if tt else None,
               "not_slower": bool(s16["median_ms"] - s32["median_ms"] <= s32["max_ms"] - s32["min_ms"]), "matches_yardstick": ok}
        out_rows.append(row)
        print(f"# {rows:>8d} x {row_len:<8d} k={k:<5d} {row['route']:6s} 16-bit {s16['median_ms']:8.3f} ms (spread {s16['spread']:.3f})  "
              f"yardstick {s32['median_ms']:8.3f} (spread {s32['spread']:.3f})  torch {stats(tt)['median_ms'] if tt else float('nan'):.3f}  ok={ok}",
              file=sys.stderr, flush=True)
        h16.close()
        h32.close()
        del x
    out = {"tool": "topk_rows16_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "note": "one box; numbers carry the pool's +-3 % band", "rows": out_rows}
    line = json.dumps(out)
    md = markdown(out_rows)
    print(md, file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:  # the table of DESIGN.md 3.11
            f.write(md + "\n")
    print(line)


if __name__ == "__main__":
    main()
