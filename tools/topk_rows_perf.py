#!/usr/bin/env python3
"""Row-wise top-k (gs_topk_select_rows_*) against what a user had before, on one GPU; prints one JSON line.

uint32 keys, preset 1, the shapes of DESIGN.md 3.10 (rows x row_len, k), keys-only and position mode.  Per shape and mode:
  rows      gs_topk_select_rows_keys / _pairs (d_vals = NULL: positions within the row), the route it takes by itself;
  loop      baseline (a): gs_topk_select_* called row by row from the host, which is what GS_TOPK_ROWS_ROUTE_LOOP enqueues.  At most
            --loop-rows rows are timed and the time is scaled to all rows (the calls are independent and equal);
  segsort   baseline (b): a device copy of the matrix (position mode: plus the in-row index array), gs_segsort_* on it, a gather of the
            k leading elements of every row;
  torch     torch.topk(dim=-1) on the int32 view, for information (another order for the top bit; the same work).
The candidates alternate in one process, all warmed, --reps timed repetitions each (device events around every single call); median
and spread (max - min over min).  read_sweep: the tuning build's read-only sweep over rows x row_len x 4 bytes, and the rows call's
time as a multiple of it.  --check compares the rows call's result with the segsort baseline's.  Numbers of one box carry the
pool's +-3 % band."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd import _lib  # noqa: E402
from topk_perf import stats, timed  # noqa: E402

SHAPES = [(1 << 20, 64, 8), (1 << 16, 256, 8), (4096, 4096, 64), (1024, 32768, 64), (256, 131072, 50), (256, 131072, 1024),
          (32, 262144, 1024), (8, 1 << 20, 64), (4, 1 << 22, 64)]
ROUTE = {0: "none", 1: "wave", 2: "tile", 3: "stream", 4: "loop"}


def markdown(rows):
    """The table of DESIGN.md 3.10."""
    def cell(t):
        return "—" if t is None else f"{t['median_ms']:.3f} ({t['spread']:.3f})"
    lines = ["| rows × row_len | k | mode | route | reads of a row | rows call ms (spread) | loop ms (spread) | segsort ms (spread) | × loop | × segsort | "
             "beats both by > spreads | read sweep ms | in sweeps | torch.topk ms |", "|" + "---|" * 14]
    for r in rows:
        a = r["select_rows"]["median_ms"]
        lines.append(f"| {r['rows']} × {r['row_len']} | {r['k']} | {r['mode']} | {r['route']} | {r['reads_of_a_row'] or '1'} | {cell(r['select_rows'])} | "
                     f"{cell(r['loop'])} | {cell(r['segsort'])} | {r['loop']['median_ms'] / a:.1f} | {r['segsort']['median_ms'] / a:.2f} | "
                     f"{'yes' if r['beats_loop_by_more_than_spreads'] and r['beats_segsort_by_more_than_spreads'] else 'NO'} | "
                     f"{r['read_sweep']['median_ms']:.3f} | {r['select_rows_in_reads']:.2f} | "
                     f"{'—' if r['torch_topk_int32'] is None else format(r['torch_topk_int32']['median_ms'], '.3f')} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", type=int, nargs="+", default=list(range(len(SHAPES))), help="indices into the shape list")
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("ROWS", "ROW_LEN", "K"), help="measure this shape instead (repeatable)")
    ap.add_argument("--loop-rows", type=int, default=64)
    ap.add_argument("--stride-extra", type=int, default=0, help="the rows call reads the same rows at row stride row_len + this (odd: rows off "
                    "the 16-byte boundary, the LOOP route's staged copies); the baselines keep the contiguous matrix")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tuning = _lib.load_tuning()
    sp = int(torch.cuda.current_stream().cuda_stream)
    out_rows = []
    for rows, row_len, k in (args.shape or [SHAPES[si] for si in args.shapes]):
        n = rows * row_len
        src, scratch = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        g.init_random(src, 12345, g.ENTROPY_PRESET_1, n=n)
        stride = row_len + args.stride_extra
        strided = src
        if args.stride_extra:
            strided = torch.zeros((rows - 1) * stride + row_len, dtype=torch.int32, device=dev)
            strided.as_strided((rows, row_len), (stride, 1)).copy_(src.view(rows, row_len))
        offsets = (torch.arange(rows + 1, dtype=torch.int64, device=dev) * row_len).to(torch.int32)
        t_read = stats(timed(lambda: tuning.gs_debug_copy_floor(src.data_ptr(), scratch.data_ptr(), n, 0, 3, sp), args.reps))
        for pos in (False, True):
            mode, vb = (g.MODE_PAIRS, 4) if pos else (g.MODE_KEYS_ONLY, 0)
            idx = torch.empty(n if pos else 1, dtype=torch.int32, device=dev)
            out_k, out_v, base_k, base_v = (torch.empty(rows * k, dtype=torch.int32, device=dev) for _ in range(4))
            kp = (k + 3) & ~3  # the 1-D call wants every output 16-byte aligned: the loop's rows lie kp apart
            loop_k, loop_v = (torch.empty(rows * kp, dtype=torch.int32, device=dev) for _ in range(2))
            sel = g.TopK(strided.numel(), k, mode=mode, value_bytes=vb)
            one = g.TopK(row_len, k, mode=mode, value_bytes=vb)
            seg = g.SegmentedSort(n, rows, mode=mode, value_bytes=vb)
            fits_lds = row_len <= seg.max_lds_segment
            loop_rows = min(rows, args.loop_rows)

            def run_rows():
                sel.select_rows(strided, rows, row_len, stride, k, out_k, None, out_v if pos else None)

            def run_loop():
                for r in range(loop_rows):
                    one.select(src[r * row_len:(r + 1) * row_len], k, loop_k[r * kp:r * kp + k], None, loop_v[r * kp:r * kp + k] if pos else None,
                               n=row_len)

            def run_segsort():
                scratch.copy_(src)
                if pos:
                    idx.view(rows, row_len).copy_(torch.arange(row_len, dtype=torch.int32, device=dev).expand(rows, row_len))
                seg.sort(scratch, offsets, idx if pos else None, n=n, max_segment_len=row_len if fits_lds else 0)
                base_k.view(rows, k).copy_(scratch.view(rows, row_len)[:, :k])
                if pos:
                    base_v.view(rows, k).copy_(idx.view(rows, row_len)[:, :k])

            t_rows, t_loop, t_seg = [], [], []
            for _ in range(2):  # alternate: half the repetitions each, twice
                t_rows += timed(run_rows, args.reps // 2)
                t_loop += timed(run_loop, args.reps // 2)
                t_seg += timed(run_segsort, args.reps // 2)
            sel.check()
            one.check()
            seg.check()
            rep = sel.rows_last()
            ok = None
            if args.check:  # (run_segsort ran last: base_* hold its result)
                ok = bool(torch.equal(out_k, base_k) and (not pos or torch.equal(out_v, base_v)))
            t_torch = None
            if not args.no_torch:
                x = src.view(rows, row_len)
                t_torch = stats(timed(lambda: torch.topk(x, k, dim=-1, largest=False), max(args.reps // 4, 3), warm=1))
            s_rows, s_seg = stats(t_rows), stats(t_seg)
            s_loop = stats([t * rows / loop_rows for t in t_loop])

            def beats(b):
                return bool(b["median_ms"] - s_rows["median_ms"] > (s_rows["max_ms"] - s_rows["min_ms"]) + (b["max_ms"] - b["min_ms"]))
            row = {"rows": rows, "row_len": row_len, "row_stride": stride, "k": k, "mode": "positions" if pos else "keys", "route": ROUTE[rep["route"]],
                   "reads_of_a_row": rep["reads"], "select_rows": s_rows, "loop": s_loop, "loop_rows_timed": loop_rows, "segsort": s_seg,
                   "beats_loop_by_more_than_spreads": beats(s_loop), "beats_segsort_by_more_than_spreads": beats(s_seg),
                   "read_sweep": t_read, "select_rows_in_reads": s_rows["median_ms"] / t_read["median_ms"], "torch_topk_int32": t_torch,
                   "matches_segsort": ok}
            out_rows.append(row)
            print(f"# {rows:>8d} x {row_len:<8d} k={k:<5d} {row['mode']:9s} {row['route']:6s} rows {s_rows['median_ms']:8.3f} ms (spread "
                  f"{s_rows['spread']:.3f})  loop {s_loop['median_ms']:10.3f}  segsort {s_seg['median_ms']:9.3f} (spread {s_seg['spread']:.3f})  "
                  f"{row['select_rows_in_reads']:.2f} sweeps  torch {t_torch['median_ms'] if t_torch else float('nan'):.3f}  ok={ok}",
                  file=sys.stderr, flush=True)
            for h in (sel, one, seg):
                h.close()
        del src, scratch, strided
    out = {"tool": "topk_rows_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "note": "one box; numbers carry the pool's +-3 % band", "rows": out_rows}
    line = json.dumps(out)
    md = markdown(out_rows)
    print(md, file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:  # the table of DESIGN.md 3.10
            f.write(md + "\n")
    print(line)


if __name__ == "__main__":
    main()
