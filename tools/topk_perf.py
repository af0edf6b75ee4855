#!/usr/bin/env python3
"""Top-k selection against sort-and-slice, on one GPU; prints one JSON line.

uint32 keys, preset 1, n = 2^27 and 2^28 (--log2 a b), k = 1, 64, 1024, 2^16, 2^20, keys-only and position mode; plus at the largest
n, k = 1024: preset 5, sorted input, and "all keys share their top 16 bits".  Per row:
  select    gs_topk_select_keys / _select_pairs (d_vals = NULL: positions);
  baseline  what a user had before: a device copy of the input into scratch (position mode: plus filling the index array),
            gs_onesweep_sort_* at the library's defaults, a device copy of the first k.  The sort's code is the same in this build as
            before the selection existed, so the baseline runs from the same library.
The two alternate in one process, both warmed, --reps timed repetitions each (device events around every single call); median and
spread (max - min over min) per row.  Recorded with no requirement: torch.topk on the same data, and the box's read rate (the
tuning build's read-only sweep over n x 4 bytes) with select's time as a multiple of one read.  --check compares select's result
with the baseline's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd import _lib  # noqa: E402


def timed(fn, reps, warm=3):
    times = []
    for i in range(warm + reps):
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
    ap.add_argument("--log2", type=int, nargs="+", default=[27, 28])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--check", action="store_true", help="compare every row's result with the baseline's")
    ap.add_argument("--no-torch", action="store_true", help="leave torch.topk out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nmax = 1 << max(args.log2)
    kmax = 1 << 20
    src, scratch, alt = (torch.empty(nmax, dtype=torch.int32, device=dev) for _ in range(3))
    idx, idx_alt = (torch.empty(nmax, dtype=torch.int32, device=dev) for _ in range(2))
    out_k, out_v, base_k, base_v = (torch.empty(kmax, dtype=torch.int32, device=dev) for _ in range(4))
    tuning = _lib.load_tuning()
    sp = int(torch.cuda.current_stream().cuda_stream)
    rows = []
    cases = [(lg, "preset 1", k) for lg in args.log2 for k in (1, 64, 1024, 1 << 16, 1 << 20)]
    cases += [(max(args.log2), name, 1024) for name in ("preset 5", "sorted", "shared top 16 bits")]
    filled = None
    for lg, data, k in cases:
        n = 1 << lg
        if filled != (lg, data):
            g.init_random(src, 12345, g.ENTROPY_PRESET_5 if data == "preset 5" else g.ENTROPY_PRESET_1, n=n)
            if data == "sorted":
                src[:n] = (torch.sort(src[:n].to(torch.int64) & 0xFFFFFFFF)[0] - (1 << 31)).to(torch.int32) ^ (-1 << 31)
            if data == "shared top 16 bits":
                src[:n] = (src[:n] & 0xFFFF) | 0x12340000
            filled = (lg, data)
            t_read = stats(timed(lambda: tuning.gs_debug_copy_floor(src.data_ptr(), scratch.data_ptr(), n, 0, 3, sp), args.reps))
        for pos in (False, True):
            mode, vb = (g.MODE_PAIRS, 4) if pos else (g.MODE_KEYS_ONLY, 0)
            sel = g.TopK(n, k, mode=mode, value_bytes=vb)
            base = g.OneSweep(n, mode=mode, value_bytes=vb)

            def run_select():
                sel.select(src, k, out_k, None, out_v if pos else None, n=n)

            def run_base():
                scratch[:n].copy_(src[:n])
                if pos:
                    torch.arange(n, dtype=torch.int32, device=dev, out=idx[:n])
                base.sort(scratch, idx if pos else None, n=n, alt_keys=alt, alt_values=idx_alt if pos else None)
                base_k[:k].copy_(scratch[:k])
                if pos:
                    base_v[:k].copy_(idx[:k])

            t_sel, t_base = [], []
            for _ in range(2):  # alternate the two: half the repetitions each, twice
                t_sel += timed(run_select, args.reps // 2)
                t_base += timed(run_base, args.reps // 2)
            sel.check()
            base.check()
            rep = sel.last()
            ok = None
            if args.check:
                ok = bool(torch.equal(out_k[:k], base_k[:k]) and (not pos or torch.equal(out_v[:k], base_v[:k])))
            t_torch = None
            if not args.no_torch:
                u = src[:n].to(torch.int64) & 0xFFFFFFFF  # torch.topk has no uint32: the same order on int64 (8 bytes per key)
                t_torch = stats(timed(lambda: torch.topk(u, k, largest=False), max(args.reps // 4, 3), warm=1))
                del u
            s_sel, s_base = stats(t_sel), stats(t_base)
            row = {"n_log2": lg, "data": data, "k": k, "mode": "positions" if pos else "keys", "select": s_sel, "baseline": s_base,
                   "speedup": s_base["median_ms"] / s_sel["median_ms"],
                   "faster_by_more_than_spreads": bool(s_base["median_ms"] - s_sel["median_ms"] > (s_sel["max_ms"] - s_sel["min_ms"]) + (s_base["max_ms"] - s_base["min_ms"])),
                   "read_sweep": t_read, "select_in_reads": s_sel["median_ms"] / t_read["median_ms"], "torch_topk_int64": t_torch,
                   "route": rep["route"], "candidates": rep["candidates"], "matches_baseline": ok}
            rows.append(row)
            print(f"# 2^{lg} {data:18s} k={k:<8d} {row['mode']:9s} select {s_sel['median_ms']:7.3f} ms (spread {s_sel['spread']:.3f})  baseline "
                  f"{s_base['median_ms']:7.3f} ms (spread {s_base['spread']:.3f})  x{row['speedup']:.2f}  {row['select_in_reads']:.2f} reads"
                  f"  torch {t_torch['median_ms'] if t_torch else float('nan'):.3f} ms  ok={ok}", file=sys.stderr, flush=True)
            sel.close()
            base.close()
    out = {"tool": "topk_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "baseline": "copy + gs_onesweep_sort_* + copy of the head, same library (the sort's code is unchanged)", "rows": rows}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
