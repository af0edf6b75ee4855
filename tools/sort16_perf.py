#!/usr/bin/env python3
"""The 16-bit sort (gs_sort16_*) against what a caller did before it existed, on one GPU; prints one JSON line.

bfloat16 keys, ascending.  Modes: keys (gs_sort16_sort_keys), argsort (gs_sort16_argsort), pairs8 (gs_sort16_sort_pairs with 8-byte
values).  Inputs: normal (logit-like: randn), uniform (uniform 16-bit patterns), equal (one value).  Per (mode, input, n):
  sort16     the 16-bit call on the bfloat16 array itself, in place;
  widen32    the route a caller had: widen to 32 bits by the order-preserving map (pattern << 16 IS the float32 of a bfloat16), the
             32-bit gpusorting_amd.sort_ / argsort, narrow again — timed together, temporaries included;
  torch      torch.sort on the bfloat16 tensor (keys and argsort: it always makes both), an outside comparator only.
The input is restored in front of every timed call, outside the timed span (device events around every single call); the candidates
alternate in one process, all warmed; median and spread (max - min over min).  bytes_per_element is the design's count of what the
16-bit call moves (keys 4 read + 2 written; argsort 24; pairs8 44), roofline_share = that traffic over the median against 8 TB/s.
--check compares the 16-bit result with the widened route's.  Numbers of one box carry the pool's +-3 % band."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402

BYTES = {"keys": 6, "argsort": 24, "pairs8": 44}
ROOFLINE_BYTES_PER_MS = 8e12 / 1e3


def stats(times):
    t = np.asarray(times)
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "spread": float((t.max() - t.min()) / t.min())}


def timed(prep, fn, reps, warm=2):
    times = []
    for i in range(warm + reps):
        prep()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if i >= warm:
            times.append(s.elapsed_time(e))
    return times


def make_input(kind, n, dev):
    if kind == "normal":
        return torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(16)).bfloat16()
    if kind == "uniform":
        w = torch.randint(-32768, 32768, (n,), device=dev, dtype=torch.int16, generator=torch.Generator(device=dev).manual_seed(17))
        return torch.where((w & 0x7F80) == 0x7F80, w & ~0x4000, w).view(torch.bfloat16)  # no NaN, no infinity: torch.sort orders those differently
    return torch.full((n,), 1.5, device=dev, dtype=torch.bfloat16)


def markdown(rows):
    lines = ["| mode | input | n | 16-bit call ms (spread) | B / element | share of 8 TB/s | widen + 32-bit + narrow ms (spread) | widened / 16-bit | torch.sort ms |",
             "|" + "---|" * 9]
    for r in rows:
        t = r["torch"]
        lines.append(f"| {r['mode']} | {r['input']} | 2^{r['log2n']} | {r['sort16']['median_ms']:.3f} ({r['sort16']['spread']:.3f}) | {r['bytes_per_element']} | "
                     f"{100 * r['roofline_share']:.1f} % | {r['widen32']['median_ms']:.3f} ({r['widen32']['spread']:.3f}) | "
                     f"{r['widen32']['median_ms'] / r['sort16']['median_ms']:.2f} | {'—' if t is None else format(t['median_ms'], '.3f')} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20, 24, 26, 28])
    ap.add_argument("--modes", nargs="+", default=["keys", "argsort", "pairs8"], choices=list(BYTES))
    ap.add_argument("--inputs", nargs="+", default=["normal", "uniform", "equal"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here (and the table next to it)")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for lg in args.log2:
        n = 1 << lg
        for kind in args.inputs:
            src = make_input(kind, n, dev)
            work = torch.empty_like(src)
            vals8 = torch.arange(n, dtype=torch.int64, device=dev)
            wv8 = torch.empty_like(vals8)
            pos = torch.empty(n, dtype=torch.int32, device=dev)
            for mode in args.modes:
                h = g.Sort16(n, g.ORDER_ASCENDING, g.KEY_BFLOAT16, g.MODE_KEYS_ONLY if mode == "keys" else g.MODE_PAIRS, {"keys": 0, "argsort": 4, "pairs8": 8}[mode])
                res = {}

                def prep():
                    work.copy_(src)
                    if mode == "pairs8":
                        wv8.copy_(vals8)

                def run16():
                    if mode == "keys":
                        h.sort(work)
                    elif mode == "argsort":
                        h.argsort(work, pos)
                    else:
                        h.sort(work, wv8)

                def run_widen():
                    wide = (work.view(torch.int16).to(torch.int32) << 16).view(torch.float32)
                    if mode == "argsort":
                        res["perm"] = g.argsort(wide)
                        return
                    g.sort_(wide, wv8 if mode == "pairs8" else None)
                    res["keys"] = (wide.view(torch.int32) >> 16).to(torch.int16)

                def run_torch():
                    res["torch"] = torch.sort(work, stable=True)

                t16, t32, tt = [], [], []
                for _ in range(2):  # alternate: half the repetitions each, twice
                    t16 += timed(prep, run16, max(args.reps // 2, 1))
                    t32 += timed(prep, run_widen, max(args.reps // 2, 1))
                    if not args.no_torch and mode != "pairs8":
                        tt += timed(prep, run_torch, max(args.reps // 4, 2), warm=1)
                ok = None
                if args.check:
                    prep(); run16(); h.check()
                    k16 = work.view(torch.int16).clone()
                    p16, v16 = pos.clone(), wv8.clone()
                    prep(); run_widen()
                    ok = bool(torch.equal(p16, res["perm"])) if mode == "argsort" else bool(torch.equal(k16, res["keys"]) and (mode == "keys" or torch.equal(v16, wv8)))
                h.check()
                last = h.last()
                s16, s32 = stats(t16), stats(t32)
                row = {"mode": mode, "input": kind, "log2n": lg, "n": n, "key_type": "bfloat16", "order": "ascending", "ranges": last["ranges"],
                       "per_range": last["per_range"], "rank_mode": last["rank_mode"], "sort16": s16, "widen32": s32, "torch": stats(tt) if tt else None,
                       "bytes_per_element": BYTES[mode], "roofline_share": BYTES[mode] * n / s16["median_ms"] / ROOFLINE_BYTES_PER_MS,
                       "not_slower": bool(s16["median_ms"] - s32["median_ms"] <= s32["max_ms"] - s32["min_ms"]), "matches_widen32": ok}
                rows.append(row)
                print(f"# {mode:8s} {kind:8s} 2^{lg:<2d} 16-bit {s16['median_ms']:9.3f} ms (spread {s16['spread']:.3f})  widen32 {s32['median_ms']:9.3f} "
                      f"(spread {s32['spread']:.3f})  torch {stats(tt)['median_ms'] if tt else float('nan'):9.3f}  ok={ok}", file=sys.stderr, flush=True)
                h.close()
                res.clear()
            del src, work, vals8, wv8, pos
            torch.cuda.empty_cache()
    out = {"tool": "sort16_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "note": "one box; numbers carry the pool's +-3 % band; the histogram flushes by global atomics (a slices + reduce flush was not built, so "
                   "not measured); input 'equal' is the all-equal case of the histogram's wave aggregation (whole keys call: clear, histogram, scan, fill)",
           "rows": rows}
    line = json.dumps(out)
    md = markdown(rows)
    print(md, file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        with open(os.path.splitext(args.out)[0] + ".md", "w") as f:  # the table of DESIGN.md 3.12
            f.write(md + "\n")
    print(line)


if __name__ == "__main__":
    main()
