#!/usr/bin/env python3
"""unique / run-length encode (gs_unique_*) against what a user does without it, on one GPU; prints one JSON line.

uint32 keys, ascending.  The keys are draws from d distinct random 31-bit values (d of --distinct; 0 = uniform 31-bit draws, about n
distinct): below 2^31 the unsigned order is torch's signed order on the same int32 storage, so every side delivers the same arrays.
Three blocks (--blocks):
  keys         gs_unique_keys (keys + counts), n = 2^--log2;
  positions    gs_unique_positions (keys, counts, first, inverse), n = 2^min(--log2, --positions-max-log2);
  consecutive  gs_unique_consecutive alone on the SORTED input (keys, counts, inverse): the run-length stage by itself, also as a share
               of --peak-tbs TB/s over the bytes DESIGN.md 3.21 counts for it: 12 n + 8 u.
Sides per block:
  unique   the call (full-capacity outputs allocated inside the timed span, no host wait);
  today    keys: copy + gs_onesweep_sort_keys + torch.unique_consecutive(return_counts); positions: copy + arange + gs_onesweep_sort_pairs
           + torch.unique_consecutive(return_inverse, return_counts) + inverse scattered through the sorted positions + first gathered at
           the run starts — the same outputs.  (consecutive: none)
  torch    keys: torch.unique(sorted=True, return_counts=True); positions: torch.unique(sorted=True, return_inverse=True,
           return_counts=True) (it has no first positions); consecutive: torch.unique_consecutive(return_inverse=True, return_counts=True).
All sides alternate in one process, every side warmed, --reps timed repetitions each in two halves, device events around every single
call; median, extremes and spread per side.  EVERY repetition's result of the call is compared with the comparators' (computed once
on the same input): u, keys, counts, and first / inverse where both sides have them.  flags: loses_to_today / loses_to_torch when that
side's median is below the call's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from topk_perf import stats  # noqa: E402

COLUMNS = ["block", "n_log2", "distinct", "u", "unique [median, min, max]", "today [median, min, max]", "torch [median, min, max]",
           "share of peak", "results_agree", "flags"]


def make_input(n, distinct, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345 + distinct)
    if distinct == 0:
        return torch.randint(0, (1 << 31) - 1, (n,), dtype=torch.int32, device=dev, generator=gen)
    pool = torch.randint(0, (1 << 31) - 1, (distinct,), dtype=torch.int32, device=dev, generator=gen)
    return pool[torch.randint(0, distinct, (n,), device=dev, generator=gen)]


def timed(fn, reps, warm, after):
    times = []
    for i in range(warm + reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        e.synchronize()
        if i >= warm:
            times.append(s.elapsed_time(e))
        after(out)
    return times


def trio(s):
    return None if s is None else [round(s["median_ms"], 3), round(s["min_ms"], 3), round(s["max_ms"], 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26, 28])
    ap.add_argument("--positions-max-log2", type=int, default=27)
    ap.add_argument("--distinct", default="16,1024,65536,1048576,0")
    ap.add_argument("--blocks", default="keys,positions,consecutive")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows_out = []
    for block in args.blocks.split(","):
        sizes = sorted({min(lg, args.positions_max_log2) if block == "positions" else lg for lg in args.log2})
        for lg in sizes:
            n = 1 << lg
            pairs = block == "positions"
            uq = g.Unique(n, g.ORDER_ASCENDING, g.KEY_UINT32, positions=pairs)
            sorter = None if block == "consecutive" else g.OneSweep(n, g.ORDER_ASCENDING, g.KEY_UINT32, g.MODE_PAIRS if pairs else g.MODE_KEYS_ONLY,
                                                                    4 if pairs else 0)
            copy = torch.empty(n, dtype=torch.int32, device=dev)
            for d in (int(x) for x in args.distinct.split(",")):
                if d > n:
                    continue
                src = make_input(n, d, dev)
                if block == "consecutive":
                    src = torch.sort(src).values.contiguous()

                def run_unique():
                    if block == "keys":
                        k, c, num = uq.unique(src)
                        return k, c, None, None, num
                    if block == "positions":
                        return uq.unique_positions(src)
                    k, c, i, num = uq.unique_consecutive(src)
                    return k, c, None, i, num

                def run_today():
                    copy.copy_(src)
                    if block == "keys":
                        sorter.sort(copy, None, n=n)
                        k, c = torch.unique_consecutive(copy, return_counts=True)
                        return k, c, None, None
                    perm = torch.arange(n, dtype=torch.int32, device=dev)
                    sorter.sort(copy, perm, n=n)
                    k, inv_sorted, c = torch.unique_consecutive(copy, return_inverse=True, return_counts=True)
                    inverse = torch.empty_like(inv_sorted)
                    inverse[perm.long()] = inv_sorted
                    first = perm[torch.cumsum(c, 0) - c]
                    return k, c, first, inverse

                def run_torch():
                    if block == "keys":
                        k, c = torch.unique(src, sorted=True, return_counts=True)
                        return k, c, None, None
                    if block == "positions":
                        k, i, c = torch.unique(src, sorted=True, return_inverse=True, return_counts=True)
                        return k, c, None, i
                    k, i, c = torch.unique_consecutive(src, return_inverse=True, return_counts=True)
                    return k, c, None, i

                fns = {"unique": run_unique, "today": run_today, "torch": run_torch}
                sides = ["unique"] + (["today"] if block != "consecutive" else []) + ["torch"]
                # the comparators' results, once, as int32 (also their first warm-up)
                expect = {}
                for s in sides[1:]:
                    k, c, f, i = fns[s]()
                    expect[s] = (k, c.to(torch.int32), None if f is None else f.to(torch.int32), None if i is None else i.to(torch.int32))
                torch.cuda.synchronize()
                agree = {s: True for s in sides[1:]}
                seen_u = []

                def compare(out):
                    k, c, f, i, num = out
                    u = int(num.item())
                    seen_u.append(u)
                    for s, (ek, ec, ef, ei) in expect.items():
                        ok = u == ek.numel() and torch.equal(k[:u], ek) and torch.equal(c[:u], ec)
                        if ok and f is not None and ef is not None:
                            ok = torch.equal(f[:u], ef)
                        if ok and i is not None and ei is not None:
                            ok = torch.equal(i, ei)
                        agree[s] = agree[s] and bool(ok)

                times = {s: [] for s in sides}
                for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                    for s in sides:
                        times[s] += timed(fns[s], max(half, 1), 1, compare if s == "unique" else (lambda out: None))
                uq.check()
                if sorter is not None:
                    sorter.check()
                st = {s: stats(t) for s, t in times.items()}
                m = st["unique"]
                u = seen_u[-1]
                share = None
                if block == "consecutive":
                    share = round((12.0 * n + 8.0 * u) / (m["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 3)
                flags = [f"loses_to_{s}" for s in sides[1:] if st[s]["median_ms"] < m["median_ms"]]
                rows_out.append([block, lg, d, u, trio(m), trio(st.get("today")), trio(st["torch"]), share, int(all(agree.values()) and len(set(seen_u)) == 1),
                                 ",".join(flags)])
                print(f"# {block:11s} 2^{lg} distinct {d:8d} u {u:10d} unique {m['median_ms']:9.3f} ms [{m['min_ms']:.3f}, {m['max_ms']:.3f}]"
                      + (f"  today {st['today']['median_ms']:9.3f} x{st['today']['median_ms'] / m['median_ms']:.2f}" if "today" in st else "")
                      + f"  torch {st['torch']['median_ms']:9.3f} x{st['torch']['median_ms'] / m['median_ms']:.2f}"
                      + (f"  share {share}" if share is not None else "") + f"  agree {agree} {flags}", file=sys.stderr, flush=True)
                del src, expect
                torch.cuda.empty_cache()
            uq.close()
            if sorter is not None:
                sorter.close()
            del copy
            torch.cuda.empty_cache()
    out = {"tool": "unique_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "key_type": "uint32 (31-bit draws)", "order": "ascending",
           "unique": "gs_unique_keys / _positions / _consecutive, outputs allocated inside the timed span",
           "today": "copy + gs_onesweep_sort_keys / _sort_pairs (positions from arange) + torch.unique_consecutive, and for positions the inverse "
                    "scattered through the sorted positions and first gathered at the run starts",
           "torch": "torch.unique(sorted=True, ...) on the same tensor; consecutive: torch.unique_consecutive on the sorted input",
           "share of peak": f"consecutive only: (12 n + 8 u) bytes / median / {args.peak_tbs} TB/s",
           "columns": COLUMNS, "rows_measured": rows_out}
    line = json.dumps(out, separators=(",", ":"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
