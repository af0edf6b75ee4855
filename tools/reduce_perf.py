#!/usr/bin/env python3
"""reduce by key (gs_reduce_*) against what a user does without it, on one GPU; prints one JSON line (and rewrites --out after every row).

Two configurations (--configs): u32_f32 (uint32 keys, float32 values) and i32_i64 (int32 keys, int64 values); op sum, ascending.  The
keys are draws from d distinct random 31-bit values (d of --distinct; 0 = uniform 31-bit draws, about n distinct): below 2^31 the
unsigned order is torch's signed order on the same int32 storage, so every side delivers the same keys.  Two blocks (--blocks):
  sorted       gs_reduce_by_key, n = 2^--log2, against
               (a) today: gpusorting_amd.unique(return_inverse=True) + zeros(u).index_add_(0, inverse, values)
               (b) parts: copy + gs_onesweep_sort_pairs + torch.unique_consecutive(return_counts) + torch.segment_reduce (integers, which
                   segment_reduce does not take: cumsum differences at the run ends)
  consecutive  gs_reduce_by_key_consecutive alone on the SORTED input against
               (c) torch.unique_consecutive(return_counts) + torch.segment_reduce (integers: as above),
               also as a share of --peak-tbs TB/s over the bytes DESIGN.md 3.23 counts for the stage: 2 n (4 + value bytes) read,
               u (8 + value bytes) written.
All sides alternate in one process, every side warmed, --reps timed repetitions each in two halves, device events around every single
call; median, extremes and spread per side.  EVERY row asserts agreement: the keys and counts with a comparator's exactly; integer sums
exactly; float sums within |got - exact| <= (m - 1) * 2^-24 * sum|v| per run of length m (exact: a float64 index_add_), and two calls
bitwise equal.  flags: loses_to_<side> when that side's median is below the call's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from topk_perf import stats  # noqa: E402
from unique_perf import make_input, timed, trio  # noqa: E402

COLUMNS = ["config", "block", "n_log2", "distinct", "u", "reduce [median, min, max]", "today (a) [median, min, max]", "parts (b/c) [median, min, max]",
           "share of peak", "results_agree", "flags"]
CONFIGS = {"u32_f32": (torch.float32, 4), "i32_i64": (torch.int64, 8)}


def segment_sum(vals, counts):
    """One sum per run of the sorted values: torch.segment_reduce on floats; integers by cumsum differences at the run ends."""
    if vals.dtype.is_floating_point:
        return torch.segment_reduce(vals, "sum", lengths=counts)
    cs = torch.cumsum(vals, 0)
    ends = torch.cumsum(counts, 0) - 1
    tot = cs[ends]
    tot[1:] -= cs[ends[:-1]]
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26, 28])
    ap.add_argument("--distinct", default="16,1024,65536,1048576,0")
    ap.add_argument("--configs", default="u32_f32,i32_i64")
    ap.add_argument("--blocks", default="sorted,consecutive")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None, help="also write the JSON here, after every row")
    args = ap.parse_args()
    assert args.reps >= 5, "medians over at least 5 timed calls"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows_out = []

    def emit():
        out = {"tool": "reduce_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "keys": "31-bit draws, ascending", "op": "sum",
               "reduce": "gs_reduce_by_key / gs_reduce_by_key_consecutive, outputs allocated inside the timed span",
               "today (a)": "gpusorting_amd.unique(return_inverse=True) + zeros(u).index_add_(0, inverse, values)",
               "parts (b/c)": "sorted: copy + gs_onesweep_sort_pairs + torch.unique_consecutive(return_counts) + torch.segment_reduce (int64: cumsum "
                              "differences); consecutive: the last two on the sorted input",
               "share of peak": f"consecutive only: (2 n (4 + vb) + u (8 + vb)) bytes / median / {args.peak_tbs} TB/s",
               "columns": COLUMNS, "rows_measured": rows_out}
        line = json.dumps(out, separators=(",", ":"))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    for cfg in args.configs.split(","):
        vdtype, vb = CONFIGS[cfg]
        for block in args.blocks.split(","):
            for lg in args.log2:
                n = 1 << lg
                rd = g.ReduceByKey(n, g.ORDER_ASCENDING, g.KEY_UINT32, vb)
                sorter = g.OneSweep(n, g.ORDER_ASCENDING, g.KEY_UINT32, g.MODE_PAIRS, vb) if block == "sorted" else None
                kcopy = torch.empty(n, dtype=torch.int32, device=dev)
                vcopy = torch.empty(n, dtype=vdtype, device=dev)
                for d in (int(x) for x in args.distinct.split(",")):
                    if d > n:
                        continue
                    keys = make_input(n, d, dev)
                    gen = torch.Generator(device=dev)
                    gen.manual_seed(99 + d)
                    if vdtype.is_floating_point:
                        vals = torch.randn(n, dtype=vdtype, device=dev, generator=gen)
                    else:
                        vals = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=vdtype, device=dev, generator=gen)
                    if block == "consecutive":
                        keys, perm = torch.sort(keys, stable=True)
                        keys, vals = keys.contiguous(), vals[perm].contiguous()
                        del perm

                    def run_reduce():
                        return (rd.reduce_by_key if block == "sorted" else rd.reduce_by_key_consecutive)(keys, vals, "sum")

                    def run_today():
                        uk, inverse = g.unique(keys, return_inverse=True)
                        return uk, torch.zeros(uk.numel(), dtype=vdtype, device=dev).index_add_(0, inverse, vals)

                    def run_parts():
                        if block == "sorted":
                            kcopy.copy_(keys)
                            vcopy.copy_(vals)
                            sorter.sort(kcopy, vcopy, n=n)
                            k, c = torch.unique_consecutive(kcopy, return_counts=True)
                            return k, segment_sum(vcopy, c), c
                        k, c = torch.unique_consecutive(keys, return_counts=True)
                        return k, segment_sum(vals, c), c

                    fns = {"reduce": run_reduce, "parts": run_parts}
                    if block == "sorted":
                        fns["today"] = run_today
                    # the comparators' results, once (also their first warm-up), and the exact sums for the float bound
                    ek, ev, ec = run_parts()
                    inverse = torch.repeat_interleave(torch.arange(ek.numel(), device=dev), ec) if block == "consecutive" else \
                        torch.searchsorted(ek, keys)
                    if vdtype.is_floating_point:
                        exact = torch.zeros(ek.numel(), dtype=torch.float64, device=dev).index_add_(0, inverse, vals.double())
                        mass = torch.zeros(ek.numel(), dtype=torch.float64, device=dev).index_add_(0, inverse, vals.double().abs())
                        bound = (ec.double() - 1) * 2.0 ** -24 * mass
                    del inverse
                    torch.cuda.synchronize()
                    agree, seen, first_bits = [True], [], []

                    def compare(out):
                        k, v, c, num = out
                        u = int(num.item())
                        seen.append(u)
                        ok = u == ek.numel() and torch.equal(k[:u], ek) and torch.equal(c[:u].long(), ec.long())
                        if ok and vdtype.is_floating_point:
                            ok = bool(((v[:u].double() - exact).abs() <= bound).all())
                            bits = v[:u].view(torch.int32)
                            if first_bits:
                                ok = ok and torch.equal(bits, first_bits[0])  # two calls: bitwise equal
                            else:
                                first_bits.append(bits.clone())
                        elif ok:
                            ok = torch.equal(v[:u], ev)
                        agree[0] = agree[0] and bool(ok)

                    sides = list(fns)
                    times = {s: [] for s in sides}
                    for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                        for s in sides:
                            times[s] += timed(fns[s], max(half, 1), 1, compare if s == "reduce" else (lambda out: None))
                    rd.check()
                    if sorter is not None:
                        sorter.check()
                    assert agree[0] and len(set(seen)) == 1, f"results disagree: {cfg} {block} 2^{lg} distinct {d}"
                    st = {s: stats(t) for s, t in times.items()}
                    m, u = st["reduce"], seen[-1]
                    share = round((2.0 * n * (4 + vb) + u * (8.0 + vb)) / (m["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 3) if block == "consecutive" else None
                    flags = [f"loses_to_{s}" for s in sides[1:] if st[s]["median_ms"] < m["median_ms"]]
                    rows_out.append([cfg, block, lg, d, u, trio(m), trio(st.get("today")), trio(st["parts"]), share, 1, ",".join(flags)])
                    print(f"# {cfg} {block:11s} 2^{lg} distinct {d:8d} u {u:10d} reduce {m['median_ms']:9.3f} ms"
                          + (f"  today {st['today']['median_ms']:9.3f}" if "today" in st else "") + f"  parts {st['parts']['median_ms']:9.3f}"
                          + (f"  share {share}" if share is not None else "") + f"  {flags}", file=sys.stderr, flush=True)
                    emit()
                    del keys, vals, ek, ev, ec
                    torch.cuda.empty_cache()
                rd.close()
                if sorter is not None:
                    sorter.close()
                del kcopy, vcopy
                torch.cuda.empty_cache()
    print(emit())


if __name__ == "__main__":
    main()
