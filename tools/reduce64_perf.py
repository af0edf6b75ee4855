#!/usr/bin/env python3
"""reduce by key on 64-bit keys (gs_reduce64_*) against what a user does without it, on one GPU; prints one JSON line (and rewrites --out
after every row).

int64 keys, op sum, ascending.  Two value configurations (--configs): f32 (float32 values) and i64 (int64 values).  The keys are draws
from d distinct random values (d of --distinct; 0 = uniform draws, about n distinct) of two key spaces (--spaces): low32 (values below
2^31: typical ids; the engine drops the four constant bytes) and full64 (the whole int64 range).  Two blocks (--blocks):
  sorted       gs_reduce64_by_key, n = 2^--log2, against
               today   torch.unique(sorted=True, return_inverse=True) + zeros(u).index_add_(0, inverse, values)
               parts   copy + gs_onesweep_sort_pairs (64-bit keys) + torch.unique_consecutive(return_counts) + torch.segment_reduce
                       (integers, which segment_reduce does not take: cumsum differences at the run ends)
               narrow  low32 only: keys.to(int32) + gs_reduce_by_key + its keys widened to int64
  consecutive  gs_reduce64_by_key_consecutive alone on the SORTED input against
               parts   torch.unique_consecutive(return_counts) + torch.segment_reduce (integers: as above)
               stage32 gs_reduce_by_key_consecutive on int32 keys with the same runs (narrowed outside the timed span),
               both stages also as a share of --peak-tbs TB/s over the bytes they move: 2 n (8 + w) + u (12 + w) for 8-byte keys and
               2 n (4 + w) + u (8 + w) for 4-byte ones, w the value width.
All sides alternate in one process, every side warmed, --reps timed repetitions each in two halves, device events around every single
call; median and extremes per side.  EVERY row asserts agreement: the keys and counts with a comparator's exactly; integer sums exactly;
float sums within |got - exact| <= (m - 1) * 2^-24 * sum|v| per run of length m (exact: a float64 index_add_), two calls bitwise equal,
and the 32-bit sides' float sums BITWISE equal to the call's (the tree is the same).  flags: loses_to_<side> when that side's median is
below the call's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from reduce_perf import segment_sum  # noqa: E402
from topk_perf import stats  # noqa: E402
from unique64_perf import make_input64  # noqa: E402
from unique_perf import timed, trio  # noqa: E402

COLUMNS = ["config", "block", "space", "n_log2", "distinct", "u", "reduce64 [median, min, max]", "today [median, min, max]", "parts [median, min, max]",
           "narrow / stage32 [median, min, max]", "share of peak", "32-bit stage's share", "results_agree", "flags"]
CONFIGS = {"f32": (torch.float32, 4), "i64": (torch.int64, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26, 28])
    ap.add_argument("--distinct", default="16,65536,0")
    ap.add_argument("--spaces", default="low32,full64")
    ap.add_argument("--configs", default="f32,i64")
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
        out = {"tool": "reduce64_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "keys": "int64 draws, ascending", "op": "sum",
               "reduce64": "gs_reduce64_by_key / gs_reduce64_by_key_consecutive, outputs allocated inside the timed span",
               "today": "torch.unique(sorted=True, return_inverse=True) + zeros(u).index_add_(0, inverse, values)",
               "parts": "sorted: copy + gs_onesweep_sort_pairs (64-bit keys) + torch.unique_consecutive(return_counts) + torch.segment_reduce (int64: "
                        "cumsum differences); consecutive: the last two on the sorted input",
               "narrow / stage32": "sorted, low32: to(int32) + gs_reduce_by_key + keys widened; consecutive: gs_reduce_by_key_consecutive on int32 keys "
                                   "with the same runs (narrowed outside the timed span)",
               "share of peak": f"consecutive only: (2 n (8 + w) + u (12 + w)) bytes / median / {args.peak_tbs} TB/s; the 32-bit stage: "
                                "(2 n (4 + w) + u (8 + w))",
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
                rd = g.ReduceByKey64(n, g.ORDER_ASCENDING, g.KEY_INT64, vb)
                rd32 = g.ReduceByKey(n, g.ORDER_ASCENDING, g.KEY_UINT32, vb)
                sorter = g.OneSweep(n, g.ORDER_ASCENDING, g.KEY_INT64, g.MODE_PAIRS, vb) if block == "sorted" else None
                kcopy = torch.empty(n, dtype=torch.int64, device=dev)
                vcopy = torch.empty(n, dtype=vdtype, device=dev)
                for space in args.spaces.split(","):
                    for d in (int(x) for x in args.distinct.split(",")):
                        if d > n:
                            continue
                        keys = make_input64(n, d, space, dev)
                        gen = torch.Generator(device=dev)
                        gen.manual_seed(99 + d)
                        if vdtype.is_floating_point:
                            vals = torch.randn(n, dtype=vdtype, device=dev, generator=gen)
                        else:
                            vals = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=vdtype, device=dev, generator=gen)
                        k32 = None
                        if block == "consecutive":
                            keys, perm = torch.sort(keys, stable=True)
                            keys, vals = keys.contiguous(), vals[perm].contiguous()
                            del perm
                            k32 = torch.unique_consecutive(keys, return_inverse=True)[1].to(torch.int32)  # int32 keys with the same runs

                        def run_reduce():
                            return (rd.reduce_by_key if block == "sorted" else rd.reduce_by_key_consecutive)(keys, vals, "sum")

                        def run_today():
                            uk, inverse = torch.unique(keys, sorted=True, return_inverse=True)
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

                        def run_narrow():
                            if block == "consecutive":
                                k, v, c, num = rd32.reduce_by_key_consecutive(k32, vals, "sum")
                                return None, v, c, num
                            k, v, c, num = rd32.reduce_by_key(keys.to(torch.int32), vals, "sum")
                            return k.to(torch.int64), v, c, num

                        fns = {"reduce64": run_reduce, "today": run_today, "parts": run_parts, "narrow": run_narrow}
                        sides = ["reduce64"] + (["today"] if block == "sorted" else []) + ["parts"] + \
                                (["narrow"] if (space == "low32" or block == "consecutive") else [])
                        # the comparators' results, once (also their first warm-up), and the exact sums for the float bound
                        try:
                            ek, ev, ec = run_parts()
                            torch.cuda.synchronize()
                        except RuntimeError as e:  # torch.segment_reduce refuses some segment counts at launch (seen: all 2^24 keys distinct)
                            if not vdtype.is_floating_point or "invalid configuration" not in str(e):  # (integers never call it: cumsum)
                                raise
                            sides.remove("parts")  # not timed on this row; keys and counts from the rest of the parts, float sums from `exact`
                            ek, ec = torch.unique_consecutive(kcopy if block == "sorted" else keys, return_counts=True)
                            ev = None
                        inverse = torch.repeat_interleave(torch.arange(ek.numel(), device=dev), ec) if block == "consecutive" else \
                            torch.searchsorted(ek, keys)
                        if vdtype.is_floating_point:
                            exact = torch.zeros(ek.numel(), dtype=torch.float64, device=dev).index_add_(0, inverse, vals.double())
                            mass = torch.zeros(ek.numel(), dtype=torch.float64, device=dev).index_add_(0, inverse, vals.double().abs())
                            bound = (ec.double() - 1) * 2.0 ** -24 * mass
                        del inverse
                        torch.cuda.synchronize()
                        agree, seen, first_bits = [True], [], []

                        def compare(out, narrowed=False):
                            k, v, c, num = out
                            u = int(num.item())
                            seen.append(u)
                            ok = u == ek.numel() and (k is None or torch.equal(k[:u], ek)) and torch.equal(c[:u].long(), ec.long())
                            if ok and vdtype.is_floating_point:
                                ok = bool(((v[:u].double() - exact).abs() <= bound).all())
                                bits = v[:u].view(torch.int32)
                                if first_bits:
                                    ok = ok and torch.equal(bits, first_bits[0])  # two calls, and the 32-bit family: bitwise equal
                                else:
                                    first_bits.append(bits.clone())
                            elif ok:
                                ok = torch.equal(v[:u], ev)
                            agree[0] = agree[0] and bool(ok)

                        after = {"reduce64": compare, "narrow": compare}
                        times = {s: [] for s in sides}
                        for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                            for s in sides:
                                times[s] += timed(fns[s], max(half, 1), 1, after.get(s, lambda out: None))
                        rd.check()
                        rd32.check()
                        if sorter is not None:
                            sorter.check()
                        assert agree[0] and len(set(seen)) == 1, f"results disagree: {cfg} {block} {space} 2^{lg} distinct {d}"
                        st = {s: stats(t) for s, t in times.items()}
                        m, u = st["reduce64"], seen[-1]
                        share = share32 = None
                        if block == "consecutive":
                            share = round((2.0 * n * (8 + vb) + u * (12.0 + vb)) / (m["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 3)
                            share32 = round((2.0 * n * (4 + vb) + u * (8.0 + vb)) / (st["narrow"]["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 3)
                        flags = [f"loses_to_{s}" for s in sides[1:] if st[s]["median_ms"] < m["median_ms"] and not (s == "narrow" and block == "consecutive")]
                        if "parts" not in sides:
                            flags.append("parts_refused_by_torch")
                        rows_out.append([cfg, block, space, lg, d, u, trio(m), trio(st.get("today")), trio(st.get("parts")), trio(st.get("narrow")), share, share32,
                                         1, ",".join(flags)])
                        print(f"# {cfg} {block:11s} {space:6s} 2^{lg} distinct {d:8d} u {u:10d} reduce64 {m['median_ms']:9.3f} ms"
                              + "".join(f"  {s} {st[s]['median_ms']:9.3f}" for s in sides[1:])
                              + (f"  share {share} (32-bit stage {share32})" if share is not None else "") + f"  {flags}", file=sys.stderr, flush=True)
                        emit()
                        del keys, vals, ek, ev, ec, k32
                        torch.cuda.empty_cache()
                rd.close()
                rd32.close()
                if sorter is not None:
                    sorter.close()
                del kcopy, vcopy
                torch.cuda.empty_cache()
    print(emit())


if __name__ == "__main__":
    main()
