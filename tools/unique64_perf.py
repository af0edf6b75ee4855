#!/usr/bin/env python3
"""unique / run-length encode on 64-bit keys (gs_unique64_*) against what a user does without it, on one GPU; prints one JSON line (and
rewrites --out after every row).

int64 keys, ascending, as draws from d distinct random values (d of --distinct; 0 = uniform draws, about n distinct) of two key spaces
(--spaces): low32 (values below 2^31: typical ids; the engine drops the four constant bytes) and full64 (the whole int64 range).  Three
blocks (--blocks):
  keys         gs_unique64_keys (keys + counts), n = 2^--log2;
  positions    gs_unique64_positions (keys, counts, first, inverse), n = 2^min(--log2, --positions-max-log2);
  consecutive  gs_unique64_consecutive alone on the SORTED input (keys, counts, inverse): the stage by itself, also as a share of
               --peak-tbs TB/s over the bytes it moves, 20 n + 12 u (two reads of the keys, the inverse, 8-byte keys and 4-byte counts
               out), beside the 32-bit stage (gs_unique_consecutive, 12 n + 8 u) on int32 keys with the same runs, in the same run.
Sides per block:
  unique64  the call (full-capacity outputs allocated inside the timed span, no host wait);
  torch     torch.unique(sorted=True, ...) on the same tensor (it has no first positions); consecutive: torch.unique_consecutive;
  parts     copy + gs_onesweep_sort_keys / _sort_pairs on 64-bit keys + torch.unique_consecutive, and for positions the inverse scattered
            through the sorted positions and first gathered at the run starts: the same outputs (consecutive: none);
  narrow    low32 only: keys.to(int32) + the 32-bit call (gs_unique_keys / _positions) + its keys widened to int64 (consecutive: the
            32-bit stage alone on keys narrowed outside the timed span, `stage32`).
All sides alternate in one process, every side warmed, --reps timed repetitions each in two halves, device events around every single
call; median and extremes per side.  EVERY repetition's result of the call is compared with the comparators' (computed once on the same
input): u, keys, counts, and first / inverse where both sides have them; the row asserts it.  flags: loses_to_<side> when that side's
median is below the call's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from topk_perf import stats  # noqa: E402
from unique_perf import timed, trio  # noqa: E402

COLUMNS = ["block", "space", "n_log2", "distinct", "u", "unique64 [median, min, max]", "torch [median, min, max]", "parts [median, min, max]",
           "narrow / stage32 [median, min, max]", "share of peak", "32-bit stage's share", "results_agree", "flags"]


def make_input64(n, distinct, space, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345 + distinct)
    lo, hi = (0, (1 << 31) - 1) if space == "low32" else (-(1 << 63), (1 << 63) - 1)
    if distinct == 0:
        return torch.randint(lo, hi, (n,), dtype=torch.int64, device=dev, generator=gen)
    pool = torch.randint(lo, hi, (distinct,), dtype=torch.int64, device=dev, generator=gen)
    return pool[torch.randint(0, distinct, (n,), device=dev, generator=gen)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26, 28])
    ap.add_argument("--positions-max-log2", type=int, default=28)
    ap.add_argument("--distinct", default="16,65536,0")
    ap.add_argument("--spaces", default="low32,full64")
    ap.add_argument("--blocks", default="keys,positions,consecutive")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None, help="also write the JSON here, after every row")
    args = ap.parse_args()
    assert args.reps >= 5, "medians over at least 5 timed calls"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows_out = []

    def emit():
        out = {"tool": "unique64_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "key_type": "int64", "order": "ascending",
               "unique64": "gs_unique64_keys / _positions / _consecutive, outputs allocated inside the timed span",
               "torch": "torch.unique(sorted=True, ...) on the same tensor; consecutive: torch.unique_consecutive on the sorted input",
               "parts": "copy + gs_onesweep_sort_keys / _sort_pairs (64-bit keys; positions from arange) + torch.unique_consecutive, and for "
                        "positions the inverse scattered through the sorted positions and first gathered at the run starts",
               "narrow / stage32": "low32: to(int32) + gs_unique_keys / _positions + keys widened; consecutive: gs_unique_consecutive on int32 keys "
                                   "with the same runs (narrowed outside the timed span)",
               "share of peak": f"consecutive only: (20 n + 12 u) bytes / median / {args.peak_tbs} TB/s; the 32-bit stage: (12 n + 8 u)",
               "columns": COLUMNS, "rows_measured": rows_out}
        line = json.dumps(out, separators=(",", ":"))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    for block in args.blocks.split(","):
        sizes = sorted({min(lg, args.positions_max_log2) if block == "positions" else lg for lg in args.log2})
        for lg in sizes:
            n = 1 << lg
            pairs = block == "positions"
            uq = g.Unique64(n, g.ORDER_ASCENDING, g.KEY_INT64, positions=pairs)
            uq32 = g.Unique(n, g.ORDER_ASCENDING, g.KEY_UINT32, positions=pairs)
            sorter = None if block == "consecutive" else g.OneSweep(n, g.ORDER_ASCENDING, g.KEY_INT64, g.MODE_PAIRS if pairs else g.MODE_KEYS_ONLY,
                                                                    4 if pairs else 0)
            copy = torch.empty(n, dtype=torch.int64, device=dev)
            for space in args.spaces.split(","):
                for d in (int(x) for x in args.distinct.split(",")):
                    if d > n:
                        continue
                    src = make_input64(n, d, space, dev)
                    k32 = None
                    if block == "consecutive":
                        src = torch.sort(src).values.contiguous()
                        k32 = torch.unique_consecutive(src, return_inverse=True)[1].to(torch.int32)  # int32 keys with the same runs

                    def run_unique():
                        if block == "keys":
                            k, c, num = uq.unique(src)
                            return k, c, None, None, num
                        if block == "positions":
                            return uq.unique_positions(src)
                        k, c, i, num = uq.unique_consecutive(src)
                        return k, c, None, i, num

                    def run_parts():
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

                    def run_narrow():
                        if block == "consecutive":  # the 32-bit stage alone
                            k, c, i, num = uq32.unique_consecutive(k32)
                            return None, c, None, i, num
                        s32 = src.to(torch.int32)
                        if block == "keys":
                            k, c, num = uq32.unique(s32)
                            return k.to(torch.int64), c, None, None, num
                        k, c, f, i, num = uq32.unique_positions(s32)
                        return k.to(torch.int64), c, f, i, num

                    fns = {"unique64": run_unique, "torch": run_torch, "parts": run_parts, "narrow": run_narrow}
                    sides = ["unique64", "torch"] + (["parts"] if block != "consecutive" else []) + \
                            (["narrow"] if (space == "low32" or block == "consecutive") else [])
                    expect = {}
                    for s in ("torch", "parts"):
                        if s in sides:
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

                    def compare_narrow(out):  # the narrowed call against the comparators as well
                        k, c, f, i, num = out
                        u = int(num.item())
                        ek, ec, ef, ei = expect["torch"]
                        ok = u == ek.numel() and (k is None or torch.equal(k[:u], ek)) and torch.equal(c[:u], ec)
                        if ok and i is not None and ei is not None:
                            ok = torch.equal(i, ei)
                        agree["narrow"] = agree["narrow"] and bool(ok)

                    after = {"unique64": compare, "narrow": compare_narrow}
                    times = {s: [] for s in sides}
                    for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                        for s in sides:
                            times[s] += timed(fns[s], max(half, 1), 1, after.get(s, lambda out: None))
                    uq.check()
                    uq32.check()
                    if sorter is not None:
                        sorter.check()
                    assert all(agree.values()) and len(set(seen_u)) == 1, f"results disagree: {block} {space} 2^{lg} distinct {d}: {agree}"
                    st = {s: stats(t) for s, t in times.items()}
                    m, u = st["unique64"], seen_u[-1]
                    share = share32 = None
                    if block == "consecutive":
                        share = round((20.0 * n + 12.0 * u) / (m["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 3)
                        share32 = round((12.0 * n + 8.0 * u) / (st["narrow"]["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 3)
                    flags = [f"loses_to_{s}" for s in sides[1:] if st[s]["median_ms"] < m["median_ms"] and not (s == "narrow" and block == "consecutive")]
                    rows_out.append([block, space, lg, d, u, trio(m), trio(st["torch"]), trio(st.get("parts")), trio(st.get("narrow")), share, share32, 1,
                                     ",".join(flags)])
                    print(f"# {block:11s} {space:6s} 2^{lg} distinct {d:8d} u {u:10d} unique64 {m['median_ms']:9.3f} ms"
                          + "".join(f"  {s} {st[s]['median_ms']:9.3f}" for s in sides[1:])
                          + (f"  share {share} (32-bit stage {share32})" if share is not None else "") + f"  {flags}", file=sys.stderr, flush=True)
                    emit()
                    del src, expect, k32
                    torch.cuda.empty_cache()
            uq.close()
            uq32.close()
            if sorter is not None:
                sorter.close()
            del copy
            torch.cuda.empty_cache()
    print(emit())


if __name__ == "__main__":
    main()
