#!/usr/bin/env python3
"""The 1-D top-k on 16-bit keys (gs_topk16_*) against what a user does without it, on one GPU; prints one JSON line.

bfloat16 keys, descending (the k largest, as torch.topk), n = 2^--log2, for every k of --ks, as keys only and with positions (--modes
keys,pos; v8 — carried 8-byte values — at the largest n only).  Inputs (--inputs): uniform (random 16-bit patterns, the NaN and
infinity patterns moved to finite ones so that widening and narrowing keep every bit), few (16 distinct values), equal (one value),
sorted (the uniform input, ascending).  Per n, input, mode and k:
  topk16  gs_topk16_select_keys / _pairs (route TILE, COUNT or SELECT: named in the row); keys only, beside it the COUNT route with
          each of its two histograms forced (gs_topk16_set_count_histogram: count_slices, count_global): the numbers its size rule
          (GS_TOPK16_COUNT_SLICES_MIN) rests on;
  widen   x.float(), gs_topk_select_* on the float32 copy, and the keys narrowed back to bfloat16, all inside the timed span;
  sort    a copy of the keys (and of carried values), gs_sort16_sort_keys / _argsort / _sort_pairs on the copy, and a copy of the head;
          the copy is inside the timed span, because the sort writes its input and the top-k does not;
  rows    k <= gs_topk_rows_max_k: gs_topk_select_rows_* with the 16-bit key type and rows = 1 on the same buffer;
  torch   torch.topk(x, k) (and a gather of the carried values), fewer repetitions.
All sides alternate in one process, every shape warmed, --reps timed repetitions each in two halves, device events around every single
call; median, extremes and spread per side.  Before the timing the result of every other side is compared bit for bit with the
top-k's on the same input (torch: the key values only — its tie and zero rules differ).

One compact row per shape (COLUMNS).  Two conditions follow from bytes moved (flags per row, the margin is the min-max band measured
in this process):
  count_behind_sort   a keys-only row whose median is above copy + sort + slice's by more than both bands;
  select_behind_widen a pos / v8 row with k <= 2^16 whose median is not below the widening route's by more than both bands."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd.topk import rows_max_k  # noqa: E402
from topk_perf import stats, timed  # noqa: E402

ROUTES = {0: "none", 1: "tile", 2: "count", 3: "select"}


def make_input(kind, n, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    if kind == "equal":
        return torch.full((n,), 1.5, dtype=torch.bfloat16, device=dev)
    if kind == "few":
        return (torch.randint(0, 16, (n,), dtype=torch.int16, device=dev, generator=gen) * 0x0111 + 0x3000).view(torch.bfloat16)
    bits = torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device=dev, generator=gen)
    bits = torch.where((bits & 0x7F80) == 0x7F80, bits & ~0x0080, bits)  # exponent all ones (inf, NaN) -> the binade below
    x = bits.view(torch.bfloat16)
    if kind == "sorted":
        x = x.clone()
        g.sort_(x)
    return x


def band(s):
    return s["max_ms"] - s["min_ms"]


# one measured row of the JSON, in this order; times in ms, rounded to a microsecond; null where a side has no route or was not run
COLUMNS = ["n_log2", "input", "mode", "k", "route", "topk16 [median, min, max]", "widen [median, min, max]", "sort [median, min, max]", "rows median",
           "torch median", "count_slices median", "count_global median", "results_agree", "flags"]


def trio(s):
    return [round(s["median_ms"], 3), round(s["min_ms"], 3), round(s["max_ms"], 3)]


def med(s):
    return None if s is None else round(s["median_ms"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26, 28])
    ap.add_argument("--ks", default="1,8,64,1024,65536,1048576")
    ap.add_argument("--modes", default="keys,pos,v8")
    ap.add_argument("--inputs", default="uniform,few,equal,sorted")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ks = [int(x) for x in args.ks.split(",")]
    kmax = max(ks)
    rows_out = []
    for lg in args.log2:
        n = 1 << lg
        copy_k = torch.empty(n, dtype=torch.bfloat16, device=dev)
        for what in args.modes.split(","):
            if what == "v8" and lg != max(args.log2):
                continue
            pairs, vb = what != "keys", {"keys": 0, "pos": 4, "v8": 8}[what]
            mode = g.MODE_PAIRS if pairs else g.MODE_KEYS_ONLY
            vdt = torch.int64 if vb == 8 else torch.int32
            vals = (torch.arange(n, dtype=torch.int64, device=dev) * 3 + 1) if what == "v8" else None
            copy_v = torch.empty(n, dtype=vdt, device=dev) if pairs else None
            top = g.TopK16(n, min(kmax, n), g.ORDER_DESCENDING, g.KEY_BFLOAT16, mode, vb)
            top32 = g.TopK(n, min(kmax, n), g.ORDER_DESCENDING, g.KEY_FLOAT32, mode, vb)
            rows = g.TopK(n, min(kmax, n), g.ORDER_DESCENDING, g.KEY_BFLOAT16, mode, vb)
            sort = g.Sort16(n, g.ORDER_DESCENDING, g.KEY_BFLOAT16, mode, vb)
            max_rows_k = rows_max_k(mode, vb)
            for kind in args.inputs.split(","):
                src = make_input(kind, n, dev)
                for k in (k for k in ks if k <= n):
                    forced = ["count_slices", "count_global"] if not pairs else []
                    sides = ["topk16", "widen", "sort"] + (["rows"] if k <= max_rows_k else []) + ["torch"] + forced
                    outs = {s: (torch.empty(k, dtype=torch.bfloat16, device=dev), torch.empty(k, dtype=vdt, device=dev) if pairs else None) for s in sides}
                    wide_out = torch.empty(k, dtype=torch.float32, device=dev)

                    def run_topk16():
                        top.select(src, k, outs["topk16"][0], vals, outs["topk16"][1], n=n)

                    def run_forced(which, name):
                        def run():
                            top.set_count_histogram(which)
                            top.select(src, k, outs[name][0], None, None, n=n)
                            top.set_count_histogram(0)
                        return run

                    def run_widen():
                        wide = src.float()
                        top32.select(wide, k, wide_out, vals, outs["widen"][1], n=n)
                        outs["widen"][0].copy_(wide_out)  # float32 -> bfloat16

                    def run_sort():
                        copy_k.copy_(src)
                        if what == "pos":
                            sort.argsort(copy_k, copy_v, n=n)
                        elif what == "v8":
                            copy_v.copy_(vals)
                            sort.sort(copy_k, copy_v, n=n)
                        else:
                            sort.sort(copy_k, None, n=n)
                        outs["sort"][0].copy_(copy_k[:k])
                        if pairs:
                            outs["sort"][1].copy_(copy_v[:k])

                    def run_rows():
                        rows.select_rows(src, 1, n, n, k, outs["rows"][0], vals, outs["rows"][1])

                    def run_torch():
                        v, i = torch.topk(src, k)
                        outs["torch"][0].copy_(v)
                        if what == "v8":
                            outs["torch"][1].copy_(vals[i])
                        elif pairs:
                            outs["torch"][1].copy_(i)

                    fns = {"topk16": run_topk16, "widen": run_widen, "sort": run_sort, "rows": run_rows, "torch": run_torch,
                           "count_slices": run_forced(1, "count_slices"), "count_global": run_forced(2, "count_global")}
                    # verify on the same input before timing (also the first warm-up of every side)
                    agree = {}
                    for s in sides:
                        fns[s]()
                    torch.cuda.synchronize()
                    top.check()
                    top32.check()
                    sort.check()
                    rows.check()
                    run_topk16()
                    route = ROUTES[top.last()["route"]] + {0: "", 1: "", 2: " (global)"}[top.last()["hist"] if not pairs else 0]
                    mine = outs["topk16"]
                    for s in sides[1:]:
                        if s == "torch":
                            agree[s] = bool(torch.equal(outs[s][0].float(), mine[0].float()))
                        else:
                            agree[s] = bool(torch.equal(outs[s][0].view(torch.int16), mine[0].view(torch.int16)) and
                                            (not pairs or torch.equal(outs[s][1], mine[1])))
                    times = {s: [] for s in sides}
                    for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                        for s in sides:
                            reps = half if s != "torch" else max(1, (args.torch_reps + 1) // 2)
                            times[s] += timed(fns[s], max(reps, 1), warm=1)
                    st = {s: stats(t) for s, t in times.items()}
                    m = st["topk16"]
                    ratio = {x: st[x]["median_ms"] / m["median_ms"] for x in st}
                    flags = [name for name, hit in (
                        ("count_behind_sort", route.startswith("count") and m["median_ms"] - st["sort"]["median_ms"] > band(m) + band(st["sort"])),
                        ("select_behind_widen", route == "select" and k <= (1 << 16) and
                         st["widen"]["median_ms"] - m["median_ms"] <= band(m) + band(st["widen"])),
                        ("loses_in_the_median", any(ratio[x] < 1.0 for x in sides[1:] if x not in forced))) if hit]
                    row = [lg, kind, what, k, route, trio(m), trio(st["widen"]), trio(st["sort"]), med(st.get("rows")), med(st["torch"]),
                           med(st.get("count_slices")), med(st.get("count_global")), int(all(agree.values())), ",".join(flags)]
                    rows_out.append(row)
                    print(f"# 2^{lg} {kind:8s} {what:4s} k {k:8d} {route:14s} topk16 {m['median_ms']:8.3f} ms [{m['min_ms']:.3f}, {m['max_ms']:.3f}]  widen "
                          f"{st['widen']['median_ms']:8.3f} x{ratio['widen']:.2f}  sort {st['sort']['median_ms']:8.3f} x{ratio['sort']:.2f}  rows "
                          + (f"{st['rows']['median_ms']:8.3f} x{ratio['rows']:.2f}" if "rows" in st else "       -") +
                          f"  torch {st['torch']['median_ms']:8.3f} x{ratio['torch']:.2f}"
                          + (f"  slices {st['count_slices']['median_ms']:.3f} global {st['count_global']['median_ms']:.3f}" if forced else "") +
                          f"  agree {agree}", file=sys.stderr, flush=True)
                    del outs, wide_out
                del src
            for h in (top, top32, rows, sort):
                h.close()
            del vals, copy_v
        del copy_k
        torch.cuda.empty_cache()
    out = {"tool": "topk16_perf", "reps": args.reps, "torch_reps": args.torch_reps, "device": torch.cuda.get_device_name(0), "key_type": "bfloat16",
           "order": "descending", "widen": "x.float() + gs_topk_select_* (float32) + the keys narrowed to bfloat16, all inside the timed span",
           "sort": "copy + gs_sort16_sort_keys / _argsort / _sort_pairs + a copy of the head, copies inside the timed span",
           "rows": "gs_topk_select_rows_* with GS_KEY_BFLOAT16, rows = 1, where k <= gs_topk_rows_max_k",
           "torch": "torch.topk(x, k) and copies of its outputs (v8: a gather of the values)",
           "flags": "count_behind_sort, select_behind_widen: the two conditions of DESIGN.md 3.20, margin = both min-max bands; loses_in_the_median: "
                    "a comparator's median below the call's", "columns": COLUMNS, "rows_measured": rows_out}
    line = json.dumps(out, separators=(",", ":"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
