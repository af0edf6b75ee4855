#!/usr/bin/env python3
"""Sorted search (gs_search_*) against torch.searchsorted, on one GPU; prints one JSON line.

Integer keys, ascending, where the answers of both must agree: uint32 (31-bit draws: the unsigned order is torch's signed order on the
same int32 storage) and int64.  The haystack is n = 2^--n-log2 sorted uniform draws, the queries m = 2^--m-log2 draws from the same
range, once in order ("sorted") and once as drawn ("shuffled").  Sides per row:
  tile     route TILE forced, queries declared sorted (sorted queries only);
  sort     route SORT forced: copy + positions, the pairs sort, the tile kernel, a scattered store;
  table    route BINARY forced with the sample table;
  plain    route BINARY forced, every level in global memory;
  auto     whatever AUTO takes for the row (queries_sorted as the row says), on a handle with the engine;
  torch    torch.searchsorted(hay, q) (int64 positions);
  today    shuffled queries only: gs_onesweep_sort_pairs of (query, position) + torch.searchsorted on the sorted queries + the result
           scattered through the positions: what a caller of this library does without gs_search_*.
All sides alternate in one process, every side warmed, --reps timed repetitions each, device events around every single call; median,
min, max per side.  EVERY side's result is compared with torch's on every row (results_agree; the tool exits 1 if any row disagrees).
share of peak: the tile side on sorted queries as a share of --peak-tbs TB/s over key_bytes * n * [share of tiles staged in LDS] +
(key_bytes + 4) * m bytes.  flags: loses_to_torch / loses_to_today per side whose median is above that comparator's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd import search as gsearch  # noqa: E402
from topk_perf import stats  # noqa: E402
from unique_perf import timed, trio  # noqa: E402

COLUMNS = ["key", "n_log2", "m_log2", "queries", "auto_route", "tile", "sort", "table", "plain", "auto", "torch", "today", "tile share of peak",
           "lds_tiles/tiles", "results_agree", "flags"]
OURS = ("tile", "sort", "table", "plain", "auto")


def draw(count, dtype, dev, seed):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    if dtype == torch.int32:
        return torch.randint(0, (1 << 31) - 1, (count,), dtype=dtype, device=dev, generator=gen)
    return torch.randint(-(1 << 62), 1 << 62, (count,), dtype=dtype, device=dev, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-log2", type=int, nargs="+", default=[20, 24, 28])
    ap.add_argument("--m-log2", type=int, nargs="+", default=[10, 16, 20, 24, 28])
    ap.add_argument("--keys", default="uint32,int64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows, all_agree = [], True
    for key in args.keys.split(","):
        dtype, kt, kb = (torch.int32, g.KEY_UINT32, 4) if key == "uint32" else (torch.int64, g.KEY_INT64, 8)
        maxn, maxm = 1 << max(args.n_log2), 1 << max(args.m_log2)
        h = g.SortedSearch(maxn, maxm, kt, sort_queries=True)
        sorter = g.OneSweep(maxm, g.ORDER_ASCENDING, kt, g.MODE_PAIRS, 4)
        for nl in args.n_log2:
            n = 1 << nl
            hay = torch.sort(draw(n, dtype, dev, 1000 + nl)).values.contiguous()
            for ml in args.m_log2:
                m = 1 << ml
                shuffled = draw(m, dtype, dev, 2000 + ml)
                for kind in ("sorted", "shuffled"):
                    q = torch.sort(shuffled).values.contiguous() if kind == "sorted" else shuffled
                    out = torch.empty(m, dtype=torch.int32, device=dev)
                    copy, perm = torch.empty_like(q), torch.empty(m, dtype=torch.int32, device=dev)
                    info = {}

                    def ours(side):
                        def run():
                            h.set_route({"tile": "tile", "sort": "sort", "auto": "auto"}.get(side, "binary"))
                            h.set_table({"table": gsearch.TABLE_ON, "plain": gsearch.TABLE_OFF}.get(side, gsearch.TABLE_AUTO))
                            h.search(hay, q, n, m, queries_sorted=(side == "tile") or (side == "auto" and kind == "sorted"), out=out)
                            return out
                        return run

                    def run_torch():
                        return torch.searchsorted(hay, q)

                    def run_today():
                        copy.copy_(q)
                        torch.arange(m, dtype=torch.int32, device=dev, out=perm)
                        sorter.sort(copy, perm, n=m)
                        res = torch.empty(m, dtype=torch.int64, device=dev)
                        res[perm.long()] = torch.searchsorted(hay, copy)
                        return res

                    fns = {s: ours(s) for s in OURS if s != "tile" or kind == "sorted"}
                    fns["torch"] = run_torch
                    if kind == "shuffled":
                        fns["today"] = run_today
                    expect = run_torch().to(torch.int32)
                    torch.cuda.synchronize()
                    agree = {}

                    def compare(side):
                        def after(res):
                            agree[side] = agree.get(side, True) and bool(torch.equal(res.to(torch.int32), expect))
                            if side in OURS:
                                info[side] = h.last()
                        return after

                    times = {s: [] for s in fns}
                    for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                        for s, fn in fns.items():
                            times[s] += timed(fn, max(half, 1), 1, compare(s))
                    st = {s: stats(t) for s, t in times.items()}
                    flags = []
                    for s in OURS:
                        if s in st:
                            flags += [f"{s}_loses_to_{c}" for c in ("torch", "today") if c in st and st[c]["median_ms"] < st[s]["median_ms"]]
                    share = frac = None
                    if "tile" in st:
                        rep = info["tile"]
                        tiles = rep["lds_tiles"] + rep["global_tiles"]
                        frac = [rep["lds_tiles"], tiles]
                        share = round((kb * n * rep["lds_tiles"] / tiles + (kb + 4.0) * m) / (st["tile"]["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 4)
                    ok = all(agree.values())
                    all_agree = all_agree and ok
                    auto_route = {1: "tile", 2: "sort", 3: "binary"}[info["auto"]["route"]] + ("+table" if info["auto"]["table"] else "")
                    rows.append([key, nl, ml, kind, auto_route] + [trio(st.get(s)) for s in OURS + ("torch", "today")] + [share, frac, int(ok), ",".join(flags)])
                    print(f"# {key} n 2^{nl} m 2^{ml} {kind:8s} auto {auto_route:12s} " +
                          " ".join(f"{s} {st[s]['median_ms']:.3f}" for s in st) + f" share {share} lds {frac} agree {int(ok)} {flags}",
                          file=sys.stderr, flush=True)
                    del q, out, copy, perm, expect
                del shuffled
                torch.cuda.empty_cache()
            del hay
            torch.cuda.empty_cache()
        h.close()
        sorter.close()
    res = {"tool": "search_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "order": "ascending", "side": "left",
           "plan": g.search_plan(1 << 20, 1 << 20, 4), "times": "[median, min, max] ms", "columns": COLUMNS, "rows_measured": rows}
    line = json.dumps(res, separators=(",", ":"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if all_agree else 1)


if __name__ == "__main__":
    main()
