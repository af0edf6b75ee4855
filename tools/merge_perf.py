#!/usr/bin/env python3
"""Merge (gs_merge_*) against what a caller does without it, on one GPU; prints one JSON line.

Integer keys, ascending, where torch's order agrees: uint32 (31-bit draws on int32 storage: the unsigned order is torch's signed order)
and int64.  A row is (na, nb) = (2^a, 2^b) and an input kind: "uniform" (both sides uniform draws over one range, sorted by this
library), "disjoint" (every key of A below every key of B: all tiles but one are copies) and "equal" (one key on both sides).  Forms per
row: keys, pairs4 / pairs8 (4- / 8-byte values) and positions.  Sides per row and form:
  merge     gs_merge_keys / _pairs / _positions into buffers that exist;
  cat_sort  what callers do today: torch.cat of the keys (and of the values; positions: an arange) + this library's sort of the n keys:
            the keys-only sort for keys, the stable pairs sort otherwise;
  torch     torch.sort(torch.cat([a, b]), stable=True); pairs: the concatenated values gathered through its indices; positions: its indices.
All sides alternate in one process, every side warmed, --reps timed repetitions each, device events around every single call; median,
min, max per side.  EVERY side's result is compared with torch's on every row (results_agree; the tool exits 1 if any row disagrees).
share of peak: the merge side as a share of --peak-tbs TB/s over 2 * (na + nb) * (key_bytes + value_bytes) bytes (positions: 4 bytes
written per key, none read).  flags: merge_loses_to_cat_sort / merge_loses_to_torch where the merge's median is above that side's."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd import _merge  # noqa: E402
from topk_perf import stats  # noqa: E402
from unique_perf import timed, trio  # noqa: E402

COLUMNS = ["key", "na_log2", "nb_log2", "input", "form", "merge", "cat_sort", "torch", "merge share of peak", "copy_tiles/tiles", "results_agree",
           "flags"]
DEFAULT_ROWS = "27:27:uniform,28:20:uniform,28:12:uniform,23:23:uniform,20:20:uniform,16:16:uniform,23:23:disjoint,23:23:equal"
FORMS = ("keys", "pairs4", "pairs8", "positions")


def draw(count, dtype, dev, seed, lo=None, hi=None):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    if dtype == torch.int32:
        return torch.randint(0 if lo is None else lo, (1 << 31) - 1 if hi is None else hi, (count,), dtype=dtype, device=dev, generator=gen)
    return torch.randint(-(1 << 62) if lo is None else lo, 1 << 62 if hi is None else hi, (count,), dtype=dtype, device=dev, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=DEFAULT_ROWS, help="na_log2:nb_log2:input, comma separated")
    ap.add_argument("--keys", default="uint32,int64")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-torch", action="store_true", help="leave torch.sort out (the expected result is then cat_sort's)")
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    specs = [(int(a), int(b), kind) for a, b, kind in (r.split(":") for r in args.rows.split(","))]
    nmax = max((1 << a) + (1 << b) for a, b, _ in specs)
    rows, all_agree = [], True
    for key in args.keys.split(","):
        dtype, kt, kb = (torch.int32, g.KEY_UINT32, 4) if key == "uint32" else (torch.int64, g.KEY_INT64, 8)
        h = _merge.Merge(nmax, kt)
        sorters = {0: g.OneSweep(nmax, g.ORDER_ASCENDING, kt, g.MODE_KEYS_ONLY, 0), 4: g.OneSweep(nmax, g.ORDER_ASCENDING, kt, g.MODE_PAIRS, 4),
                   8: g.OneSweep(nmax, g.ORDER_ASCENDING, kt, g.MODE_PAIRS, 8)}
        for al, bl, kind in specs:
            na, nb = 1 << al, 1 << bl
            n = na + nb
            if kind == "equal":
                a, b = torch.full((na,), 12345, dtype=dtype, device=dev), torch.full((nb,), 12345, dtype=dtype, device=dev)
            else:
                a = draw(na, dtype, dev, 1000 + al, hi=(1 << 30) if kind == "disjoint" else None)
                b = draw(nb, dtype, dev, 2000 + bl, lo=(1 << 30) if kind == "disjoint" else None)
                sorters[0].sort(a)  # sorted by this library
                sorters[0].sort(b)
            for form in args.forms.split(","):
                vb = {"pairs4": 4, "pairs8": 8, "positions": 4}.get(form, 0)
                vdtype = torch.int64 if vb == 8 else torch.int32
                out = torch.empty(n, dtype=dtype, device=dev)
                aux = torch.empty(n, dtype=vdtype, device=dev) if vb else None
                va = vbv = None
                if form.startswith("pairs"):
                    va = torch.arange(na, dtype=vdtype, device=dev) * 3 + 1
                    vbv = torch.arange(nb, dtype=vdtype, device=dev) * 5 + 2
                info = {}

                def run_merge():
                    if form == "keys":
                        h.merge(a, b, na, nb, out=out)
                    elif form == "positions":
                        h.merge_positions(a, b, na, nb, out_keys=out, out_src=aux)
                    else:
                        h.merge_pairs(a, va, b, vbv, na, nb, out_keys=out, out_values=aux)
                    return out, aux

                def run_cat_sort():
                    k = torch.cat([a, b])
                    if form == "keys":
                        sorters[0].sort(k)
                        return k, None
                    v = torch.arange(n, dtype=torch.int32, device=dev) if form == "positions" else torch.cat([va, vbv])
                    sorters[vb].sort(k, v)
                    return k, v

                def run_torch():
                    k, idx = torch.sort(torch.cat([a, b]), stable=True)
                    if form == "keys":
                        return k, None
                    return k, (idx if form == "positions" else torch.cat([va, vbv])[idx])

                fns = {"merge": run_merge, "cat_sort": run_cat_sort}
                if not args.no_torch:
                    fns["torch"] = run_torch
                ek, ea = (run_cat_sort if args.no_torch else run_torch)()
                ea = None if ea is None else ea.to(vdtype)
                torch.cuda.synchronize()
                agree = {}

                def compare(side):
                    def after(res):
                        k, x = res
                        same = bool(torch.equal(k, ek)) and (x is None or bool(torch.equal(x.to(vdtype), ea)))
                        agree[side] = agree.get(side, True) and same
                        if side == "merge":
                            info["last"] = h.last()
                    return after

                times = {s: [] for s in fns}
                for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                    for s, fn in fns.items():
                        times[s] += timed(fn, max(half, 1), 1, compare(s))
                st = {s: stats(t) for s, t in times.items()}
                flags = [f"merge_loses_to_{c}" for c in ("cat_sort", "torch") if c in st and st[c]["median_ms"] < st["merge"]["median_ms"]]
                moved = n * (2 * kb + 4) if form == "positions" else 2 * n * (kb + vb)
                share = round(moved / (st["merge"]["median_ms"] * 1e-3) / (args.peak_tbs * 1e12), 4)
                rep = info["last"]
                ok = all(agree.values())
                all_agree = all_agree and ok
                rows.append([key, al, bl, kind, form] + [trio(st.get(s)) for s in ("merge", "cat_sort", "torch")] +
                            [share, [rep["copy_tiles"], rep["tiles"]], int(ok), ",".join(flags)])
                print(f"# {key} na 2^{al} nb 2^{bl} {kind:8s} {form:9s} " + " ".join(f"{s} {st[s]['median_ms']:.3f}" for s in st) +
                      f" share {share} copy {rep['copy_tiles']}/{rep['tiles']} agree {int(ok)} {flags}", file=sys.stderr, flush=True)
                del out, aux, va, vbv, ek, ea
                torch.cuda.empty_cache()
            del a, b
            torch.cuda.empty_cache()
        h.close()
        for s in sorters.values():
            s.close()
    res = {"tool": "merge_perf", "reps": args.reps, "device": torch.cuda.get_device_name(0), "order": "ascending",
           "plan": {"4": _merge.merge_plan(1 << 20, 1 << 20, 4), "8": _merge.merge_plan(1 << 20, 1 << 20, 8)}, "times": "[median, min, max] ms",
           "columns": COLUMNS, "rows_measured": rows}
    line = json.dumps(res, separators=(",", ":"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if all_agree else 1)


if __name__ == "__main__":
    main()
