#!/usr/bin/env python3
"""unique / run-length encode on 16-bit keys (gs_unique16_*) against what a user does without it, on one GPU; prints one JSON line.

bfloat16 and int16 keys, ascending.  The keys are draws from d distinct values (d of --distinct; 65536 stands for "every pattern the
type has that is equal to no other by value": all 65 536 for int16; for bfloat16 every pattern but the NaNs and -0.0, 65 281).  Without
-0.0 / +0.0 pairs and NaNs bitwise equality is equality by value, so every side delivers the same arrays.
Blocks (--blocks):
  keys         gs_unique16_unique, keys + counts;
  all          gs_unique16_unique, keys, counts, first and inverse;
  consecutive  gs_unique16_consecutive on the SORTED input (keys, counts, inverse);
  forms        gs_unique16_unique, keys + inverse, with the inverse lookup forced to the LDS table and to the gather
               (gs_unique16_set_inverse_form): the two numbers behind GS_UNIQUE16_INVERSE_LDS_MIN.  No comparator.
Sides per block:
  unique16  the call (outputs allocated inside the timed span, no host wait);
  widen     the detour the call replaces: a widening pass (bfloat16 -> float32, int16 -> int32), gs_unique_keys (keys) or
            gs_unique_positions (all) on the 32-bit keys, and the narrowing of the u distinct keys (one host wait for u); consecutive:
            widening + gs_unique_consecutive + narrowing;
  torch     keys: torch.unique(sorted=True, return_counts=True); all: torch.unique(sorted=True, return_inverse=True, return_counts=True)
            (it has no first positions); consecutive: torch.unique_consecutive(return_inverse=True, return_counts=True).
All sides alternate in one process, every side warmed, --reps timed repetitions each in two halves (torch: --torch-reps), device events
around every single call; median, extremes and spread per side.  EVERY repetition's result of the call is compared with the comparators'
(computed once on the same input): u, keys, counts, and first / inverse where both sides have them.  flags: loses_to_widen /
loses_to_torch when that side's median is below the call's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from gpusorting_amd.unique16 import INVERSE_AUTO, INVERSE_GATHER, INVERSE_LDS, INVERSE_LDS_MIN  # noqa: E402
from topk_perf import stats  # noqa: E402
from unique_perf import timed, trio  # noqa: E402

COLUMNS = ["block", "dtype", "n_log2", "distinct", "u", "unique16 [median, min, max]", "widen [median, min, max]", "torch [median, min, max]",
           "results_agree", "flags"]
FORM_COLUMNS = ["block", "dtype", "n_log2", "distinct", "u", "lds [median, min, max]", "gather [median, min, max]", "auto picks", "flags"]


def pool_of(dtype, distinct, gen_seed):
    """`distinct` distinct 16-bit patterns of the type, as an int16 host array: no NaN, no -0.0."""
    rng = np.random.default_rng(gen_seed)
    if dtype == "int16":
        every = np.arange(1 << 16, dtype=np.uint16)
    else:  # bfloat16: the finite values and the infinities of both signs, without -0.0
        every = np.concatenate([np.arange(0x0000, 0x7F81), np.arange(0x8001, 0xFF81)]).astype(np.uint16)
    distinct = min(distinct, every.size)
    return rng.permutation(every)[:distinct].view(np.int16)


def make_input(dtype, n, distinct, dev):
    pool = torch.from_numpy(pool_of(dtype, distinct, 777 + distinct).copy()).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345 + distinct)
    src = pool[torch.randint(0, pool.numel(), (n,), device=dev, generator=gen)]
    return src.view(torch.bfloat16) if dtype == "bfloat16" else src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 24, 26, 28])
    ap.add_argument("--dtypes", default="bfloat16,int16")
    ap.add_argument("--distinct", default="16,1024,65536")
    ap.add_argument("--blocks", default="keys,all,consecutive,forms")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows_out, form_rows = [], []
    for dtype in args.dtypes.split(","):
        kt16, kt32, wide = (g.KEY_BFLOAT16, g.KEY_FLOAT32, torch.float32) if dtype == "bfloat16" else (g.KEY_INT16, g.KEY_INT32, torch.int32)
        tdtype = torch.bfloat16 if dtype == "bfloat16" else torch.int16
        for block in args.blocks.split(","):
            for lg in args.log2:
                n = 1 << lg
                uq16 = g.Unique16(n, g.ORDER_ASCENDING, kt16)
                uq32 = None if block == "forms" else g.Unique(n, g.ORDER_ASCENDING, kt32, positions=block == "all")
                for d in (int(x) for x in args.distinct.split(",")):
                    src = make_input(dtype, n, d, dev)
                    if block == "consecutive":
                        src = torch.sort(src.view(torch.int16)).values.contiguous().view(tdtype)
                    if block == "forms":
                        per_form, us = {}, set()
                        for half in (args.reps // 2, args.reps - args.reps // 2):
                            for name, form in (("lds", INVERSE_LDS), ("gather", INVERSE_GATHER)):
                                uq16.set_inverse_form(form)
                                per_form.setdefault(name, [])
                                per_form[name] += timed(lambda: uq16.unique(src, counts=False, first=False), max(half, 1), 1,
                                                        lambda out: us.add(int(out[4].item())))
                        uq16.set_inverse_form(INVERSE_AUTO)
                        uq16.check()
                        st = {k: stats(v) for k, v in per_form.items()}
                        auto = "lds" if n >= INVERSE_LDS_MIN else "gather"
                        best = min(st, key=lambda k: st[k]["median_ms"])
                        flags = "" if best == auto else f"auto_picks_the_slower_{auto}"
                        form_rows.append([block, dtype, lg, d, sorted(us)[0], trio(st["lds"]), trio(st["gather"]), auto, flags])
                        print(f"# forms {dtype:8s} 2^{lg} distinct {d:6d} lds {st['lds']['median_ms']:.3f} gather {st['gather']['median_ms']:.3f} "
                              f"auto {auto} {flags}", file=sys.stderr, flush=True)
                        continue

                    def run_unique16():
                        if block == "keys":
                            k, c, f, i, num = uq16.unique(src, first=False, inverse=False)
                        elif block == "all":
                            k, c, f, i, num = uq16.unique(src)
                        else:
                            k, c, i, num = uq16.unique_consecutive(src)
                            f = None
                        return k.view(tdtype), c, f, i, num

                    def run_widen():
                        w = src.to(wide)
                        if block == "keys":
                            k, c, num = uq32.unique(w)
                            f = i = None
                        elif block == "all":
                            k, c, f, i, num = uq32.unique_positions(w)
                        else:
                            k, c, i, num = uq32.unique_consecutive(w)
                            f = None
                        u = int(num.item())
                        return k[:u].view(wide).to(tdtype), c[:u], None if f is None else f[:u], i

                    def run_torch():
                        if block == "keys":
                            k, c = torch.unique(src, sorted=True, return_counts=True)
                            return k, c, None, None
                        if block == "all":
                            k, i, c = torch.unique(src, sorted=True, return_inverse=True, return_counts=True)
                            return k, c, None, i
                        k, i, c = torch.unique_consecutive(src, return_inverse=True, return_counts=True)
                        return k, c, None, i

                    fns = {"unique16": run_unique16, "widen": run_widen, "torch": run_torch}
                    sides = list(fns)
                    expect = {}
                    for s in sides[1:]:  # the comparators' results, once, as int32 (also their first warm-up)
                        try:
                            k, c, f, i = fns[s]()
                        except (RuntimeError, NotImplementedError) as err:  # this torch has no such kernel for the dtype: the side is left out
                            print(f"# {s} left out for {dtype}: {str(err).splitlines()[0]}", file=sys.stderr, flush=True)
                            continue
                        expect[s] = (k, c.to(torch.int32), None if f is None else f.to(torch.int32), None if i is None else i.to(torch.int32))
                    torch.cuda.synchronize()
                    sides = ["unique16"] + list(expect)
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
                    for part in (0, 1):  # alternate the sides: half the repetitions each, twice
                        for s in sides:
                            reps = args.torch_reps if s == "torch" else args.reps
                            half = reps // 2 if part == 0 else reps - reps // 2
                            times[s] += timed(fns[s], max(half, 1), 1, compare if s == "unique16" else (lambda out: None))
                    uq16.check()
                    uq32.check()
                    st = {s: stats(t) for s, t in times.items()}
                    m = st["unique16"]
                    flags = [f"loses_to_{s}" for s in sides[1:] if st[s]["median_ms"] < m["median_ms"]]
                    rows_out.append([block, dtype, lg, d, seen_u[-1], trio(m), trio(st.get("widen")), trio(st.get("torch")),
                                     int(all(agree.values()) and len(set(seen_u)) == 1), ",".join(flags)])
                    print(f"# {block:11s} {dtype:8s} 2^{lg} distinct {d:6d} u {seen_u[-1]:6d} unique16 {m['median_ms']:8.3f} ms [{m['min_ms']:.3f}, "
                          f"{m['max_ms']:.3f}]" + "".join(f"  {s} {st[s]['median_ms']:8.3f} x{st[s]['median_ms'] / m['median_ms']:.2f}" for s in sides[1:])
                          + f"  agree {agree} {flags}", file=sys.stderr, flush=True)
                    del src, expect
                    torch.cuda.empty_cache()
                uq16.close()
                if uq32 is not None:
                    uq32.close()
                torch.cuda.empty_cache()
    out = {"tool": "unique16_perf", "reps": args.reps, "torch_reps": args.torch_reps, "device": torch.cuda.get_device_name(0), "order": "ascending",
           "unique16": "gs_unique16_unique / _consecutive, outputs allocated inside the timed span",
           "widen": "x.to(float32 / int32) + gs_unique_keys / _positions / _consecutive + one host wait for u + narrowing of the u keys",
           "torch": "torch.unique(sorted=True, ...) on the same tensor; consecutive: torch.unique_consecutive on the sorted input",
           "columns": COLUMNS, "rows_measured": rows_out, "form_columns": FORM_COLUMNS, "form_rows_measured": form_rows}
    line = json.dumps(out, separators=(",", ":"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
