#!/usr/bin/env python3
"""The segmented top-k (gs_segtopk_*) against what a user does without it, on one GPU; prints one JSON line.

--n uint32 keys under a list of offset sets (--shapes):
  fixedL     uniform segments of L elements (16, 256, 2048, 16384, 131072), as many as n holds;
  mix        the heavy-tailed mix of tools/segsort16_perf.py (the one tools/segsort_long_perf.py measures): about two million segments,
             a few hundred of them long;
  RxL        R segments of L elements (32x4194304: few huge segments, one workgroup each).
Each as keys only and with positions (--modes keys,pos), for every k of --ks.  A (shape, k) whose dense output num_segments x k would
exceed --max-out elements is skipped and named in the JSON (fixed16 at k = 64 would write 4 x the input).  Per shape, mode and k:
  segtopk    gs_segtopk_select_keys / _pairs with max_segment_len = 0;
  sort       (a) what a user does today: a copy of the keys (and, for positions, of an index array), gs_segsort_sort_keys / _sort_pairs on
             the copy with max_segment_len = 0 on the device long route, and a gather of the heads (one indexing kernel per output, its
             index matrix made beforehand); the copy is inside the timed span, because the segmented sort writes its input and the
             top-k does not;
  rows       (b) uniform shapes only: gs_topk_select_rows_* on the same buffer as a [segments, L] matrix;
  overhead   the segmented top-k on num_segments EMPTY segments of a one-element array: reset, classify, fill and a packed launch
             that finds nothing (no other kernel is launched for one element): the launches (b) does not have.
All sides alternate in one process, warmed, --reps timed repetitions each in two halves, device events around every single call,
fresh outputs (refilled) before each repetition, outside the events; median, extremes and spread per side.  The result of EVERY
repetition of (a) and (b) is compared bit for bit with the segmented top-k's on the slots it writes (positions of (b) after adding
the row starts)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from segsort16_perf import lengths  # noqa: E402
from sort_rows_perf import stats  # noqa: E402

SHAPES = ("fixed16", "fixed256", "fixed2048", "fixed16384", "fixed131072", "mix", "32x4194304")
FILL = 0x5EEDBEEF


def shape_lengths(shape: str, n: int) -> np.ndarray:
    if shape.startswith("fixed"):
        length = int(shape[5:])
        return np.full(n // length, length, dtype=np.int64)
    return lengths(shape, n, 32768)


def timed(fn, reset, reps, warm, verify):
    times, same = [], True
    for i in range(warm + reps):
        reset()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if i >= warm:
            times.append(s.elapsed_time(e))
        if verify is not None:
            same = same and verify()
    return times, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--modes", default="keys,pos")
    ap.add_argument("--ks", default="8,64,1024")
    ap.add_argument("--max-out", type=int, default=1 << 28, help="skip a (shape, k) whose dense output has more elements")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    total = args.n
    src = torch.empty(total, dtype=torch.int32, device=dev)
    g.init_random(src, 12345, g.ENTROPY_PRESET_1)
    index = torch.arange(total, dtype=torch.int32, device=dev)
    copy_k, copy_v = torch.empty_like(src), torch.empty_like(src)
    rows_out, skipped = [], []
    for shape in args.shapes.split(","):
        lens = shape_lengths(shape, total)
        offsets = np.concatenate(([0], np.cumsum(lens)))
        n, segs = int(offsets[-1]), int(lens.size)
        uniform = bool((lens == lens[0]).all())
        d_off = torch.from_numpy(offsets.astype(np.int32)).to(dev)
        d_empty = torch.zeros(segs + 1, dtype=torch.int32, device=dev)
        d_len = torch.from_numpy(lens).to(dev)
        for what in args.modes.split(","):
            pos = what == "pos"
            mode, vb = (g.MODE_PAIRS, 4) if pos else (g.MODE_KEYS_ONLY, 0)
            for k in (int(x) for x in args.ks.split(",")):
                if segs * k > args.max_out or (uniform and k > int(lens[0])):
                    skipped.append({"shape": shape, "mode": what, "k": k, "segments": segs, "output_elements": segs * k,
                                    "why": "k above the segment length" if segs * k <= args.max_out else "dense output above --max-out"})
                    continue
                top = g.SegmentedTopK(n, segs, k, key_type=g.KEY_UINT32, mode=mode, value_bytes=vb)
                sort = g.SegmentedSort(n, segs, key_type=g.KEY_UINT32, mode=mode, value_bytes=vb, long_route="device")
                rows = g.TopK(n, k, key_type=g.KEY_UINT32, mode=mode, value_bytes=vb) if uniform else None
                outs = {side: (torch.empty(segs * k, dtype=torch.int32, device=dev), torch.empty(segs * k, dtype=torch.int32, device=dev) if pos else None)
                        for side in ("segtopk", "sort", "rows")}
                # the heads of the sorted copy: element j of segment s where j < its length (the other slots read element 0 and are not compared)
                col = torch.arange(k, dtype=torch.int64, device=dev)
                written = col[None, :] < d_len[:, None]
                gather = torch.where(written, d_off[:-1].to(torch.int64)[:, None] + col[None, :], torch.zeros((), dtype=torch.int64, device=dev)).reshape(-1)
                written = written.reshape(-1)
                starts = d_off[:-1].repeat_interleave(k) if pos else None

                def reset():
                    for ok, ov in outs.values():
                        ok.fill_(FILL)
                        if ov is not None:
                            ov.fill_(FILL)

                def run_top(off=d_off, count=n):
                    top.select(src, off, k, outs["segtopk"][0], None, outs["segtopk"][1], n=count)

                def run_sort():
                    copy_k[:n].copy_(src[:n])
                    if pos:
                        copy_v[:n].copy_(index[:n])
                    sort.sort(copy_k, d_off, copy_v if pos else None, n=n)
                    torch.index_select(copy_k, 0, gather, out=outs["sort"][0])
                    if pos:
                        torch.index_select(copy_v, 0, gather, out=outs["sort"][1])

                def run_rows():
                    rows.select_rows(src, segs, int(lens[0]), int(lens[0]), k, outs["rows"][0], None, outs["rows"][1])

                def same_as_top(side):
                    def verify():
                        ok = bool(((outs[side][0] == outs["segtopk"][0]) | ~written).all())
                        if pos:
                            theirs = outs[side][1] + starts if side == "rows" else outs[side][1]
                            ok = ok and bool(((theirs == outs["segtopk"][1]) | ~written).all())
                        return ok
                    return verify

                reset()
                run_top()
                top.check()
                last = top.last()
                sides = {"segtopk": (run_top, None), "sort": (run_sort, same_as_top("sort"))}
                if uniform:
                    sides["rows"] = (run_rows, same_as_top("rows"))
                times = {side: [] for side in sides}
                times["overhead"] = []
                agree = True
                for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                    for side, (fn, verify) in sides.items():
                        if verify is not None:  # the other side's repetition is compared with a segmented top-k result of this half
                            reset()
                            run_top()
                            keep = tuple(None if t is None else t.clone() for t in outs["segtopk"])

                            def reset_side(keep=keep):
                                reset()
                                outs["segtopk"][0].copy_(keep[0])
                                if pos:
                                    outs["segtopk"][1].copy_(keep[1])
                            t, ok = timed(fn, reset_side, max(half, 1), 2, verify)
                        else:
                            t, ok = timed(fn, reset, max(half, 1), 2, None)
                        times[side] += t
                        agree = agree and ok
                    t, _ = timed(lambda: run_top(d_empty, 1), reset, max(half, 1), 2, None)
                    times["overhead"] += t
                top.check()
                sort.check()
                if rows is not None:
                    rows.check()
                st = {side: stats(t) for side, t in times.items()}
                row = {"shape": shape, "mode": what, "k": k, "n": n, "segments": segs, "longest": last["longest"], "class_counts": last["counts"],
                       "reads": last["reads"], "segtopk": st["segtopk"], "sort_and_gather": st["sort"], "rows": st.get("rows"),
                       "overhead": st["overhead"], "sort_over_segtopk": st["sort"]["median_ms"] / st["segtopk"]["median_ms"],
                       "rows_over_segtopk": st["rows"]["median_ms"] / st["segtopk"]["median_ms"] if uniform else None,
                       # behind (b) by more than the 3 % band plus the launches (b) does not have
                       "behind_rows": bool(uniform and st["segtopk"]["median_ms"] > 1.03 * st["rows"]["median_ms"] + st["overhead"]["median_ms"]),
                       "loses_to_sort": bool(st["segtopk"]["median_ms"] > st["sort"]["median_ms"]), "results_agree": bool(agree)}
                rows_out.append(row)
                print(f"# {shape:12s} {what:4s} k {k:5d} segs {segs:8d}  segtopk {st['segtopk']['median_ms']:9.3f} ms [{st['segtopk']['min_ms']:.3f}, "
                      f"{st['segtopk']['max_ms']:.3f}]  sort+gather {st['sort']['median_ms']:9.3f} ms x{row['sort_over_segtopk']:.2f}  rows "
                      + (f"{st['rows']['median_ms']:9.3f} ms x{row['rows_over_segtopk']:.2f}" if uniform else "        -") +
                      f"  overhead {st['overhead']['median_ms']:.3f} ms  agree {agree}", file=sys.stderr, flush=True)
                top.close()
                sort.close()
                if rows is not None:
                    rows.close()
                del outs, gather, written, starts
    out = {"tool": "segtopk_perf", "n": args.n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "key_type": "uint32", "ks": args.ks,
           "baseline_a": "copy + gs_segsort_sort_keys / _sort_pairs (max_segment_len = 0, device long route) + a gather of the heads, copy inside the timed span",
           "baseline_b": "gs_topk_select_rows_* on the same buffer as a matrix (uniform shapes)",
           "overhead": "the segmented top-k on as many EMPTY segments of a one-element array: reset, classify, fill and a packed launch that finds nothing",
           "rows": rows_out, "skipped": skipped}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
