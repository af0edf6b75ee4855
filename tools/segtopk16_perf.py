#!/usr/bin/env python3
"""The segmented top-k on 16-bit keys (gs_segtopk16_*) against what a user does without it, on one GPU; prints one JSON line.

--n bfloat16 keys (uniform 16-bit patterns, the NaN and infinity patterns moved to finite ones so that widening and narrowing keep every
bit) under the offset sets of tools/segtopk_perf.py (--shapes: fixedL, mix, RxL), as keys only and with positions (--modes keys,pos),
for every k of --ks, ascending.  A (shape, k) whose dense output would exceed --max-out elements, or whose k is above a uniform
length, is skipped and named in the JSON.  Per shape, mode and k:
  segtopk16  gs_segtopk16_select_keys / _pairs with max_segment_len = 0;
  widen      (a) x.float(), gs_segtopk_select_* on the float32 copy, and the keys narrowed back to bfloat16: twice the bytes read and an
             n-sized copy, all inside the timed span;
  sort       (b) a copy of the keys, gs_segsort16_sort_keys (positions: gs_segsort16_argsort, which makes the indices itself) on the
             copy with max_segment_len = 0, and a gather of the heads (one indexing kernel per output, its index matrix made
             beforehand); the copy is inside the timed span, because the sort writes its input and the top-k does not;
  rows       (c) uniform shapes only: gs_topk_select_rows_* with the 16-bit key type on the same buffer as a [segments, L] matrix;
  overhead   the segmented top-k on num_segments EMPTY segments of a one-element array: reset, classify, fill and a packed launch
             that finds nothing: the launches (c) does not have.
All sides alternate in one process, warmed, --reps timed repetitions each in two halves, device events around every single call,
fresh outputs (refilled) before each repetition, outside the events; median, extremes and spread per side.  The result of EVERY
repetition of (a), (b) and (c) is compared bit for bit with the segmented top-k's on the slots it writes (positions of (c) after
adding the row starts)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402
from segtopk_perf import SHAPES, shape_lengths, timed  # noqa: E402
from sort_rows_perf import stats  # noqa: E402

FILL = 0x5EED
BASELINES = ("widen", "sort", "rows")


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
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    bits = torch.randint(-(1 << 15), 1 << 15, (total,), dtype=torch.int16, device=dev, generator=gen)
    bits = torch.where((bits & 0x7F80) == 0x7F80, bits & ~0x0080, bits)  # exponent all ones (inf, NaN) -> the binade below
    src = bits.view(torch.bfloat16)
    del bits
    copy_k, copy_v = torch.empty_like(src), torch.empty(total, dtype=torch.int32, device=dev)
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
                top = g.SegmentedTopK16(n, segs, k, key_type=g.KEY_BFLOAT16, mode=mode, value_bytes=vb)
                top32 = g.SegmentedTopK(n, segs, k, key_type=g.KEY_FLOAT32, mode=mode, value_bytes=vb)
                sort = g.SegmentedSort16(n, segs, key_type=g.KEY_BFLOAT16, mode=mode, value_bytes=vb)
                rows = g.TopK(n, k, key_type=g.KEY_BFLOAT16, mode=mode, value_bytes=vb) if uniform else None
                outs = {side: (torch.empty(segs * k, dtype=torch.bfloat16, device=dev), torch.empty(segs * k, dtype=torch.int32, device=dev) if pos else None)
                        for side in ("segtopk16",) + BASELINES}
                wide_out = torch.empty(segs * k, dtype=torch.float32, device=dev)
                # the heads of the sorted copy: element j of segment s where j < its length (the other slots read element 0 and are not compared)
                col = torch.arange(k, dtype=torch.int64, device=dev)
                written = col[None, :] < d_len[:, None]
                gather = torch.where(written, d_off[:-1].to(torch.int64)[:, None] + col[None, :], torch.zeros((), dtype=torch.int64, device=dev)).reshape(-1)
                written = written.reshape(-1)
                starts = d_off[:-1].repeat_interleave(k) if pos else None

                def reset():
                    for ok, ov in outs.values():
                        ok.view(torch.int16).fill_(FILL)
                        if ov is not None:
                            ov.fill_(FILL)
                    wide_out.view(torch.int32).fill_(FILL << 16)

                def run_top(off=d_off, count=n):
                    top.select(src, off, k, outs["segtopk16"][0], None, outs["segtopk16"][1], n=count)

                def run_widen():
                    wide = src[:n].float()
                    top32.select(wide, d_off, k, wide_out, None, outs["widen"][1], n=n)
                    outs["widen"][0].copy_(wide_out)  # float32 -> bfloat16

                def run_sort():
                    copy_k[:n].copy_(src[:n])
                    if pos:
                        sort.argsort(copy_k, d_off, copy_v, n=n)
                    else:
                        sort.sort(copy_k, d_off, None, n=n)
                    torch.index_select(copy_k, 0, gather, out=outs["sort"][0])
                    if pos:
                        torch.index_select(copy_v, 0, gather, out=outs["sort"][1])

                def run_rows():
                    rows.select_rows(src, segs, int(lens[0]), int(lens[0]), k, outs["rows"][0], None, outs["rows"][1])

                def same_as_top(side):
                    def verify():
                        ok = bool(((outs[side][0].view(torch.int16) == outs["segtopk16"][0].view(torch.int16)) | ~written).all())
                        if pos:
                            theirs = outs[side][1] + starts if side == "rows" else outs[side][1]
                            ok = ok and bool(((theirs == outs["segtopk16"][1]) | ~written).all())
                        return ok
                    return verify

                reset()
                run_top()
                top.check()
                last = top.last()
                sides = {"segtopk16": (run_top, None), "widen": (run_widen, same_as_top("widen")), "sort": (run_sort, same_as_top("sort"))}
                if uniform:
                    sides["rows"] = (run_rows, same_as_top("rows"))
                times = {side: [] for side in sides}
                times["overhead"] = []
                agree = {side: True for side in sides if side != "segtopk16"}
                for half in (args.reps // 2, args.reps - args.reps // 2):  # alternate the sides: half the repetitions each, twice
                    for side, (fn, verify) in sides.items():
                        if verify is not None:  # the other side's repetition is compared with a segmented top-k result of this half
                            reset()
                            run_top()
                            keep = tuple(None if t is None else t.clone() for t in outs["segtopk16"])

                            def reset_side(keep=keep):
                                reset()
                                outs["segtopk16"][0].copy_(keep[0])
                                if pos:
                                    outs["segtopk16"][1].copy_(keep[1])
                            t, ok = timed(fn, reset_side, max(half, 1), 2, verify)
                            agree[side] = agree[side] and ok
                        else:
                            t, _ = timed(fn, reset, max(half, 1), 2, None)
                        times[side] += t
                    t, _ = timed(lambda: run_top(d_empty, 1), reset, max(half, 1), 2, None)
                    times["overhead"] += t
                top.check()
                top32.check()
                sort.check()
                if rows is not None:
                    rows.check()
                st = {side: stats(t) for side, t in times.items()}
                mine = st["segtopk16"]["median_ms"]
                row = {"shape": shape, "mode": what, "k": k, "n": n, "segments": segs, "longest": last["longest"], "class_counts": last["counts"],
                       "reads": last["reads"], "segtopk16": st["segtopk16"], "widen_and_segtopk": st["widen"], "sort16_and_gather": st["sort"],
                       "rows16": st.get("rows"), "overhead": st["overhead"],
                       "widen_over_segtopk16": st["widen"]["median_ms"] / mine, "sort_over_segtopk16": st["sort"]["median_ms"] / mine,
                       "rows_over_segtopk16": st["rows"]["median_ms"] / mine if uniform else None,
                       "loses_to_widen": bool(mine > st["widen"]["median_ms"]), "loses_to_sort": bool(mine > st["sort"]["median_ms"]),
                       # behind (c) by more than the 3 % band plus the launches (c) does not have
                       "behind_rows": bool(uniform and mine > 1.03 * st["rows"]["median_ms"] + st["overhead"]["median_ms"]),
                       "results_agree": agree}
                rows_out.append(row)
                print(f"# {shape:12s} {what:4s} k {k:5d} segs {segs:8d}  segtopk16 {mine:8.3f} ms [{st['segtopk16']['min_ms']:.3f}, "
                      f"{st['segtopk16']['max_ms']:.3f}]  widen {st['widen']['median_ms']:8.3f} x{row['widen_over_segtopk16']:.2f}  sort+gather "
                      f"{st['sort']['median_ms']:8.3f} x{row['sort_over_segtopk16']:.2f}  rows "
                      + (f"{st['rows']['median_ms']:8.3f} x{row['rows_over_segtopk16']:.2f}" if uniform else "       -") +
                      f"  overhead {st['overhead']['median_ms']:.3f}  agree {agree}", file=sys.stderr, flush=True)
                top.close()
                top32.close()
                sort.close()
                if rows is not None:
                    rows.close()
                del outs, gather, written, starts, wide_out
    out = {"tool": "segtopk16_perf", "n": args.n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "key_type": "bfloat16", "ks": args.ks,
           "baseline_a": "x.float() + gs_segtopk_select_* (float32, max_segment_len = 0) + the keys narrowed to bfloat16, all inside the timed span",
           "baseline_b": "copy + gs_segsort16_sort_keys / _argsort (max_segment_len = 0) + a gather of the heads, copy inside the timed span",
           "baseline_c": "gs_topk_select_rows_* with GS_KEY_BFLOAT16 on the same buffer as a matrix (uniform shapes)",
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
