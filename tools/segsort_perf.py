#!/usr/bin/env python3
"""Segmented sort against the composite-key baseline, on one GPU; prints one JSON line.

At a total of 2^27 uint32 elements (--log2 N), keys-only and (u32, u32) pairs: random segment lengths uniform in [0, max] for
max = 32, 256, 2048, 8192 and the LDS limit, plus fixed lengths 16 and 1024.  Per row:
  segsort   gs_segsort_sort_* with a fitting max_segment_len (no host wait);
  baseline  what a user had before: the same data as GS_KEY_UINT64 keys (segment index << 32) | key through gs_onesweep_sort_keys /
            _sort_pairs at the library's defaults, the sort only (packing and unpacking are not charged to it).  The 64-bit path is
            the same code in this build as before the segmented sort existed, so it is run from the same library.
The two alternate in one process, both warmed, --reps timed repetitions each (device events around every single call, fresh input
copied in before it, outside the events); median and spread (max - min over min) per row; GB/s = 2 x element bytes x n over the
median, next to the box's copy rate (a device-to-device copy of the same bytes, timed the same way).  The long-segment route (three
segments of 2^25, max_segment_len = 0, one host wait) is timed and recorded with no requirement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpusorting_amd as g  # noqa: E402


def timed(fn, reset, reps, warm=3):
    times = []
    for i in range(warm + reps):
        reset()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if i >= warm:
            times.append(s.elapsed_time(e))
    return times


def stats(times):
    t = np.asarray(times)
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "spread": float((t.max() - t.min()) / t.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--check", action="store_true", help="compare every row's result with the baseline's unpacked result")
    args = ap.parse_args()
    total = 1 << args.log2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(1)
    src = torch.empty(total, dtype=torch.int32, device=dev)
    g.init_random(src, 12345, g.ENTROPY_PRESET_1)
    idx = torch.arange(total, dtype=torch.int32, device=dev)
    keys, vals = torch.empty_like(src), torch.empty_like(src)
    k64, k64_src, a64 = (torch.empty(total, dtype=torch.int64, device=dev) for _ in range(3))
    avals = torch.empty_like(src)
    copy_dst = torch.empty(total, dtype=torch.int64, device=dev)
    rows = []
    for vb in (0, 4):
        mode = g.MODE_PAIRS if vb else g.MODE_KEYS_ONLY
        limit = {0: 32768, 4: 16384}[vb]
        base = g.OneSweep(total, key_type=g.KEY_UINT64, mode=mode, value_bytes=vb)
        for name, max_len in (("random max 32", 32), ("random max 256", 256), ("random max 2048", 2048), ("random max 8192", 8192),
                              (f"random max {limit} (LDS limit)", limit), ("fixed 16", -16), ("fixed 1024", -1024), ("long 3 x 2^25", 0)):
            if max_len > 0:
                lengths = rng.integers(0, max_len + 1, size=2 * total // max_len + 64)
                lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), total))]
            elif max_len < 0:
                lengths = np.full(total // -max_len, -max_len)
            else:
                lengths = np.full(3, total // 4)
            offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
            n, num_segments = int(offsets[-1]), offsets.size - 1
            d_off = torch.from_numpy(offsets.view(np.int32)).to(dev)
            seg = g.SegmentedSort(n, num_segments, mode=mode, value_bytes=vb)
            seg_id = torch.repeat_interleave(torch.arange(num_segments, dtype=torch.int64, device=dev), torch.from_numpy(lengths).to(dev))
            k64_src[:n] = (seg_id << 32) | (src[:n].to(torch.int64) & 0xFFFFFFFF)
            del seg_id
            promise = abs(max_len)

            def reset_seg():
                keys[:n].copy_(src[:n])
                if vb:
                    vals[:n].copy_(idx[:n])

            def reset_base():
                k64[:n].copy_(k64_src[:n])
                if vb:
                    vals[:n].copy_(idx[:n])

            run_seg = lambda: seg.sort(keys, d_off, vals if vb else None, n=n, max_segment_len=promise)  # noqa: E731
            run_base = lambda: base.sort(k64, vals if vb else None, n=n, alt_keys=a64, alt_values=avals if vb else None)  # noqa: E731
            run_copy = lambda: copy_dst.view(torch.int32)[:n * (4 + vb) // 4].copy_(k64_src.view(torch.int32)[:n * (4 + vb) // 4])  # noqa: E731
            t_seg, t_base = [], []
            for r in range(2):  # alternate the two: half the repetitions each, twice
                t_seg += timed(run_seg, reset_seg, args.reps // 2)
                t_base += timed(run_base, reset_base, args.reps // 2)
            seg.check()
            base.check()
            t_copy = timed(run_copy, lambda: None, args.reps)
            ok = None
            if args.check:
                reset_seg()
                run_seg()
                reset_base()
                base.sort(k64, None if not vb else vals.clone(), n=n, alt_keys=a64, alt_values=avals if vb else None)
                ok = bool(torch.equal(keys[:n], (k64[:n] & 0xFFFFFFFF).to(torch.int32)))
            s_seg, s_base, s_copy = stats(t_seg), stats(t_base), stats(t_copy)
            byts = 2 * (4 + vb) * n
            row = {"row": name, "value_bytes": vb, "n": n, "num_segments": num_segments, "classes": seg.last_classes()["counts"],
                   "segsort": s_seg, "baseline_u64": s_base, "speedup": s_base["median_ms"] / s_seg["median_ms"],
                   "faster_by_more_than_spread": bool(s_seg["max_ms"] < s_base["min_ms"]) if max_len else None,
                   "segsort_gbps": byts / s_seg["median_ms"] / 1e6, "copy_gbps": byts / s_copy["median_ms"] / 1e6, "matches_baseline": ok}
            rows.append(row)
            print(f"# vb={vb} {name:32s} segsort {s_seg['median_ms']:8.3f} ms (spread {s_seg['spread']:.3f})  baseline {s_base['median_ms']:8.3f} ms "
                  f"(spread {s_base['spread']:.3f})  x{row['speedup']:.2f}  {row['segsort_gbps']:.0f} GB/s of {row['copy_gbps']:.0f}", file=sys.stderr, flush=True)
            seg.close()
        base.close()
    out = {"tool": "segsort_perf", "log2_total": args.log2, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "baseline": "GS_KEY_UINT64 composite keys through gs_onesweep_sort_*, same library (the 64-bit path is unchanged)", "rows": rows}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
