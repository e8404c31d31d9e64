#!/usr/bin/env python3
"""The id histogram of one large batch and the compression curve from it: bpe_count_resident and bpe_count_fold against
what the API allowed before.

The batch is tools/project_ab.py's: the ids of the GPT-4-split encode of synth_text (seed 4, --bytes) with the merges of
the headline training run (synth_text seed 2, --train-bytes, vocab 32000), kept in --ids (an .npz) for the next run.
Everything is measured in one run:

  (a)  Engine.count_resident into a resident array: device ms of the library's hipEvents around its kernels
       (bpe_prof_read, option profile = 2), and wall ms of the whole call
  (b)  torch.bincount(ids, minlength=256 + M) on the same tensor, by CUDA events -- timed twice, before and after (a), so
       that its own run-to-run spread is known
  (c)  the whole curve from one count plus bpe_count_fold (device ms + host ms, the read-back of the counts included)
       against projected_count -- the count-only projection -- at the sizes of --sizes; the cost of all M + 1 points by
       that route is their sum times (M + 1) / len(sizes): an EXTRAPOLATION, said so in the line
  (d)  (a) under count_lds_bins of --lds, each with count_combine 1 and 0
  (e)  the share of the batch's ids below each of those L, from the histogram itself
  (f)  (a) on the first n / 8, n / 4, n / 2 and n ids and the line through the four: its constant is what a call costs
       whatever n is (clearing the scratch, the launches, the flush of every workgroup's table)
Warm-up first, medians of --reps.  Every result -- each setting of (d), both id widths -- is compared element for element
with np.bincount on the host and with (b) before anything is timed.  One JSON line per figure; the verdict line says
whether (a) beats (b) by more than the full range of (b)'s repetitions, and gives 4 n bytes / time against the HBM peak
and against the 0.71 of it the project measures for a plain stream read."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import HBM_PEAK, build_batch, stats  # noqa: E402

STREAM_READ = 0.71  # of the peak: what a plain read of a resident stream reaches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--ids", default=None, help=".npz holding the batch (written when missing)")
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--train-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--sizes", default="256,4096,16384,31999")
    ap.add_argument("--lds", default="4096,8192,16384,32768")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("count_ab: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    ids, pairs = build_batch(args, T, native)
    eng = T.engine()
    n, M = len(ids), len(pairs)
    top = 256 + M
    med = statistics.median
    say = lambda d: print(json.dumps(d), flush=True)
    say({"batch_tokens": n, "merges": M, "version": native.version()})
    d_ids = torch.from_numpy(ids).to("cuda")
    d_wide = d_ids.to(torch.int64)
    eng.project_set_merges(pairs)
    counts = torch.empty(top, dtype=torch.int64, device="cuda")
    lds_settings = [int(s) for s in args.lds.split(",")]

    def set_form(lds, combine):
        eng.set_option("count_lds_bins", lds)
        eng.set_option("count_combine", combine)

    def device_ms(fn, kind="decode"):
        for _ in range(args.warmup):
            fn()
        eng.set_option("profile", 2)
        out = []
        for _ in range(args.reps):
            eng.prof_reset()
            fn()
            out.append(eng.prof_read()[kind]["ms"])
        eng.set_option("profile", 0)
        return out

    def wall_ms(fn):
        out = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def event_ms(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    count = lambda: eng.count_resident(d_ids.data_ptr(), 4, n, counts.data_ptr(), top)
    count_wide = lambda: eng.count_resident(d_wide.data_ptr(), 8, n, counts.data_ptr(), top)
    bincount = lambda: torch.bincount(d_ids, minlength=top)

    # ---- everything equal, element for element, before anything is timed
    want = np.bincount(ids, minlength=top).astype(np.int64)
    same = {"torch_bincount": bool(np.array_equal(bincount().cpu().numpy(), want))}
    for lds in lds_settings:
        for combine in (1, 0):
            set_form(lds, combine)
            for name, fn in (("int32", count), ("int64", count_wide)):
                counts.fill_(-1)
                fn()
                same[f"lds{lds}_combine{combine}_{name}"] = bool(np.array_equal(counts.cpu().numpy(), want))
    say({"figure": "equal_to_np_bincount", **same, "all": all(same.values())})
    if not all(same.values()):
        sys.exit("count_ab: results differ, nothing timed")

    # ---- (e) the share of ids below each L
    below = np.cumsum(want)
    say({"figure": "e_share_below_L", **{str(L): round(float(below[min(L, top) - 1]) / n, 6) for L in (256, 1024, 2048, *lds_settings)},
         "distinct_ids": int(np.count_nonzero(want)), "largest_bin": int(want.max()), "largest_bin_id": int(want.argmax())})

    # ---- (d) settings, then the default by the fastest
    grid = {}
    for lds in lds_settings:
        for combine in (1, 0):
            set_form(lds, combine)
            grid[(lds, combine)] = device_ms(count)
            say({"figure": "d_setting", "count_lds_bins": lds, "count_combine": combine, "device_ms": stats(grid[(lds, combine)])})
    best = min(grid, key=lambda k: med(grid[k]))
    say({"figure": "d_fastest", "count_lds_bins": best[0], "count_combine": best[1], "device_ms": round(med(grid[best]), 4)})
    set_form(*best)

    # ---- (b) before, (a), (b) after
    b1 = event_ms(bincount)
    a_dev, a_wall = device_ms(count), wall_ms(count)
    a_wide = device_ms(count_wide)
    b2 = event_ms(bincount)
    b = b1 + b2
    say({"figure": "a_count_resident", "count_lds_bins": best[0], "count_combine": best[1], "device_ms": stats(a_dev),
         "wall_ms": stats(a_wall), "int64_device_ms": stats(a_wide)})
    say({"figure": "b_torch_bincount", "event_ms_before": stats(b1), "event_ms_after": stats(b2)})
    margin, b_range = med(b) - med(a_dev), max(b) - min(b)
    say({"figure": "verdict", "b_over_a": round(med(b) / med(a_dev), 3), "margin_ms": round(margin, 4),
         "b_range_ms": round(b_range, 4), "faster_than_b_beyond_its_range": bool(margin > b_range),
         "algorithmic_bytes": 4 * n, "GBps_device": round(4 * n / med(a_dev) / 1e6, 1),
         "of_hbm_peak": round(4 * n / (med(a_dev) * 1e-3) / HBM_PEAK, 4),
         "of_stream_read": round(4 * n / (med(a_dev) * 1e-3) / (STREAM_READ * HBM_PEAK), 4)})

    # ---- (f) what does not depend on n: prefixes of the batch, and the line through them
    fracs = (8, 4, 2, 1)
    prefix = {n // f: med(device_ms(lambda m=n // f: eng.count_resident(d_ids.data_ptr(), 4, m, counts.data_ptr(), top)))
              for f in fracs}
    slope, fixed = np.polyfit(np.array(list(prefix), dtype=np.float64), np.array(list(prefix.values())), 1)
    say({"figure": "f_prefixes", "device_ms_by_n": {str(m): round(t, 4) for m, t in prefix.items()},
         "fit_fixed_ms": round(float(fixed), 4), "fit_ms_per_million_ids": round(float(slope) * 1e6, 5),
         "fit_GBps_of_the_slope": round(4 / float(slope) / 1e6, 1)})

    # ---- (c) the curve: one count + the fold, against count-only projections
    sizes = [int(s) for s in args.sizes.split(",")]
    fold = lambda: native.count_fold(pairs, counts.cpu().numpy(), None, want_curve=True)[1]
    count()
    curve = fold()
    points, point_ms = {}, {}
    for vs in sizes:
        project = lambda: eng.project_resident(d_ids.data_ptr(), 4, n, vs)
        points[vs] = project()
        point_ms[vs] = device_ms(project)
    fold_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fold()
        fold_ms.append((time.perf_counter() - t0) * 1e3)
    four = sum(med(point_ms[vs]) for vs in sizes)
    say({"figure": "c_curve", "curve_equals_projected_count": {str(vs): bool(curve[vs - 256] == points[vs]) for vs in sizes},
         "tokens_at": {str(vs): int(curve[vs - 256]) for vs in sizes}, "fold_host_ms_with_read_back": stats(fold_ms),
         "count_plus_fold_ms": round(med(a_dev) + med(fold_ms), 4),
         "projected_count_device_ms": {str(vs): round(med(point_ms[vs]), 4) for vs in sizes},
         "all_points_by_projected_count_ms_EXTRAPOLATED": round(four * (M + 1) / len(sizes), 1),
         "extrapolation": f"sum of the {len(sizes)} measured sizes x (M + 1) / {len(sizes)}"})


if __name__ == "__main__":
    main()
