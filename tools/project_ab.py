#!/usr/bin/env python3
"""Projection of one large batch onto smaller vocabularies: bpe_project_resident against what the API allowed before
(DESIGN 4.6).

The batch is tools/decode_bench.py's: the ids of the GPT-4-split encode of synth_text (seed 4, --bytes) with the merges of
the headline training run (synth_text seed 2, --train-bytes, vocab 32000), kept in --ids (an .npz) for the next run.
For every vocab_size of --sizes:

  project   Engine.project_resident into a pre-sized buffer, and the count-only call
  (a)       the composition: decode_batch_resident with a vocab table whose entries are the expansions as little-endian
            int32 bytes, the result viewed as int32 -- timed twice, before and after `project`, so that its own
            run-to-run spread is known
  (b)       encoding the text again with the truncated merge list: device ms of encode_batch_resident, and wall ms of
            host split + upload + call
Device ms are the library's hipEvents around its kernels (bpe_prof_read, option profile = 2); warm-up first, medians of
--reps.  The three results are compared element for element before anything is timed.  One JSON line per figure; the
verdict line says whether `project` beats (a) by more than (a)'s spread (its two runs' medians apart, or the interquartile
range of all its repetitions, whichever is larger), and gives the fraction of the HBM peak in
algorithmic bytes, id_width x (n + n_out).  --geometry times `project` under other tile and window sizes as well."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import HBM_PEAK, build_batch, stats  # noqa: E402


def expansion_table(pairs, vs):
    """entry t of [0, 256 + M): E(t) at vocab_size vs, as int32 arrays"""
    table = [np.array([t], dtype=np.int32) for t in range(vs)]
    for t in range(vs, 256 + len(pairs)):
        a, b = pairs[t - 256]
        table.append(np.concatenate([table[a], table[b]]))
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--ids", default=None, help=".npz holding the batch (written when missing)")
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--train-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--sizes", default="256,4096,16384,31999")
    ap.add_argument("--geometry", default="", help="proj_tile:proj_window settings to time `project` under besides the "
                    "defaults 256:2048, comma separated")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("project_ab: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    ids, pairs = build_batch(args, T, native)
    eng = T.engine()
    n, M = len(ids), len(pairs)
    plist = pairs.tolist()
    say = lambda d: print(json.dumps(d), flush=True)
    say({"batch_tokens": n, "merges": M, "version": native.version()})
    d_ids = torch.from_numpy(ids).to("cuda")
    data = native.synth_text(args.bytes, 4)
    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
    eng.project_set_merges(pairs)

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

    def wall_ms(fn, reps=None):
        out = []
        for _ in range(reps or args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    for vs in (int(s) for s in args.sizes.split(",")):
        n_out = eng.project_resident(d_ids.data_ptr(), 4, n, vs)
        out = torch.empty(n_out, dtype=torch.int32, device="cuda")
        project = lambda: eng.project_resident(d_ids.data_ptr(), 4, n, vs, 0, 0, out.data_ptr(), n_out)
        count = lambda: eng.project_resident(d_ids.data_ptr(), 4, n, vs)
        project()
        # (a) the composition through decode
        table = expansion_table(plist, vs)
        offs = np.zeros(len(table) + 1, np.uint64)
        np.cumsum([4 * len(t) for t in table], out=offs[1:])
        blob = np.concatenate(table).astype("<i4").tobytes()
        out_a = torch.empty(4 * n_out, dtype=torch.uint8, device="cuda")

        def set_table():
            eng.decode_set_vocab(blob, offs)
            eng.decode_set_sparse(np.empty(0, np.int32), len(table))
            eng._decode_owner = (None, False)

        compose = lambda: eng.decode_batch_resident(d_ids.data_ptr(), 4, n, 0, 0, out_a.data_ptr(), 4 * n_out, 0)
        set_table()
        assert compose() == 4 * n_out
        same_a = torch.equal(out_a.view(torch.int32), out)
        # (b) encoding again
        offs_b = native.split_offsets(data, 4)
        d_offs = torch.from_numpy(np.asarray(offs_b).astype(np.int64)).to("cuda")
        d_enc = torch.empty(len(data), dtype=torch.int32, device="cuda")
        d_ooff = torch.empty(len(offs_b) + 1, dtype=torch.int64, device="cuda")
        tp = np.ascontiguousarray(pairs[:vs - 256])
        encode = lambda: eng.encode_batch_resident(tp, None, d_bytes.data_ptr(), len(data), d_offs.data_ptr(), len(offs_b),
                                                   d_enc.data_ptr(), d_ooff.data_ptr())

        def encode_wall():
            o = native.split_offsets(data, 4)
            b = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
            f = torch.from_numpy(np.asarray(o).astype(np.int64)).to("cuda")
            torch.cuda.synchronize()
            return eng.encode_batch_resident(tp, None, b.data_ptr(), len(data), f.data_ptr(), len(o), d_enc.data_ptr(),
                                             d_ooff.data_ptr())

        try:
            same_b = encode() == n_out and torch.equal(d_enc[:n_out], out)
            b_dev, b_wall = device_ms(encode, "encode"), wall_ms(encode_wall, 5)
        except Exception as e:  # (the lines of the other figures must still come out)
            same_b, b_dev, b_wall = f"failed: {type(e).__name__}: {e}", None, None
        a1 = device_ms(compose)
        p_dev, p_wall = device_ms(project), wall_ms(project)
        c_dev = device_ms(count)
        a2 = device_ms(compose)
        a_wall = wall_ms(compose)
        med = statistics.median
        q = statistics.quantiles(a1 + a2, n=4)
        spread = max(abs(med(a1) - med(a2)), q[2] - q[0])  # the two runs' medians apart, or the interquartile range of all
        alg = 4 * (n + n_out)
        say({"figure": "project", "vocab_size": vs, "n_out": n_out, "equals_a": same_a, "equals_b": same_b,
             "device_ms": stats(p_dev), "wall_ms": stats(p_wall), "count_only_device_ms": stats(c_dev)})
        say({"figure": "a_decode_composition", "vocab_size": vs, "device_ms_before": stats(a1), "device_ms_after": stats(a2),
             "wall_ms": stats(a_wall)})
        if b_dev is not None:
            say({"figure": "b_encode_again", "vocab_size": vs, "device_ms": stats(b_dev), "wall_ms_with_split_and_upload": stats(b_wall)})
        say({"figure": "verdict", "vocab_size": vs, "a_over_project_device": round(med(a1 + a2) / med(p_dev), 3),
             "margin_ms": round(med(a1 + a2) - med(p_dev), 4), "a_spread_ms": round(spread, 4),
             "a_range_ms": round(max(a1 + a2) - min(a1 + a2), 4),
             "faster_than_a_beyond_its_spread": bool(med(a1 + a2) - med(p_dev) > spread),
             "algorithmic_bytes": alg, "GBps_device": round(alg / med(p_dev) / 1e6, 1),
             "of_hbm_peak": round(alg / (med(p_dev) * 1e-3) / HBM_PEAK, 4)})
        for g in filter(None, args.geometry.split(",")):
            tile, window = (int(x) for x in g.split(":"))
            eng.set_option("proj_tile", tile)
            eng.set_option("proj_window", window)
            out.zero_()
            project()
            say({"figure": "project_geometry", "vocab_size": vs, "proj_tile": tile, "proj_window": window,
                 "equals_a": torch.equal(out_a.view(torch.int32), out), "device_ms": stats(device_ms(project))})
            eng.set_option("proj_tile", 256)
            eng.set_option("proj_window", 2048)
        del out, out_a, d_offs, d_enc, d_ooff


if __name__ == "__main__":
    main()
