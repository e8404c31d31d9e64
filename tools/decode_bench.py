#!/usr/bin/env python3
"""Batch decode of one large batch, host form against resident form.

The batch: the ids of the GPT-4-split encode of synth_text (seed 4, --bytes) with the merges of the headline training run
(synth_text seed 2, --train-bytes, vocab 32000), built once and kept in --ids (an .npz) for the next run.

  --form host      (a) wall time of Tokenizer.decode_batch, (b) device ms of its length + scan + copy kernels (bpe_prof_read)
  --form resident  (c) wall time and device ms of decode_batch_resident into a pre-sized `out`, (d) the same for the
                   count-only call; the copy pass alone = (c) - (d), also as a share of the HBM peak in physical bytes
                   (resolved index + offset read per token, decoded bytes written), for every --copy setting
  --root DIR       import minbpe_amd from another checkout (the parent commit has only the host form: figures (a) and (b)
                   are taken there)
One JSON line per figure: every repetition's value, their minimum, median and maximum."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification


def stats(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4),
            "all": [round(x, 4) for x in xs]}


def build_batch(args, T, native):
    if args.ids and os.path.exists(args.ids):
        z = np.load(args.ids)
        return z["ids"], z["pairs"]
    eng = T.engine()
    train = native.synth_text(args.train_bytes, 2)
    eng.load_bytes(train, native.split_offsets(train, 4))
    pairs = np.array(eng.train(32000 - 256)["pairs"], dtype=np.int32)
    del train
    data = native.synth_text(args.bytes, 4)
    ids, _ = eng.encode_batch(pairs, None, data, native.split_offsets(data, 4))
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    if args.ids:
        os.makedirs(os.path.dirname(os.path.abspath(args.ids)), exist_ok=True)
        np.savez(args.ids, ids=ids, pairs=pairs)
    return ids, pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--form", choices=("host", "resident", "both"), default="both")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--ids", default=None, help=".npz holding the batch (written when missing)")
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--train-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--copy", default="1:8192:1024,0:8192:1024,1:16384:2048,1:8192:2048,1:16384:4096,1:32768:4096,1:4096:512,1:8192:1536,1:16384:1024",
                    help="dec_copy:dec_window:dec_tile settings of the resident copy pass, the first one the default")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("decode_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    ids, pairs = build_batch(args, T, native)
    tok = T.RegexTokenizer()
    tok.merges = {(int(a), int(b)): 256 + i for i, (a, b) in enumerate(pairs.tolist())}
    tok.vocab = tok._build_vocab()
    eng = T.engine()
    n = len(ids)
    say = lambda d: print(json.dumps(d), flush=True)
    say({"batch_tokens": n, "vocab": len(tok.vocab), "root": args.root, "version": native.version()})

    def device_ms(fn):
        eng.set_option("profile", 2)
        out = []
        for _ in range(args.reps):
            eng.prof_reset()
            fn()
            out.append(eng.prof_read()["decode"]["ms"])
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

    digest = None
    if args.form in ("host", "both"):
        for _ in range(args.warmup):
            raw = tok.decode_batch(ids)
        digest, total = hashlib.sha256(raw).hexdigest(), len(raw)
        say({"figure": "a", "what": "host form, wall ms", "bytes": total, **stats(wall_ms(lambda: tok.decode_batch(ids)))})
        say({"figure": "b", "what": "host form, device ms (length + scan + copy)",
             **stats(device_ms(lambda: tok.decode_batch(ids)))})
        say({"host_form_sha256": digest})
    if args.form in ("resident", "both"):
        for dt in (torch.int32, torch.int64):
            t = torch.from_numpy(ids).to("cuda").to(dt)
            width = t.element_size()
            total = tok.decode_batch_resident(t).numel()
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
            count = lambda: eng.decode_batch_resident(t.data_ptr(), width, n, 0, 0, 0, 0, 0)
            full = lambda: tok.decode_batch_resident(t, out=out)
            for _ in range(args.warmup):
                count(), full()
            d_wall, d_dev = wall_ms(count), device_ms(count)
            say({"figure": "d", "ids": str(dt), "what": "resident count-only, wall ms", **stats(d_wall)})
            say({"figure": "d", "ids": str(dt), "what": "resident count-only, device ms (length + scan)", **stats(d_dev)})
            settings = [tuple(int(x) for x in s.split(":")) for s in args.copy.split(",")]
            walls, devs, shas = {s: [] for s in settings}, {s: [] for s in settings}, {}
            reps, args.reps = args.reps, 1
            for _ in range(reps):  # the settings alternate inside every repetition
                for s in settings:
                    for name, v in zip(("dec_copy", "dec_window", "dec_tile"), s):
                        eng.set_option(name, v)
                    out.zero_()
                    full()
                    if s not in shas:  # every setting's bytes, once
                        shas[s] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
                    walls[s] += wall_ms(full)
                    devs[s] += device_ms(full)
            args.reps = reps
            for name, v in zip(("dec_copy", "dec_window", "dec_tile"), settings[0]):
                eng.set_option(name, v)
            got = shas[settings[0]]
            for s in settings:
                copy_ms = statistics.median(devs[s]) - statistics.median(d_dev)
                phys = 12 * n + total
                say({"figure": "c", "ids": str(dt), "dec_copy:window:tile": "%d:%d:%d" % s, "bytes": total,
                     "same_bytes_as_first_setting": shas[s] == got, "wall_ms": stats(walls[s]), "device_ms": stats(devs[s]), "copy_pass_ms": round(copy_ms, 4),
                     "copy_pass_physical_bytes": phys, "copy_pass_GBps": round(phys / copy_ms / 1e6, 1),
                     "copy_pass_share_of_hbm_peak": round(phys / (copy_ms * 1e-3) / HBM_PEAK, 4)})
            say({"resident_sha256": got, "ids": str(dt), "equals_host_form": None if digest is None else got == digest})


if __name__ == "__main__":
    main()
