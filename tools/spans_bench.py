#!/usr/bin/env python3
"""Token spans of one large batch: Tokenizer.token_spans_resident against the same result composed in torch.

The batch is tools/decode_bench.py's: the ids of the GPT-4-split encode of synth_text (seed 4, --bytes) with the merges of
the headline training run (synth_text seed 2, --train-bytes, vocab 32000), kept in --ids (an .npz) for the next run; --docs
documents of random lengths cover it.

  spans     unit="both", unit="byte" and unit="both" without documents: wall ms of the call (ends in a synchronise) and
            device ms of its kernels (bpe_prof_read), for int32 and int64 ids
  torch     what a user would write today on the same device tensors: gather of a length / lead / cont table by id, two
            cumsums, searchsorted for the document, gather of the bases, subtract, stack -- wall ms and device ms (events)
There is no parent-commit form of this call: the composition is what the numbers are set against.  The two results are
compared element for element before anything is timed.  One JSON line per figure: every repetition, minimum, median and
maximum; the ratio and the achieved bytes/s (id read + 32 B of spans written per token, over device time) at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import build_batch, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--ids", default=None, help=".npz holding the batch (written when missing)")
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--train-bytes", type=int, default=1_000_000_000)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("spans_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    ids, pairs = build_batch(args, T, native)
    tok = T.RegexTokenizer()
    tok.merges = {(int(a), int(b)): 256 + i for i, (a, b) in enumerate(pairs.tolist())}
    tok.vocab = tok._build_vocab()
    eng = T.engine()
    n = len(ids)
    rng = np.random.default_rng(5)
    doff = np.concatenate([[0], np.sort(rng.integers(0, n + 1, args.docs - 1)), [n]]).astype(np.int64)
    say = lambda d: print(json.dumps(d), flush=True)
    say({"batch_tokens": n, "docs": len(doff) - 1, "vocab": len(tok.vocab), "version": native.version()})

    V = len(tok.vocab)
    lens = np.array([len(tok.vocab[i]) for i in range(V)], dtype=np.int64)
    leads = np.array([sum((b & 0xC0) != 0x80 for b in tok.vocab[i]) for i in range(V)], dtype=np.int64)
    cont = np.array([1 if (tok.vocab[i][0] & 0xC0) == 0x80 else 0 for i in range(V)], dtype=np.int64)
    len_t, lead_t, cont_t = (torch.from_numpy(a).to("cuda") for a in (lens, leads, cont))
    d_doff = torch.from_numpy(doff).to("cuda")
    pos = torch.arange(n, device="cuda")

    def torch_form(t, with_docs=True, chars=True):
        idx = t.long()
        L = len_t[idx]
        B = torch.cumsum(L, 0) - L
        if with_docs:
            d = torch.searchsorted(d_doff, pos, right=True) - 1
            start = d_doff[d]               # (every token lies in a document: off[0] = 0, off[n_docs] = n)
            B = B - B[start]
        bs = torch.stack((B, B + L), dim=1)
        if not chars:
            return bs
        K = lead_t[idx]
        C = torch.cumsum(K, 0) - K
        if with_docs:
            C = C - C[start]
        return bs, torch.stack(((C - cont_t[idx]).clamp_(min=0), C + K), dim=1)

    def wall_ms(fn):
        out = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def prof_ms(fn):
        eng.set_option("profile", 2)
        out = []
        for _ in range(args.reps):
            eng.prof_reset()
            fn()
            out.append(eng.prof_read()["decode"]["ms"])
        eng.set_option("profile", 0)
        return out

    def event_ms(fn):
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

    for dt in (torch.int32, torch.int64):
        t = torch.from_numpy(ids).to("cuda").to(dt)
        cases = {
            "both": (lambda: tok.token_spans_resident(t, d_doff, unit="both"), lambda: torch_form(t)),
            "byte": (lambda: tok.token_spans_resident(t, d_doff, unit="byte"), lambda: torch_form(t, chars=False)),
            "both_no_docs": (lambda: tok.token_spans_resident(t, unit="both"), lambda: torch_form(t, with_docs=False)),
        }
        for name, (ours, theirs) in cases.items():
            a, b = ours(), theirs()
            same = torch.equal(a, b) if name == "byte" else (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
            del a, b
            for _ in range(args.warmup):
                ours(), theirs()
            w_ours, w_torch = [], []
            reps, args.reps = args.reps, 1
            for _ in range(reps):  # the two alternate inside every repetition
                w_ours += wall_ms(ours)
                w_torch += wall_ms(theirs)
            args.reps = reps
            d_ours, d_torch = prof_ms(ours), event_ms(theirs)
            width = t.element_size()
            phys = n * (width + (16 if name == "byte" else 32))
            say({"figure": "spans", "unit": name, "ids": str(dt), "equals_torch_form": same, "wall_ms": stats(w_ours),
                 "device_ms": stats(d_ours)})
            say({"figure": "torch", "unit": name, "ids": str(dt), "wall_ms": stats(w_torch), "device_ms": stats(d_torch)})
            say({"figure": "ratio", "unit": name, "ids": str(dt),
                 "torch_over_spans_wall": round(statistics.median(w_torch) / statistics.median(w_ours), 2),
                 "torch_over_spans_device": round(statistics.median(d_torch) / statistics.median(d_ours), 2),
                 "algorithmic_bytes": phys, "spans_GBps_device": round(phys / statistics.median(d_ours) / 1e6, 1),
                 "spans_GBps_wall": round(phys / statistics.median(w_ours) / 1e6, 1)})


if __name__ == "__main__":
    main()
