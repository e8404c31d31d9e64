#!/usr/bin/env python3
"""Resident training rows of one large batch against two yardsticks taken in the same run.

The batch: the ids of the GPT-4-split encode of synth_text (seed 4, --bytes) under a vocabulary trained on synth_text
(seed 2, --train-bytes, --vocab), left in HBM by the resident encode; documents of --doc-bytes on average, cut at chunk
starts.

  rows      bpe_rows_resident into a pre-sized buffer, wall ms of the whole call (validation kernel, three counters to the
            host, row kernel, synchronise) and of the count-only call (everything but the row kernel); the row kernel
            alone = their difference, for every --settings entry (rows_tile:rows_stage, the first one the default),
            the settings alternating inside every repetition
  copy      a plain device copy of as many elements at the same widths: copy_ for int32, .to(int64) for int64
  torch     the composition a user would otherwise write: searchsorted + gather + where
Shapes: pack with L = --row-len at S = L and S = L - 1 with a separator, S = L without one, both widths; per-document
with L = --doc-len.  The rows of every setting are compared with the composition's, element for element.
One JSON line per figure: every repetition's value, their minimum, median and maximum.  For kernel times proper run the
tool under a kernel trace with --reps 1 --settings <one>."""
import argparse
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--train-bytes", type=int, default=100_000_000)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--doc-bytes", type=int, default=300, help="documents of 100 .. 2 * this - 100 bytes")
    ap.add_argument("--row-len", type=int, default=2048)
    ap.add_argument("--doc-len", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settings", default="4096:1024,1024:256,2048:512,8192:1024,16384:2048,65536:4096,4096:64,4096:0",
                    help="rows_tile:rows_stage settings of the pack kernel, the first one the default")
    ap.add_argument("--no-torch-form", action="store_true", help="skip the torch composition (and the comparison with it)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("rows_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    dev = torch.device("cuda", T._default_device())
    # ---- the batch, left in HBM
    train = native.synth_text(args.train_bytes, 2)
    eng.load_bytes(train, native.split_offsets(train, 4))
    pairs = np.array(eng.train(args.vocab - 256)["pairs"], dtype=np.int32)
    del train
    data = native.synth_text(args.bytes, 4)
    offs = native.split_offsets(data, 4)
    rng = np.random.default_rng(9)
    cuts = np.cumsum(rng.integers(100, 2 * args.doc_bytes - 100, size=2 * len(data) // args.doc_bytes + 8))
    first = np.unique(np.searchsorted(offs, cuts[cuts < len(data)].astype(np.uint64)))   # first chunk of every document but 0
    first = np.concatenate([[0], first[(first > 0) & (first < len(offs))], [len(offs)]]).astype(np.int64)
    d_bytes = torch.from_numpy(np.frombuffer(bytearray(data), dtype=np.uint8)).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_buf = torch.empty(len(data), dtype=torch.int32, device=dev)
    d_ooff = torch.empty(len(offs) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    n = eng.encode_batch_resident(pairs, None, d_bytes.data_ptr(), len(data), d_offs.data_ptr(), len(offs), d_buf.data_ptr(),
                                  d_ooff.data_ptr())
    ids = d_buf[:n]
    doff = d_ooff[torch.from_numpy(first).to(dev)].contiguous()
    n_docs = len(first) - 1
    del d_bytes, d_offs, data
    say({"batch_tokens": n, "documents": n_docs, "tokens_per_document": round(n / n_docs, 1), "vocab": 256 + len(pairs),
         "version": native.version()})

    def wall_ms(fn, reps=None):
        out = []
        for _ in range(args.reps if reps is None else reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def torch_pack(L, S, sep, pad, dtype):
        """the rows by searchsorted + gather + where"""
        nd = doff.numel() - 1
        sh = doff - doff[0] + (torch.arange(nd + 1, device=dev) if sep is not None else 0)
        total = int(sh[-1])
        R = T.rows_count(total, L, S)
        q = torch.arange(R, device=dev)[:, None] * S + torch.arange(L, device=dev)[None, :]
        valid = q < total
        q = q.clamp(max=max(total - 1, 0))
        if sep is None:
            vals = ids[q + doff[0]]
        else:
            d = torch.searchsorted(sh, q, right=True) - 1
            vals = torch.where(q == sh[d + 1] - 1, sep, ids[(q - d + doff[0]).clamp(max=n - 1)])
        return torch.where(valid, vals, pad).to(dtype)

    settings = [tuple(int(x) for x in s.split(":")) for s in args.settings.split(",")]

    def set_form(s):
        eng.set_option("rows_tile", s[0])
        eng.set_option("rows_stage", s[1])

    sep_id, pad_id = 100257, 0
    shapes = [("pack", args.row_len, args.row_len, sep_id), ("pack", args.row_len, args.row_len - 1, sep_id),
              ("pack", args.row_len, args.row_len, None), ("per_doc", args.doc_len, args.doc_len, sep_id)]
    for mode, L, S, sep in shapes:
        for dtype in (torch.int32, torch.int64):
            width = 4 if dtype == torch.int32 else 8
            pack = mode == "pack"
            flags = native.ROWS_HAS_SEP if sep is not None else 0
            m = native.ROWS_PACK if pack else native.ROWS_PER_DOC
            call = lambda dst, cap, ln=0: eng.rows_resident(ids.data_ptr(), n, doff.data_ptr(), n_docs, m, flags, L, S,
                                                            sep or 0, pad_id, dst, width, cap, 0, 0, ln)
            R = call(0, 0)
            E = R * L
            out = torch.empty((R, L), dtype=dtype, device=dev)
            lengths = torch.empty(n_docs if not pack else 1, dtype=torch.int32, device=dev)
            ln = 0 if pack else lengths.data_ptr()
            torch.cuda.synchronize()
            label = {"mode": mode, "L": L, "S": S, "sep": sep is not None, "dtype": str(dtype), "rows": R, "elements": E}
            # ---- yardstick 1: a plain copy of as many elements
            src = torch.empty(E, dtype=torch.int32, device=dev).random_(0, 32000)
            if dtype == torch.int32:
                dst = torch.empty_like(src)
                copy = lambda: dst.copy_(src)
            else:
                copy = lambda: src.to(torch.int64)
            for _ in range(args.warmup):
                copy()
            copy_ms = wall_ms(copy)
            copy_bytes = E * (4 + width)
            say({**label, "figure": "copy", "what": "copy_ of int32" if width == 4 else ".to(int64) of int32", "bytes": copy_bytes,
                 "wall_ms": stats(copy_ms), "GBps": round(copy_bytes / statistics.median(copy_ms) / 1e6, 1)})
            # ---- yardstick 2: the torch composition (pack only)
            ref = None
            if pack and not args.no_torch_form:
                for _ in range(args.warmup):
                    ref = torch_pack(L, S, sep, pad_id, dtype)
                comp_ms = wall_ms(lambda: torch_pack(L, S, sep, pad_id, dtype))
                say({**label, "figure": "torch", "what": "searchsorted + gather + where", "wall_ms": stats(comp_ms)})
            # ---- the rows, every setting
            count = lambda: call(0, 0)
            full = lambda: call(out.data_ptr(), R, ln)
            walls, counts, same = {s: [] for s in settings}, [], {}
            for s in settings if pack else settings[:1]:
                set_form(s)
                for _ in range(args.warmup):
                    count(), full()
            for _ in range(args.reps):  # the settings alternate inside every repetition
                counts += wall_ms(count, 1)
                for s in settings if pack else settings[:1]:
                    set_form(s)
                    if s not in same:
                        out.fill_(-1)
                        full()
                        same[s] = None if ref is None else bool(torch.equal(out, ref))
                    walls[s] += wall_ms(full, 1)
            set_form(settings[0])
            rows_bytes = 4 * min(n, E) + width * E   # ids read once (S = L - 1 reads a few of them twice), rows written
            say({**label, "figure": "count", "what": "count-only call (validation, counters, synchronise), wall ms", **stats(counts)})
            for s in settings if pack else settings[:1]:
                k_ms = statistics.median(walls[s]) - statistics.median(counts)
                say({**label, "figure": "rows", "rows_tile:rows_stage": "%d:%d" % s, "equals_torch_form": same[s],
                     "wall_ms": stats(walls[s]), "row_kernel_ms": round(k_ms, 4), "bytes": rows_bytes,
                     "row_kernel_GBps": round(rows_bytes / k_ms / 1e6, 1) if k_ms > 0 else None,
                     "share_of_hbm_peak": round(rows_bytes / (k_ms * 1e-3) / HBM_PEAK, 4) if k_ms > 0 else None,
                     "copy_over_row_kernel": round(statistics.median(copy_ms) / k_ms, 3) if k_ms > 0 else None})
            del src, out, ref


if __name__ == "__main__":
    main()
