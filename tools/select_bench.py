#!/usr/bin/env python3
"""Resident document selection of one large batch against two yardsticks taken in the same run.

The batch has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(18.9 on average: 18.9 M ids), made from a seed on the device -- a selection moves ids whatever their values, so no
text is encoded for it.

  select    bpe_select_docs_resident into a pre-sized buffer: wall ms of the whole call (offset check, length pass, scan,
            counters to the host, placement, the offsets' copy, synchronise) and of the count-only call (everything but
            the placement); the placement alone = their difference, for every --settings entry (sel_tile:sel_stage, the
            first one the default), the settings alternating inside every repetition
  torch     (a) the composition a user would otherwise write: diff, gather of the lengths, cumsum, repeat_interleave of the
            per-document shifts, arange, add, gather -- first checked equal to the call's result
  clone     (b) torch.clone of a tensor of the output's size: the HBM copy rate
Forms: a full permutation, a 50 % mask, the permutation at max_len = 512; int32 and int64 ids.
Every timed figure is the mean of --inner back-to-back calls between two synchronises; one JSON line per figure with every
repetition's value, their minimum, median and maximum.  For kernel times proper run the tool under a kernel trace with
--reps 1 --settings <one>."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def stats(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4),
            "all": [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--doc-tokens", type=float, default=18.9, help="documents of 1 .. 2 * this - 1 ids")
    ap.add_argument("--max-len", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settings", default="4096:1024,1024:256,16384:2048,65536:4096,4096:0",
                    help="sel_tile:sel_stage settings of the placement kernel, the first one the default")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("select_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    dev = torch.device("cuda", T._default_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    n_docs = args.docs
    lens = torch.randint(1, int(round(2 * args.doc_tokens)), (n_docs,), generator=gen, device=dev)
    doff = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    doff[1:] = torch.cumsum(lens, 0)
    n = int(doff[-1])
    ids32 = torch.randint(0, 32000, (n,), generator=gen, device=dev, dtype=torch.int32)
    perm = torch.randperm(n_docs, generator=gen, device=dev)
    mask = torch.rand(n_docs, generator=gen, device=dev) < 0.5
    say({"batch_tokens": n, "documents": n_docs, "tokens_per_document": round(n / n_docs, 1), "version": native.version()})

    def wall_ms(fn, reps=None):
        out = []
        for _ in range(args.reps if reps is None else reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / args.inner)
        return out

    def torch_select(ids, index, max_len):
        """(out, out_offsets) by diff + gather + cumsum + repeat_interleave + arange + add + gather"""
        length = torch.diff(doff)[index]
        if max_len:
            length = length.clamp(max=max_len)
        ooff = torch.zeros(index.numel() + 1, dtype=torch.int64, device=dev)
        ooff[1:] = torch.cumsum(length, 0)
        shift = doff[index] - ooff[:-1]
        src = torch.repeat_interleave(shift, length) + torch.arange(int(ooff[-1]), device=dev)
        return ids[src], ooff

    settings = [tuple(int(x) for x in s.split(":")) for s in args.settings.split(",")]

    def set_form(s):
        eng.set_option("sel_tile", s[0])
        eng.set_option("sel_stage", s[1])

    forms = [("permutation", perm, 0), ("mask_50", torch.nonzero(mask).reshape(-1), 0),
             ("permutation_max_len", perm, args.max_len)]
    for dtype in (torch.int32, torch.int64):
        ids = ids32.to(dtype)
        width = ids.element_size()
        for name, index, max_len in forms:
            index = index.contiguous()
            m = index.numel()
            ooff = torch.empty(m + 1, dtype=torch.int64, device=dev)
            call = lambda dst, cap: eng.select_docs_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, index.data_ptr(),
                                                             m, max_len, 0, dst, cap, ooff.data_ptr())
            total = call(0, 0)
            out = torch.empty(total, dtype=dtype, device=dev)
            label = {"form": name, "dtype": str(dtype), "selections": m, "max_len": max_len, "out_ids": total}
            # ---- yardstick (b): the HBM copy rate at the output's size
            src = torch.empty(total, dtype=dtype, device=dev).random_(0, 32000)
            for _ in range(args.warmup):
                src.clone()
            clone_ms = wall_ms(lambda: src.clone())
            moved = 2 * width * total  # every output id is read once and written once
            say({**label, "figure": "clone", "bytes": moved, "wall_ms": stats(clone_ms),
                 "GBps": round(moved / statistics.median(clone_ms) / 1e6, 1)})
            del src
            # ---- yardstick (a): the torch composition
            for _ in range(args.warmup):
                ref, ref_off = torch_select(ids, index, max_len)
            comp_ms = wall_ms(lambda: torch_select(ids, index, max_len))
            say({**label, "figure": "torch", "what": "diff + gather + cumsum + repeat_interleave + arange + add + gather",
                 "wall_ms": stats(comp_ms)})
            # ---- the call, every setting
            count = lambda: call(0, 0)
            full = lambda: call(out.data_ptr(), total)
            walls, counts, same = {s: [] for s in settings}, [], {}
            for s in settings:
                set_form(s)
                for _ in range(args.warmup):
                    count(), full()
            for _ in range(args.reps):  # the settings alternate inside every repetition
                counts += wall_ms(count, 1)
                for s in settings:
                    set_form(s)
                    if s not in same:
                        out.fill_(-1)
                        ooff.fill_(-1)
                        full()
                        same[s] = bool(torch.equal(out, ref)) and bool(torch.equal(ooff, ref_off))
                        if not same[s]:
                            sys.exit(f"select_bench: {label} at {s} differs from the torch composition")
                    walls[s] += wall_ms(full, 1)
            set_form(settings[0])
            say({**label, "figure": "count", "what": "count-only call (checks, lengths, scan, counters, offsets), wall ms",
                 **stats(counts)})
            for s in settings:
                w_ms = statistics.median(walls[s])
                k_ms = w_ms - statistics.median(counts)
                say({**label, "figure": "select", "sel_tile:sel_stage": "%d:%d" % s, "equals_torch_form": same[s],
                     "wall_ms": stats(walls[s]), "placement_ms": round(k_ms, 4), "bytes": moved,
                     "placement_GBps": round(moved / k_ms / 1e6, 1) if k_ms > 0 else None,
                     "placement_share_of_clone": round(statistics.median(clone_ms) / k_ms, 3) if k_ms > 0 else None,
                     "call_share_of_clone": round(statistics.median(clone_ms) / w_ms, 3),
                     "torch_over_call": round(statistics.median(comp_ms) / w_ms, 2)})
            del out, ref, ref_off


if __name__ == "__main__":
    main()
