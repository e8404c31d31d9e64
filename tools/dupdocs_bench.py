#!/usr/bin/env python3
"""Resident document de-duplication of one large batch against the yardsticks of DESIGN 4.9, all taken in the same run.

The batch has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(18.9 on average: 18.9 M ids), made from a seed on the device.  Corpora: a share of 0 %, 30 % and 99 % of the documents
are copies of one of the others (made by select_docs_resident from the distinct ones), and "single": --docs copies of
one document.  int32 and int64 ids.

  call      bpe_dup_docs_resident with counts: wall ms of the whole call (offset check and its counters, init, hash pass,
            insert pass, finish pass, the group counter, synchronise), for every --settings entry
            (dup_tile:dup_wave_len, the first one the default), the settings alternating inside every repetition
  passes    device ms of {init + hash pass} and of {insert + finish pass}: the two hipEvent brackets of the call under
            option profile = 2 (kinds "decode" and "table"), at the default setting
  clone     torch.clone of the same ids between two hipEvents: the rate of a read of the stream, the ceiling of the hash
            pass
  torch     the closest composition in torch, HASH-ONLY AND NOT EXACT: diff, repeat_interleave, a mixed value per id,
            index_add_ per document, torch.unique(return_inverse=True), scatter_reduce(amin); whether its `first` equals
            the call's is reported, not required
  host      for scale, once: download the ids, a dict from the bytes of every document, upload the mask

Every wall figure is the mean of --inner back-to-back calls between two synchronises; one JSON line per figure with every
repetition's value, their minimum, median and maximum."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--corpora", default="dup_0,dup_30,dup_99,single")
    ap.add_argument("--settings", default="4096:64,1024:64,16384:64,65536:64,4096:16,4096:32,4096:128,4096:1024",
                    help="dup_tile:dup_wave_len settings, the first one the default")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("dupdocs_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    tok = T.BasicTokenizer()
    dev = torch.device("cuda", T._default_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    n_docs = args.docs
    hi = int(round(2 * args.doc_tokens))

    def corpus(name):
        """(ids int64, doff) of the corpus: distinct documents of random ids, the copies chosen among them"""
        if name == "single":
            doc = torch.randint(0, 32000, (int(round(args.doc_tokens)),), generator=gen, device=dev)
            return doc.repeat(n_docs), torch.arange(n_docs + 1, device=dev) * doc.numel()
        share = int(name.split("_")[1]) / 100
        n_src = max(1, int(round(n_docs * (1 - share))))
        lens = torch.randint(1, hi, (n_src,), generator=gen, device=dev)
        soff = torch.zeros(n_src + 1, dtype=torch.int64, device=dev)
        soff[1:] = torch.cumsum(lens, 0)
        src = torch.randint(0, 32000, (int(soff[-1]),), generator=gen, device=dev)
        index = torch.cat([torch.arange(n_src, device=dev), torch.randint(0, n_src, (n_docs - n_src,), generator=gen, device=dev)])
        index = index[torch.randperm(n_docs, generator=gen, device=dev)]
        return tok.select_docs_resident(src, soff, index)

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

    def event_ms(fn):
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / args.inner)
        return out

    def torch_first(ids, doff):
        """hash-only: a 64-bit sum of mixed values per document, its length folded in; equal sums count as equal"""
        lens = torch.diff(doff)
        doc = torch.repeat_interleave(torch.arange(n_docs, device=dev), lens)
        pos = torch.arange(ids.numel(), device=dev) - doff[doc]
        z = ids.to(torch.int64) ^ ((pos + 1) * -7046029254386353131)
        z = (z ^ (z >> 30)) * -4658895280553007687
        z = (z ^ (z >> 27)) * -7723592293110705685
        h = torch.zeros(n_docs, dtype=torch.int64, device=dev).index_add_(0, doc, z ^ (z >> 31))
        h = h * 31 + lens
        _, inv = torch.unique(h, return_inverse=True)
        low = torch.full((int(inv.max()) + 1,), n_docs, dtype=torch.int64, device=dev)
        low.scatter_reduce_(0, inv, torch.arange(n_docs, device=dev), "amin")
        return low[inv]

    settings = [tuple(int(x) for x in s.split(":")) for s in args.settings.split(",")]

    def set_form(s):
        eng.set_option("dup_tile", s[0])
        eng.set_option("dup_wave_len", s[1])

    say({"documents": n_docs, "version": native.version()})
    for name in args.corpora.split(","):
        ids64, doff = corpus(name)
        doff = doff.contiguous()
        n = ids64.numel()
        for dtype in (torch.int32, torch.int64):
            ids = ids64.to(dtype).contiguous()
            width = ids.element_size()
            first = torch.empty(n_docs, dtype=torch.int64, device=dev)
            counts = torch.empty(n_docs, dtype=torch.int64, device=dev)
            call = lambda: eng.dup_docs_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, 0, 0, first.data_ptr(),
                                                 counts.data_ptr())
            set_form(settings[0])
            n_distinct = call()
            label = {"corpus": name, "dtype": str(dtype), "ids": n, "distinct": n_distinct}
            ref = first.clone()
            # ---- the read rate
            for _ in range(args.warmup):
                ids.clone()
            clone_ms = event_ms(lambda: ids.clone())
            say({**label, "figure": "clone", "bytes_read": width * n, "event_ms": stats(clone_ms),
                 "read_GBps": round(width * n / statistics.median(clone_ms) / 1e6, 1)})
            # ---- the torch composition
            for _ in range(args.warmup):
                tf = torch_first(ids, doff)
            comp_ms = wall_ms(lambda: torch_first(ids, doff))
            say({**label, "figure": "torch", "what": "hash-only, NOT exact: diff + repeat_interleave + mix + index_add_ + unique + "
                 "scatter_reduce(amin)", "equals_call": bool(torch.equal(tf, ref)), "wall_ms": stats(comp_ms)})
            del tf
            # ---- the call, every setting
            walls = {s: [] for s in settings}
            for s in settings:
                set_form(s)
                for _ in range(args.warmup):
                    call()
                if not torch.equal(first, ref):
                    sys.exit(f"dupdocs_bench: {label} at {s} differs from the default setting's result")
            for _ in range(args.reps):  # the settings alternate inside every repetition
                for s in settings:
                    set_form(s)
                    walls[s] += wall_ms(call, 1)
            set_form(settings[0])
            # ---- the passes, at the default: the call's two hipEvent brackets
            eng.set_option("profile", 2)
            eng.prof_reset()
            for _ in range(args.reps * args.inner):
                call()
            prof = eng.prof_read()
            eng.set_option("profile", 0)
            k = args.reps * args.inner
            hash_ms, insert_ms = prof["decode"]["ms"] / k, prof["table"]["ms"] / k
            for s in settings:
                w_ms = statistics.median(walls[s])
                line = {**label, "figure": "call", "dup_tile:dup_wave_len": "%d:%d" % s, "wall_ms": stats(walls[s]),
                        "call_share_of_read": round(statistics.median(clone_ms) / w_ms, 3),
                        "torch_over_call": round(statistics.median(comp_ms) / w_ms, 2)}
                if s == settings[0]:
                    line.update({"hash_pass_ms": round(hash_ms, 4), "insert_finish_ms": round(insert_ms, 4),
                                 "hash_pass_GBps": round(width * n / hash_ms / 1e6, 1) if hash_ms > 0 else None,
                                 "hash_pass_share_of_read": round(statistics.median(clone_ms) / hash_ms, 3) if hash_ms > 0 else None})
                say(line)
            # ---- the host route, once per corpus
            if dtype == torch.int32 and not args.no_host:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h_ids, h_off = ids.cpu().numpy(), doff.cpu().tolist()
                seen, keep = {}, np.zeros(n_docs, dtype=bool)
                for d in range(n_docs):
                    keep[d] = seen.setdefault(h_ids[h_off[d]:h_off[d + 1]].tobytes(), d) == d
                mask = torch.from_numpy(keep).to(dev)
                torch.cuda.synchronize()
                say({**label, "figure": "host", "what": "download, dict of bytes, upload the mask", "wall_ms": round((time.perf_counter() - t0) * 1e3, 1),
                     "equals_call": bool(torch.equal(mask, ref == torch.arange(n_docs, device=dev)))})
            del ids, first, counts, ref
        del ids64, doff


if __name__ == "__main__":
    main()
