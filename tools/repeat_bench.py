#!/usr/bin/env python3
"""Resident repetition statistics of one large batch against the yardsticks of DESIGN 4.12, all taken in the same run.

The corpus has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(19.0 on average: 19.0 M ids) of random ids below 32000, made from a seed on the device.  Three corpora: as made (no
repeat but by accident), with the first third of 1 % of the documents copied onto their last third ("few"), and with
that done to every document ("many").  Windows --ngrams (3 and 10), int32 and int64 ids.

  call      bpe_repeat_stats_resident into columns that exist: wall ms of the whole call (offset check and its counters,
            prefill, the passes, synchronise) for `distinct` alone (no cover pass), for all six columns, and with the
            marks too; for every --tiles entry (rp_tile, the first one the default) on the "few" corpus, the settings
            alternating inside every repetition
  passes    device ms of the passes over the stream (insert, read, cover) and of the prefill and the finish pass: the
            hipEvent brackets of the call under option profile = 2 (kinds "decode" and "table"), at the default setting
  clone     (a) torch.clone of the same ids between two hipEvents: the rate of a read of the stream
  torch     (b) `distinct` composed in torch on the WHOLE corpus: unfold, a 64-bit polynomial hash of every window with
            the document's number mixed in, sort, unique_consecutive, index_add_ per document.  Hash-only, not exact;
            its answer is compared with the call's

Every wall figure is the mean of --inner back-to-back calls between two synchronises; one JSON line per figure with every
repetition's value, their minimum, median and maximum.  The widths run as steps of their own, each a child process under
its own time limit (--step-limit seconds); the first step that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

STEPS = ("int32", "int64")


def stats(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4),
            "all": [round(x, 4) for x in xs]}


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--doc-tokens", type=float, default=18.9, help="documents of 1 .. 2 * this - 1 ids")
    ap.add_argument("--ngrams", default="3,10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", default="4096,256,1024,2048,16384,65536", help="rp_tile settings, the first one the default")
    ap.add_argument("--step", choices=STEPS, help="run this step alone, in this process")
    ap.add_argument("--step-limit", type=int, default=240, help="seconds a step may take")
    return ap.parse_args()


def main():
    args = parse()
    if args.step:
        return step(args)
    for name in STEPS:  # every step under a limit of its own; nothing more is started after one that failed
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + sys.argv[1:],
                                timeout=args.step_limit, stdin=subprocess.DEVNULL).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"repeat_bench: step {name} ran out of its {args.step_limit} s")
        if rc:
            sys.exit(f"repeat_bench: step {name} ended with {rc}")


def step(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("repeat_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    dev = torch.device("cuda", T._default_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    dtype = torch.int32 if args.step == "int32" else torch.int64
    n_docs = args.docs
    hi = int(round(2 * args.doc_tokens))
    tiles = [int(x) for x in args.tiles.split(",")]

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

    # ---- the corpora
    lens = torch.randint(1, hi, (n_docs,), generator=gen, device=dev)
    doff = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    doff[1:] = torch.cumsum(lens, 0)
    n = int(doff[-1])
    plain = torch.randint(0, 32000, (n,), generator=gen, device=dev).to(dtype)
    doc_of = torch.repeat_interleave(torch.arange(n_docs, device=dev), lens)
    within = torch.arange(n, device=dev) - doff[doc_of]

    def corpus(share):
        """the first third of `share` % of the documents copied onto their last third"""
        ids = plain.clone()
        chosen = torch.rand(n_docs, generator=gen, device=dev) * 100 < share
        third = lens // 3
        last = chosen[doc_of] & (within >= (lens - third)[doc_of])
        at = torch.nonzero(last).reshape(-1)
        ids[at] = plain[at - (lens - third)[doc_of[at]]]
        torch.cuda.synchronize()  # (the engine runs on a stream of its own: torch's writes are done before it reads)
        return ids, int(chosen.sum())

    width = plain.element_size()
    label = {"dtype": str(dtype), "documents": n_docs, "ids": n}
    say({**label, "version": native.version()})

    # ---- (a) the read rate
    for _ in range(args.warmup):
        plain.clone()
    clone_ms = event_ms(lambda: plain.clone())
    say({**label, "figure": "clone", "bytes_read": width * n, "event_ms": stats(clone_ms),
         "read_GBps": round(width * n / statistics.median(clone_ms) / 1e6, 1)})

    # ---- (b) the torch composition: hash-only, `distinct` alone
    K = 0x9E3779B97F4A7C15 - (1 << 64)

    def torch_distinct(ids, w):
        win = ids.to(torch.int64).unfold(0, w, 1)
        doc = doc_of[:win.shape[0]]
        h = doc * K
        for k in range(w):
            h = h * K + win[:, k]
        inside = torch.arange(win.shape[0], device=dev) + w <= doff[doc + 1]
        h, doc = h[inside], doc[inside]
        order = torch.sort(h).indices          # (equal windows of one document: next to one another)
        h, doc = h[order], doc[order]
        lead = torch.ones_like(h, dtype=torch.bool)
        lead[1:] = (h[1:] != h[:-1]) | (doc[1:] != doc[:-1])
        out = torch.zeros(n_docs, dtype=torch.int64, device=dev)
        out.index_add_(0, doc, lead.to(torch.int64))
        return out

    cols = [torch.empty(n_docs, dtype=torch.int64, device=dev) for _ in range(6)]
    marks = torch.empty(n, dtype=torch.uint8, device=dev)
    ptrs = [c.data_ptr() for c in cols]
    forms = (("distinct", [0, 0, ptrs[2], 0, 0, 0, 0]), ("columns", ptrs + [0]), ("columns+marks", ptrs + [marks.data_ptr()]))
    for w in [int(x) for x in args.ngrams.split(",")]:
        for kind, share in (("none", 0), ("few", 1), ("many", 100)):
            ids, n_changed = corpus(share)
            call = lambda out: eng.repeat_stats_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, w, 0, 0, *out)
            eng.set_option("rp_tile", tiles[0])
            n_rep = call(forms[2][1])
            want = [c.clone() for c in cols]
            sane = bool(int((marks & 1).sum()) == int((want[1] - want[2]).sum()) and int((marks >> 1).sum()) == int(want[3].sum())
                        and n_rep == int((want[2] < want[1]).sum()))
            for _ in range(args.warmup):
                td = torch_distinct(ids, w)
            comp_ms = wall_ms(lambda: torch_distinct(ids, w), max(2, args.reps // 2))
            say({**label, "ngram": w, "repeats": kind, "changed_documents": n_changed, "figure": "torch",
                 "what": "unfold + 64-bit polynomial hash with the document mixed in + sort + neighbours + index_add_, whole corpus, "
                         "hash-only, distinct alone", "equals_call": bool(torch.equal(td, want[2])), "wall_ms": stats(comp_ms)})
            del td
            walls = {}
            for name, out in forms:
                for _ in range(args.warmup):
                    call(out)
                walls[name] = wall_ms(lambda: call(out))
            for name, out in forms:
                eng.set_option("profile", 2)
                eng.prof_reset()
                for _ in range(args.reps * args.inner):
                    call(out)
                prof = eng.prof_read()
                eng.set_option("profile", 0)
                k = args.reps * args.inner
                pass_ms, table_ms = prof["decode"]["ms"] / k, prof["table"]["ms"] / k
                w_ms = statistics.median(walls[name])
                say({**label, "ngram": w, "repeats": kind, "figure": "call", "form": name, "rp_tile": tiles[0],
                     "repeat_documents": n_rep, "repeat_windows": int((want[1] - want[2]).sum()), "covered": int(want[3].sum()),
                     "consistent": sane, "wall_ms": stats(walls[name]), "over_clone": round(w_ms / statistics.median(clone_ms), 1),
                     "torch_over_call": round(statistics.median(comp_ms) / w_ms, 1), "passes_ms": round(pass_ms, 4),
                     "prefill_and_finish_ms": round(table_ms, 4)})
            if kind == "few":
                # ---- every tile setting, all columns; the answers must agree
                sweep = {s: [] for s in tiles}
                for _ in range(args.reps):
                    for s in tiles:
                        eng.set_option("rp_tile", s)
                        sweep[s] += wall_ms(lambda: call(forms[1][1]), 1)
                for s in tiles:
                    eng.set_option("rp_tile", s)
                    call(forms[1][1])
                    if not all(torch.equal(c, x) for c, x in zip(cols, want)):
                        sys.exit(f"repeat_bench: rp_tile = {s} differs from the default setting's result")
                    say({**label, "ngram": w, "repeats": kind, "figure": "tile", "rp_tile": s, "wall_ms": stats(sweep[s])})
                eng.set_option("rp_tile", tiles[0])
            del ids


if __name__ == "__main__":
    main()
