#!/usr/bin/env python3
"""Resident n-gram overlap of one large batch with a reference set against the yardsticks of DESIGN 4.11, all taken in
the same run.

The corpus has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(19.0 on average: 19.0 M ids) of random ids below 32000, made from a seed on the device.  The reference: --ref-docs
documents of --ref-len ids (1 M ids), window --ngram (13).  Of the documents that are long enough to hold a window, a
share of 0 %, 1 % and 100 % (--planted) carries one reference window, copied to a random place in it.  int32 and int64 ids
(corpus and reference alike).

  build     bpe_ngram_index_resident: wall ms of the whole call (offset check, copy, table, counters)
  call      bpe_ngram_overlap_resident into columns that exist: wall ms of the whole call (offset check and its
            counters, prefill, pass, finish, synchronise) for hits alone, with first / ref_pos, and with starts too, at
            every planted share; for every --tiles entry (ng_tile, the first one the default) at the middle share, the
            settings alternating inside every repetition
  passes    device ms of the pass over the stream and of the table passes: the hipEvent brackets of the call under
            option profile = 2 (kinds "decode" and "table"), at the default setting
  probe     the same call on the corpus as made (no hit) against an index of ONE reference document, whose table stays
            in the caches, and against the whole reference, each at the window of the run and at a window of 4 ids:
            what the table's size and the length of the hash cost
  clone     (a) torch.clone of the same ids between two hipEvents: the rate of a read of the stream
  torch     (b) the same answer composed in torch on the WHOLE corpus: unfold, a 64-bit polynomial hash of every window
            of corpus and reference, torch.isin, index_add_ per document.  Hash-only, not exact; its hits are compared
            with the call's

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
    ap.add_argument("--ref-docs", type=int, default=1000)
    ap.add_argument("--ref-len", type=int, default=1000)
    ap.add_argument("--ngram", type=int, default=13)
    ap.add_argument("--planted", default="0,1,100", help="shares (%%) of the documents that hold a window which carry a planted one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", default="4096,256,1024,2048,16384,65536", help="ng_tile settings, the first one the default")
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
            sys.exit(f"ngram_bench: step {name} ran out of its {args.step_limit} s")
        if rc:
            sys.exit(f"ngram_bench: step {name} ended with {rc}")


def step(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("ngram_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    dev = torch.device("cuda", T._default_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    dtype = torch.int32 if args.step == "int32" else torch.int64
    n_docs, w = args.docs, args.ngram
    hi = int(round(2 * args.doc_tokens))
    tiles = [int(x) for x in args.tiles.split(",")]
    shares = [int(x) for x in args.planted.split(",")]

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

    # ---- the reference, the corpus, and the planted corpora
    n_ref = args.ref_docs * args.ref_len
    ref = torch.randint(0, 32000, (n_ref,), generator=gen, device=dev).to(dtype)
    roff = torch.arange(args.ref_docs + 1, dtype=torch.int64, device=dev) * args.ref_len
    lens = torch.randint(1, hi, (n_docs,), generator=gen, device=dev)
    doff = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    doff[1:] = torch.cumsum(lens, 0)
    n = int(doff[-1])
    plain = torch.randint(0, 32000, (n,), generator=gen, device=dev).to(dtype)
    holds = torch.nonzero(lens >= w).reshape(-1)

    def corpus(share):
        ids = plain.clone()
        take = holds[torch.rand(holds.numel(), generator=gen, device=dev) * 100 < share]
        at = doff[take] + (torch.rand(take.numel(), generator=gen, device=dev) * (lens[take] - w + 1)).to(torch.int64)
        src = torch.randint(0, args.ref_docs, (take.numel(),), generator=gen, device=dev) * args.ref_len \
            + torch.randint(0, args.ref_len - w + 1, (take.numel(),), generator=gen, device=dev)
        for k in range(w):
            ids[at + k] = ref[src + k]
        torch.cuda.synchronize()  # (the engine runs on a stream of its own: torch's writes are done before it reads)
        return ids, take.numel()

    width = ref.element_size()
    label = {"dtype": str(dtype), "documents": n_docs, "ids": n, "ref_ids": n_ref, "ngram": w}
    say({**label, "version": native.version(), "documents_that_hold_a_window": holds.numel()})

    # ---- (a) the read rate
    for _ in range(args.warmup):
        plain.clone()
    clone_ms = event_ms(lambda: plain.clone())
    say({**label, "figure": "clone", "bytes_read": width * n, "event_ms": stats(clone_ms),
         "read_GBps": round(width * n / statistics.median(clone_ms) / 1e6, 1)})

    # ---- the build
    eng.set_option("ng_tile", tiles[0])
    build = lambda: eng.ngram_index_resident(ref.data_ptr(), width, n_ref, roff.data_ptr(), args.ref_docs, w)
    for _ in range(args.warmup):
        build()
    build_ms = wall_ms(build)
    eng.set_option("profile", 2)
    eng.prof_reset()
    iid, n_windows, n_distinct = build()
    prof = eng.prof_read()
    eng.set_option("profile", 0)
    say({**label, "figure": "build", "windows": n_windows, "distinct": n_distinct, "wall_ms": stats(build_ms),
         "copy_ms": round(prof["decode"]["ms"], 4), "table_ms": round(prof["table"]["ms"], 4)})

    # ---- (b) the torch composition: hash-only
    K = 0x9E3779B97F4A7C15 - (1 << 64)

    def window_hashes(x, off, n_seg):
        """(hash of the window that starts at every position but the last w - 1, whether it stays inside its segment, segment)"""
        win = x.to(torch.int64).unfold(0, w, 1)
        h = torch.zeros(win.shape[0], dtype=torch.int64, device=dev)
        for k in range(w):
            h = h * K + win[:, k]
        seg = torch.repeat_interleave(torch.arange(n_seg, device=dev), torch.diff(off))[:win.shape[0]]
        inside = torch.arange(win.shape[0], device=dev) + w <= off[seg + 1]
        return h, inside, seg

    def torch_hits(ids):
        rh, rin, _ = window_hashes(ref, roff, args.ref_docs)
        h, inside, doc = window_hashes(ids, doff, n_docs)
        hit = torch.isin(h, rh[rin]) & inside
        out = torch.zeros(n_docs, dtype=torch.int64, device=dev)
        out.index_add_(0, doc, hit.to(torch.int64))
        return out

    hits = torch.empty(n_docs, dtype=torch.int64, device=dev)
    first = torch.empty(n_docs, dtype=torch.int64, device=dev)
    ref_pos = torch.empty(n_docs, dtype=torch.int64, device=dev)
    starts = torch.empty(n, dtype=torch.uint8, device=dev)
    forms = (("hits", (0, 0, 0)), ("hits+first", (first.data_ptr(), ref_pos.data_ptr(), 0)),
             ("hits+first+starts", (first.data_ptr(), ref_pos.data_ptr(), starts.data_ptr())))
    for share in shares:
        ids, n_planted = corpus(share)
        call = lambda extra=(0, 0, 0): eng.ngram_overlap_resident(iid, ids.data_ptr(), width, n, doff.data_ptr(), n_docs, 0, 0,
                                                                  hits.data_ptr(), *extra)
        eng.set_option("ng_tile", tiles[0])
        n_hit = call(forms[2][1])
        want = hits.clone()
        sane = bool(int(starts.sum()) == int(want.sum()) and n_hit == int((want > 0).sum()) and n_hit >= n_planted)
        for _ in range(args.warmup):
            th = torch_hits(ids)
        comp_ms = wall_ms(lambda: torch_hits(ids), max(2, args.reps // 2))
        say({**label, "planted_percent": share, "planted_documents": n_planted, "figure": "torch",
             "what": "unfold + 64-bit polynomial hash + isin + index_add_, whole corpus, hash-only", "equals_call": bool(torch.equal(th, want)),
             "wall_ms": stats(comp_ms)})
        del th
        walls = {}
        for name, extra in forms:
            for _ in range(args.warmup):
                call(extra)
            walls[name] = wall_ms(lambda: call(extra))
        eng.set_option("profile", 2)
        eng.prof_reset()
        for _ in range(args.reps * args.inner):
            call()
        prof = eng.prof_read()
        eng.set_option("profile", 0)
        k = args.reps * args.inner
        pass_ms, table_ms = prof["decode"]["ms"] / k, prof["table"]["ms"] / k
        for name, _ in forms:
            w_ms = statistics.median(walls[name])
            line = {**label, "planted_percent": share, "figure": "call", "form": name, "ng_tile": tiles[0], "hit_documents": n_hit,
                    "hit_windows": int(want.sum()), "consistent": sane, "wall_ms": stats(walls[name]),
                    "over_clone": round(w_ms / statistics.median(clone_ms), 1),
                    "torch_over_call": round(statistics.median(comp_ms) / w_ms, 1)}
            if name == "hits":
                line.update({"pass_ms": round(pass_ms, 4), "table_passes_ms": round(table_ms, 4),
                             "pass_read_GBps": round(width * n / pass_ms / 1e6, 1) if pass_ms > 0 else None,
                             "windows_per_ns": round(n / pass_ms / 1e6, 2) if pass_ms > 0 else None})
            say(line)
        if share == shares[len(shares) // 2]:
            # ---- every tile setting of the query, hits alone; the answers must agree
            sweep = {s: [] for s in tiles}
            for _ in range(args.reps):
                for s in tiles:
                    eng.set_option("ng_tile", s)
                    sweep[s] += wall_ms(call, 1)
            for s in tiles:
                eng.set_option("ng_tile", s)
                call()
                if not torch.equal(hits, want):
                    sys.exit(f"ngram_bench: ng_tile = {s} differs from the default setting's result")
                say({**label, "planted_percent": share, "figure": "tile", "ng_tile": s, "wall_ms": stats(sweep[s])})
            eng.set_option("ng_tile", tiles[0])
        del ids

    # ---- what the probe costs: the corpus as made (no hit) against an index of ONE reference document, whose table
    # (2048 slots, 16 KiB) stays in the caches, at the window of the run and at a window of 4 ids (nine hash steps fewer;
    # more positions hold a window); then the index of the whole reference again, at that window too
    torch.cuda.synchronize()
    for what, n_small, docs_small, ww in (("one_reference_document", args.ref_len, 1, w), ("one_reference_document", args.ref_len, 1, 4),
                                          ("whole_reference", n_ref, args.ref_docs, 4), ("whole_reference", n_ref, args.ref_docs, w)):
        iid, n_windows, _ = eng.ngram_index_resident(ref.data_ptr(), width, n_small, roff.data_ptr(), docs_small, ww)
        call = lambda: eng.ngram_overlap_resident(iid, plain.data_ptr(), width, n, doff.data_ptr(), n_docs, 0, 0, hits.data_ptr(), 0, 0, 0)
        for _ in range(args.warmup):
            call()
        walls = wall_ms(call)
        eng.set_option("profile", 2)
        eng.prof_reset()
        for _ in range(args.reps * args.inner):
            n_hit = call()
        prof = eng.prof_read()
        eng.set_option("profile", 0)
        say({**label, "figure": "probe", "index": what, "ngram": ww, "windows": n_windows, "hit_documents": n_hit,
             "positions_with_a_window": int((lens - ww + 1).clamp(min=0).sum()), "wall_ms": stats(walls),
             "pass_ms": round(prof["decode"]["ms"] / (args.reps * args.inner), 4)})


if __name__ == "__main__":
    main()
