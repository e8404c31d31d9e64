#!/usr/bin/env python3
"""Resident span de-duplication of one large batch against the yardsticks of DESIGN 4.13, all taken in the same run.

The corpus has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(19.0 on average: 19.0 M ids) of random ids below 32000, made from a seed on the device.  Three states of it: as made
(no window seen but by accident), with one block of --block (60) ids planted at the end of 1 % of the documents ("few",
the documents lengthened by it), and with the same block at the end of every document ("all").  Windows --ngrams (13 and
50), int32 and int64 ids.

  call      bpe_dup_spans_resident into columns that exist: wall ms of the whole call (offset check and its counters,
            prefill, the passes, synchronise) for `seen` alone (no cover pass), for all six columns, and with the marks
            too, in the default scope; all six columns with BPE_SPANS_ANYWHERE; for every --tiles entry (ds_tile, the
            first one the default) on the "few" corpus, the settings alternating inside every repetition
  passes    device ms of the passes over the stream (build, query, cover) and of the prefill and the finish pass: the
            hipEvent brackets of the call under option profile = 2 (kinds "decode" and "table"), at the default setting
  scratch   bytes of the call's own scratch per id of the stream: slots x 16 + rows x 16 (+ n without d_marks)
  keep      bpe_keep_ids_resident(bits = 2, BPE_KEEP_DROP) on the resulting marks into an output that exists, against
            ids[mask] plus a cumsum gather of the offsets in torch
  clone     (a) torch.clone of the same ids between two hipEvents: the rate of a read of the stream
  siblings  (b) ngram_overlap (index = the first 1 M ids of the corpus) and repeat_stats on the same corpus and window
  torch     (c) `seen` composed in torch on the WHOLE corpus: unfold, a 64-bit polynomial hash of every window, sort,
            first-of-run, the lowest position of every run, index_add_ per document.  Hash-only, not exact; its answer is
            compared with the call's

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
    ap.add_argument("--block", type=int, default=60, help="ids of the planted block")
    ap.add_argument("--ngrams", default="13,50")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", default="4096,256,1024,2048,16384,65536", help="ds_tile settings, the first one the default")
    ap.add_argument("--step", choices=STEPS, help="run this step alone, in this process")
    ap.add_argument("--step-limit", type=int, default=270, help="seconds a step may take")
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
            sys.exit(f"dupspans_bench: step {name} ran out of its {args.step_limit} s")
        if rc:
            sys.exit(f"dupspans_bench: step {name} ended with {rc}")


def step(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("dupspans_bench: no GPU")
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
    B = args.block

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

    # ---- the corpora: the same random documents, lengthened by the block where it is planted
    base_lens = torch.randint(1, hi, (n_docs,), generator=gen, device=dev)
    block = torch.randint(0, 32000, (B,), generator=gen, device=dev).to(dtype)
    pick = torch.rand(n_docs, generator=gen, device=dev)
    n_base = int(base_lens.sum())
    base = torch.randint(0, 32000, (n_base,), generator=gen, device=dev).to(dtype)

    def corpus(share):
        """(ids, doff, documents with the block): the block behind `share` % of the documents"""
        chosen = pick * 100 < share
        lens = base_lens + B * chosen.to(torch.int64)
        doff = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
        doff[1:] = torch.cumsum(lens, 0)
        n = int(doff[-1])
        doc_of = torch.repeat_interleave(torch.arange(n_docs, device=dev), lens)
        within = torch.arange(n, device=dev) - doff[doc_of]
        own = within < base_lens[doc_of]
        ids = torch.empty(n, dtype=dtype, device=dev)
        ids[own] = base
        ids[~own] = block[(within - base_lens[doc_of])[~own]]
        torch.cuda.synchronize()  # (the engine runs on a stream of its own: torch's writes are done before it reads)
        return ids, doff, doc_of, int(chosen.sum())

    width = base.element_size()
    say({"dtype": str(dtype), "documents": n_docs, "ids_as_made": n_base, "version": native.version()})

    # ---- (c) the torch composition: hash-only, `seen` alone, the default scope
    K = 0x9E3779B97F4A7C15 - (1 << 64)

    def torch_seen(ids, doff, doc_of, w):
        win = ids.to(torch.int64).unfold(0, w, 1)
        doc = doc_of[:win.shape[0]]
        h = torch.zeros(win.shape[0], dtype=torch.int64, device=dev)
        for k in range(w):
            h = h * K + win[:, k]
        pos = torch.arange(win.shape[0], device=dev)
        inside = pos + w <= doff[doc + 1]
        h, doc, pos = h[inside], doc[inside], pos[inside]
        h, order = torch.sort(h, stable=True)          # (equal windows next to one another, in stream order)
        doc, pos = doc[order], pos[order]
        lead = torch.ones_like(h, dtype=torch.bool)
        lead[1:] = h[1:] != h[:-1]
        run = torch.cumsum(lead.to(torch.int64), 0) - 1
        low = pos[lead][run]                           # the lowest position of every run: its first entry
        seen = low < doff[doc]
        out = torch.zeros(n_docs, dtype=torch.int64, device=dev)
        out.index_add_(0, doc, seen.to(torch.int64))
        return out

    for w in [int(x) for x in args.ngrams.split(",")]:
        for kind, share in (("none", 0), ("few", 1), ("all", 100)):
            ids, doff, doc_of, n_planted = corpus(share)
            n = ids.numel()
            label = {"dtype": str(dtype), "documents": n_docs, "ids": n, "ngram": w, "planted": kind, "planted_documents": n_planted}
            cols = [torch.empty(n_docs, dtype=torch.int64, device=dev) for _ in range(6)]
            marks = torch.empty(n, dtype=torch.uint8, device=dev)
            ptrs = [c.data_ptr() for c in cols]
            forms = (("seen", 0, [0, 0, ptrs[2], 0, 0, 0, 0]), ("columns", 0, ptrs + [0]),
                     ("columns+marks", 0, ptrs + [marks.data_ptr()]), ("columns, anywhere", native.SPANS_ANYWHERE, ptrs + [0]))
            call = lambda flags, out: eng.dup_spans_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, w, 0, flags, *out)
            eng.set_option("ds_tile", tiles[0])
            # ---- (a) the read rate
            for _ in range(args.warmup):
                ids.clone()
            clone_ms = event_ms(lambda: ids.clone())
            say({**label, "figure": "clone", "bytes_read": width * n, "event_ms": stats(clone_ms),
                 "read_GBps": round(width * n / statistics.median(clone_ms) / 1e6, 1)})
            counters = call(0, forms[2][2])
            want = [c.clone() for c in cols]
            sane = bool(int((marks & 1).sum()) == int(want[2].sum()) and int((marks >> 1).sum()) == int(want[3].sum())
                        and counters[0] == int((want[2] > 0).sum()) and counters[1] == int(want[1].sum()))
            for _ in range(args.warmup):
                ts = torch_seen(ids, doff, doc_of, w)
            comp_ms = wall_ms(lambda: torch_seen(ids, doff, doc_of, w), max(2, args.reps // 2))
            say({**label, "figure": "torch", "what": "unfold + 64-bit polynomial hash + stable sort + first-of-run + index_add_, whole "
                 "corpus, hash-only, seen alone", "equals_call": bool(torch.equal(ts, want[2])), "wall_ms": stats(comp_ms)})
            del ts
            # ---- (b) the siblings on the same corpus and window
            n_ref = min(1_000_000, n)
            roff = torch.tensor([0, n_ref], dtype=torch.int64, device=dev)
            iid, _, _ = eng.ngram_index_resident(ids.data_ptr(), width, n_ref, roff.data_ptr(), 1, w)
            sib = {"ngram_overlap": lambda: eng.ngram_overlap_resident(iid, ids.data_ptr(), width, n, doff.data_ptr(), n_docs, 0, 0,
                                                                       ptrs[0], ptrs[1], ptrs[2]),
                   "repeat_stats": lambda: eng.repeat_stats_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, w, 0, 0, *ptrs)}
            sib_ms = {}
            for name, fn in sib.items():
                for _ in range(args.warmup):
                    fn()
                sib_ms[name] = wall_ms(fn)
                say({**label, "figure": "sibling", "call": name, "what": "hits, first, ref_pos against an index of the first 1 M ids"
                     if name == "ngram_overlap" else "all six columns", "wall_ms": stats(sib_ms[name])})
            walls = {}
            for name, flags, out in forms:
                for _ in range(args.warmup):
                    call(flags, out)
                walls[name] = wall_ms(lambda: call(flags, out))
            for name, flags, out in forms:
                eng.set_option("profile", 2)
                eng.prof_reset()
                for _ in range(args.reps * args.inner):
                    call(flags, out)
                prof = eng.prof_read()
                eng.set_option("profile", 0)
                k = args.reps * args.inner
                pass_ms, table_ms = prof["decode"]["ms"] / k, prof["table"]["ms"] / k
                w_ms = statistics.median(walls[name])
                scratch = (2 * n + 1) * 16 + 16 * n_docs + (0 if out[6] else n)
                say({**label, "figure": "call", "form": name, "ds_tile": tiles[0], "documents_seen": counters[0],
                     "windows": counters[1], "distinct_windows": counters[2], "seen_windows": int(want[2].sum()),
                     "covered": int(want[3].sum()), "consistent": sane, "wall_ms": stats(walls[name]),
                     "over_clone": round(w_ms / statistics.median(clone_ms), 1),
                     "torch_over_call": round(statistics.median(comp_ms) / w_ms, 1),
                     "over_ngram_overlap": round(w_ms / statistics.median(sib_ms["ngram_overlap"]), 2),
                     "over_repeat_stats": round(w_ms / statistics.median(sib_ms["repeat_stats"]), 2),
                     "passes_ms": round(pass_ms, 4), "prefill_and_finish_ms": round(table_ms, 4),
                     "scratch_bytes_per_id": round(scratch / n, 2)})
            # ---- keep_ids on the marks of the default scope, against ids[mask] + a cumsum gather of the offsets
            call(0, forms[2][2])
            out = torch.empty_like(ids)
            ooff = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
            keep = lambda: eng.keep_ids_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, marks.data_ptr(), 2,
                                                 native.KEEP_DROP, out.data_ptr(), n, ooff.data_ptr())

            def torch_keep():
                m = (marks & 2) == 0
                kept = ids[m]
                c = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                c[1:] = torch.cumsum(m.to(torch.int64), 0)
                return kept, c[doff]

            total = keep()
            t_ids, t_off = torch_keep()
            same = bool(total == t_ids.numel() and torch.equal(out[:total], t_ids) and torch.equal(ooff, t_off))
            del t_ids, t_off
            for _ in range(args.warmup):
                keep(), torch_keep()
            keep_ms, tk_ms = wall_ms(keep), wall_ms(torch_keep)
            say({**label, "figure": "keep", "what": "bits = 2, drop: the covered positions go", "kept_ids": total,
                 "equals_torch": same, "wall_ms": stats(keep_ms), "torch_wall_ms": stats(tk_ms),
                 "torch_over_call": round(statistics.median(tk_ms) / statistics.median(keep_ms), 2),
                 "over_clone": round(statistics.median(keep_ms) / statistics.median(clone_ms), 1)})
            del out, ooff
            if kind == "few":
                # ---- every tile setting, all columns; the answers must agree
                call(0, forms[1][2])
                want = [c.clone() for c in cols]
                sweep = {s: [] for s in tiles}
                for _ in range(args.reps):
                    for s in tiles:
                        eng.set_option("ds_tile", s)
                        sweep[s] += wall_ms(lambda: call(0, forms[1][2]), 1)
                for s in tiles:
                    eng.set_option("ds_tile", s)
                    call(0, forms[1][2])
                    if not all(torch.equal(c, x) for c, x in zip(cols, want)):
                        sys.exit(f"dupspans_bench: ds_tile = {s} differs from the default setting's result")
                    say({**label, "figure": "tile", "ds_tile": s, "wall_ms": stats(sweep[s])})
                eng.set_option("ds_tile", tiles[0])
            del ids, doff, doc_of, cols, marks


if __name__ == "__main__":
    main()
