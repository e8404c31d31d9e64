#!/usr/bin/env python3
"""Resident segments (lines) of one large batch against the yardsticks of DESIGN 4.14, all taken in the same run.

The corpus has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(19.0 on average: 19.0 M ids) of random ids below 32000, made from a seed on the device.  The class table has 32000
entries: the ids below --newlines (2000: one id in 16) end a line and belong to none, the --blanks (3000) ids behind them
belong to none.  One line of --line (6) content ids with a newline in front is planted behind 1 % of the documents, so
that the stream holds duplicate lines.  int32 and int64 ids.

  clone     torch.clone of the same ids between two hipEvents: the rate of a read of the stream
  call      bpe_segment_docs_resident into outputs that exist: wall ms of the whole call (offset check and its counters,
            the passes, the totals, synchronise) count-only, with every column, with every column and BPE_SEG_TAG_DOC;
            for every --tiles entry (seg_tile, the first one the default), the settings alternating inside every repetition
  passes    device ms of the passes: the hipEvent brackets of the call under option profile = 2 (kind "decode")
  marks     bpe_segment_marks_resident over the call's ranges, against the values laid over the positions in torch
            (index_add_ of + v at every start and - v at every end, cumsum)
  torch     the same segment stream composed in torch on the whole corpus: the classes gathered, a cumsum of the
            boundaries, a key per position, boolean indexing, first-of-run; its out, seg_offsets and seg_doc are compared
            with the call's
  lines     Tokenizer.duplicate_lines_resident end to end, both scopes, and its steps on their own: the segments, the
            exact de-duplication of the segment stream, the fold in torch, the marks; against a hash-only composition in
            torch (a 64-bit hash per line by index_add_, stable sort, first-of-run), whose count of duplicates is compared

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
    ap.add_argument("--newlines", type=int, default=2000, help="ids below this end a line")
    ap.add_argument("--blanks", type=int, default=3000, help="ids behind them that belong to no line")
    ap.add_argument("--line", type=int, default=6, help="content ids of the planted line")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", default="4096,256,1024,16384,65536", help="seg_tile settings, the first one the default")
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
            sys.exit(f"segments_bench: step {name} ran out of its {args.step_limit} s")
        if rc:
            sys.exit(f"segments_bench: step {name} ended with {rc}")


def step(args):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("segments_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    tok = T.BasicTokenizer()
    dev = torch.device("cuda", T._default_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    dtype = torch.int32 if args.step == "int32" else torch.int64
    n_docs = args.docs
    hi = int(round(2 * args.doc_tokens))
    tiles = [int(x) for x in args.tiles.split(",")]
    L = args.line

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

    # ---- the corpus: random documents, the planted line behind 1 % of them; the class table
    base_lens = torch.randint(1, hi, (n_docs,), generator=gen, device=dev)
    line = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                      torch.randint(args.newlines + args.blanks, 32000, (L,), generator=gen, device=dev)]).to(dtype)
    chosen = torch.rand(n_docs, generator=gen, device=dev) < .01
    lens = base_lens + (L + 1) * chosen.to(torch.int64)
    doff = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    doff[1:] = torch.cumsum(lens, 0)
    n = int(doff[-1])
    doc_of = torch.repeat_interleave(torch.arange(n_docs, device=dev), lens)
    within = torch.arange(n, device=dev) - doff[doc_of]
    own = within < base_lens[doc_of]
    ids = torch.empty(n, dtype=dtype, device=dev)
    ids[own] = torch.randint(0, 32000, (int(base_lens.sum()),), generator=gen, device=dev).to(dtype)
    ids[~own] = line[(within - base_lens[doc_of])[~own]]
    table = torch.zeros(32000, dtype=torch.uint8, device=dev)
    table[:args.newlines] = native.SEG_BREAK | native.SEG_SKIP
    table[args.newlines:args.newlines + args.blanks] = native.SEG_SKIP
    del within, own
    torch.cuda.synchronize()  # (the engine runs on a stream of its own: torch's writes are done before it reads)
    width = ids.element_size()
    label = {"dtype": str(dtype), "documents": n_docs, "ids": n, "planted_documents": int(chosen.sum())}
    say({**label, "version": native.version()})

    # ---- the read rate
    for _ in range(args.warmup):
        ids.clone()
    clone_ms = event_ms(lambda: ids.clone())
    clone = statistics.median(clone_ms)
    say({**label, "figure": "clone", "bytes_read": width * n, "event_ms": stats(clone_ms),
         "read_GBps": round(width * n / clone / 1e6, 1)})

    # ---- the call
    dso = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    common = (ids.data_ptr(), width, n, doff.data_ptr(), n_docs, table.data_ptr(), table.numel())
    results = {}
    for tag in (0, native.SEG_TAG_DOC):
        n_out, n_seg = eng.segment_docs_resident(*common, tag, d_doc_seg_off=dso.data_ptr())
        out = torch.empty(n_out, dtype=dtype, device=dev)
        so = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)
        sd, ss, se = (torch.empty(n_seg, dtype=torch.int64, device=dev) for _ in range(3))
        results[tag] = (out, so, sd, ss, se)
        fill = lambda tag=tag, r=results[tag]: eng.segment_docs_resident(*common, tag, r[0].data_ptr(), r[0].numel(), r[1].data_ptr(),
                                                                         r[2].numel(), r[2].data_ptr(), r[3].data_ptr(),
                                                                         r[4].data_ptr(), dso.data_ptr())
        count = lambda tag=tag: eng.segment_docs_resident(*common, tag, d_doc_seg_off=dso.data_ptr())
        for name, fn in (("count-only", count), ("every column", fill)):
            eng.set_option("seg_tile", tiles[0])
            for _ in range(args.warmup):
                fn()
            w_ms = wall_ms(fn)
            eng.set_option("profile", 2)
            eng.prof_reset()
            for _ in range(args.reps * args.inner):
                fn()
            pass_ms = eng.prof_read()["decode"]["ms"] / (args.reps * args.inner)
            eng.set_option("profile", 0)
            say({**label, "figure": "call", "form": name, "tags": bool(tag), "seg_tile": tiles[0], "segment_ids": n_out,
                 "segments": n_seg, "wall_ms": stats(w_ms), "passes_ms": round(pass_ms, 4),
                 "over_clone": round(statistics.median(w_ms) / clone, 1)})
        if not tag:
            want = [t.clone() for t in results[tag]]
            sweep = {s: [] for s in tiles}
            for _ in range(args.reps):
                for s in tiles:
                    eng.set_option("seg_tile", s)
                    sweep[s] += wall_ms(fill, 1)
            for s in tiles:
                eng.set_option("seg_tile", s)
                fill()
                if not all(torch.equal(c, x) for c, x in zip(results[tag], want)):
                    sys.exit(f"segments_bench: seg_tile = {s} differs from the default setting's result")
                say({**label, "figure": "tile", "seg_tile": s, "wall_ms": stats(sweep[s])})
            eng.set_option("seg_tile", tiles[0])
            del want
    out, so, sd, ss, se = results[0]
    n_seg = sd.numel()

    # ---- the same stream composed in torch
    def torch_segments():
        cls = table[ids.to(torch.int64)]
        content = (cls & 2) == 0
        brk = (cls & 1).to(torch.int64)
        key = doc_of * (n + 1) + (torch.cumsum(brk, 0) - brk)      # document and line of every position
        pc = torch.nonzero(content).reshape(-1)
        kc = key[pc]
        lead = torch.ones_like(kc, dtype=torch.bool)
        lead[1:] = kc[1:] != kc[:-1]
        t_so = torch.nonzero(lead).reshape(-1)
        return ids[pc], t_so, doc_of[pc[t_so]]

    for _ in range(args.warmup):
        t_out, t_so, t_sd = torch_segments()
    same = bool(torch.equal(t_out, out) and torch.equal(t_so, so[:-1]) and torch.equal(t_sd, sd))
    del t_out, t_so, t_sd
    if not same:
        sys.exit("segments_bench: the segment stream differs from the torch composition's")
    comp_ms = wall_ms(torch_segments, max(2, args.reps // 2))
    fill_ms = wall_ms(lambda: eng.segment_docs_resident(*common, 0, out.data_ptr(), out.numel(), so.data_ptr(), n_seg, sd.data_ptr(),
                                                        ss.data_ptr(), se.data_ptr(), dso.data_ptr()))
    say({**label, "figure": "torch", "what": "classes gathered, cumsum of the boundaries, a key per position, boolean indexing, "
         "first-of-run: out, seg_offsets, seg_doc (no source ranges, no doc_seg_offsets)", "equals_call": same,
         "wall_ms": stats(comp_ms), "torch_over_call": round(statistics.median(comp_ms) / statistics.median(fill_ms), 2)})

    # ---- the marks
    values = (torch.arange(n_seg, device=dev) % 3 == 0).to(torch.uint8)
    marks = torch.empty(n, dtype=torch.uint8, device=dev)
    mark = lambda: eng.segment_marks_resident(ss.data_ptr(), se.data_ptr(), n_seg, values.data_ptr(), n, marks.data_ptr())

    def torch_marks():
        # (a document of skipped ids only has no line and lies in no range: the values are laid over [0, n) as steps,
        # + v where a range begins and - v where it ends, and summed up)
        v = values.to(torch.int32)
        steps = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        steps.index_add_(0, ss, v)
        steps.index_add_(0, se, -v)
        return torch.cumsum(steps, 0)[:n].to(torch.uint8)

    torch.cuda.synchronize()  # (torch's writes to the values are done before the engine's stream reads them)
    mark()
    tm = torch_marks()
    same = bool(tm.numel() == n and torch.equal(tm, marks))
    del tm
    if not same:
        sys.exit("segments_bench: the marks differ from the torch composition's")
    for _ in range(args.warmup):
        mark(), torch_marks()
    m_ms, tm_ms = wall_ms(mark), wall_ms(torch_marks)
    say({**label, "figure": "marks", "segments": n_seg, "positions_in_no_range": int(n - (se - ss).sum()), "equals_torch": same, "wall_ms": stats(m_ms), "torch_wall_ms": stats(tm_ms),
         "torch_over_call": round(statistics.median(tm_ms) / statistics.median(m_ms), 2),
         "over_clone": round(statistics.median(m_ms) / clone, 1)})
    del marks, values, results, out, so, sd, ss, se

    # ---- duplicate lines end to end, and step by step
    K1, K2 = 0x9E3779B97F4A7C15 - (1 << 64), 0xC2B2AE3D27D4EB4F - (1 << 64)

    def torch_dups(scope):
        cls = table[ids.to(torch.int64)]
        content = (cls & 2) == 0
        brk = (cls & 1).to(torch.int64)
        key = doc_of * (n + 1) + (torch.cumsum(brk, 0) - brk)
        pc = torch.nonzero(content).reshape(-1)
        kc = key[pc]
        lead = torch.ones_like(kc, dtype=torch.bool)
        lead[1:] = kc[1:] != kc[:-1]
        seg_of = torch.cumsum(lead.to(torch.int64), 0) - 1
        first = torch.nonzero(lead).reshape(-1)
        rank = torch.arange(pc.numel(), device=dev) - first[seg_of]
        e = (ids[pc].to(torch.int64) + 1) * K1 + (rank + 1) * K2
        e = (e ^ (e >> 29)) * K2
        h = torch.zeros(first.numel(), dtype=torch.int64, device=dev).index_add_(0, seg_of, e)
        if scope == "in_doc":
            h = h + doc_of[pc[first]] * K1
        h, _ = torch.sort(h)
        return int((h[1:] == h[:-1]).sum())

    for scope in ("in_doc", "stream"):
        call = lambda: tok.duplicate_lines_resident(ids, doff, scope=scope, classes=table, return_marks=True)
        for _ in range(args.warmup):
            call()
        dups = tok.n_duplicate_lines
        whole = wall_ms(call)
        seg = tok.segments_resident(ids, doff, classes=table, tag_docs=scope == "in_doc")
        parts = {"segments": lambda: tok.segments_resident(ids, doff, classes=table, tag_docs=scope == "in_doc"),
                 "duplicate_docs on the segment stream": lambda: tok.duplicate_docs_resident(seg.ids, seg.seg_offsets)}
        first = tok.duplicate_docs_resident(seg.ids, seg.seg_offsets)
        dup = first != torch.arange(first.numel(), device=dev)
        clen = seg.seg_offsets[1:] - seg.seg_offsets[:-1]
        parts["fold in torch"] = lambda: [torch.zeros(n_docs, dtype=torch.int64, device=dev).index_add_(0, seg.seg_doc, v)
                                          for v in (dup.to(torch.int64), clen, clen * dup)]
        parts["marks"] = lambda: tok.segment_marks_resident(seg, dup, n)
        shares = {}
        for name, fn in parts.items():
            for _ in range(args.warmup):
                fn()
            shares[name] = round(statistics.median(wall_ms(fn)), 4)
        for _ in range(args.warmup):
            t_dups = torch_dups(scope)
        if t_dups != dups:
            sys.exit(f"segments_bench: {dups} duplicate lines, the torch composition counts {t_dups}")
        td_ms = wall_ms(lambda: torch_dups(scope), max(2, args.reps // 2))
        say({**label, "figure": "lines", "scope": scope, "duplicate_lines": dups, "segments": int(first.numel()),
             "wall_ms": stats(whole), "steps_ms": shares, "over_clone": round(statistics.median(whole) / clone, 1),
             "torch": "hash-only: a 64-bit hash per line by index_add_, sort, equal neighbours; the count alone",
             "torch_duplicate_lines": t_dups, "torch_wall_ms": stats(td_ms),
             "torch_over_call": round(statistics.median(td_ms) / statistics.median(whole), 2)})
        del seg, first, dup, clen, parts


if __name__ == "__main__":
    main()
