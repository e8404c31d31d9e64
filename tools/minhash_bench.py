#!/usr/bin/env python3
"""Resident MinHash signatures and near-duplicate groups of one large batch against the yardsticks of DESIGN 4.10, all
taken in the same run.

The batch has the shape of the README's encode batch: --docs documents (1 M) of 1 .. 2 * --doc-tokens - 1 ids each
(18.9 on average: 18.9 M ids), made from a seed on the device.  int32 and int64 ids, --perms permutations, window --ngram.

  call      bpe_minhash_resident into a signature matrix that exists: wall ms of the whole call (offset check and its
            counters, prefill pass, signature pass, synchronise), for every --tiles entry (mh_tile, the first one the
            default) at the first of --perms, the settings alternating inside every repetition
  passes    device ms of the prefill pass and of the signature pass: the two hipEvent brackets of the call under option
            profile = 2 (kinds "table" and "decode"), at the default setting
  clone     torch.clone of the same ids between two hipEvents: the rate of a read of the stream
  fill      fill_ of an int32 tensor of the signature's size: the rate of a write of the output, the larger stream
  torch     the same signature composed in torch on the first --slice-docs documents: unfold, the hashes in int64 tensors,
            scatter_reduce(amin) per document; its [n, n_perm] int64 intermediate is why it is a slice.  Documents
            shorter than the window are left out of it (and of the comparison with the call); the wall ms is scaled to
            the whole batch by the ids
  near      near_duplicate_docs_resident end to end on corpora of which 0 % and 30 % of the documents are copies of
            another with one id changed: wall ms, split into signature, the band calls, agreement and what is left
            (candidate lists and connected components, in torch)

Every wall figure is the mean of --inner back-to-back calls between two synchronises; one JSON line per figure with every
repetition's value, their minimum, median and maximum."""
import argparse
import json
import os
import statistics
import sys
import time


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
    ap.add_argument("--perms", default="128,64,256")
    ap.add_argument("--ngram", type=int, default=5)
    ap.add_argument("--tiles", default="2048,256,1024,4096,16384,65536", help="mh_tile settings, the first one the default")
    ap.add_argument("--slice-docs", type=int, default=50_000)
    ap.add_argument("--near", default="0,30", help="shares (%%) of near-copies of the end-to-end corpora; empty: none")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("minhash_bench: no GPU")
    import minbpe_amd.tokenizer as T
    from minbpe_amd import _native as native

    say = lambda d: print(json.dumps(d), flush=True)
    eng = T.engine()
    tok = T.BasicTokenizer()
    dev = torch.device("cuda", T._default_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    n_docs, w = args.docs, args.ngram
    hi = int(round(2 * args.doc_tokens))
    perms = [int(x) for x in args.perms.split(",")]
    tiles = [int(x) for x in args.tiles.split(",")]

    def corpus(share):
        """(ids int64, doff): distinct documents of random ids; `share` of the documents are copies of one of them with
        one id changed, in shuffled order"""
        n_src = max(1, int(round(n_docs * (1 - share))))
        lens = torch.randint(1, hi, (n_src,), generator=gen, device=dev)
        soff = torch.zeros(n_src + 1, dtype=torch.int64, device=dev)
        soff[1:] = torch.cumsum(lens, 0)
        src = torch.randint(0, 32000, (int(soff[-1]),), generator=gen, device=dev)
        if n_src == n_docs:
            return src, soff
        index = torch.cat([torch.arange(n_src, device=dev), torch.randint(0, n_src, (n_docs - n_src,), generator=gen, device=dev)])
        order = torch.randperm(n_docs, generator=gen, device=dev)
        ids, doff = tok.select_docs_resident(src, soff, index[order])
        copy = torch.nonzero(order >= n_src).reshape(-1)               # the documents that are copies: one id of each changes
        dl = doff[copy + 1] - doff[copy]
        at = doff[copy] + (torch.rand(copy.numel(), generator=gen, device=dev) * dl).to(torch.int64).clamp(max=dl - 1)
        ids[at] = ids[at] + 32000
        return ids, doff

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

    M32 = 0xFFFFFFFF

    def fmix32(h):
        h = h ^ (h >> 16)
        h = (h * 0x85EBCA6B) & M32
        h = h ^ (h >> 13)
        h = (h * 0xC2B2AE35) & M32
        return h ^ (h >> 16)

    def signed(x):
        return x - (1 << 64) if x >= 1 << 63 else x

    def torch_sig(ids, doff, k_docs, P, seed, ab):
        """the signatures of documents [0, k_docs) with at least w ids, in int64 tensors (values below 2^32 but for the last
        product, which wraps as uint64 does); rows of the other documents are left at 0x7FFFFFFF"""
        n = int(doff[k_docs])
        x = ids[:n].to(torch.int64)
        lo, hi_ = x & M32, (x >> 32) & M32
        t = fmix32(lo ^ ((hi_ * 0x9E3779B1) & M32))
        win = t.unfold(0, w, 1)                                        # [n - w + 1, w]
        s = torch.zeros(win.shape[0], dtype=torch.int64, device=dev)
        for k in range(w):
            s = (s * 0x01000193 + win[:, k]) & M32
        S = fmix32(s ^ ((seed ^ w) & M32))
        lens = torch.diff(doff[:k_docs + 1])
        doc = torch.repeat_interleave(torch.arange(k_docs, device=dev), lens)[:win.shape[0]]
        pos = torch.arange(win.shape[0], device=dev)
        ok = pos + w <= doff[doc + 1]                                  # the window stays inside its document
        h = ((S[ok, None] * ab[0][None, :] + ab[1][None, :]) >> 33) & 0x7FFFFFFF   # [windows, P] int64
        sig = torch.full((k_docs, P), 0x7FFFFFFF, dtype=torch.int64, device=dev)
        sig.scatter_reduce_(0, doc[ok, None].expand(-1, P), h, "amin")
        return sig.to(torch.int32), lens >= w

    def params(seed, P):
        mask, z, out = (1 << 64) - 1, seed, []
        for _ in range(2 * P):
            z = (z + 0x9E3779B97F4A7C15) & mask
            r = z
            r = ((r ^ (r >> 30)) * 0xBF58476D1CE4E5B9) & mask
            r = ((r ^ (r >> 27)) * 0x94D049BB133111EB) & mask
            out.append(r ^ (r >> 31))
        return (torch.tensor([signed(x | 1) for x in out[0::2]], dtype=torch.int64, device=dev),
                torch.tensor([signed(x) for x in out[1::2]], dtype=torch.int64, device=dev))

    say({"documents": n_docs, "ngram": w, "version": native.version()})
    ids64, doff = corpus(0.0)
    doff = doff.contiguous()
    n = ids64.numel()
    k_docs = min(args.slice_docs, n_docs)
    for dtype in (torch.int32, torch.int64):
        ids = ids64.to(dtype).contiguous()
        width = ids.element_size()
        for _ in range(args.warmup):
            ids.clone()
        clone_ms = event_ms(lambda: ids.clone())
        say({"dtype": str(dtype), "ids": n, "figure": "clone", "bytes_read": width * n, "event_ms": stats(clone_ms),
             "read_GBps": round(width * n / statistics.median(clone_ms) / 1e6, 1)})
        for pi, P in enumerate(perms):
            label = {"dtype": str(dtype), "ids": n, "n_perm": P}
            sig = torch.empty(n_docs * P, dtype=torch.int32, device=dev)
            call = lambda: eng.minhash_resident(ids.data_ptr(), width, n, doff.data_ptr(), n_docs, 0, 0, w, P, 0, sig.data_ptr(),
                                                sig.numel())
            eng.set_option("mh_tile", tiles[0])
            call()
            ref = sig.clone()
            # ---- the write rate
            for _ in range(args.warmup):
                sig.fill_(7)
            fill_ms = event_ms(lambda: sig.fill_(7))
            say({**label, "figure": "fill", "bytes_written": 4 * sig.numel(), "event_ms": stats(fill_ms),
                 "write_GBps": round(4 * sig.numel() / statistics.median(fill_ms) / 1e6, 1)})
            # ---- the torch composition, on a slice
            ab = params(0, P)
            for _ in range(args.warmup):
                ts, full = torch_sig(ids, doff, k_docs, P, 0, ab)
            comp_ms = wall_ms(lambda: torch_sig(ids, doff, k_docs, P, 0, ab))
            slice_ids = int(doff[k_docs])
            scale = n / slice_ids
            equal = bool(torch.equal(ts[full], ref.view(n_docs, P)[:k_docs][full]))
            say({**label, "figure": "torch", "what": "unfold + int64 hashes + scatter_reduce(amin)", "slice_docs": k_docs,
                 "slice_ids": slice_ids, "rows_compared": int(full.sum()), "equals_call": equal, "wall_ms_slice": stats(comp_ms),
                 "wall_ms_scaled": round(statistics.median(comp_ms) * scale, 2)})
            del ts, full
            # ---- the call, every setting (all of them at the first n_perm, the default alone at the others)
            use = tiles if pi == 0 else tiles[:1]
            walls = {s: [] for s in use}
            for s in use:
                eng.set_option("mh_tile", s)
                for _ in range(args.warmup):
                    call()
                if not torch.equal(sig, ref):
                    sys.exit(f"minhash_bench: {label} at mh_tile = {s} differs from the default setting's result")
            for _ in range(args.reps):
                for s in use:
                    eng.set_option("mh_tile", s)
                    walls[s] += wall_ms(call, 1)
            eng.set_option("mh_tile", tiles[0])
            eng.set_option("profile", 2)
            eng.prof_reset()
            for _ in range(args.reps * args.inner):
                call()
            prof = eng.prof_read()
            eng.set_option("profile", 0)
            k = args.reps * args.inner
            pre_ms, sig_ms = prof["table"]["ms"] / k, prof["decode"]["ms"] / k
            for s in use:
                w_ms = statistics.median(walls[s])
                line = {**label, "figure": "call", "mh_tile": s, "wall_ms": stats(walls[s]),
                        "torch_scaled_over_call": round(statistics.median(comp_ms) * scale / w_ms, 1)}
                if s == tiles[0]:
                    line.update({"prefill_ms": round(pre_ms, 4), "signature_pass_ms": round(sig_ms, 4),
                                 "fill_ms": round(statistics.median(fill_ms), 4), "clone_ms": round(statistics.median(clone_ms), 4),
                                 "signature_pass_write_GBps": round(4 * sig.numel() / sig_ms / 1e6, 1) if sig_ms > 0 else None,
                                 "multiply_add_min_per_ns": round(n * P / sig_ms / 1e6, 1) if sig_ms > 0 else None})
                say(line)
            del sig, ref
        del ids
    del ids64, doff
    # ---- near-duplicate groups, end to end
    for share in [int(x) for x in args.near.split(",") if x]:
        ids64, doff = corpus(share / 100)
        ids = ids64.to(torch.int32).contiguous()
        doff = doff.contiguous()
        spent = {}

        def timed(name, fn):
            def wrapper(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                spent[name] = spent.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
                return out
            return wrapper

        plain = T.BasicTokenizer()
        for _ in range(args.warmup):
            first = plain.near_duplicate_docs_resident(ids, doff)
        total = wall_ms(lambda: plain.near_duplicate_docs_resident(ids, doff))
        split = T.BasicTokenizer()
        split.minhash_resident = timed("signature", split.minhash_resident)
        split.duplicate_docs_resident = timed("band_calls", split.duplicate_docs_resident)
        split.minhash_agreement_resident = timed("agreement", split.minhash_agreement_resident)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            split.near_duplicate_docs_resident(ids, doff)
        torch.cuda.synchronize()
        whole = (time.perf_counter() - t0) * 1e3 / args.reps
        parts = {k: round(v / args.reps, 3) for k, v in spent.items()}
        parts["candidates_and_components_torch"] = round(whole - sum(parts.values()), 3)
        say({"figure": "near", "near_copies_percent": share, "ids": ids.numel(), "groups": plain.n_distinct_docs,
             "documents_joined": int((first != torch.arange(n_docs, device=dev)).sum()), "wall_ms": stats(total),
             "split_run_wall_ms": round(whole, 3), "split_ms": parts,
             "glue_share": round(parts["candidates_and_components_torch"] / whole, 3)})
        del ids64, ids, doff, first


if __name__ == "__main__":
    main()
