"""Shared helpers for the parity tests."""
import numpy as np
import regex as re

from minbpe_amd.tokenizer import GPT4_SPLIT_PATTERN

_PAT = re.compile(GPT4_SPLIT_PATTERN)


def case_text(case, native):
    if "text" in case:
        return case["text"]
    n, seed = case["synth"]
    return native.synth_text(n, seed).decode("utf-8")


def split_chunks(text, pattern=_PAT):
    """(data, start offsets) the way RegexTokenizer.train chunks its input."""
    chunks = [c.encode("utf-8") for c in re.findall(pattern, text)]
    chunks = [c for c in chunks if c]
    offs = np.zeros(len(chunks), dtype=np.uint64)
    if len(chunks) > 1:
        np.cumsum(np.fromiter((len(c) for c in chunks[:-1]), dtype=np.uint64), out=offs[1:])
    return b"".join(chunks), offs


def pattern_of(case):
    """compiled split pattern of a golden case (default: the GPT-4 pattern, regex.py:29)"""
    return re.compile(case["pattern"]) if case.get("pattern") else _PAT


def data_for(case, native):
    text = case_text(case, native)
    if case["kind"] == "basic":
        return text.encode("utf-8"), None
    return split_chunks(text, pattern_of(case))


def toy_rank_table(base_tok, seed):
    """A cl100k-shaped {token bytes: rank} table from a trained tokenizer: single bytes get a
    permutation of 0..255 (tiktoken's byte order is not the identity), merged tokens rank = id."""
    import random
    perm = list(range(256))
    random.Random(seed).shuffle(perm)
    ranks = {bytes([b]): perm[b] for b in range(256)}
    for idx in range(256, 256 + len(base_tok.merges)):
        assert base_tok.vocab[idx] not in ranks  # vocabularies this small have no duplicate byte strings
        ranks[base_tok.vocab[idx]] = idx
    return perm, ranks


def cl100k_shaped_table(base_pairs, total, seed, ids="rank"):
    """A rank table of cl100k_base's SIZE (cl100k: 100,000 merges, ids up to 100,255; its ranks are not
    available offline) around a trained merge list: the `base_pairs` (ids 256 + position) keep their order
    but are spread over `total` ranks, the ranks in between are filled with merges of tokens defined so
    far (half of them pairs of early tokens, which do occur in text and change how it encodes).
    ids = "rank": merge r writes id 256 + r (RegexTokenizer; None is returned for the id list);
    ids = "sparse": merge r writes 1000 + 3 r (a merges dict whose values are not consecutive, as
    GPT4Tokenizer's are ranks: gpt4.py:65).  Returns (pairs as an (total, 2) int32 array, ids or None)."""
    rng = np.random.default_rng(seed)
    nb = len(base_pairs)
    assert total >= nb
    real_at = np.zeros(total, dtype=bool)
    real_at[rng.choice(total, nb, replace=False)] = True
    id_of = (lambda r: 256 + r) if ids == "rank" else (lambda r: 1000 + 3 * r)
    new_of_old = list(range(256)) + [0] * nb      # old id (256 + k) -> id in the big table
    old_of_new = {i: i for i in range(256)}
    real_old = {tuple(p) for p in base_pairs}
    defined = list(range(256))
    used = set()
    out = np.empty((total, 2), dtype=np.int32)
    k = 0
    coin = rng.random(total)
    pick = rng.integers(0, 1 << 30, size=(total, 2))
    for r in range(total):
        if real_at[r]:
            a, b = base_pairs[k]
            pair = (new_of_old[a], new_of_old[b])
            new_of_old[256 + k] = id_of(r)
            old_of_new[id_of(r)] = 256 + k
            k += 1
        else:
            j = 0
            while True:
                lim = min(len(defined), 400) if coin[r] < 0.5 else len(defined)
                pair = (defined[(pick[r, 0] + j) % lim], defined[(pick[r, 1] + 7 * j) % lim])
                old = (old_of_new.get(pair[0]), old_of_new.get(pair[1]))
                if pair not in used and old not in real_old:
                    break
                j += 1
        used.add(pair)
        out[r] = pair
        defined.append(id_of(r))
    mids = None if ids == "rank" else np.array([id_of(r) for r in range(total)], dtype=np.int32)
    return out, mids


def checkpoint_digests(pairs, counts, lens, step):
    """[[k, sha256-prefix of the first k merges], ...] every `step` merges and at the end.
    The digest covers pairs, counts AND stream lengths, as little-endian int64 triples
    (a, b, count, len) -- cheap to recompute for tens of thousands of merges."""
    import hashlib
    n = len(pairs)
    arr = np.empty((n, 4), dtype="<i8")
    if n:
        arr[:, 0:2] = np.asarray(pairs, dtype=np.int64).reshape(n, 2)
        arr[:, 2] = np.asarray(counts, dtype=np.int64)
        arr[:, 3] = np.asarray(lens, dtype=np.int64)
    h = hashlib.sha256()
    out = []
    k = 0
    while k < n:
        k2 = min(k + step, n)
        h.update(arr[k:k2].tobytes())
        out.append([k2, h.copy().hexdigest()[:16]])
        k = k2
    return out


def first_divergence(got, want):
    """Compare two checkpoint lists; returns None if every common checkpoint agrees, else the
    merge count of the first checkpoint that differs."""
    want_d = {k: d for k, d in want}
    for k, d in got:
        if k in want_d and want_d[k] != d:
            return k
    return None


# The inputs of the comparisons with the reference's recorded answers (tests/golden/live_reference.json,
# written by tests/golden/gen_live_reference.py): rebuilt here at test time, pinned there by sha256.

def random_texts(native):
    """tie-heavy alphabets, runs, multi-byte text"""
    import random
    rng = random.Random(424242)
    texts = []
    for k, n in [(2, 400), (3, 900), (5, 1500), (26, 2500)]:
        texts.append("".join(rng.choice([chr(97 + rng.randrange(k)), " ", chr(97 + rng.randrange(k))]) for _ in range(n)))
    texts.append("aaaa" * 50 + " " + "ab" * 80 + "   \n\n" + "aaa " * 40)
    texts.append(native.synth_text(6000, 99).decode())
    return texts


def tie_heavy_texts(native):
    import random
    rng = random.Random(77)
    texts = []
    for k, n in [(2, 3000), (3, 5000), (6, 8000)]:
        words = ["".join(chr(97 + rng.randrange(k)) for _ in range(rng.randrange(1, 6))) for _ in range(30)]
        texts.append(" ".join(rng.choice(words) for _ in range(n)))
    texts.append("aaaa " * 40 + "ab ab  ab\n\n" * 30 + "aaaa" * 9 + " x")
    texts.append(native.synth_text(300_000, 31).decode())
    return texts


def weighted_texts(native):
    return tie_heavy_texts(native)[:4] + [native.synth_text(40_000, 33).decode()]


def cl100k_probe(native):
    return native.synth_text(30_000, 52).decode() + " don't  stop 12345 ünïcödé 😉"


def cl100k_base_pairs(native):
    """the merge list the cl100k-sized tables are built around (the weighted oracle, 3000 merges)"""
    import oracle
    data, offs = split_chunks(native.synth_text(400_000, 51).decode())
    d2, o2, wts, _ = oracle.dedup(data, offs)
    return oracle.train(d2, 3000, o2, weights=wts)[0]


def saved_files_text(golden_dir):
    """train.py's flow on a slice of the reference's sample text, with control characters and a lone byte"""
    import os
    text = open(os.path.join(golden_dir, "taylorswift.txt"), encoding="utf-8").read()[:40_000]
    return text + "\x00\x07 control ​ chars � and a lone \x80 byte".encode(
        "utf-8", "surrogatepass").decode("utf-8", "replace")


def sha256_text(text):
    import hashlib
    return hashlib.sha256(text.encode("utf-8")).hexdigest()


# ---------------------------------------------------------------------------
# engine variants and chain-step options (shared by test_gpu_parity.py and test_gpu_weighted.py)

# engine variants: (mode, merge impl, slots, sparse, lean) -- slots 2 = the second slotted form (default);
# sparse 2 = every a != b pass goes through the inverted index and the sparse kernel; lean 1 (default) =
# lean iterations (k_lean.hip: three launches, table updated at the merge sites, a == b deferred to the
# general path) once the host has seen a count <= lean_count, 2 = from the first merge on, 0 = never,
# 3 = as 2 but every selection reads the whole row-maxima array (k_rowsel_lean; option lean_sum = 0)
# instead of the previous table update's per-wave records (k_sel_lean, the default), 4 = as 2 but every
# iteration selects (option lean_chain = 0: no tied pair is merged off an earlier selection's list), 5 = as 2
# but a == b passes visit every slot and mark what they rewrite for an index rebuild (option aa_sparse = 0)
VARIANTS = [(0, 0, 0, 1, 1), (1, 0, 1, 1, 1), (1, 0, 0, 1, 1), (1, 1, 0, 1, 1), (0, 1, 0, 1, 1), (1, 0, 2, 1, 1),
            (1, 0, 2, 2, 1), (1, 0, 2, 0, 1), (1, 0, 2, 1, 0), (1, 0, 2, 2, 0), (1, 0, 2, 1, 2), (1, 0, 2, 2, 2),
            (1, 0, 2, 2, 3), (1, 0, 2, 2, 4), (1, 0, 2, 2, 5), (1, 0, 2, 1, 7), (1, 0, 2, 2, 7), (1, 0, 2, 1, 8),
            (1, 0, 2, 1, 9), (1, 0, 2, 2, 9), (1, 0, 2, 2, 10)]


def set_variant(engine, mode, mimpl, slots, sparse, lean=1):
    """lean: 0 never | 1 the default engine (chain steps, k_chain.hip, wherever lean iterations would run with the
    index live) | 2 lean iterations forced onto every merge, no chain steps | 3, 4, 5 variants of 2 (selection from
    the whole row-maxima array; no chained merges; a == b passes over every slot) | 7 = 2 with chain steps |
    8 = 1 without chain steps (round 3's default engine) | 9 = 1 and 10 = 7 with the re-packing into 256-id slots (kernels of
    namespace bpe_g1) forced onto streams of any size at the first index build (option small_slots = 2; the default does
    it for streams of more than 16 Ki slots only)"""
    engine.set_option("mode", mode)
    engine.set_option("merge", mimpl)
    engine.set_option("slots", slots)
    engine.set_option("sparse", sparse)
    engine.set_option("lean", 1 if lean in (1, 8, 9) else (2 if lean >= 2 else 0))
    engine.set_option("chain", 1 if lean in (1, 7, 9, 10) else 0)
    engine.set_option("small_slots", 2 if lean in (9, 10) else 1)
    engine.set_option("lean_sum", 0 if lean == 3 else 1)
    engine.set_option("lean_chain", 0 if lean == 4 else 1)
    engine.set_option("aa_sparse", 0 if lean == 5 else 1)
    # lean >= 2 forces the lean iterations onto every merge (coverage of their kernels and of the hand-back):
    # no general-path stretches after clustered deferrals there
    engine.set_option("lean_backoff", 0 if lean in (2, 3, 4, 5, 7, 10) else 1)


def reset_variant(engine):
    set_variant(engine, 1, 0, 2, 1, 1)
    engine.set_option("depth", 8)


CHAIN_OPTIONS = [
    (("chain_kcap", 1),), (("chain_kcap", 4),), (("chain_kcap", 8),),   # batches of one, four, eight (default 15)
    (("count_is_removed", 0),),                      # the ids a merge removes are counted, not taken from the pair's count
    (("chain_prefetch", 0),),                        # no register prefetch of the next candidate slot
    (("small_slots", 0),), (("small_slots", 2),),    # 1024-id slots throughout / 256-id slots from the first index build
    (("small_slots", 2), ("chain_kcap", 2), ("pool_hint", 64)),
    (("chain_scan", 1),), (("chain_scan", 63),), (("chain_scan", 255),),    # one / 63 / 255 scanning workgroups in a pool rebuild (default 127)
    # a step as ONE launch (k_step: selection -> published batch -> merge pass -> grid barrier -> table update) instead of three
    (("fuse_step", 1),), (("fuse_step", 1), ("chain_kcap", 4)), (("fuse_step", 1), ("count_is_removed", 0)),
    (("fuse_step", 1), ("small_slots", 2)), (("fuse_step", 1), ("small_slots", 0)),
    (("fuse_step", 1), ("lean_grid", 8)), (("fuse_step", 1), ("lean_grid", 70)),   # ... on a grid of 8 / 70 workgroups (its phases deal the work by the grid)
    (("lean_grid", 8),),
]
CHAIN_DEFAULTS = {"chain_kcap": 15, "count_is_removed": 1, "chain_prefetch": 1,
                  "small_slots": 1, "pool_hint": 0, "chain_scan": 127, "fuse_step": 0, "lean_grid": 256}


# ---------------------------------------------------------------------------
# weighted inputs (tests/test_gpu_weighted.py, tests/test_dedup.py): chunk lists whose chunks carry a weight
# exponent e -- every pair inside the chunk counts 2^e times (bpe_load_bytes_weighted)

def chunk_offsets(chunks):
    offs = np.zeros(len(chunks), dtype=np.uint64)
    if len(chunks) > 1:
        np.cumsum(np.fromiter((len(c) for c in chunks[:-1]), dtype=np.uint64), out=offs[1:])
    return offs


def stands_for_bytes(offs, exps, n):
    """bytes of the text a weighted chunk list stands for: sum of len(chunk) * 2^e (Python integers: no wrap)"""
    lens = np.diff(np.append(np.asarray(offs, dtype=np.uint64), np.uint64(n)).astype(np.int64))
    return sum(int(length) << int(e) for length, e in zip(lens, exps))


def ties_chunks(n_chunks, seed):
    """the three-letter " xyz" chunk corpus of test_chain_step_options_cross_check, any size (bytes() of an int64
    array: every letter is followed by seven zero bytes, so (0, 0) heads the table and a == b merges come first)"""
    rng = np.random.default_rng(seed)
    return [b" " + bytes(97 + rng.integers(0, 3, size=rng.integers(1, 6))) for _ in range(n_chunks)]


def runs_text():
    """_weighted_cases' third text (runs of one symbol longer than a 4096-id slot, repeated so that they carry weight),
    and runs of more than 1024 ids -- one symbol and a two-symbol period -- repeated 8, 56 and 9 times: their copies
    carry exponents 3 | 3, 4, 5 | 0, 3"""
    return (("a" * 9001 + " ") * 3 + "aaaaaaa " * 5000 + "aaaa bbbb abab " * 3000 + ("b" * 4097 + " ") * 6
            + ("c" * 1500 + " ") * 8 + ("d" * 5000 + " ") * 56 + ("cd" * 700 + " ") * 9)


def hand_weighted(n_chunks, max_exp, run_exp, seed, big_every=150):
    """(data, offsets, exponents uint8, edges) with the exponents set by hand, not by a de-duplication: words over
    a small alphabet (ties, a == b pairs) with exponents drawn from 0 .. max_exp // 2, every `big_every`-th chunk a
    short one with an exponent from the top third of 0 .. max_exp (so that the text stood for stays small) -- and
    the edges a kernel can get wrong:
      - one-byte chunks (no pair) with exponent max_exp, next to chunks with exponent 0;
      - empty chunks (repeated offsets), with exponents of their own;
      - chunks that start exactly at multiples of 256, 1024 and 4096 ids, exponent max_exp after exponent 0;
      - one run of a single symbol, 2500 ids from position 900 mod 1024 on (it crosses two boundaries of 1024-id
        slots and nine or ten of 256-id slots), exponent run_exp.
    edges = dict(aligned=[(multiple, chunk index)], run=chunk index, singles=[...], empties=[...])."""
    rng = np.random.default_rng(seed)
    chunks, exps = [], []
    edges = dict(aligned=[], run=None, singles=[], empties=[])
    pos = 0

    def add(chunk, e):
        nonlocal pos
        chunks.append(chunk)
        exps.append(e)
        pos += len(chunk)
        return len(chunks) - 1

    def word(lo, hi, k=4):
        return bytes(97 + rng.integers(0, k, size=int(rng.integers(lo, hi))).astype(np.uint8))

    def pad_to(mult, rem=0):
        gap = (rem - pos) % mult
        while gap:  # filler words; the last one, exponent 0, ends exactly where the next chunk must start
            step = gap if gap <= 12 else int(rng.integers(1, 9))
            add(b" " + word(step, step + 1)[1:] if step > 1 else b" ", 0 if step == gap else int(rng.integers(0, max_exp // 2 + 1)))
            gap -= step

    todo = [4096, 1024, 256, "run", 4096, 256, 1024]
    spacing = max(n_chunks // 10, 30)
    mark = int(rng.integers(20, spacing))  # ordinary chunks go between the edges (the fillers of an edge do not count)
    while len(chunks) < n_chunks or todo:
        i = len(chunks)
        if todo and (i >= mark or len(chunks) >= n_chunks):
            kind = todo.pop(0)
            if kind == "run":
                pad_to(1024, 900)
                edges["run"] = add(b"z" * 2500, run_exp)
            else:
                pad_to(kind)
                assert pos % kind == 0
                edges["aligned"].append((kind, add(b" " + word(2, 7), max_exp)))
            mark = len(chunks) + int(rng.integers(20, spacing))
            continue
        r = i % big_every
        if r == 7:
            edges["singles"].append(add(bytes([97 + i // big_every % 4]), max_exp))
        elif r == 8:
            add(b" " + word(1, 5), 0)
        elif r == 31:
            edges["empties"].append(add(b"", int(rng.integers(0, max_exp + 1))))
        elif r == 20:
            add(b" " + word(1, 4), int(rng.integers(max_exp - max_exp // 3, max_exp + 1)))
        elif r == 21:
            add(b" " + word(1, 6, 2), 0)
        else:
            add(b" " + word(1, 8, 2 if i % 3 == 0 else 4), int(rng.integers(0, max_exp // 2 + 1)))
    data = b"".join(chunks)
    return data, chunk_offsets(chunks), np.array(exps, dtype=np.uint8), edges


def two_letter_weighted(n_ids, seed):
    """two letters in chunks of 6 .. 40 ids, exponents 8 and 9: every position weighs 256 or 512, so that a
    workgroup's LDS table (k_pair_count_lds) passes 2^14 for each of the four pairs after a few dozen positions"""
    rng = np.random.default_rng(seed)
    data = rng.integers(97, 99, size=n_ids, dtype=np.uint8).tobytes()
    lens = rng.integers(6, 41, size=n_ids // 6 + 1)
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < n_ids].astype(np.uint64)
    exps = rng.integers(8, 10, size=len(offs)).astype(np.uint8)
    return data, offs, exps


def expand_weighted(data, offs, exps):
    """the chunk list a weighted one stands for: every chunk written out 2^e times in place"""
    ends = np.append(offs[1:], len(data)).astype(np.int64)
    chunks = []
    for a, b, e in zip(offs.astype(np.int64), ends, exps):
        chunks += [data[int(a):int(b)]] * (1 << int(e))
    return b"".join(chunks), chunk_offsets(chunks)
