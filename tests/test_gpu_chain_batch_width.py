"""Chain steps at every batch width: the two places where a step's cost used to grow with the batch, and now spread the
batch over threads instead (minbpe_amd/csrc/kernels/k_chain.hip):

  merge_chain_body          the candidate masks of a round: 1024 threads, thread tid holds mask word tid & 127 and the pairs
                            p = tid >> 7 (mod 8); the groups' masks of a word meet in LDS.  Seams: widths 8 | 9, 16 | 17, 24 | 25.
  apply_chain_tokens_wide   the delta fold: a workgroup is 64 tokens x (wave =) one of four pair groups, group pg takes the pairs
                            p = pg (mod 4), four a turn (seams 4 | 5, 8 | 9, 12 | 13 and the turn's 16 | 17); a row's flag is
                            the OR of its groups' flags, met in LDS; one thread per token writes the flag word and the 64-row
                            record.

Every case is one stream trained twice -- up to the end of the batch under test (train_stats()["steps"] must say that the K
merges took exactly ONE step more than the merges before them: a batch that did not form FAILS) and on through a tail --
and compared with oracle.train on pairs, counts and lens.

The streams (batch_stream): K listed pairs over bytes of their own tie at `count`; every listed pair p has a left neighbour
TL[p % 5] and a right neighbour TR[p % 7] in some of its chunks, with counts of their own below `count` -- so a token is the
left neighbour of sites of pairs in DIFFERENT pair groups, the maximum of its row is a (t, a_p) that the batch lowers (a lost
flag leaves a stale maximum: a wrong merge when the tail reaches that level), and the tail merges (t, Z_p) and (Z_p, u) for
every p, pair K - 1 included.  A pair (q, q) below them hands the 1024-id geometry back to a lean iteration, which selects
from the 64-row records.  Everything else is one-byte chunks (no pair at all), so that most slots hold sites of ONE pair: a
pair group missing from the mask leaves sites unmerged.  Sites stand at multiples of 8 ids; the caller may pin some.

Where the batch starts (z0): a prelude of words over 16 bytes, word s = (i s mod 17) for i = 1 .. 16 -- the bigrams of two
words never coincide (they differ by s), a word's 15 merges chain left to right, a word per level above `count` -- gives 15
merges a word; the batch's first pair starts with the last byte of the last word, which ends the step before it."""
import numpy as np
import pytest

import oracle
from helpers import reset_variant, set_variant
from test_chain_kcap31 import KCAP, model_batch, same

TL = [130, 131, 132, 133, 134]
TR = [140, 141, 142, 143, 144, 145, 146]
AA = 150
HEAD = (252, 253)
CH_REP_COUNT = 16384
_CACHE = {}


def prelude_words(n_merges, count):
    """chunks whose merges are the first n_merges of the stream, and the byte the batch's first pair must start with"""
    words, left, s = [], n_merges, 1
    while left > 0:
        length = min(16, left + 1)
        words.append([(i * s) % 17 for i in range(1, length + 1)])
        left -= length - 1
        s += 1
    assert s <= 17
    chunks = []
    for k, w in enumerate(words):
        chunks += [w] * (count + 3 + 2 * (len(words) - k))
    return chunks, words[-1][-1]


def batch_stream(K, count=20, n_ids=96_000, seed=1, prelude=0, pinned=(), weighted=False):
    """(data, offs, None, listed, n_before[, exps]): pinned = [(id position, listed pair index)] sites at given positions"""
    rng = np.random.default_rng(seed)
    firsts = [60 + 2 * i for i in range(K)]
    seconds = [61 + 2 * i for i in range(K)]
    lead = []
    if prelude:
        lead, firsts[0] = prelude_words(prelude, count)
        lead = lead + [[firsts[0], seconds[0]]]  # (the first of the tied pairs to occur)
    site = lambda p: [firsts[p], seconds[p]]
    used = [0] * K
    used[0] += 1 if prelude else 0
    for _, p in pinned:
        used[p] += 1
    placed = []
    for p in range(K):
        ml, mr = min(2 + (p * 7) % 9, count // 4), min(2 + (p * 5) % 8, count // 4)
        placed += [[TL[p % 5]] + site(p)] * ml + [site(p) + [TR[p % 7]]] * mr + [site(p) + site(p)]  # (the last: adj)
        used[p] += ml + mr + 2
        if K > 1:  # a site directly before a site of another pair of the batch
            q = (p + 1) % K
            placed.append(site(p) + site(q))
            used[p] += 1
            used[q] += 1
    for p in range(K):
        assert used[p] <= count
        placed += [site(p)] * (count - used[p])
    placed += [[AA, AA]] * (count // 3)
    if not prelude:
        placed += [list(HEAD)] * (count + 1)
    lead_len = sum(len(c) for c in lead)
    lo = (lead_len + 15) // 8 * 8
    taken = {pos for pos, _ in pinned}
    free = np.array([x for x in range(lo, n_ids - 8, 8) if x not in taken])
    assert len(free) > 4 * len(placed)
    where = rng.choice(free, size=len(placed), replace=False)
    order = rng.permutation(len(placed))
    at = {int(w): placed[int(i)] for w, i in zip(where, order)}
    for pos, p in pinned:
        assert pos % 8 == 0 and lo <= pos < n_ids - 8
        at[pos] = site(p)
    pos = 0
    for c in lead:
        at[pos] = c
        pos += len(c)
    ids = rng.integers(200, 250, size=n_ids).astype(np.uint8)  # one-byte chunks wherever nothing is placed
    start = np.ones(n_ids, dtype=bool)
    for w, c in at.items():
        ids[w:w + len(c)] = c
        start[w + 1:w + len(c)] = False
    data = ids.tobytes()
    offs = np.flatnonzero(start).astype(np.uint64)
    listed = list(zip(firsts, seconds))
    n_before = prelude if prelude else 1
    if weighted:  # the placed chunks weigh 2 (the listed pairs still tie), the one-byte chunks 1, 2 or 4
        e = rng.integers(0, 3, size=len(offs)).astype(np.uint8)
        e[np.diff(np.append(offs, n_ids).astype(np.int64)) > 1] = 1
        return data, offs, None, listed, n_before, e
    return data, offs, None, listed, n_before


def stream(name, *args, **kw):
    if name not in _CACHE:
        _CACHE[name] = batch_stream(*args, **kw)
    return _CACHE[name]


def expected(name, data, offs, nm, exps=None):
    key = ("exp", name, nm)
    if key not in _CACHE:
        if exps is None:
            _CACHE[key] = oracle.train(data, nm, offs)
        else:  # (lengths of the resident stream, not of the text it stands for: tests/test_gpu_weighted.py)
            pairs, counts, _ = oracle.train(data, nm, offs, weights=(1 << exps.astype(np.int64)))
            ids, o, lens = np.frombuffer(data, dtype=np.uint8).astype(np.int32), offs, []
            for i, p in enumerate(pairs):
                ids, off_full = oracle.merge_chunks(ids, o, p, 256 + i)
                o = off_full[:-1]
                lens.append(len(ids))
            _CACHE[key] = (pairs, counts, lens)
    return _CACHE[key]


OPTION_DEFAULTS = (("chain_kcap", KCAP), ("small_slots", 1), ("chain_hash_kmin", 0), ("fuse_step", 0), ("lean_grid", 256))


def train(engine, data, offs, nm, opts, exps=None):
    set_variant(engine, 1, 0, 2, 2, 7)  # every merge after the first a chain step through the index
    try:
        engine.set_option("chain_kcap", KCAP)
        for k, v in opts:
            engine.set_option(k, v)
        engine.load_bytes(data, offs, exps)
        res = engine.train(nm)
        return res, engine.train_stats()
    finally:
        for k, v in OPTION_DEFAULTS:
            engine.set_option(k, v)
        reset_variant(engine)


def check(engine, name, st, K, opts, tail=None, exps=None):
    """the K listed pairs are merges n_before .. n_before + K - 1, in ONE step; then the tail"""
    data, offs, chunks, listed, n_before = st[:5]
    tail = 2 * K + 1 if tail is None else tail  # (the neighbour pairs of every listed pair, and (q, q))
    nm = n_before + K + tail
    exp = expected(name, data, offs, nm, exps)
    assert sorted(exp[0][n_before:n_before + K]) == sorted(listed), name
    assert len(set(exp[1][n_before:n_before + K])) == 1 and exp[1][n_before - 1] > exp[1][n_before] > exp[1][n_before + K]
    cut = lambda n: (exp[0][:n], exp[1][:n], exp[2][:n])
    steps_before = 0
    if n_before > 1:
        res, s = train(engine, data, offs, n_before, opts, exps)
        assert same(res, cut(n_before)), name
        steps_before = s["steps"]
    res, s = train(engine, data, offs, n_before + K, opts, exps)
    print(name, opts, "steps before / with the batch:", steps_before, s["steps"], "slot ids", s["slot_ids"])
    assert same(res, cut(n_before + K)), name
    assert s["steps"] == steps_before + 1, (name, "the batch of %d did not form" % K, steps_before, s["steps"])
    assert s["slot_ids"] == (1024 if ("small_slots", 0) in opts else 256)
    res, s2 = train(engine, data, offs, nm, opts, exps)
    for i in range(nm):
        assert (res["pairs"][i], res["counts"][i], res["lens"][i]) == (exp[0][i], exp[1][i], exp[2][i]), (name, "merge", i)
    return exp, s2


# ---------------------------------------------------------------------------
# CPU: the pool model takes the K pairs in one batch (small streams; the large ones are the same construction)

def chunks_after(data, offs, pairs):
    ids, o = np.frombuffer(data, dtype=np.uint8).astype(np.int32), offs
    for i, p in enumerate(pairs):
        ids, off_full = oracle.merge_chunks(ids, o, p, 256 + i)
        o = off_full[:-1]
    cuts = np.asarray(o, dtype=np.int64)[1:]
    return [c.astype(np.int64) for c in np.split(ids, cuts) if len(c)]


@pytest.mark.parametrize("K,prelude", [(1, 0), (2, 0), (9, 0), (31, 0), (31, 45), (31, 234)])
def test_the_pool_model_takes_the_listed_pairs_in_one_batch(K, prelude):
    data, offs, chunks, listed, n_before = stream(("w", K, prelude), K, prelude=prelude, n_ids=40_000)
    exp = expected(("w", K, prelude), data, offs, n_before + K + 2)
    assert sorted(exp[0][n_before:n_before + K]) == sorted(listed)
    assert exp[1][n_before - 1] > exp[1][n_before] == exp[1][n_before + K - 1] > exp[1][n_before + K]
    now = chunks_after(data, offs, exp[0][:n_before])
    assert sorted(model_batch(now, KCAP)) == sorted(listed)
    if prelude:  # the step before ends at the batch's first pair: it starts with the last prelude merge's second token
        before = model_batch(chunks_after(data, offs, exp[0][:n_before - 1]), KCAP)
        assert before == [exp[0][n_before - 1]], before
        z0 = 256 + n_before
        assert z0 // 64 != (z0 + K - 1) // 64 and (prelude != 234 or z0 // 256 != (z0 + K - 1) // 256)


# ---------------------------------------------------------------------------
# GPU

WIDTHS = [1, 2, 8, 9, 16, 17, 24, 25, 31]


@pytest.mark.gpu
@pytest.mark.parametrize("K", WIDTHS)
def test_every_batch_width_in_256_id_slots(engine, K):
    check(engine, ("w256", K), stream(("w256", K), K), K, (("small_slots", 2),))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [9, 17, 25, 31])
def test_a_width_per_seam_in_1024_id_slots(engine, K):
    """(the pair (q, q) of the tail is handed back to a lean iteration here: its selection reads the 64-row records)"""
    check(engine, ("w256", K), stream(("w256", K), K), K, (("small_slots", 0),))


@pytest.mark.gpu
@pytest.mark.parametrize("K,kcap", [(4, 16), (5, 16), (13, 16), (16, 16), (8, 8)])
def test_widths_at_the_seams_of_four_pair_groups_under_caps_of_16_and_8(engine, K, kcap):
    check(engine, ("w256", K), stream(("w256", K), K), K, (("small_slots", 2), ("chain_kcap", kcap)))


@pytest.mark.gpu
@pytest.mark.parametrize("small_slots", [2, 0])
def test_the_one_launch_step_at_its_cap_of_15(engine, small_slots):
    check(engine, ("w256", 15), stream(("w256", 15), 15), 15, (("small_slots", small_slots), ("fuse_step", 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [9, 31])
def test_the_compare_fall_back(engine, K):
    check(engine, ("w256", K), stream(("w256", K), K), K, (("small_slots", 2), ("chain_hash_kmin", 32)))


@pytest.mark.gpu
@pytest.mark.parametrize("prelude,small_slots", [(45, 2), (234, 2), (234, 0)])
def test_new_ids_across_a_multiple_of_64_and_of_256(engine, prelude, small_slots):
    """ids 301 .. 331 straddle 320 (a 64-row record, a workgroup of the fold); 490 .. 520 straddle 512"""
    name = ("seam", prelude)
    check(engine, name, stream(name, 31, prelude=prelude), 31, (("small_slots", small_slots),))


@pytest.mark.gpu
@pytest.mark.parametrize("lean_grid,n_slots", [(1, 5000), (2, 8400)])
def test_more_than_128_mask_words_per_workgroup(engine, lean_grid, n_slots):
    """a second round of mask words, partly filled, the last word partial; sites pinned into the first and the last word
    of each round and into the last slot"""
    n_ids = n_slots * 256 - 8 * 11  # (Tl is no multiple of 32 slots)
    per = ((n_slots + 31) // 32 + lean_grid - 1) // lean_grid
    assert per > 128 and per % 128 != 0 and n_slots % 32 != 0
    slots = []
    for g in range(lean_grid):
        w0 = g * per
        slots += [32 * w0 + 1, 32 * (w0 + 127) + 31, 32 * (w0 + 128), min(n_slots - 1, 32 * (w0 + per) - 1)]
    pinned = [(s * 256 + 64, (5 * i + 30) % 31) for i, s in enumerate(slots)]  # (pairs 30, 4, 9, ...: several groups)
    name = ("rounds", lean_grid)
    st = stream(name, 31, n_ids=n_ids, pinned=pinned, seed=3)
    check(engine, name, st, 31, (("small_slots", 2), ("lean_grid", lean_grid)), tail=20)


def tier_stream(counts, seed):
    """pairs back to back, no filler: pair p counts counts[p]; left and right neighbours as in batch_stream"""
    rng = np.random.default_rng(seed)
    K = len(counts)
    firsts = np.array([60 + 2 * i for i in range(K)], dtype=np.uint8)
    seconds = firsts + 1
    ml = [3 + (p * 7) % 9 for p in range(K)]
    mr = [3 + (p * 5) % 8 for p in range(K)]
    which = np.concatenate([np.full(counts[p] - ml[p] - mr[p], p, dtype=np.int64) for p in range(K)])
    which = which[rng.permutation(len(which))]
    body = np.stack([firsts[which], seconds[which]], axis=1).ravel()
    extra = []
    for p in range(K):
        extra += [[TL[p % 5], int(firsts[p]), int(seconds[p])]] * ml[p] + [[int(firsts[p]), int(seconds[p]), TR[p % 7]]] * mr[p]
    extra += [[AA, AA]] * 2 + [list(HEAD)] * (max(counts) + 1)
    ex = bytes(b for c in extra for b in c)
    data = body.tobytes() + ex
    offs = np.concatenate([2 * np.arange(len(which), dtype=np.uint64),
                           2 * len(which) + np.cumsum([0] + [len(c) for c in extra[:-1]]).astype(np.uint64)])
    return data, offs, None, list(zip(firsts.tolist(), seconds.tolist())), 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,counts", [
    ("all_above", [17_000] * 31),                  # sixteen replica blocks per pair, 31 pairs: two rounds a thread
    ("one_above", [CH_REP_COUNT + 16] + [13_000] * 30),   # one pair just above the count, the rest far below
    ("at_the_count", [CH_REP_COUNT] * 9),          # four replica blocks: not MORE than the count
])
def test_both_replica_tiers(engine, name, counts):
    K = len(counts)
    if name not in _CACHE:
        _CACHE[name] = tier_stream(counts, 5)
    data, offs, _, listed, n_before = _CACHE[name]
    nm = 1 + K + 12
    exp = expected(name, data, offs, nm)
    assert sorted(exp[0][1:1 + K]) == sorted(listed) and sorted(exp[1][1:1 + K]) == sorted(counts)
    res, s = train(engine, data, offs, 1 + K, (("small_slots", 2),))
    assert same(res, (exp[0][:1 + K], exp[1][:1 + K], exp[2][:1 + K])), name
    assert s["steps"] == 1, (name, "the batch did not form", s["steps"])
    res, s = train(engine, data, offs, nm, (("small_slots", 2),))
    assert same(res, exp), name


@pytest.mark.gpu
def test_weighted_chunks_at_31(engine):
    st = stream("weighted", 31, seed=7, weighted=True)
    exp, s = check(engine, "weighted", st, 31, (("small_slots", 2),), exps=st[5])
    assert exp[1][1] == 40  # (twenty sites of weight 2)
