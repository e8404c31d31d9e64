"""Chain steps of up to 31 pairs (CH_KSWEEP = 31): the merge pass keeps "which pair is this word a site of, + 1" in a BYTE
per word (merge_chain_wave, minbpe_amd/csrc/kernels/k_chain.hip; a nibble and 15 pairs before), the selection hands out up
to 31 pairs (k_pool.hip) and the table update loops over them.

The streams here are built so that MANY pairs tie at the maximum without sharing a token that would end the batch: every
listed pair (a_i, b_i) occurs exactly C times, its occurrences kept apart by chunk boundaries, and nothing else reaches C.
The reference then merges the listed pairs in order of first occurrence, and the engine may take up to 31 of them in one
step.  Chunks of two and three sites in a row (a_i b_i a_j b_j ...) put a site directly after a site of the same pair
(format B's adj), of a lower-numbered and of a higher-numbered pair of the batch; single-byte chunks between them shift the
parity, so that sites start on every position of a slot -- its first word, its last two words, across its end.  What is
compared is always pairs, counts and lens against oracle.train.

CPU side: the pool model (tests/test_pool_model.py) and the level model (tests/test_level_model.py) at a cap of 31, on the
cases they already run, and the pool model's batch on the streams of this file (the input must form a batch of more than
15 before the GPU is asked to)."""
import random

import numpy as np
import pytest

import oracle
import test_level_model
import test_pool_model
from helpers import reset_variant, set_variant
from test_list_model import STREAMS, table_of

KCAP = 31  # CH_KSWEEP


def tied_stream(firsts, seconds, count, seed, hot=(), n_adj=0, n_single=0, n_filler=0):
    """(data, offsets, chunks as int64 arrays, the listed pairs): pair i = (firsts[i], seconds[i]) occurs exactly `count`
    times.  hot = [(i, j, reps)]: the chunk a_i b_i a_j b_j `reps` times (the pair (b_i, a_j) then counts reps: below
    `count`, but high enough to sit in the pool while the batch is merged); n_adj chunks of two or three sites of random
    listed pairs in a row; the rest of every pair's occurrences as two-byte chunks; n_single one-byte chunks and n_filler
    three-byte chunks over an alphabet of their own (bytes 200..249: pairs that count a dozen at most)."""
    rng = random.Random(seed)
    n = len(firsts)
    left = [count] * n
    chunks = []

    def site(i):
        left[i] -= 1
        return [firsts[i], seconds[i]]

    for i, j, reps in hot:
        for _ in range(reps):
            chunks.append(site(i) + site(j))
    for _ in range(n_adj):
        k = rng.choice([2, 2, 3])
        idx = [rng.randrange(n) for _ in range(k)]
        if rng.random() < 0.2:
            idx[1] = idx[0]  # the same pair twice in a row
        if all(left[i] - idx.count(i) >= 0 for i in idx):
            chunks.append(sum((site(i) for i in idx), []))
    assert min(left) >= 0
    for i in range(n):
        chunks += [[firsts[i], seconds[i]] for _ in range(left[i])]
    chunks += [[rng.randrange(200, 250)] for _ in range(n_single)]
    chunks += [[rng.randrange(200, 250) for _ in range(3)] for _ in range(n_filler)]
    rng.shuffle(chunks)
    data = bytes(b for c in chunks for b in c)
    offs = np.cumsum([0] + [len(c) for c in chunks[:-1]]).astype(np.uint64)
    return data, offs, [np.array(c, dtype=np.int64) for c in chunks], list(zip(firsts, seconds))


def check_ties(chunks, listed, count):
    """the listed pairs count exactly `count`, everything else less"""
    table = table_of(chunks)
    for p in listed:
        assert table[p] == count, (p, table[p])
    assert max(c for p, c in table.items() if p not in set(listed)) < count


def model_batch(chunks, cap):
    """the first batch the pool model takes off this stream"""
    pool = test_pool_model.Pool(cap, 256, 6, random.Random(1))
    pool.rebuild(chunks)
    batch, _, _ = pool.batch(chunks, 10 ** 6)
    return batch


def train_with(engine, data, offs, nm, kcap, extra=()):
    set_variant(engine, 1, 0, 2, 2, 7)  # every merge after the first a chain step through the index
    try:
        engine.set_option("chain_kcap", kcap)
        for k, v in extra:
            engine.set_option(k, v)
        engine.load_bytes(data, offs)
        res = engine.train(nm)
        return res, engine.train_stats()
    finally:
        engine.set_option("chain_kcap", KCAP)
        engine.set_option("small_slots", 1)
        reset_variant(engine)


def same(res, exp):
    return res["pairs"] == exp[0] and res["counts"] == exp[1] and res["lens"] == exp[2]


# ---------------------------------------------------------------------------
# wide batches: 40 pairs of 80 distinct bytes, 50 occurrences each

def wide_stream():
    firsts = [60 + 2 * i for i in range(40)]
    seconds = [61 + 2 * i for i in range(40)]
    return tied_stream(firsts, seconds, 50, 5, n_adj=300, n_single=6000, n_filler=6000)


def test_wide_stream_forms_a_batch_of_more_than_15_on_the_cpu():
    data, offs, chunks, listed = wide_stream()
    assert 20_000 <= len(data) <= 50_000
    check_ties(chunks, listed, 50)
    assert len(set(sum(listed, ()))) == 80
    assert len(model_batch(chunks, KCAP)) == KCAP
    assert len(model_batch(chunks, 15)) == 15


@pytest.mark.gpu
def test_wide_batches_take_fewer_steps_and_give_the_same_merges(engine):
    data, offs, chunks, listed = wide_stream()
    nm = 60
    exp = oracle.train(data, nm, offs)
    # the reference merges the 40 tied pairs in order of first occurrence
    assert sorted(exp[0][:40]) == sorted(listed) and set(exp[1][:40]) == {50}
    wide, st_wide = train_with(engine, data, offs, nm, KCAP)
    narrow, st_narrow = train_with(engine, data, offs, nm, 15)
    print("chain steps at kcap 31 / 15:", st_wide["steps"], st_narrow["steps"])
    assert same(wide, exp)
    assert same(narrow, exp)
    assert wide["pairs"] == narrow["pairs"] and wide["counts"] == narrow["counts"] and wide["lens"] == narrow["lens"]
    assert 0 < st_wide["steps"] < st_narrow["steps"]


# ---------------------------------------------------------------------------
# codes above 15 at every position the window reads

def dense_stream():
    """64 tied pairs, most of the stream sites: two batches of 31 and more whatever the first merges are; a site starts on
    about every third word"""
    firsts = [64 + 2 * i for i in range(64)]
    seconds = [65 + 2 * i for i in range(64)]
    return tied_stream(firsts, seconds, 250, 9, n_adj=5000, n_single=5000, n_filler=1500)


def test_dense_stream_puts_high_codes_on_every_position_a_slot_reads():
    """Nominal layout (slots filled at load, S ids each; the handful of ids the merges before a batch remove moves a site
    by a word or two, which the counts below leave room for): sites of pairs that stand at index 16 or above in a batch
    of 31 -- the listed pairs 16 .. 30 and 47 .. 61 in order of first occurrence, give or take the first merge -- on a
    slot's first word, on its last two words and across its end, and directly after a site of the same / a lower / a
    higher pair."""
    data, offs, chunks, listed = dense_stream()
    check_ties(chunks, listed, 250)
    assert len(model_batch(chunks, KCAP)) == KCAP
    exp = oracle.train(data, 64, offs)
    rank = {p: i for i, p in enumerate(exp[0])}
    assert sorted(rank) == sorted(listed)
    high = {p for p, r in rank.items() if 17 <= r % 31 <= 29 and r < 62}  # (index >= 16 whether or not merge 0 goes alone)
    ids = np.frombuffer(data, dtype=np.uint8)
    starts = np.zeros(len(ids) + 1, dtype=bool)
    starts[np.asarray(offs, dtype=np.int64)] = True
    starts[len(ids)] = True
    site = [q for q in range(len(ids) - 1) if not starts[q + 1] and (int(ids[q]), int(ids[q + 1])) in high]
    for S in (256, 1024):
        first = sum(1 for q in site if q % S == 0)
        last2 = sum(1 for q in site if q % S == S - 2)
        across = sum(1 for q in site if q % S == S - 1)
        after_across = sum(1 for q in site if q % S == 1)  # (its left neighbour may end a site that began in the slot before)
        print(f"S = {S}: high-code sites on the first word {first}, the last two words {last2}, across the end {across}, "
              f"second word {after_across}")
        assert min(first, last2, across, after_across) >= 3, (S, first, last2, across, after_across)
    # neighbours: the site before / after in the same chunk is of the same, a lower or a higher pair of the same batch of 31
    both = lambda q: (int(ids[q]), int(ids[q + 1]))
    sset = set(site)
    same_p = lower = higher = 0
    for q in site:
        if q >= 2 and not starts[q] and not starts[q - 1] and both(q - 2) in rank:
            r0, r1 = rank[both(q - 2)], rank[both(q)]
            if (r0 - 1) // 31 == (r1 - 1) // 31 and r0 // 31 == r1 // 31:
                same_p += r0 == r1
                lower += r0 < r1
                higher += r0 > r1
    print("high-code sites directly after a site of the same / a lower / a higher pair:", same_p, lower, higher)
    assert min(same_p, lower, higher) >= 20
    assert len(sset) > 3000


@pytest.mark.gpu
@pytest.mark.parametrize("small_slots", [0, 2])
def test_high_codes_at_slot_edges_and_next_to_other_sites(engine, small_slots):
    """both slot geometries: 1024-id slots throughout / 256-id slots from the first index build"""
    data, offs, chunks, listed = dense_stream()
    nm = 100
    exp = oracle.train(data, nm, offs)
    res, st = train_with(engine, data, offs, nm, KCAP, (("small_slots", small_slots),))
    assert same(res, exp)
    assert st["slot_ids"] == (1024 if small_slots == 0 else 256)
    assert st["steps"] > 0


# ---------------------------------------------------------------------------
# the first-token look-up table's fallback: ids 0 and 1 fall into bucket 0 under every multiplier
# ((id * m >> 8) & 255 with m < 256), so a batch that holds both has no collision-free table and compares

@pytest.mark.gpu
def test_batch_of_31_whose_first_tokens_defeat_every_multiplier(engine):
    firsts = [40] + list(range(0, 32))
    seconds = [100 + i for i in range(33)]
    data, offs, chunks, listed = tied_stream(firsts, seconds, 40, 3, n_adj=250, n_single=3000, n_filler=3000)
    # (40, 100) comes first and is the first merge; ids 0 and 1 follow it, next to each other in every batch
    first_chunks = bytes([40, 100, 0, 101, 1, 102])
    data = first_chunks + data
    offs = np.concatenate([np.array([0, 2, 4], dtype=np.uint64), offs + np.uint64(6)])
    for m in range(129, 256, 2):
        assert (0 * m >> 8) & 255 == (1 * m >> 8) & 255
    nm = 50
    exp = oracle.train(data, nm, offs)
    assert exp[0][:3] == [(40, 100), (0, 101), (1, 102)] and exp[1][:33] == [41] * 3 + [40] * 30
    res, st = train_with(engine, data, offs, nm, KCAP)
    narrow, st_narrow = train_with(engine, data, offs, nm, 15)
    assert same(res, exp)
    assert same(narrow, exp)
    assert st["steps"] <= st_narrow["steps"]


# ---------------------------------------------------------------------------
# shared second tokens above index 15 (round 6's rule meets the wide codes)

def shared_stream():
    firsts = [60 + i for i in range(40)]
    seconds = [120 + i % 4 for i in range(40)]
    # (b, a_j) pairs that count 40: in the pool while the batches are merged -- x = b is the second token of several
    # batch pairs, also of pairs at index 16 and above (k_pool.hip: the variants (Z_p, y), one per such pair)
    hot = [(2 * k, 2 * k + 1, 40) for k in range(6, 20)]
    return tied_stream(firsts, seconds, 60, 7, hot=hot, n_adj=200, n_single=5000, n_filler=5000)


def test_shared_stream_forms_a_batch_of_31_with_shared_second_tokens_on_the_cpu():
    data, offs, chunks, listed = shared_stream()
    check_ties(chunks, listed, 60)
    batch = model_batch(chunks, KCAP)
    assert len(batch) == KCAP and len({b for _, b in batch}) == 4


@pytest.mark.gpu
def test_shared_second_tokens_above_index_15(engine):
    data, offs, chunks, listed = shared_stream()
    nm = 90
    exp = oracle.train(data, nm, offs)
    assert sorted(exp[0][:40]) == sorted(listed)
    res, st = train_with(engine, data, offs, nm, KCAP)
    narrow, st_narrow = train_with(engine, data, offs, nm, 15)
    print("chain steps at kcap 31 / 15:", st["steps"], st_narrow["steps"])
    assert same(res, exp)
    assert same(narrow, exp)
    assert st["steps"] < st_narrow["steps"]


# ---------------------------------------------------------------------------
# CPU: the models at a cap of 31, on the cases they already run

@pytest.mark.parametrize("name,k,n", STREAMS)
@pytest.mark.parametrize("capacity,depth", [(96, 6), (40, 40)])
def test_pool_model_at_cap_31(name, k, n, capacity, depth):
    test_pool_model.test_pool_steps_are_the_references_merges(name, k, n, KCAP, capacity, depth, 11)


def test_level_model_at_cap_31():
    test_level_model.test_batches_through_tied_levels_are_the_reference_merges(KCAP)
    test_level_model.test_batches_that_share_second_tokens_are_the_reference_merges(KCAP)
