"""Sharded training (dp_train_loop in api_rccl.hip, the per-merge bpe_dp_select / merge / apply protocol) on the shards
a friendly corpus never makes: empty ranks, ranks without a pair, shards of very different size, ties whose first
occurrences are spread over the ranks, rank numbers up to 1023, a rank that objects (short slots about), levels of more
than TIE_CAP tied pairs, hand-set weight exponents, rank-local options that differ between the ranks.  Several ranks
are emulated on one GPU by the two drivers of test_gpu_parity.py (_chain_ranks: bpe_dp_train_cb, one thread per rank;
_lockstep: the per-merge protocol through GpuShard), the all-reduces are done on the host.

The loop's contract: "Rank-local choices (re-packing, sparse or dense pass, index builds) change which kernels a rank
runs, never what is exchanged."  Integer work: every comparison is exact.

References, computed on the host once per corpus (_REF):
  R1  oracle.train on the concatenation of the shards in rank order (weights = 2^e where chunks carry exponents):
      pairs and counts;
  R3  per rank, R1's pairs replayed over that rank's resident shard with oracle.merge_chunks: the rank's final ids, its
      final chunk starts and its resident length after every merge.
Every case asserts on every rank: pairs, counts and n_done equal R1; lens[i] = the sum over the ranks of R3's lengths
after merge i; where the oracle runs out of pairs, ValueError (status BPE_E_EMPTY_STATS in the per-merge protocol) on
every rank at the same merge; after a run that went to the end, read_ids(), read_chunk_starts() and len() equal R3 and
no id carries weight bits; the same number of collectives on every rank (asserted inside _chain_ranks).

Every corpus builder has a test without the gpu mark that asserts, on the CPU, the property its cases rely on."""
import random

import numpy as np
import pytest

import oracle
from helpers import chunk_offsets, hand_weighted, ties_chunks
from test_chain_kcap31 import check_ties, tied_stream
from test_gpu_parity import _chain_ranks, _lockstep, _space_chunks

gpu = pytest.mark.gpu
_REF = {}     # references, by case
_CORPUS = {}  # corpora, by builder
WAIT = 30  # seconds a rank waits at a barrier for its peers: a wrong schedule fails the test, it does not stall it
TIE_CAP = 96  # bpe_device.h
EMPTY_STATS = -3  # BPE_E_EMPTY_STATS


# ---------------------------------------------------------------------------
# references

def _resident(native, mine, dedup):
    """(data, offsets) of the stream a rank holds: its chunks, or their de-duplicated form"""
    data, offs = b"".join(mine), chunk_offsets(mine)
    if dedup and mine:
        data, offs, _, _ = native.dedup_chunks(data, offs)
    return data, offs


def _replay(data, offs, pairs):
    """R3 of one rank: (final ids, final chunk starts, resident length after every merge)"""
    ids = np.frombuffer(data, dtype=np.uint8).astype(np.int32)
    if len(ids) == 0:
        return ids, [], [0] * len(pairs)
    off_full = np.append(offs, np.uint64(len(ids)))
    lens = []
    for i, p in enumerate(pairs):
        ids, off_full = oracle.merge_chunks(ids, off_full[:-1], p, 256 + i)
        if off_full[-1] != len(ids) or len(off_full) < 2:  # (never: the terminator is kept)
            raise AssertionError("replay lost the end of the stream")
        lens.append(len(ids))
    starts = sorted(set(int(off_full[c]) for c in range(len(off_full) - 1) if off_full[c + 1] > off_full[c]))
    return ids, starts, lens


def _reference(native, key, shards, nm, weights=None, dedup=False):
    """R1 and every rank's R3 for a list of per-rank chunk lists, computed once per `key`"""
    if key in _REF:
        return _REF[key]
    chunks = [c for mine in shards for c in mine]
    assert chunks and len(chunks[-1]) > 0  # (oracle.train reads a last offset == n as the terminator)
    w = None
    if weights is not None:
        exps = np.concatenate([np.asarray(e, dtype=np.uint64) for e, mine in zip(weights, shards) if mine])
        assert len(exps) == len(chunks)
        w = np.uint64(1) << exps
    r1 = oracle.train(b"".join(chunks), nm, chunk_offsets(chunks), raise_on_empty=False, weights=w)
    ranks = []
    for mine in shards:
        data, offs = _resident(native, mine, dedup)
        ranks.append(_replay(data, offs, r1[0]))
    sums = [sum(r[2][i] for r in ranks) for i in range(len(r1[0]))]
    _REF[key] = dict(pairs=r1[0], counts=r1[1], ranks=ranks, lens=sums, nm=nm)
    return _REF[key]


def _inspect(r, eng):
    return dict(ids=eng.read_ids().copy(), starts=eng.read_chunk_starts().tolist(), n=len(eng))


def _check_state(ref, kept, tag):
    for r, (got, (ids, starts, lens)) in enumerate(zip(kept, ref["ranks"])):
        assert got["n"] == len(ids) == (lens[-1] if lens else len(ids)), (tag, r)
        assert len(got["ids"]) == 0 or int(got["ids"].max()) < (1 << 26), (tag, r)  # (no weight bits leak)
        assert np.array_equal(got["ids"], ids), (tag, r)
        assert got["starts"] == starts, (tag, r)


def _run_chain(native, ref, shards, opts=(), tag=None, **kw):
    """bpe_dp_train_cb on every rank -> the common assertions; returns every rank's train_stats"""
    nm, full = ref["nm"], len(ref["pairs"])
    out, errs, stats, kept = _chain_ranks(native, None, nm, len(shards), opts, shards=shards, inspect=_inspect,
                                          timeout=WAIT, **kw)
    if full < nm:
        assert all(isinstance(e, ValueError) for e in errs), (tag, errs)
    else:
        assert not any(errs), (tag, errs)
    for r, res in enumerate(out):
        print(tag, "rank", r, stats[r])
        assert res["n_done"] == full, (tag, r, res["n_done"], full)
        assert res["pairs"] == ref["pairs"], (tag, r, _first_diff(res["pairs"], ref["pairs"]))
        assert res["counts"] == ref["counts"], (tag, r, _first_diff(res["counts"], ref["counts"]))
        assert res["lens"] == ref["lens"], (tag, r, _first_diff(res["lens"], ref["lens"]))
    if full == nm:
        _check_state(ref, kept, tag)
    return stats


def _run_lockstep(native, ref, shards, slots=2, sparse=1, tag=None, **kw):
    """the per-merge protocol on every rank -> the common assertions (_lockstep itself asserts that the ranks report
    the same pair, count and status at every merge)"""
    nm, full = ref["nm"], len(ref["pairs"])
    pairs, counts, lens, kept, status = _lockstep(native, None, nm, len(shards), slots, sparse=sparse, shards=shards,
                                                  inspect=_inspect, **kw)
    assert len(pairs) == full, (tag, len(pairs), full)
    assert status == (EMPTY_STATS if full < nm else 0), (tag, status)
    assert pairs == ref["pairs"], (tag, _first_diff(pairs, ref["pairs"]))
    assert counts == ref["counts"], (tag, _first_diff(counts, ref["counts"]))
    assert lens == ref["lens"], (tag, _first_diff(lens, ref["lens"]))
    if full == nm:
        _check_state(ref, kept, tag)


def _same_schedule(stats, plain):
    """Rank numbers only have to keep the ranks' order: the reduced keys of ranks (0, 128, 1023) order every level as
    those of ranks (0, 1, 2) do, so the runs take the same steps, defer the same merges and launch the same passes.  A
    rank field that runs into the epoch of a chain key (rank << 33 under an epoch at bit 40) makes a level look as if
    it were of several epochs: the merges stay right -- the step defers, the general path decides -- but not these."""
    for s, p in zip(stats, plain):
        assert s == p, (s, p)


def _first_diff(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"first difference at {k}: got {got[k:k + 3]}, want {want[k:k + 3]} ({len(got)} of {len(want)})"


# ---------------------------------------------------------------------------
# A. shard shapes

A_NM = 200
A_RANKS_1024 = (0, 127, 128, 1023)
A_CASES = ["empty_first", "empty_middle", "empty_last", "two_empty", "one_byte_rank", "two_byte_rank", "split_97_2_1",
           "ranks_to_1023"]


def _a_corpus(native):
    if "A" not in _CORPUS:
        _CORPUS["A"] = _space_chunks(native.synth_text(200_000, 61))
    return _CORPUS["A"]


def _a_shards(native, case):
    chunks = _a_corpus(native)
    n = len(chunks)
    if case == "empty_first":
        return [[], chunks[:n // 2], chunks[n // 2:]]
    if case == "empty_middle":
        return [chunks[:n // 2], [], chunks[n // 2:]]
    if case == "empty_last":
        return [chunks[:n // 2], chunks[n // 2:], []]
    if case == "two_empty":
        return [[], chunks, []]
    if case == "one_byte_rank":
        # the chunks n/2 .. n/2 + 200 cut into one-byte chunks: ids, every position a chunk start, no pair
        mid = b"".join(chunks[n // 2:n // 2 + 200])
        return [chunks[:n // 2], [mid[i:i + 1] for i in range(len(mid))], chunks[n // 2 + 200:]]
    if case == "two_byte_rank":
        i = next(j for j in range(n // 2, n) if len(chunks[j]) == 2)
        return [chunks[:i], [chunks[i]], chunks[i + 1:]]
    if case == "split_97_2_1":
        return [chunks[:n * 97 // 100], chunks[n * 97 // 100:n * 99 // 100], chunks[n * 99 // 100:]]
    if case == "ranks_to_1023":
        return [chunks[n * r // 4:n * (r + 1) // 4] for r in range(4)]
    raise KeyError(case)


@pytest.mark.parametrize("case", A_CASES)
def test_shard_shapes_are_as_stated(native, case):
    chunks = _a_corpus(native)
    shards = _a_shards(native, case)
    sizes = [sum(len(c) for c in mine) for mine in shards]
    total = sum(len(c) for c in chunks)
    assert 150_000 <= total <= 250_000
    assert b"".join(c for mine in shards for c in mine) == b"".join(chunks)
    if case.startswith("empty"):
        assert sorted(sizes)[0] == 0 and sorted(sizes)[1] > total // 3
        assert sizes.index(0) == {"empty_first": 0, "empty_middle": 1, "empty_last": 2}[case]
    elif case == "two_empty":
        assert sizes == [0, total, 0]
    elif case == "one_byte_rank":
        assert sizes[1] > 500 and all(len(c) == 1 for c in shards[1]) and min(sizes) > 500
    elif case == "two_byte_rank":
        assert sizes[1] == 2 and len(shards[1]) == 1 and min(sizes[0], sizes[2]) > total // 10
    elif case == "split_97_2_1":
        assert [round(100 * s / total) for s in sizes] == [97, 2, 1]
        assert sizes[0] > 64 * 1024 and sizes[2] < 4096  # (rank 0 re-packs, rank 2 never does: slot_T > 64 in dp_train_loop)
    else:
        assert len(shards) == 4 and max(sizes) - min(sizes) < total // 50
    ref = _reference(native, ("A", case), shards, A_NM)
    assert len(ref["pairs"]) == A_NM
    assert ref["lens"][-1] == sum(len(r[0]) for r in ref["ranks"])


def _a_kw(case):
    return dict(rank_ids=A_RANKS_1024, nranks=1024) if case == "ranks_to_1023" else {}


@gpu
@pytest.mark.parametrize("case", A_CASES)
def test_shard_shapes_chain_steps(native, case):
    pytest.importorskip("torch")
    shards = _a_shards(native, case)
    ref = _reference(native, ("A", case), shards, A_NM)
    stats = _run_chain(native, ref, shards, tag=case, **_a_kw(case))
    assert all(s["steps"] > 0 for s in stats), stats
    if case == "ranks_to_1023":
        _same_schedule(stats, _run_chain(native, ref, shards, tag="ranks 0 .. 3"))


@gpu
@pytest.mark.parametrize("case", A_CASES)
def test_shard_shapes_per_merge_protocol(native, case):
    pytest.importorskip("torch")
    shards = _a_shards(native, case)
    ref = _reference(native, ("A", case), shards, A_NM)
    _run_lockstep(native, ref, shards, tag=case, **_a_kw(case))


# ---------------------------------------------------------------------------
# B. ties whose first occurrences are spread over the ranks

def _split_ties(chunks, listed, world, seed, early):
    """tied_stream's chunks re-ordered into `world` shards: the first `early` single-site chunks of listed pair i go to
    rank i mod world, whose order is shuffled; everything else that holds a listed pair (its later occurrences, the
    chunks of several sites) forms a later block at the end of the last rank; the filler is dealt round."""
    rng = random.Random(seed)
    index = {p: i for i, p in enumerate(listed)}
    seen = [0] * len(listed)
    main, later, k = [[] for _ in range(world)], [], 0
    for c in chunks:
        c = bytes(c.tolist())
        if len(c) == 2 and tuple(c) in index:
            i = index[tuple(c)]
            seen[i] += 1
            (main[i % world] if seen[i] <= early else later).append(c)
        elif any(tuple(c[j:j + 2]) in index for j in range(len(c) - 1)):
            later.append(c)
        else:
            main[k % world].append(c)
            k += 1
    for m in main:
        rng.shuffle(m)
    rng.shuffle(later)
    main[-1] += later
    return main


def _first_occurrences(shards, listed):
    """{pair: (rank, local position)} of each listed pair's first occurrence, straight from the shards"""
    want = set(listed)
    first = {}
    for r, mine in enumerate(shards):
        ids = np.frombuffer(b"".join(mine), dtype=np.uint8)
        inner = np.ones(max(len(ids) - 1, 0), dtype=bool)  # position q is a pair unless q + 1 starts a chunk
        starts = chunk_offsets(mine).astype(np.int64)
        inner[starts[starts > 0] - 1] = False
        for q in np.flatnonzero(inner):
            p = (int(ids[q]), int(ids[q + 1]))
            if p in want and p not in first:
                first[p] = (r, int(q))
    return first


def _b_corpus(which):
    """(shards of 3 ranks, listed pairs, count, nm)"""
    if ("B", which) in _CORPUS:
        return _CORPUS[("B", which)]
    if which == "wide":  # 40 pairs x 50, the filler over bytes 200 .. 249
        firsts, seconds, count = [60 + 2 * i for i in range(40)], [61 + 2 * i for i in range(40)], 50
        _, _, chunks, listed = tied_stream(firsts, seconds, count, 5, n_adj=300, n_single=6000, n_filler=6000)
        out = _split_ties(chunks, listed, 3, 17, 25), listed, count, 60
    else:  # 120 pairs x 20 over bytes 10 .. 249, no filler: one level of more than TIE_CAP entries
        firsts, seconds, count = [10 + 2 * i for i in range(120)], [11 + 2 * i for i in range(120)], 20
        _, _, chunks, listed = tied_stream(firsts, seconds, count, 6, n_adj=250)
        out = _split_ties(chunks, listed, 3, 18, 10), listed, count, 140
    _CORPUS[("B", which)] = out
    return out


@pytest.mark.parametrize("which", ["wide", "level_over_tie_cap"])
def test_tie_corpus_spreads_first_occurrences_over_the_ranks(native, which):
    shards, listed, count, nm = _b_corpus(which)
    chunks = [c for mine in shards for c in mine]
    assert sum(len(c) for c in chunks) <= 150_000
    check_ties([np.frombuffer(c, dtype=np.uint8).astype(np.int64) for c in chunks], listed, count)
    first = _first_occurrences(shards, listed)
    assert len(first) == len(listed)
    on = [sum(1 for r, _ in first.values() if r == k) for k in range(3)]
    assert min(on) >= 10, on
    order = sorted(listed, key=lambda p: first[p])
    # an ordering by position alone, or by rank alone (ties by the pair's number), gives a different list
    assert sorted(listed, key=lambda p: (first[p][1], first[p][0])) != order
    assert sorted(listed, key=lambda p: (first[p][0], listed.index(p))) != order
    assert any(first[p][1] > first[q][1] for p, q in zip(order, order[1:]) if first[p][0] < first[q][0])
    # every listed pair also occurs on the last rank: the rank that finds a pair first is not the only one that holds it
    last = _first_occurrences([shards[2]], listed)
    assert len(last) == len(listed)
    ref = _reference(native, ("B", which), shards, nm)
    assert len(ref["pairs"]) == nm
    assert ref["pairs"][:len(listed)] == order and set(ref["counts"][:len(listed)]) == {count}
    if which == "level_over_tie_cap":
        assert len(listed) > TIE_CAP


@gpu
def test_split_ties_dp_kcap_1_8_15(native):
    """every step goes through the index (sparse = 2); dp_kcap = 15 is the widest SUM payload"""
    pytest.importorskip("torch")
    shards, listed, count, nm = _b_corpus("wide")
    ref = _reference(native, ("B", "wide"), shards, nm)
    steps = {}
    for kcap in (1, 8, 15):
        stats = _run_chain(native, ref, shards, (("dp_kcap", kcap), ("sparse", 2)), tag=("kcap", kcap))
        assert all(s["steps"] > 0 for s in stats), stats
        assert len({s["steps"] for s in stats}) == 1, stats  # (the step records are replicas)
        steps[kcap] = stats[0]["steps"]
    print("chain steps at dp_kcap 1 / 8 / 15:", steps)
    assert steps[15] < steps[8] < steps[1]


@gpu
@pytest.mark.parametrize("driver", ["chain", "per_merge"])
def test_split_ties_rank_numbers_to_1023(native, driver):
    """rank << 33 in a chain key, rank << 32 in the general path's: ranks 128 and 1023 of 1024"""
    pytest.importorskip("torch")
    shards, listed, count, nm = _b_corpus("wide")
    ref = _reference(native, ("B", "wide"), shards, nm)
    kw = dict(rank_ids=(0, 128, 1023), nranks=1024)
    if driver == "chain":
        opts = (("dp_kcap", 15), ("sparse", 2))
        stats = _run_chain(native, ref, shards, opts, tag=driver, **kw)
        assert all(s["steps"] > 0 for s in stats), stats
        _same_schedule(stats, _run_chain(native, ref, shards, opts, tag="ranks 0, 1, 2"))
    else:
        _run_lockstep(native, ref, shards, sparse=2, tag=driver, **kw)


@gpu
@pytest.mark.parametrize("where", [0, 2])
def test_split_ties_with_an_empty_rank(native, where):
    """an empty rank before / between the ranks that hold the first occurrences: it names the same levels and finds nothing"""
    pytest.importorskip("torch")
    shards, listed, count, nm = _b_corpus("wide")
    shards = shards[:where] + [[]] + shards[where:]
    ref = _reference(native, ("B", "wide", "empty", where), shards, nm)
    assert ref["pairs"] == _reference(native, ("B", "wide"), _b_corpus("wide")[0], nm)["pairs"]
    stats = _run_chain(native, ref, shards, (("dp_kcap", 15), ("sparse", 2)), tag=("empty", where))
    assert all(s["steps"] > 0 for s in stats), stats


@gpu
@pytest.mark.parametrize("kcap", [15, 8])
def test_level_of_more_than_tie_cap_pairs_sharded(native, kcap):
    pytest.importorskip("torch")
    shards, listed, count, nm = _b_corpus("level_over_tie_cap")
    ref = _reference(native, ("B", "level_over_tie_cap"), shards, nm)
    stats = _run_chain(native, ref, shards, (("dp_kcap", kcap), ("sparse", 2)), tag=("over", kcap))
    assert all(s["steps"] > 0 for s in stats), stats


# ---------------------------------------------------------------------------
# C. one rank objects

C_NM = 60
C_RUN = b"ab" * 512


def _c_corpus(objector, control=False):
    """(shards of 2 ranks, exponents, listed pairs, index of the run's chunk in the objector's shard).  The listed pairs
    (bytes 100 .. 179) tie at 50; rank `objector`'s shard starts with exactly 1024 filler bytes (512 two-byte chunks
    over bytes 200 .. 249: pairs that count a few), then one chunk "ab" x 512 with exponent 10 -- ids 1024 .. 2047, the
    whole of slot 1 of the 1024-id slots the shard is loaded into.  control: the run is the shard's last chunk instead
    (it covers no whole slot, and the last slot raises no flag)."""
    key = ("C", objector, control)
    if key in _CORPUS:
        return _CORPUS[key]
    firsts, seconds = [100 + 2 * i for i in range(40)], [101 + 2 * i for i in range(40)]
    _, _, chunks, listed = tied_stream(firsts, seconds, 50, 8, n_adj=300, n_single=1500, n_filler=1500)
    shards = _split_ties(chunks, listed, 2, 19, 25)
    rng = random.Random(23)
    filler = [bytes([rng.randrange(200, 250), rng.randrange(200, 250)]) for _ in range(512)]
    mine = shards[objector]
    shards[objector] = filler + mine + [C_RUN] if control else filler + [C_RUN] + mine
    at = len(shards[objector]) - 1 if control else 512
    exps = [np.zeros(len(s), dtype=np.uint8) for s in shards]
    exps[objector][at] = 10
    _CORPUS[key] = shards, exps, listed, at
    return _CORPUS[key]


@pytest.mark.parametrize("objector", [0, 1])
def test_objection_corpus_collapses_slot_1_before_the_ties(native, objector):
    """st->gap is raised by the merge passes when a slot other than the last keeps fewer than 3 ids (k_slots2.hip,
    k_chain.hip: `total < 3 && t + 1 < Tl`) and cleared only by k_slot2_init, i.e. by a re-pack: dp_train_loop re-packs
    when `slot_T > 64 && n * den < slot_T * ts * (den - 1)` -- never for a shard of at most 64 slots, which this one
    is -- and plan_pass2 re-packs into 256-id slots only with small_slots = 2 or above 16 Ki slots.  So the flag stands
    through the tied phase, the objector's k_pool_sel sets dpkey[1] = -1 at every level it is asked to order, and
    k_pool_sel_dp leaves those levels without an order on EVERY rank: the step defers, the general path decides."""
    shards, exps, listed, at = _c_corpus(objector)
    mine = shards[objector]
    assert sum(len(c) for c in mine[:at]) == 1024 and mine[at] == C_RUN and len(C_RUN) == 1024
    assert 2048 + 1024 < sum(len(c) for c in mine) <= 64 * 1024  # (slots after slot 1; at most 64 slots: no re-pack)
    ref = _reference(native, ("C", objector), shards, C_NM, weights=exps)
    assert len(ref["pairs"]) == C_NM
    # the run's pairs win the first ten merges: (a, b), then nine a == b merges, 512 ids down to one
    assert ref["pairs"][0] == (97, 98) and all(a == b for a, b in ref["pairs"][1:10])
    assert ref["counts"][:10] == [512 << 10] + [((512 >> i) - 1) << 10 for i in range(9)]
    # replay on the objector's shard: the ids that came from positions [1024, 2048) after merge k
    ids = np.frombuffer(b"".join(mine), dtype=np.uint8).astype(np.int32)
    off = np.append(chunk_offsets(mine), np.uint64(len(ids)))
    k = None
    for i, p in enumerate(ref["pairs"][:12]):
        ids, off = oracle.merge_chunks(ids, off[:-1], p, 256 + i)
        if k is None and int(off[at + 1] - off[at]) < 3:
            k = i
            assert int(off[at]) == 1024  # (nothing in front of the run has merged)
    assert k is not None and k <= 9
    # ... and at that point every listed tie is still unmerged
    assert set(ref["pairs"][k + 1:k + 1 + 40]) >= set(listed[:20]) and not set(ref["pairs"][:k + 1]) & set(listed)
    assert sorted(ref["pairs"][10:50]) == sorted(listed) and set(ref["counts"][10:50]) == {50}
    # the control: the same merges in the same order, the run in no slot of its own
    cshards, cexps, _, cat = _c_corpus(objector, control=True)
    cref = _reference(native, ("C", objector, "control"), cshards, C_NM, weights=cexps)
    start = sum(len(c) for c in cshards[objector][:cat])
    assert start % 1024 != 0 and start + 1024 == sum(len(c) for c in cshards[objector])  # (the run straddles the last two slots)
    assert cref["pairs"][:10] == ref["pairs"][:10]


@gpu
@pytest.mark.parametrize("objector", [0, 1])
def test_one_rank_objects_and_nobody_orders_the_level(native, objector):
    """objector = 0 is the sharper one: rank 0 holds the global first occurrence of every pair it holds, and writes no
    position while it objects -- a k_pool_sel_dp that went on ordering the level by rank 1's positions alone would
    merge in rank 1's order.  The control run has the same a == b deferrals and no objection: fewer deferrals."""
    pytest.importorskip("torch")
    shards, exps, listed, at = _c_corpus(objector)
    ref = _reference(native, ("C", objector), shards, C_NM, weights=exps)
    stats = _run_chain(native, ref, shards, weights=exps, tag=("objector", objector))
    assert all(s["deferred"] > 0 for s in stats), stats
    cshards, cexps, _, _ = _c_corpus(objector, control=True)
    cref = _reference(native, ("C", objector, "control"), cshards, C_NM, weights=cexps)
    cstats = _run_chain(native, cref, cshards, weights=cexps, tag=("control", objector))
    print("deferred with / without the objection:", [s["deferred"] for s in stats], [s["deferred"] for s in cstats])
    assert len({s["deferred"] for s in stats}) == 1 and len({s["deferred"] for s in cstats}) == 1
    assert stats[0]["deferred"] > cstats[0]["deferred"]


# ---------------------------------------------------------------------------
# D. hand-weighted shards

D_NM = 300


def _d_corpus():
    """W_hand (helpers.hand_weighted(3000, 24, 12, seed=7)) cut into 3 ranks at chunk indices: the first cut directly
    before an aligned exponent-24 chunk, the 2500-id run on rank 1, the second cut between two empty chunks -- W_hand
    has no two empty chunks in a row, so one more empty chunk (exponent 5) is put next to the one the cut follows."""
    if "D" in _CORPUS:
        return _CORPUS["D"]
    data, offs, exps, edges = hand_weighted(3000, 24, 12, seed=7)
    ends = np.append(offs[1:], np.uint64(len(data))).astype(np.int64)
    chunks = [data[int(a):int(b)] for a, b in zip(offs.astype(np.int64), ends)]
    run = edges["run"]
    cut1 = max(i for _, i in edges["aligned"] if i < run)
    e2 = min(i for i in edges["empties"] if i > run)
    chunks.insert(e2 + 1, b"")
    exps = np.insert(exps, e2 + 1, 5)
    cut2 = e2 + 1
    shards = [chunks[:cut1], chunks[cut1:cut2], chunks[cut2:]]
    wexp = [exps[:cut1], exps[cut1:cut2], exps[cut2:]]
    _CORPUS["D"] = shards, wexp, edges, (cut1, cut2), (data, offs)
    return _CORPUS["D"]


def test_hand_weighted_cuts_are_where_they_should_be(native):
    shards, wexp, edges, (cut1, cut2), (data, offs) = _d_corpus()
    assert b"".join(c for s in shards for c in s) == data and sum(map(len, shards)) == len(offs) + 1
    assert all(len(s) == len(e) for s, e in zip(shards, wexp))
    # rank 1 starts with an aligned exponent-24 chunk that follows an exponent-0 chunk
    assert int(offs[cut1]) % 256 == 0 and wexp[1][0] == 24 and wexp[0][-1] == 0 and len(shards[1][0]) > 1
    assert b"z" * 2500 in shards[1] and wexp[1][shards[1].index(b"z" * 2500)] == 12
    assert shards[1][-1] == b"" and shards[2][0] == b"" and len(shards[2][-1]) > 0
    for s, e in zip(shards, wexp):
        lens = np.array([len(c) for c in s])
        assert ((lens == 1) & (e == 24)).any() and (lens == 0).any() and int(e.max()) == 24 and int(e.min()) == 0
    ref = _reference(native, "D", shards, D_NM, weights=wexp)
    assert len(ref["pairs"]) == D_NM


@gpu
def test_hand_weighted_shards_chain_steps(native):
    pytest.importorskip("torch")
    shards, wexp, _, _, _ = _d_corpus()
    ref = _reference(native, "D", shards, D_NM, weights=wexp)
    stats = _run_chain(native, ref, shards, weights=wexp, tag="hand")
    assert all(s["steps"] > 0 for s in stats), stats


@gpu
@pytest.mark.parametrize("slots", [1, 2])
def test_hand_weighted_shards_per_merge_protocol(native, slots):
    pytest.importorskip("torch")
    shards, wexp, _, _, _ = _d_corpus()
    ref = _reference(native, "D", shards, D_NM, weights=wexp)
    _run_lockstep(native, ref, shards, slots, weights=wexp, tag=("hand", slots))


def _d_ties():
    chunks = ties_chunks(600, 9)
    return [chunks[:300], [], chunks[300:]]


def test_exhaustion_corpus_runs_out_with_an_empty_rank(native):
    shards = _d_ties()
    assert [len(s) for s in shards] == [300, 0, 300]
    ref = _reference(native, "D_ties", shards, 400, dedup=True)
    assert 0 < len(ref["pairs"]) < 400
    data, offs = b"".join(shards[0]), chunk_offsets(shards[0])
    assert len(native.dedup_chunks(data, offs)[1]) < len(offs)  # (the ranks' de-duplication does something)


@gpu
@pytest.mark.parametrize("driver", ["chain", "per_merge"])
def test_exhaustion_with_an_empty_rank_and_per_rank_dedup(native, driver):
    pytest.importorskip("torch")
    shards = _d_ties()
    ref = _reference(native, "D_ties", shards, 400, dedup=True)
    if driver == "chain":
        _run_chain(native, ref, shards, dedup=True, tag="ties")
    else:
        _run_lockstep(native, ref, shards, dedup=True, tag="ties")


# ---------------------------------------------------------------------------
# E. rank-local options differ between the ranks

E_SETS = [(("sparse", 2), ("small_slots", 2), ("chain_prefetch", 0), ("lean_grid", 8)),
          (("sparse", 0), ("aa_sparse", 0), ("count_is_removed", 0)),
          (("chain_scan", 1), ("repack_acc", 0))]


@gpu
@pytest.mark.parametrize("turn", [0, 1, 2])
def test_rank_local_options_differ_between_the_ranks(native, turn):
    """Read off dp_train_loop, bpe_dp_select / merge and launch_chain_step:
    rank-local (they change which kernels a rank launches, their grids and its slot geometry; nothing that is exchanged):
      sparse 0 / 1 / 2 (plan_pass2: sparse or dense pass; the index is built for the ties whatever it says),
      small_slots 0 / 1 / 2 (plan_pass2 re-packs into 256-id slots when a pass goes sparse: honoured by the sharded loop),
      chain_prefetch, lean_grid, chain_scan (grids and loads of the merge pass and the pool rebuild),
      aa_sparse (a == b passes through the index or over every slot), count_is_removed (sharded steps always count the
      removed ids), repack_acc (the single-GPU loop's policy: the sharded loop re-packs at a fill of 31/32, 7/8 with an index),
      fuse_step (off while a communicator is set), rep_min / rep_max (replicas of the delta buffer, folded before the SUM).
    global (every rank must set the same: they decide which unit comes next, a payload's size or the replicated pool):
      dp_kcap and chain_kcap (batch size, the SUM payload), lean_count, lean, chain, chain_dense, lean_select, tie_index,
      lds_delta (which kind of unit), depth (how many units are enqueued behind a deferral: their collectives),
      lean_backoff (the stretch a deferral hands to the general path), pool_hint (when the replicated pool is rebuilt),
      mode / slots / merge (refused unless 1 / 2 / 0).
    The 97 / 2 / 1 split: rank 0 holds more than 64 slots (it re-packs), ranks 1 and 2 never do."""
    pytest.importorskip("torch")
    shards = _a_shards(native, "split_97_2_1")
    ref = _reference(native, ("A", "split_97_2_1"), shards, A_NM)
    sets = E_SETS[turn:] + E_SETS[:turn]
    stats = _run_chain(native, ref, shards, rank_opts=sets, tag=("turn", turn))
    for s, o in zip(stats, sets):
        assert s["steps"] > 0, (o, s)
        if ("sparse", 2) in o:
            assert s["sparse"] > 0 and s["dense"] <= 1 and s["slot_ids"] == 256, (o, s)  # (dense: merge 0, before any count is known)
        if ("sparse", 0) in o:
            assert s["sparse"] == 0 and s["dense"] > 0 and s["slot_ids"] == 1024, (o, s)


# ---------------------------------------------------------------------------
# F. nothing stays behind

def _solo_after(ref, whole, wexp, nm):
    """inspect callback: rank 0's engine, straight after its sharded run, on the whole corpus by itself -- train(), then
    bpe_dp_train_cb as a world of one whose all-reduce is the identity"""
    def inspect(r, eng):
        got = _inspect(r, eng)
        if r == 0:
            data, offs = b"".join(whole), chunk_offsets(whole)
            eng.load_bytes(data, offs, wexp)
            got["train"] = eng.train(nm)
            eng.load_bytes(data, offs, wexp)
            got["solo"] = eng.dp_train_cb(nm, 0, 1, lambda ptr, count, dtype, op, stream: None)
        return got
    return inspect


@gpu
@pytest.mark.parametrize("which", ["ties", "hand"])
def test_nothing_of_a_sharded_run_stays_behind(native, which):
    pytest.importorskip("torch")
    if which == "ties":
        shards, listed, count, nm = _b_corpus("wide")
        ref = _reference(native, ("B", "wide"), shards, nm)
        opts, weights, wexp = (("dp_kcap", 15), ("sparse", 2)), None, None
    else:
        shards, weights, _, _, _ = _d_corpus()
        nm = D_NM
        ref = _reference(native, "D", shards, nm, weights=weights)
        opts, wexp = (), np.concatenate(weights)
    whole = [c for s in shards for c in s]
    out, errs, stats, kept = _chain_ranks(native, None, nm, 3, opts, shards=shards, weights=weights, timeout=WAIT,
                                          inspect=_solo_after(ref, whole, wexp, nm))
    assert not any(errs)
    assert all(res["pairs"] == ref["pairs"] for res in out)
    for name in ("train", "solo"):
        res = kept[0][name]
        assert res["pairs"] == ref["pairs"] and res["counts"] == ref["counts"] and res["lens"] == ref["lens"], name
