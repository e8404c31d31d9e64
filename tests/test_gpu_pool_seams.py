"""Training at the capacity seams of the pool (k_pool.hip; the streams and what each is built to reach: pool_cases.py,
pinned on the CPU by test_pool_cases_cpu.py) against the CPU oracle: pairs, counts, stream lengths, the resident stream
and the chunk starts of every run are oracle.train's and oracle.merge_chunks'.  Integer work: every comparison is exact.

Base setting: every merge after the head a chain step through the index, set_variant(engine, 1, 0, 2, 2, 7), with
lean_backoff = 0 -- a hand-back is followed by exactly one merge of the general path.

What train_stats() must say, read from the code (pool_sel_body, pool_finish, api_train.hip: handle_deferral), not measured:
  within capacity   steps > 0, selections >= 1 (a rebuild selected), deferred == 0;
  over capacity     deferred >= 1 and steps > 0: the chain steps take over again once the general path has merged below the
                    limit.  At the base setting the figure is exact (pool_cases.DEFERRED):
      rows_N            N - 96 for N = 127, 128 and 129 alike.  N rows with one pair each at the maximum are N tied pairs:
                        129 rows leave `ks < 0` (one hand-back), and 128 rows and fewer are gathered but their level is
                        over TIE_CAP, stays without an order, K == 0 -- one hand-back per pair until 96 are left.  No
                        stream can hold 128 rows AT the maximum and stay within TIE_CAP, so rows_127 and rows_128 are
                        over capacity here -- by the other limit;
      rows_depth        4: its 100 rows at the maximum are a level of 100;
      gather_1025       1: `ng > PL_GATHER`; one merge later 1024 pairs are gathered and 256 kept;
      cap_one_level_257 161: the `cut--` loop runs to 0 once (the pool is looked at before the levels), then a level of
                        256 .. 97 is over TIE_CAP;
      tied_97           1, then 96 tied pairs are left and located;
  fused_steps > 0 exactly when fuse_step = 1."""
import numpy as np
import pytest

import oracle
import pool_cases as pc
from helpers import chunk_offsets, reset_variant, set_variant
from test_gpu_sharded_seams import _run_chain

pytestmark = pytest.mark.gpu

# every option a run here sets, with the engine's default (api_ctx.hip)
BASE = {"chain_kcap": pc.CHAIN_KCAP, "chain_share_first": 1, "chain_scan": pc.CHAIN_SCAN, "pool_hint": 0, "depth": 8,
        "chain_hash_kmin": 0, "fuse_step": 0, "small_slots": 1}
NAMES = list(pc.CASES)
# (the issue's list, and rows_depth_all: the one case whose 128 rows are gathered by a rebuild that then selects -- rows at the
# maximum itself are a level over TIE_CAP and hand back; on 127 scanning workgroups and fewer the gather's loop goes round again)
SEAMS = ["rows_128", "rows_129", "rows_depth_all", "gather_1024", "gather_1025", "cap_257", "tied_96", "tied_97",
         "below_reach_17"]
OVER = [n for n in NAMES if pc.CAPACITY[n] == "over"]
SWEEPS = [(k, v) for k, vs in (("chain_kcap", (1, 15, 31)), ("chain_share_first", (0, 1)), ("chain_scan", (1, 3, 127)),
                               ("pool_hint", (0, 1, 128)), ("depth", (0, 8)), ("chain_hash_kmin", (0, 32))) for v in vs]
SHARDED = ["rows_128", "rows_129", "tied_95", "tied_96", "tied_97", "cap_257", "gather_1025"]


def run(engine, name, form, opts=(), forced=True, nm=None, loads=1):
    """load_bytes + train (`loads` times over, from the same bytes) -> [(result, train_stats, ids, chunk starts)]"""
    data, offs = pc.stream(name, form)
    nm = pc.CASES[name].num_merges(form) if nm is None else nm
    out = []
    try:
        if forced:
            set_variant(engine, 1, 0, 2, 2, 7)
        else:
            reset_variant(engine)
        for k, v in tuple(BASE.items()) + (pc.CASES[name].opts if forced else ()) + tuple(opts):
            engine.set_option(k, v)
        for _ in range(loads):
            engine.load_bytes(data, offs)
            res = engine.train(nm)
            out.append((res, engine.train_stats(), engine.read_ids().copy(), engine.read_chunk_starts().tolist()))
    finally:
        for k, v in BASE.items():
            engine.set_option(k, v)
        reset_variant(engine)
    return out


def first_diff(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"first difference at {k}: got {got[k:k + 3]}, want {want[k:k + 3]} ({len(got)} of {len(want)})"


def check_parity(got, exp, tag):
    res, st, ids, starts = got
    pairs, counts, lens, want_ids, want_starts = exp
    assert res["pairs"] == pairs, (tag, first_diff(res["pairs"], pairs), st)
    assert res["counts"] == counts, (tag, first_diff(res["counts"], counts))
    assert res["lens"] == lens, (tag, first_diff(res["lens"], lens))
    assert len(ids) == len(want_ids) and np.array_equal(ids, want_ids), tag
    assert starts == want_starts, tag


def check_stats(name, st, fused, exact, tag):
    assert st["steps"] > 0, (tag, st)
    if pc.CAPACITY[name] == "within":
        assert st["selections"] >= 1 and st["deferred"] == 0, (tag, st)
    else:
        assert st["deferred"] >= 1, (tag, st)
        if exact:
            assert st["deferred"] == pc.DEFERRED[name], (tag, st, pc.DEFERRED[name])
    assert (st["fused_steps"] > 0) == bool(fused), (tag, st)


def test_every_case_states_its_capacity():
    assert set(pc.CAPACITY) == set(NAMES) and all(pc.CAPACITY[n] in ("within", "over") for n in NAMES)
    assert set(pc.DEFERRED) == set(OVER) and set(SEAMS) <= set(NAMES) and set(SHARDED) <= set(NAMES)


@pytest.mark.parametrize("small_slots", [0, 2])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_every_case_at_the_base_setting(engine, name, form, fuse, small_slots):
    tag = (name, form, fuse, small_slots)
    got = run(engine, name, form, (("fuse_step", fuse), ("small_slots", small_slots)))[0]
    print(tag, got[1])
    check_parity(got, pc.expected(name, form), tag)
    check_stats(name, got[1], fuse, True, tag)
    assert got[1]["slot_ids"] == (1024 if small_slots == 0 else 256), got[1]


@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_every_case_at_the_defaults(engine, name, form):
    """no variant forced: whatever the default engine makes of the stream, its merges are the reference's"""
    got = run(engine, name, form, forced=False)[0]
    print(name, form, got[1])
    check_parity(got, pc.expected(name, form), (name, form))


@pytest.mark.parametrize("option,value", SWEEPS)
@pytest.mark.parametrize("name", SEAMS)
def test_option_sweeps_on_the_seam_cases(engine, name, option, value):
    """one option at a time, everything else at the base setting (the body form: merges with neighbours).  What is within
    capacity stays so, and a hand-back stays one, whatever the option: none of them moves a limit."""
    tag = (name, option, value)
    got = run(engine, name, "body", ((option, value),))[0]
    print(tag, got[1])
    check_parity(got, pc.expected(name, "body"), tag)
    check_stats(name, got[1], 0, True, tag)


@pytest.mark.parametrize("fuse", [0, 1])
def test_training_ends_inside_the_first_batch(engine, fuse):
    """tied_96 and ten merges after the head: kmax = min(kcap, num_merges - iter) cuts the walk at 10 of the 96"""
    name, nm = pc.MID_BATCH
    got = run(engine, name, "bare", (("fuse_step", fuse),), nm=nm)[0]
    check_parity(got, pc.expected(name, "bare", nm), (name, nm, fuse))
    check_stats(name, got[1], fuse, True, (name, nm, fuse))
    # the first batch is the last: one step, a rebuild's, whose ten merges needed one selection (api_train.hip: chained += k - 1)
    assert got[1]["steps"] == 1 and got[1]["selections"] == 1 and got[1]["chained"] == nm - 2, got[1]


@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("name", OVER)
def test_a_hand_back_leaves_nothing_behind(engine, name, form):
    """the same bytes loaded and trained twice on one ctx: the second run is the first"""
    first, second = run(engine, name, form, loads=2)
    exp = pc.expected(name, form)
    check_parity(first, exp, (name, form, "first"))
    check_parity(second, exp, (name, form, "second"))
    assert first[1] == second[1], (first[1], second[1])
    check_stats(name, second[1], 0, True, (name, form, "second"))


@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("small,large,field", pc.NEIGHBOURS)
def test_neighbours_back_to_back(engine, small, large, field, order):
    """the two sides of a limit one after the other on one ctx, then the first again: the gather buffer and the pool of
    the larger case do not leak into the smaller"""
    seq = [small, large, small] if order == "up" else [large, small, large]
    seen = {}
    for name in seq:
        got = run(engine, name, "body")[0]
        check_parity(got, pc.expected(name, "body"), (seq, name))
        check_stats(name, got[1], 0, True, (seq, name))
        assert seen.setdefault(name, got[1]) == got[1], (name, seen[name], got[1])


# ---------------------------------------------------------------------------
# sharded: the loop of chain steps on emulated ranks, the all-reduces done on the host (k_pool_sel leaves the MIN payload,
# k_pool_sel_dp finishes the selection from the reduced words).  depth = 0 on every rank: dp_train_loop takes a chain step
# only once the host has read a count (`last_count != ~0ull`), and at the default depth of 8 it has enqueued nine merges
# of the general path by then -- the first rebuild would see 88 of tied_97's pairs.  With depth 0 merge 0 is the head and
# merge 1 a chain step.  lean_backoff stays at its default there: after hand-backs in a row the general path gets a stretch,
# so `deferred` is at least one where a case is over capacity and no exact figure.
DP_OPTS = (("sparse", 2), ("depth", 0))

def _shards(name, split):
    """the bare form's chunks on the ranks.  "one": a world of one.  "both": the stream's first round -- the first
    occurrence of every designed pair, shuffled -- dealt alternately to ranks 0 and 1, the rest cut in half: the tied pairs'
    first occurrences fall on both ranks, and every pair occurs on both.  "empty": everything on rank 0, rank 1 empty."""
    data, offs = pc.stream(name, "bare")
    chunks = pc.chunks_of(data, offs)
    if split == "one":
        return [chunks]
    if split == "empty":
        return [chunks, []]
    n1 = len(pc.CASES[name].pairs)
    rest = chunks[n1:]
    return [chunks[0:n1:2] + rest[:len(rest) // 2], chunks[1:n1:2] + rest[len(rest) // 2:]]


_REF = {}


def _reference(name, split):
    """what test_gpu_sharded_seams._run_chain compares with: oracle.train on the shards laid end to end in rank order
    (pairs, counts; lens: no pair spans a chunk start, so the ranks' lengths add up to the whole stream's), and per rank
    the resident stream and chunk starts those merges leave.  (The gather case by the fast oracle and oracle.encode, as
    pool_cases.expected does.)"""
    if (name, split) not in _REF:
        shards = _shards(name, split)
        chunks = [c for mine in shards for c in mine]
        nm = pc.CASES[name].num_merges("bare")
        big = pc.is_big(name)
        pairs, counts, lens = (oracle.train_fast if big else oracle.train)(b"".join(chunks), nm, chunk_offsets(chunks))
        ranks = []
        for mine in shards:
            if not mine:
                ranks.append((np.zeros(0, np.int32), [], [0]))
                continue
            ids, starts = (pc.replay_by_encode if big else pc.replay)(b"".join(mine), chunk_offsets(mine), pairs)
            ranks.append((ids, starts, [len(ids)]))
        assert sum(len(r[0]) for r in ranks) == lens[-1]
        _REF[(name, split)] = shards, dict(pairs=pairs, counts=counts, ranks=ranks, lens=lens, nm=nm)
    return _REF[(name, split)]


def test_split_puts_first_occurrences_on_both_ranks():
    for name in SHARDED:
        shards = _shards(name, "both")
        designed = set(pc.CASES[name].designed())
        first = {}
        for r, mine in enumerate(shards):
            for c in mine:
                if len(c) == 2 and tuple(c) in designed:
                    first.setdefault(tuple(c), r)
        on = [sum(1 for r in first.values() if r == k) for k in range(2)]
        assert len(first) == len(designed) and min(on) >= len(designed) // 8, (name, on)
        assert sum(map(len, shards)) == len(pc.stream(name, "bare")[1])


@pytest.mark.parametrize("dp_kcap", [1, 8, 15])
@pytest.mark.parametrize("split", ["one", "both"])
@pytest.mark.parametrize("name", SHARDED)
def test_sharded_seams(native, name, split, dp_kcap):
    """tied_96 fills the MIN payload to its last word (DP_KEY_WORDS = TIE_CAP + 2), tied_97 must not write a 99th: its
    level is not located, every rank hands back alike"""
    pytest.importorskip("torch")
    shards, ref = _reference(name, split)
    assert len(ref["pairs"]) == ref["nm"] and sorted(ref["pairs"]) == sorted(pc.expected(name, "bare")[0])
    stats = _run_chain(native, ref, shards, (("dp_kcap", dp_kcap),) + DP_OPTS, tag=(name, split, dp_kcap))
    for st in stats:
        assert st["steps"] > 0, st
        assert (st["deferred"] == 0) == (pc.CAPACITY[name] == "within"), st
    assert len({(st["steps"], st["deferred"]) for st in stats}) == 1, stats  # (the step records are replicas)


@pytest.mark.parametrize("name", SHARDED)
def test_sharded_seams_with_an_empty_rank(native, name):
    """rank 1 holds nothing: it names the same levels and finds no occurrence"""
    pytest.importorskip("torch")
    shards, ref = _reference(name, "empty")
    exp = pc.expected(name, "bare")
    assert ref["pairs"] == exp[0] and ref["counts"] == exp[1]
    stats = _run_chain(native, ref, shards, (("dp_kcap", 15),) + DP_OPTS, tag=(name, "empty"))
    for st in stats:
        assert st["steps"] > 0 and (st["deferred"] == 0) == (pc.CAPACITY[name] == "within"), st
