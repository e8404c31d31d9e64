"""Chain steps whose batch holds a FIRST token twice (option chain_share_first; k_pool.hip: pool_finish and the mirrored
maintenance; k_chain.hip: merge_chain_wave finds a site by its PAIR, one look-up in a table of 8-byte entries) -- against
the CPU oracle, and against the same engine with the option off.

Every case trains one stream of 20-50 KB with chain_share_first = 1 and 0: pairs, counts and lens must be oracle.train's
both times, the run with the option on may not take more chain steps, and on the streams built for it takes strictly fewer
and reports shared_first > 0.  The streams are built like test_chain_kcap31.tied_stream: listed pairs that occur exactly
`count` times and tie at the maximum, so that the reference merges them in order of first occurrence and the engine may take
them in one step -- here with pairs (a, b1) .. (a, b4) among them.  Chunks of two and three sites in a row put "a b1 a b2"
and "a b2 a b1" next to each other (the left and the right neighbour of a site are sites of a sibling with a lower and a
higher number) and the same pair twice in a row (adj); single-byte chunks shift the parity so that sites of every sibling
start on a slot's last word (the carry into the next slot must name the right sibling), on its last two words and on its
first (counted on the CPU below, for both slot sizes).

What the device cannot reach and the CPU model covers instead (tests/test_level_model_shared_firsts.py): an entry with
SEVERAL surviving variants, and more variants than PL_GATHER.  A rebuild's threshold is at least three quarters of the
maximum and only rises afterwards, an entry's variants share its old count among them, so at most ONE variant of an
entry reaches theta on the device -- the test here makes that one the variant the mirrored loops reach last."""
import numpy as np
import pytest

import oracle
from helpers import reset_variant, set_variant
from test_chain_kcap31 import KCAP, check_ties, same, tied_stream

A, B1, B2, B3, B4 = 40, 50, 51, 52, 53
LEAN_COUNT_DEFAULT = 1 << 20
_EXP = {}


def with_head(data, offs, chunks, head=(252, 253), reps=None, count=0):
    """a pair of its own, `count` + 1 times at the END of the stream: it is the first merge (the general path's; every merge
    after it is a chain step) and removes nothing before the sites this file is about -- the slots hold what they held"""
    reps = count + 1 if reps is None else reps
    extra = [list(head)] * reps
    offs = np.concatenate([offs, len(data) + 2 * np.arange(reps, dtype=np.uint64)])
    return data + bytes(b for c in extra for b in c), offs, chunks + [np.array(c, dtype=np.int64) for c in extra]


def fan_stream(count=400, seed=21):
    """(a, b1) .. (a, b4) and eight pairs that share nothing, all tied at `count`"""
    firsts = [A, A, A, A] + [60 + 2 * i for i in range(8)]
    seconds = [B1, B2, B3, B4] + [61 + 2 * i for i in range(8)]
    data, offs, chunks, listed = tied_stream(firsts, seconds, count, seed, n_adj=1200, n_single=8000, n_filler=3500)
    data, offs, chunks = with_head(data, offs, chunks, count=count)
    return data, offs, chunks, listed


def ladder_stream(count=300, seed=27):
    """the fan stream with every listed pair on a level of its own: pair i counts `count` + 12 - i.  A dense step has no
    index to order a tied level by and hands a tie back; levels of one pair each it walks freely -- (a, b1) .. (a, b4) at
    the top, then the pairs that share nothing"""
    firsts = [A, A, A, A] + [60 + 2 * i for i in range(8)]
    seconds = [B1, B2, B3, B4] + [61 + 2 * i for i in range(8)]
    data, offs, chunks, listed = tied_stream(firsts, seconds, count, seed, n_adj=900, n_single=8000, n_filler=3500)
    extra = [[a, b] for i, (a, b) in enumerate(listed) for _ in range(12 - i)]
    offs = np.concatenate([offs, len(data) + 2 * np.arange(len(extra), dtype=np.uint64)])
    data = data + bytes(b for c in extra for b in c)
    chunks = chunks + [np.array(c, dtype=np.int64) for c in extra]
    data, offs, chunks = with_head(data, offs, chunks, count=count + 12)
    return data, offs, chunks, listed


def both_stream():
    """a first and a second token twice in one batch: (a, b), (a, c), (d, c) -- and pairs that share nothing"""
    firsts = [A, A, 45] + [60 + 2 * i for i in range(6)]
    seconds = [B1, B2, B2] + [61 + 2 * i for i in range(6)]
    data, offs, chunks, listed = tied_stream(firsts, seconds, 300, 22, n_adj=700, n_single=7000, n_filler=4000)
    data, offs, chunks = with_head(data, offs, chunks, count=300)
    return data, offs, chunks, listed


def chain_stream():
    """pairs that must still end a batch, in this order of first occurrence (one chunk of every listed pair leads the
    stream): (a, b) then (b, c) and (f, d) then (d, e) -- the later pair's FIRST token is a second token of the batch --,
    (g, h) then (i, g) -- its SECOND token is a first token of the batch; next to pairs that may share"""
    firsts = [A, B1, 47, 45, 90, 92, 70, 70, 80, 82]
    seconds = [B1, 54, 45, 46, 91, 90, 71, 72, 81, 83]
    data, offs, chunks, listed = tied_stream(firsts, seconds, 299, 23, n_single=7000, n_filler=4000)
    lead = [list(p) for p in listed]
    offs = np.concatenate([2 * np.arange(len(lead), dtype=np.uint64), offs + np.uint64(2 * len(lead))])
    data = bytes(b for c in lead for b in c) + data
    chunks = [np.array(c, dtype=np.int64) for c in lead] + chunks
    data, offs, chunks = with_head(data, offs, chunks, count=300)
    return data, offs, chunks, listed


def boundary_stream():
    """the fan stream, and chunks that END in a followed by chunks that START with b2: no site spans them"""
    data, offs, chunks, listed = fan_stream(300, 24)
    extra = [[205, A], [B2, 206]] * 150 + [[A], [B3]] * 100
    offs = np.concatenate([offs, len(data) + np.cumsum([0] + [len(c) for c in extra[:-1]]).astype(np.uint64)])
    data = data + bytes(b for c in extra for b in c)
    return data, offs, chunks + [np.array(c, dtype=np.int64) for c in extra], listed


def maintenance_stream():
    """Two batch pairs end in x, two start with y, and the pool entry (x, y) -- 94 of a maximum of 100 -- stands almost
    wholly inside "q x y s": after the batch (Zqx, Zys) counts 90 and is the next merge but one, between (u, v) at 92 and
    (u2, v2) at 88.  The same with x2, y2 inside "p2 x2 y2 r2" (the FIRST pair on either side).  Whichever single pair per
    token a maintenance looked at, one of the two heirs would be missing from the pool and be merged late."""
    chunks = []

    def group(p, q, x, y, r, s, heavy):
        hl, hr = (q, s) if heavy == "last" else (p, r)
        ol, orr = (p, r) if heavy == "last" else (q, s)
        out = [[hl, x, y, hr]] * 90 + [[ol, x, y, orr]] * 4
        out += [[ol, x]] * 96 + [[hl, x]] * 10 + [[y, orr]] * 96 + [[y, hr]] * 10
        return out

    first = [[1, 3], [2, 3], [4, 5], [4, 6], [11, 13], [12, 13], [14, 15], [14, 16]]  # (the order of first occurrence)
    body = group(1, 2, 3, 4, 5, 6, "last") + group(11, 12, 13, 14, 15, 16, "first")
    for f in first:
        body.remove(f)
    body += [[20, 21]] * 92 + [[22, 23]] * 88 + [[24, 25]] * 91 + [[26, 27]] * 89
    rng = np.random.default_rng(25)
    body += [[int(rng.integers(200, 250))] for _ in range(6000)]
    body += [[int(v) for v in rng.integers(200, 250, 3)] for _ in range(5000)]
    order = rng.permutation(len(body))
    chunks = first + [body[i] for i in order]
    data = bytes(b for c in chunks for b in c)
    offs = np.cumsum([0] + [len(c) for c in chunks[:-1]]).astype(np.uint64)
    data, offs, arrs = with_head(data, offs, [np.array(c, dtype=np.int64) for c in chunks], count=100)
    return data, offs, arrs, [(1, 3), (2, 3), (4, 5), (4, 6), (11, 13), (12, 13), (14, 15), (14, 16)]


def expected(name, data, offs, nm, weights=None):
    """oracle.train, once per stream.  Weighted chunks: the oracle's lengths are those of the text the chunks STAND FOR,
    the engine's those of the resident stream -- the oracle's pairs replayed over the chunks as they are (as
    tests/test_gpu_weighted.py does)"""
    if name not in _EXP:
        pairs, counts, lens = oracle.train(data, nm, offs, weights=weights)
        if weights is not None:
            ids, o, lens = np.frombuffer(data, dtype=np.uint8).astype(np.int32), offs, []
            for i, p in enumerate(pairs):
                ids, off_full = oracle.merge_chunks(ids, o, p, 256 + i)
                o = off_full[:-1]
                lens.append(len(ids))
        _EXP[name] = (pairs, counts, lens)
    return _EXP[name]


def train_opts(engine, data, offs, nm, opts, dense=False, weight_exp=None):
    """sparse: every merge after the first a chain step through the index (variant 7); dense: the default engine with a
    lean_count that keeps a small stream in the dense phase (chain steps of up to six pairs at 1024-id slots)"""
    if dense:
        reset_variant(engine)
        engine.set_option("lean_count", 1)
    else:
        set_variant(engine, 1, 0, 2, 2, 7)
    try:
        engine.set_option("chain_kcap", KCAP)
        for k, v in opts:
            engine.set_option(k, v)
        engine.load_bytes(data, offs, weight_exp)
        res = engine.train(nm)
        return res, engine.train_stats()
    finally:
        for k, v in (("chain_kcap", KCAP), ("small_slots", 1), ("chain_share_first", 1), ("chain_hash_kmin", 0),
                     ("fuse_step", 0), ("lean_count", LEAN_COUNT_DEFAULT)):
            engine.set_option(k, v)
        reset_variant(engine)


def on_and_off(engine, name, stream, nm, opts=(), dense=False, strict=True, weight_exp=None, weights=None):
    data, offs, chunks, listed = stream
    assert 20_000 <= len(data) <= 50_000, len(data)
    exp = expected(name, data, offs, nm, weights)
    on, st_on = train_opts(engine, data, offs, nm, tuple(opts) + (("chain_share_first", 1),), dense, weight_exp)
    off, st_off = train_opts(engine, data, offs, nm, tuple(opts) + (("chain_share_first", 0),), dense, weight_exp)
    print(name, opts, "steps on / off:", st_on["steps"], st_off["steps"], "shared_first:", st_on["shared_first"])
    assert same(on, exp), name
    assert same(off, exp), name
    assert st_off["shared_first"] == 0
    assert 0 < st_on["steps"] <= st_off["steps"]
    if strict:
        assert st_on["steps"] < st_off["steps"] and st_on["shared_first"] > 0, (st_on, st_off)
    return exp, st_on, st_off


# ---------------------------------------------------------------------------
# CPU: the streams tie what they are meant to tie, and the seams occur

def test_fan_stream_ties_siblings_and_puts_them_on_every_seam():
    data, offs, chunks, listed = fan_stream()
    check_ties(chunks[:-401], listed, 400)
    exp = expected("fan", data, offs, 40)
    assert exp[0][0] == (252, 253) and sorted(exp[0][1:13]) == sorted(listed) and set(exp[1][1:13]) == {400}
    ids = np.frombuffer(data, dtype=np.uint8)
    starts = np.zeros(len(ids) + 1, dtype=bool)
    starts[np.asarray(offs, dtype=np.int64)] = True
    starts[len(ids)] = True
    sib = {(A, B1): 0, (A, B2): 1, (A, B3): 2, (A, B4): 3}
    site = {q: sib[(int(ids[q]), int(ids[q + 1]))] for q in range(len(ids) - 1)
            if not starts[q + 1] and (int(ids[q]), int(ids[q + 1])) in sib}
    for S in (256, 1024):
        for name, r in (("first word", 0), ("last two words", S - 2), ("across the end", S - 1)):
            per = [sum(1 for q, k in site.items() if q % S == r and k == want) for want in range(4)]
            print(f"S = {S}: sites of (a, b1..b4) on the slot's {name}: {per}")
            if S == 256:
                assert sum(per[1:]) >= 2 and sum(per) >= 4, (S, name, per)  # (a sibling other than the first among them)
    lower = higher = adj = 0
    for q, k in site.items():
        if q + 2 in site and not starts[q + 2]:
            lower += k < site[q + 2]
            higher += k > site[q + 2]
            adj += k == site[q + 2]
    print("a bi a bj in a row with i < j / i > j / i == j:", lower, higher, adj)
    assert min(lower, higher, adj) >= 10


def test_maintenance_stream_is_what_it_says():
    data, offs, chunks, listed = maintenance_stream()
    exp = expected("maint", data, offs, 20)
    assert exp[0][0] == (252, 253) and exp[0][1:9] == listed and set(exp[1][1:9]) == {100}
    z = {p: 257 + i for i, p in enumerate(listed)}
    heirs = [(z[(2, 3)], z[(4, 6)]), (z[(11, 13)], z[(14, 15)])]
    # (u, v) 92, 24-25 91, the two heirs 90, 26-27 89, (u2, v2) 88: the heirs in the middle of what the pool holds
    assert exp[1][9:15] == [92, 91, 90, 90, 89, 88]
    assert sorted(exp[0][11:13]) == sorted(heirs)


# ---------------------------------------------------------------------------
# GPU

@pytest.mark.gpu
@pytest.mark.parametrize("opts", [
    (("small_slots", 2),),                            # 256-id slots, batches of 12: the table
    (("small_slots", 2), ("chain_kcap", 4)),          # batches of four: the table on a handful of keys
    (("small_slots", 2), ("chain_kcap", 4), ("chain_hash_kmin", 5)),  # ... the small-batch compare path
    (("small_slots", 0),),                            # 1024-id slots, sparse
    (("small_slots", 2), ("chain_hash_kmin", 32)),    # the fall-back of a batch without a multiplier, forced: every batch compares
    (("small_slots", 0), ("chain_hash_kmin", 32)),
], ids=lambda o: "-".join(f"{k}{v}" for k, v in o))
def test_siblings_in_the_sparse_phase(engine, opts):
    exp, st_on, st_off = on_and_off(engine, "fan", fan_stream(), 40, opts)
    assert st_on["slot_ids"] == (256 if ("small_slots", 2) in opts else 1024)


@pytest.mark.gpu
def test_siblings_in_the_dense_phase(engine):
    exp, st_on, st_off = on_and_off(engine, "ladder", ladder_stream(), 13, (("small_slots", 0),), dense=True)
    assert exp[0][1:13] == ladder_stream()[3] and exp[1][1:13] == list(range(312, 300, -1))
    assert st_on["dense"] > 0 and st_on["sparse"] == 0 and st_on["slot_ids"] == 1024, st_on
    assert st_on["steps"] >= 2 and st_on["deferred"] == 0, st_on  # (dense CHAIN steps of up to six pairs, nothing handed back)


@pytest.mark.gpu
@pytest.mark.parametrize("small_slots", [0, 2])
def test_a_first_and_a_second_token_twice_in_one_batch(engine, small_slots):
    stream = both_stream()
    check_ties(stream[2][:-301], stream[3], 300)
    on_and_off(engine, "both", stream, 30, (("small_slots", small_slots),))


@pytest.mark.gpu
def test_pairs_that_chain_still_cut_the_batch(engine):
    """(a, b) then (b, c), and (d, e) then (f, d): never in one batch, whatever the option; (70, 71), (70, 72) may share"""
    stream = chain_stream()
    exp, st_on, st_off = on_and_off(engine, "chain", stream, 24, (("small_slots", 2),), strict=False)
    assert exp[0][1:11] == stream[3] and set(exp[1][1:11]) == {300}
    # (a, b) | (b, c), (f, d) | (d, e), (g, h) | (i, g), ...: the ten tied pairs alone need four batches
    assert st_on["steps"] >= 4


@pytest.mark.gpu
def test_a_chunk_boundary_between_a_and_b2_is_no_site(engine):
    on_and_off(engine, "boundary", boundary_stream(), 40, (("small_slots", 2),))


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True])
def test_siblings_in_weighted_chunks(engine, dense):
    data, offs, chunks, listed = ladder_stream(300, 28) if dense else fan_stream(300, 26)
    rng = np.random.default_rng(3)
    # the listed pairs' chunks all weigh 2 (they still tie), the filler weighs 1, 2 or 4
    e = np.array([1 if int(c[0]) < 200 or int(c[0]) >= 250 else int(rng.integers(0, 3)) for c in chunks], dtype=np.uint8)
    w = (1 << e.astype(np.int64))
    stream = (data, offs, chunks, listed)
    exp, st_on, st_off = on_and_off(engine, "weighted_dense" if dense else "weighted", stream, 13 if dense else 40,
                                    (("small_slots", 0 if dense else 2),), dense=dense, weight_exp=e, weights=w)
    assert exp[1][1:13] == (list(range(624, 600, -2)) if dense else [600] * 12)


@pytest.mark.gpu
@pytest.mark.parametrize("small_slots,kcap", [(0, KCAP), (2, KCAP), (2, 4), (0, 4)])
def test_maintenance_looks_at_every_pair_that_starts_with_y(engine, small_slots, kcap):
    """(a cap of four: the two groups are two batches, and the pool -- never short of four entries -- is maintained from
    the first batch to the heirs' merges; at a cap of 31 a pool of fewer entries than the cap is gathered afresh, which
    finds the heirs whatever the maintenance did)"""
    # (at a cap of four the twenty merges are cap-bound either way: the step counts may be equal)
    on_and_off(engine, "maint", maintenance_stream(), 20, (("small_slots", small_slots), ("chain_kcap", kcap)), strict=kcap == KCAP)


@pytest.mark.gpu
def test_the_one_launch_step_keeps_first_tokens_distinct(engine):
    data, offs, chunks, listed = fan_stream()
    exp = expected("fan", data, offs, 40)
    res, st = train_opts(engine, data, offs, 40, (("small_slots", 2), ("fuse_step", 1), ("chain_kcap", 15)))
    assert same(res, exp)
    assert st["fused_steps"] > 0 and st["shared_first"] == 0, st


@pytest.mark.gpu
def test_a_forced_replay_keeps_first_tokens_distinct(engine):
    """encode_batch of ONE chunk of a megabyte and more replays the merge list through the training engine (k_forced_sel
    forms the batches: distinct first tokens, whatever the option)"""
    data, offs, chunks, listed = fan_stream()
    exp = expected("fan", data, offs, 40)
    text = data * (1 + (1 << 20) // len(data))
    want, _ = oracle.encode(exp[0], text)
    pairs = np.array(exp[0], dtype=np.int32)
    for share in (1, 0):
        engine.set_option("chain_share_first", share)
        try:
            ids, _ = engine.encode_batch(pairs, None, text)
        finally:
            engine.set_option("chain_share_first", 1)
        assert np.array_equal(np.asarray(ids), np.asarray(want)), share
        assert engine.train_stats()["shared_first"] == 0
