"""Chain steps that merge a pair with a == b themselves (option chain_aa, k_chain.hip: merge_aa_wave) -- against the CPU
oracle, on 256-id slots with the index live: set_variant(engine, 1, 0, 2, 2, 9).

Every GPU case compares pairs, counts and lens with oracle.train, the resident stream (read_ids) with a replay of
oracle.merge_chunks, and runs with chain_aa = 1 and chain_aa = 0: both must give the oracle's answer, hence each other's.
The cases are built so that the merges that matter are a == b ones and come AFTER the first merge: the first merge of a
train always takes the general path (it needs every row maximum), so each stream starts with a pair (x, y) that outnumbers
everything else, and the cases that count merges run at depth 0 -- the host then knows merge 0 before it enqueues merge
1, and every later merge is a chain step's.  train_stats()["aa_in_chain"] says how many a == b merges the chain steps
did themselves; every case asserts it, so a case that never reached the new pass fails.

The tests WITHOUT the gpu mark check on the CPU, with the oracle alone, that every constructed stream selects a == b
pairs where its case claims them: an input that never selects such a pair would prove nothing."""
import random

import numpy as np
import pytest

import oracle
from helpers import chunk_offsets, reset_variant, set_variant, split_chunks

A, X, Y = 97, 120, 121  # the run symbol; the pair that heads every stream
_REF = {}


def _filler(rng, n, avoid=(A, X, Y)):
    """n bytes of other symbols, no symbol twice in a row: its pairs are rare (asserted by the CPU tests through the
    order of the oracle's merges)"""
    syms = [s for s in range(1, 250) if s not in avoid]
    out, last = [], -1
    for _ in range(n):
        s = rng.choice(syms)
        while s == last:
            s = rng.choice(syms)
        out.append(s)
        last = s
    return bytes(out)


def _case(name, chunks, nm, exps=None, same_from=1, same_to=None):
    """chunks -> a case; merges [same_from, same_to) of the oracle must all have a == b"""
    data = b"".join(chunks)
    return dict(name=name, data=data, offs=chunk_offsets(chunks), nm=nm,
                exps=None if exps is None else np.asarray(exps, dtype=np.uint8), same=(same_from, nm if same_to is None else same_to))


def _xy(n):
    return [bytes([X, Y])] * n


# ---- the streams ------------------------------------------------------------------------------------------------------

def runs_case(length, d):
    """runs of `length` a's starting at ids 256 + d, 512 + d, 768 + d, other bytes around them; a run of 64 a's further on, so
    that (a, a), (Z, Z), (Z', Z'), (Z'', Z'') head the table in turn after (x, y)"""
    rng = random.Random(1000 * length + d + 7)
    body = bytearray(_filler(rng, 1100))
    for b in (256, 512, 768):
        body[b + d:b + d + length] = bytes([A]) * length
    body[900:964] = bytes([A]) * 64
    return _case(f"runs_{length}_{d}", [bytes(body)] + _xy(200), 5)


def whole_slot_case(run, prefix):
    """a run of `run` a's after `prefix` other bytes: the carry through slots that are all one run, in both parities"""
    rng = random.Random(run * 10 + prefix)
    body = _filler(rng, prefix) + bytes([A]) * run + _filler(rng, 20)
    return _case(f"whole_{run}_{prefix}", [body] + _xy(1100), 5)


def chunk_boundary_cases():
    """aaaa split as aa|aa, a|aaa, aaa|a; a chunk boundary exactly at a slot's first word (ids 256 and 512) inside a run"""
    rng = random.Random(5)
    a = lambda n: bytes([A]) * n
    head = [_filler(rng, 30), a(2), a(2), _filler(rng, 9), a(1), a(3), _filler(rng, 11), a(3), a(1)]
    used = sum(len(c) for c in head)
    c1 = head + [_filler(rng, 252 - used), a(4), a(4), _filler(rng, 512 - 260 - 3), a(3), a(5), _filler(rng, 40), a(64)]
    assert sum(len(c) for c in c1[:c1.index(a(4)) + 1]) == 256
    c2 = [_filler(rng, 255), a(1), a(7), _filler(rng, 248), a(8), a(1), a(6), _filler(rng, 30), a(64)]
    assert sum(len(c) for c in c2[:2]) == 256 and sum(len(c) for c in c2[:5]) == 512 + 7
    return [_case("chunks_1", c1 + _xy(200), 5), _case("chunks_2", c2 + _xy(200), 5)]


def weighted_case():
    """weight exponents 0..3 on chunks that hold runs (short ones, and one longer than a slot)"""
    rng = random.Random(11)
    chunks, exps = [], []
    for e in (0, 1, 2, 3):
        for n in (5, 300, 2 + e):
            chunks += [_filler(rng, 17 + e), bytes([A]) * n]
            exps += [e ^ 1, e]
    chunks += [bytes([X, Y])]
    exps += [14]
    return _case("weighted", chunks, 5, exps=exps)


def ties_case(where):
    """(a, a) tied at the maximum with (b, c), (d, e), (f, g), which share no token; the first occurrence of (a, a) comes
    first / in the middle / last.  Single-byte chunks (no pairs) spread the occurrences over several slots."""
    rng = random.Random(20 + where)
    others = [bytes([98, 99]), bytes([100, 101]), bytes([102, 103])]
    first = others[:where] + [bytes([A, A])] + others[where:]
    rest = (others + [bytes([A, A])]) * 9
    rng.shuffle(rest)
    chunks = []
    for c in first + rest:
        chunks += [c] + [bytes([rng.randrange(130, 250)]) for _ in range(19)]
    c = _case(f"ties_{where}", chunks + _xy(200), 5, same_from=1 + where, same_to=2 + where)
    return c


def consecutive_case():
    """an a == b merge directly after a batch -- (b, c) and (d, e) tied above (a, a) -- then (Z, Z), (Z', Z') in the steps
    that follow"""
    rng = random.Random(31)
    chunks = []
    for c in [bytes([98, 99]), bytes([100, 101])] * 40:
        chunks += [c, bytes([rng.randrange(130, 250)])]
    chunks += [_filler(rng, 200), bytes([A]) * 37, _filler(rng, 300), bytes([A]) * 3]
    return _case("consecutive", chunks + _xy(200), 6, same_from=3)


def left_neighbour_case():
    """'q' as the LAST id of a slot, 'aa' as the first two of the next, six times over: the slot that holds q has no (a, a)
    of its own, yet it owes the table (q, a) -> (q, Z) -- the a == b pass charges a pair to its left element, which is why
    a slot is visited when the NEXT one is a candidate.  (q, Z) is the merge after (a, a), with all six of its occurrences
    across a slot boundary: a pass that skips those slots leaves (q, a) at 6 and (q, Z) at 0, and selects the wrong pair."""
    rng = random.Random(41)
    chunks, pos = [], 0
    for k in range(2, 13, 2):  # (every other slot boundary: the slot before a run holds no a at all)
        while pos < 256 * k - 1:  # (single-byte chunks: no pairs)
            chunks.append(bytes([rng.randrange(130, 250)]))
            pos += 1
        chunks.append(bytes([113, A, A]))  # (... this chunk's q)
        pos += 3
    # (more (a, a) than (q, a): ten more after the last run, so that (a, a) comes first)
    chunks += [bytes([A, A])] * 10 + [bytes([rng.randrange(130, 250)]) for _ in range(40)]
    return _case("left_neighbour", chunks + _xy(200), 3, same_from=1, same_to=2)


def realistic_case(native):
    data, offs = split_chunks(native.synth_text(2_000_000, 11).decode())
    return dict(name="synth2mb", data=data, offs=offs, nm=400, exps=None, same=None)


RUN_LENGTHS = range(1, 10)
RUN_OFFSETS = range(-3, 4)
WHOLE_RUNS = (255, 256, 257, 511, 512, 513, 1025)


# ---- references ---------------------------------------------------------------------------------------------------------

def _ref(case):
    """oracle.train + the replay of its merges: computed once per case and session"""
    if case["name"] in _REF:
        return _REF[case["name"]]
    data, offs, exps, nm = case["data"], case["offs"], case["exps"], case["nm"]
    if exps is None:
        pairs, counts, lens = oracle.train(data, nm, offs)
    else:
        pairs, counts, _ = oracle.train(data, nm, offs, weights=np.uint64(1) << exps.astype(np.uint64))
        lens = None
    ids = np.frombuffer(data, dtype=np.uint8).astype(np.int32)
    o, res_lens = offs, []
    for i, p in enumerate(pairs):
        ids, off_full = oracle.merge_chunks(ids, o, p, 256 + i)
        o = off_full[:-1]
        res_lens.append(len(ids))
    assert lens is None or lens == res_lens
    _REF[case["name"]] = dict(pairs=pairs, counts=counts, lens=res_lens, ids=ids)
    return _REF[case["name"]]


def _check_claim(case):
    """the merges the case claims are a == b ones, the first merge is (x, y)"""
    ref = _ref(case)
    assert len(ref["pairs"]) == case["nm"], case["name"]
    assert tuple(ref["pairs"][0]) == (X, Y), (case["name"], ref["pairs"])
    lo, hi = case["same"]
    assert hi > lo
    for k in range(lo, hi):
        assert ref["pairs"][k][0] == ref["pairs"][k][1], (case["name"], k, ref["pairs"])


def _n_same(ref, start=0):
    return sum(int(a == b) for a, b in ref["pairs"][start:])


# ---- CPU: the streams do what the cases claim --------------------------------------------------------------------------

@pytest.mark.parametrize("d", RUN_OFFSETS)
def test_cpu_runs_streams_select_same_token_pairs(d):
    for length in RUN_LENGTHS:
        case = runs_case(length, d)
        _check_claim(case)
        ref = _ref(case)
        assert tuple(ref["pairs"][1]) == (A, A) and tuple(ref["pairs"][2]) == (257, 257) and tuple(ref["pairs"][3]) == (258, 258)
        body = case["data"][:1100]
        for b in (256, 512, 768):  # the runs are where the case says, and are runs of exactly that length
            assert body[b + d:b + d + length] == bytes([A]) * length and body[b + d - 1] != A and body[b + d + length] != A


@pytest.mark.parametrize("run", WHOLE_RUNS)
def test_cpu_whole_slot_streams_select_same_token_pairs(run):
    for prefix in range(4):
        case = whole_slot_case(run, prefix)
        _check_claim(case)
        assert case["data"][prefix:prefix + run] == bytes([A]) * run and case["data"][prefix + run] != A
        assert _ref(case)["counts"][1] == run - 1


def test_cpu_other_streams_select_same_token_pairs():
    for case in chunk_boundary_cases() + [weighted_case(), consecutive_case()]:
        _check_claim(case)
    c1 = chunk_boundary_cases()[0]
    starts = set(int(o) for o in c1["offs"])
    assert 256 in starts and c1["data"][252:260] == bytes([A]) * 8  # a chunk starts exactly at a slot's first word, inside a's
    w = weighted_case()
    assert sorted(set(int(e) for e, o, n in zip(w["exps"], w["offs"], np.append(w["offs"][1:], len(w["data"])))
                      if w["data"][int(o):int(n)].count(A) == int(n) - int(o))) == [0, 1, 2, 3]
    ref = _ref(consecutive_case())
    assert sorted(map(tuple, ref["pairs"][1:3])) == [(98, 99), (100, 101)] and ref["counts"][1] == ref["counts"][2]
    assert tuple(ref["pairs"][3]) == (A, A)


def test_cpu_left_neighbour_stream_charges_the_slot_before():
    case = left_neighbour_case()
    _check_claim(case)
    ref = _ref(case)
    assert [tuple(p) for p in ref["pairs"]] == [(X, Y), (A, A), (113, 257)] and ref["counts"][1:] == [16, 6]
    for k in range(2, 13, 2):  # q ends a slot, the run starts the next one, and they share a chunk
        assert case["data"][256 * k - 1:256 * k + 2] == bytes([113, A, A]) and 256 * k - 1 in set(int(o) for o in case["offs"])
        assert A not in case["data"][256 * (k - 1):256 * k]  # (the slot before holds no a: the index cannot name it)


@pytest.mark.parametrize("where", [0, 1, 3])
def test_cpu_tie_streams_tie_same_token_pair_at_the_maximum(where):
    case = ties_case(where)
    _check_claim(case)
    ref = _ref(case)
    assert len(set(ref["counts"][1:5])) == 1  # four pairs tied at the maximum ...
    assert tuple(ref["pairs"][1 + where]) == (A, A)  # ... merged in order of first occurrence
    toks = [t for k in range(1, 5) for t in ref["pairs"][k] if k != 1 + where]
    assert len(set(toks)) == 6 and A not in toks


def test_cpu_realistic_stream_has_same_token_merges(native):
    ref = _ref(realistic_case(native))
    assert _n_same(ref, 20) >= 1, ref["pairs"]


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def _run(engine, case, chain_aa, depth=0):
    """train the case with the option set; the oracle's pairs, counts, lens and final stream -> train_stats"""
    ref = _ref(case)
    tag = (case["name"], chain_aa)
    engine.set_option("chain_aa", chain_aa)
    engine.set_option("depth", depth)
    engine.load_bytes(case["data"], case["offs"], case["exps"])
    res = engine.train(case["nm"])
    stats = engine.train_stats()
    assert res["pairs"] == ref["pairs"], tag
    assert res["counts"] == ref["counts"], tag
    assert res["lens"] == ref["lens"], tag
    assert np.array_equal(engine.read_ids(), ref["ids"]), tag
    # (with the option off a step headed by a == b is a no-op that hands back, and is not counted: a case whose later
    # merges all have a == b then counts no step at all)
    assert stats["slot_ids"] == 256 and (stats["steps"] > 0 or not chain_aa), (tag, stats)
    return stats


def _both(engine, cases, depth=0, exact=True):
    """every case with chain_aa = 1 and 0 (identical results: both are the oracle's).  exact: every a == b merge after
    the first merge was a chain step's own with the option on, and none with it off"""
    set_variant(engine, 1, 0, 2, 2, 9)
    try:
        for case in cases:
            on = _run(engine, case, 1, depth)
            off = _run(engine, case, 0, depth)
            want = _n_same(_ref(case), 1)
            assert off["aa_in_chain"] == 0, (case["name"], off)
            if exact:
                assert on["aa_in_chain"] == want, (case["name"], on)
                assert off["deferred"] >= want and on["deferred"] == off["deferred"] - want, (case["name"], on, off)
    finally:
        engine.set_option("chain_aa", 1)
        reset_variant(engine)


@pytest.mark.gpu
@pytest.mark.parametrize("d", RUN_OFFSETS)
def test_runs_around_slot_boundaries(engine, d):
    _both(engine, [runs_case(length, d) for length in RUN_LENGTHS])


@pytest.mark.gpu
@pytest.mark.parametrize("run", WHOLE_RUNS)
def test_runs_that_fill_whole_slots(engine, run):
    _both(engine, [whole_slot_case(run, prefix) for prefix in range(4)])


@pytest.mark.gpu
def test_chunk_boundaries_inside_runs(engine):
    _both(engine, chunk_boundary_cases())


@pytest.mark.gpu
def test_left_neighbour_in_the_slot_before(engine):
    _both(engine, [left_neighbour_case()])


@pytest.mark.gpu
def test_weighted_chunks(engine):
    _both(engine, [weighted_case()])


@pytest.mark.gpu
@pytest.mark.parametrize("where", [0, 1, 3])
def test_same_token_pair_tied_at_the_maximum(engine, where):
    # (the batch stops before (a, a), (a, a) goes alone, the rest follows: the oracle's order, one a == b merge in a chain step)
    _both(engine, [ties_case(where)])


@pytest.mark.gpu
def test_consecutive_merges(engine):
    _both(engine, [consecutive_case()])


@pytest.mark.gpu
def test_statistics(engine):
    case = runs_case(9, 0)
    ref = _ref(case)
    n_same, after_first = _n_same(ref), _n_same(ref, 1)
    assert after_first == 4
    set_variant(engine, 1, 0, 2, 2, 9)
    try:
        on = _run(engine, case, 1)
        off = _run(engine, case, 0)
        # (the first index build comes before merge 0, which takes the general path: every a == b merge after it)
        assert on["aa_in_chain"] == after_first and on["index_builds"] == off["index_builds"] == 1, (on, off)
        assert on["deferred"] == off["deferred"] - after_first, (on, off)
        assert off["aa_in_chain"] == 0 and off["deferred"] >= n_same, off
    finally:
        engine.set_option("chain_aa", 1)
        reset_variant(engine)


@pytest.mark.gpu
def test_realistic_shape(engine, native):
    # (test_train_synth_2mb_vs_oracle's shape, at the default depth: how many a == b merges the chain steps get depends on
    # where the host stands when they come up -- at least one of them does)
    case = realistic_case(native)
    _both(engine, [case], depth=8, exact=False)
    set_variant(engine, 1, 0, 2, 2, 9)
    try:
        assert _run(engine, case, 1, depth=8)["aa_in_chain"] >= 1
    finally:
        reset_variant(engine)
