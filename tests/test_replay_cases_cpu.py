"""CPU: the cases of replay_cases.py, small (n = 4096) -- oracle.encode against a plain replay (merge r applied
everywhere, for r = 0 .. M - 1) and against the reference's encode loop restated with oracle/pyref.py (lowest-ranked
pair present, merged everywhere, until none is left: base.py / basic.py:57-74), so that the oracle is pinned on exactly
these lists before tests/test_gpu_replay.py compares the GPU with it; and every case's structure -- the run lengths that
k_forced_sel's rule (replay_cases.forced_run) gives behind each barrier, the counts of cold_then_hot -- so that no case
silently stops being what it was built for."""
import os
import re

import numpy as np
import pytest

import oracle
import replay_cases as rc
from oracle import pyref

N = 4096


def pyref_encode(pairs, data, mids=None):
    """the reference's encode: while a pair of the merges dict is present, merge the one with the lowest id"""
    merges = {(int(a), int(b)): (256 + r if mids is None else int(mids[r])) for r, (a, b) in enumerate(pairs)}
    ids = list(data)
    while len(ids) >= 2:
        stats = pyref.get_stats(ids)
        pair = min(stats, key=lambda p: merges.get(p, float("inf")))
        if pair not in merges:
            break
        ids = pyref.merge(ids, pair, merges[pair])
    return ids


def plain_replay(pairs, data):
    ids = list(data)
    for r, (a, b) in enumerate(pairs):
        ids = pyref.merge(ids, (int(a), int(b)), 256 + r)
    return ids


def test_constants_match_the_sources():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minbpe_amd", "csrc")
    src = ""
    for f in ("bpe_device.h", "kernels/k_chain.hip", "api/api_encode.hip", "api/api_ctx.hip"):
        with open(os.path.join(root, f), encoding="utf-8") as fh:
            src += fh.read()
    assert re.search(r"\bCH_KSWEEP = (\d+)", src).group(1) == str(rc.CH_KSWEEP)
    assert re.search(r"\bCH_KDENSE = (\d+)", src).group(1) == str(rc.CH_KDENSE)
    assert "REPLAY_MIN_BYTES = 1u << 20" in src and rc.REPLAY_MIN_BYTES == 1 << 20
    assert "int chain_kcap = CH_KSWEEP;" in src
    assert max(rc.KCAPS) == rc.CH_KSWEEP and max(l for _, l in rc.JL) == rc.CH_KSWEEP - 1


@pytest.mark.parametrize("name", list(rc.CASES))
def test_oracle_is_the_plain_replay_and_the_reference_loop(name):
    pairs, data = rc.CASES[name](N)
    assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2
    assert rc.training_shape(pairs)   # both conditions of merges_training_shape
    if not name.startswith("collapse"):
        assert len(data) == N + rc.D and rc.D % 2 == 1
    ids, off = oracle.encode(pairs, data, None)
    assert off.tolist() == [0, len(ids)]
    assert ids.tolist() == plain_replay(pairs, data)
    assert ids.tolist() == pyref_encode(pairs, data)
    *_, (m, last) = rc.plain_replay(pairs, data)   # (the same replay with oracle.merge: what the full-size checks below walk)
    assert m == len(pairs) and np.array_equal(last, ids)


@pytest.mark.parametrize("label", ["pair_twice", "forward_reference", "merge_ids_identity", "merge_ids_sparse"])
def test_gate_lists(label):
    """the lists the gate must keep off the replay: the oracle follows the reference's dict (a pair listed twice keeps
    its LAST rank and id, as api_encode.hip's rank table does), and the lists differ from the plain one where they
    claim to"""
    pairs, mids = rc.gate_lists(N)[label]
    _, data = rc.CASES["disjoint_run"](N)
    ids, _ = oracle.encode(pairs, data, None, merge_ids=mids)
    assert ids.tolist() == pyref_encode(pairs, data, mids)
    plain_pairs, _ = rc.CASES["disjoint_run"](N)
    plain = oracle.encode(plain_pairs, data, None)[0]
    if label == "pair_twice":
        assert not rc.training_shape(pairs) and 306 in ids and 259 not in ids and len(ids) > len(plain)
        assert ids.tolist() != plain_replay(pairs, data)   # (a replay in list order would merge leaf 3 at rank 3)
    elif label == "forward_reference":
        assert not rc.training_shape(pairs) and pairs[40][0] == 297 >= 256 + 40 and 296 in ids
    elif label == "merge_ids_identity":
        assert np.array_equal(ids, plain)
    else:
        rename = np.concatenate([np.arange(256), mids])
        assert np.array_equal(ids, rename[plain])


# ---------------------------------------------------------------------------
# structure

def test_forced_run_rule():
    """forced_run on lists small enough to read"""
    run = rc.forced_run
    assert run([(1, 2), (3, 4), (5, 6)], 0, 31) == 3 and run([(1, 2), (3, 4), (5, 6)], 0, 2) == 2
    assert run([(1, 1), (3, 4)], 0, 31) == 0 and run([(1, 2), (3, 3)], 0, 31) == 1
    for shared in ((1, 9), (9, 1), (2, 9), (9, 2)):
        assert run([(1, 2), (3, 4), shared], 0, 31) == 2
    assert run([(1, 2), (3, 4), (256, 9)], 0, 31) == 2 and run([(1, 2), (3, 4), (9, 257)], 0, 31) == 2
    assert run([(1, 2), (3, 4), (256, 9), (5, 6)], 1, 31) == 3   # (256 is older than the run that starts at merge 1)
    assert rc.forced_runs([(1, 1), (1, 2), (3, 4), (2, 5), (6, 6)], 0, 31) == [(0, 0), (1, 2), (3, 1), (4, 0)]


@pytest.mark.parametrize("name", list(rc.MARKED))
@pytest.mark.parametrize("kcap", rc.KCAPS)
def test_runs_behind_the_barriers(name, kcap):
    pairs, _ = rc.CASES[name](N)
    for start, cut in rc.marks(name, N):
        assert pairs[start - 1][0] == pairs[start - 1][1]   # the barrier
        assert rc.forced_run(pairs, start, kcap) == min(kcap, cut), (name, start, cut)
        assert (start, min(kcap, cut)) in rc.forced_runs(pairs, 1, kcap)   # ... and the steps do arrive there


def test_marks_cover_what_the_cases_claim():
    assert sorted(cut for _, cut in rc.marks("aa_in_run", N)) == sorted(
        lane for k in rc.KCAPS for lane in {0, 1, k - 1, k})
    assert [cut for _, cut in rc.marks("shared_token_cut", N)] == [l for _, l in rc.JL for _ in rc.WAYS]
    assert [cut for _, cut in rc.marks("fresh_token_cut", N)] == [l for _, l in rc.JL for _ in range(2)]
    pairs, _ = rc.CASES["shared_token_cut"](N)
    ways = []
    for (start, l), (j, _) in zip(rc.marks("shared_token_cut", N), [jl for jl in rc.JL for _ in rc.WAYS]):
        (aj, bj), (a, b) = pairs[start + j].tolist(), pairs[start + l].tolist()
        ways.append((aj == a, aj == b, bj == a, bj == b))
        assert sum(ways[-1]) == 1
        others = [t for i in range(l) if i != j for t in pairs[start + i].tolist()]
        assert a not in others and b not in others   # lane j is the only reason for the cut
    assert ways == [(True, False, False, False), (False, True, False, False), (False, False, True, False),
                    (False, False, False, True)] * 3
    pairs, _ = rc.CASES["fresh_token_cut"](N)
    got = []
    for (start, l), (j, _) in zip(rc.marks("fresh_token_cut", N), [jl for jl in rc.JL for _ in range(2)]):
        a, b = pairs[start + l].tolist()
        got.append((a == 256 + start + j, b == 256 + start + j))
        assert min(a, b) < 256 and min(a, b) not in pairs[start:start + l]
    assert got == [(True, False), (False, True)] * 3


def test_disjoint_run_runs():
    pairs, data = rc.CASES["disjoint_run"](N)
    assert len(pairs) == 79
    for start in range(9):
        assert rc.forced_run(pairs, start, 31) == 31
        for kcap in rc.KCAPS:
            assert rc.forced_run(pairs, start, kcap) == kcap
    # the general path takes merge 0; the steps behind it: 31 leaves, 8 leaves + level one (its tokens are older than
    # the run), then the tree level by level
    # (level one from (288, 289) on, level two from (312, 313) on, ... name tokens that the run itself would create)
    assert [k for _, k in rc.forced_runs(pairs, 1, 31)] == [31, 8 + 16, 4 + 8, 2 + 4, 1 + 2, 1, 1]
    assert set(data) > set(range(0x30, 0x80))   # (every leaf's bytes, and bytes outside the alphabet)


def test_short_lists():
    assert len(rc.CASES["short_m1"](N)[0]) == 1 and len(rc.CASES["short_m2"](N)[0]) == 2
    for tail in rc.TAILS:
        pairs, _ = rc.CASES[f"short_tail{tail}"](N)
        assert len(pairs) == 2 + tail
        for kcap in rc.KCAPS:
            last = rc.forced_runs(pairs, 2, kcap)[-1][1]
            assert last == (tail - 1) % kcap + 1
    # the last run holds 1, kcap - 1 and kcap merges, for every kcap
    for kcap in rc.KCAPS:
        lasts = {(t - 1) % kcap + 1 for t in rc.TAILS}
        assert {1, max(kcap - 1, 1), kcap} <= lasts, kcap


def test_shuffled_trained_shape():
    pairs, data = rc.CASES["shuffled_trained"](N)
    assert len(pairs) == 2100 and 256 + len(pairs) > 2048 and set(data) == {97, 98, 99, 100}
    runs = [k for _, k in rc.forced_runs(pairs, 1, 31)]
    assert max(runs) > rc.CH_KDENSE and runs.count(0) > 20   # long batches and a == b merges, as they come


@pytest.mark.parametrize("name", list(rc.CASES))
def test_every_merge_list_is_used(name):
    """no case is inert: the small text already changes under the list"""
    pairs, data = rc.CASES[name](N)
    ids, _ = oracle.encode(pairs, data, None)
    assert len(ids) < len(data) and ids.max() >= 256


def test_full_size_counts_and_collapse():
    """Once, at full size (oracle.get_stats along the plain replay): cold_then_hot's counts rise from 0 -- merge 0 --
    to the most frequent pair but one -- merge 1 --, fall to 0 three hundred times and rise to 2^18 or more at rank
    340; the collapse family ends in 1, 2 and 21 ids."""
    n = rc.REPLAY_MIN_BYTES
    pairs, data = rc.CASES["cold_then_hot"](n)
    assert len(data) == n + rc.D
    counts = []
    for r, ids in rc.plain_replay(pairs, data):
        if r < len(pairs) and (r < 40 or r >= rc.HOT_RANK - 2):
            stats = {p: c for p, c, _ in oracle.get_stats(ids)}
            counts.append((r, stats.get((int(pairs[r][0]), int(pairs[r][1])), 0)))
            if r == 1:
                top = sorted(stats.values())
                assert top[-1] == stats[(0x70, 0x71)] and top[-2] == counts[-1][1]
    by_rank = dict(counts)
    print("cold_then_hot counts:", counts)
    assert by_rank[0] == 0 and by_rank[1] >= n // 6 - 64
    assert all(by_rank[r] == 0 for r in range(0, 40, 2)) and all(by_rank[r] > 0 for r in range(1, 40, 2) if r != 11)
    assert by_rank[rc.HOT_RANK - 1] == 0 and by_rank[rc.HOT_RANK - 2] == 0
    assert by_rank[rc.HOT_RANK] >= 1 << 18 and rc.HOT_RANK >= 340
    assert tuple(pairs[rc.HOT_RANK]) == (0x70, 0x71) and not (set(pairs[:rc.HOT_RANK].ravel().tolist()) & {0x70, 0x71})
    for name, length, want in (("collapse_pow2", n, 1), ("collapse_plus1", n + 1, 2), ("collapse_ones", 2 * n - 1, 21)):
        cp, cd = rc.CASES[name](n)
        assert len(cp) == 24 and cd == b"a" * length
        assert rc.collapse_ids(n, length) == want
        assert len(oracle.encode(cp, cd, None)[0]) == want
