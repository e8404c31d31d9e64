"""GPU: training on WEIGHTED chunks (bpe_load_bytes_weighted: a weight exponent in bits 26..30 of every id word,
DESIGN 4.3) through every engine variant, chain-step option and slot geometry -- against the CPU oracle.  An
unweighted stream has those five bits zero, so a kernel that drops, ignores or mis-shifts them passes every
unweighted test; these do not.  Integer work: every comparison is exact.

References, all from oracle/ (d2, o2, e = the de-duplicated or hand-weighted form of an input):
  R1  oracle.train(data, nm, offs) on the full chunk list: pairs, counts (inputs made by de-duplication);
  R2  oracle.train(d2, nm, o2, weights=2^e): pairs, counts, and the length of the list the weighted chunks STAND
      FOR after every merge (orc_train_weighted: sum of weight x chunk length);
  R3  R2's pairs replayed with oracle.merge_chunks over (d2, o2): the resident stream and its chunk starts at the
      end, and the length of the resident stream after every merge.
The engine's `lens` and len(engine) are lengths of the RESIDENT stream (every distinct chunk once), so they are
compared with R3's lengths; R3's replay also re-derives the stood-for lengths, which must equal R2's (and R1's): the
three references are tied to one another on the host before anything runs on the GPU.
Each input's references are computed once per session (_REF), not once per variant."""
import numpy as np
import pytest

import oracle
from helpers import (CHAIN_DEFAULTS, CHAIN_OPTIONS, VARIANTS, chunk_offsets, hand_weighted, reset_variant, runs_text,
                     set_variant, split_chunks, stands_for_bytes, ties_chunks, two_letter_weighted)

pytestmark = pytest.mark.gpu

_REF = {}


def _weights(e):
    return np.uint64(1) << np.asarray(e, dtype=np.uint64)


def _replay(d2, o2, e, pairs):
    """R3: (final ids, final chunk starts, resident length after every merge, stood-for length after every merge)"""
    ids = np.frombuffer(d2, dtype=np.uint8).astype(np.int32)
    w = _weights(e).astype(np.int64)  # (the caller has checked that the stood-for text is below 2^31 bytes)
    o, off_full = o2, np.append(o2, np.uint64(len(ids)))
    res_lens, full_lens = [], []
    for i, p in enumerate(pairs):
        ids, off_full = oracle.merge_chunks(ids, o, p, 256 + i)
        o = off_full[:-1]
        res_lens.append(len(ids))
        full_lens.append(int(np.dot(np.diff(off_full.astype(np.int64)), w)))
    starts = sorted(set(int(off_full[c]) for c in range(len(off_full) - 1) if off_full[c + 1] > off_full[c]))
    return ids, starts, res_lens, full_lens


def _make_input(native, name):
    """(d2, o2, e, nm, full) -- full = (data, offs) of the chunk list a de-duplicated input was made from"""
    if name == "W_regex":
        # GPT-4-split text, 341 k chunks -> 41 k weighted ones, 274 k ids (268 slots of 1024 ids): a default train runs
        # dense sweeps, then builds the index, then runs chain steps (asserted through train_stats below)
        data, offs = split_chunks(native.synth_text(2_000_000, 171).decode())
        nm = 400
    elif name == "W_ties":
        # three letters, 200 k chunks of 363 kinds: multiplicities with many set bits; ties at the maximum, a == b
        # heads and an empty table, all with weights
        chunks = ties_chunks(200_000, 12)
        data, offs = b"".join(chunks), chunk_offsets(chunks)
        nm = 400
    elif name == "W_runs":
        data, offs = split_chunks(runs_text())
        nm = 60
    elif name == "W_shard":
        # (the corpus of test_dp_chain_steps_weighted_shards)
        from test_gpu_parity import _space_chunks
        chunks = _space_chunks(native.synth_text(600_000, 53))
        return b"".join(chunks), chunk_offsets(chunks), None, 300, chunks
    elif name == "W_shard_ties":
        # (the corpus of test_dp_chain_steps_ties_and_exhaustion)
        chunks = ties_chunks(3000, 9)
        return b"".join(chunks), chunk_offsets(chunks), None, 400, chunks
    elif name == "W_hand":
        d2, o2, e, edges = hand_weighted(3000, 24, 12, seed=7)
        lens = np.diff(np.append(o2, len(d2)).astype(np.int64))
        assert all(lens[i] == 1 and e[i] == 24 and e[i + 1] == 0 for i in edges["singles"]) and len(edges["singles"]) >= 5
        assert all(lens[i] == 0 for i in edges["empties"]) and any(e[i] >= 8 for i in edges["empties"])
        assert sorted({m for m, _ in edges["aligned"]}) == [256, 1024, 4096]
        assert all(int(o2[i]) % m == 0 and o2[i] > 0 and e[i] == 24 and e[i - 1] == 0 for m, i in edges["aligned"])
        r = edges["run"]
        assert d2[int(o2[r]):int(o2[r]) + int(lens[r])] == b"z" * 2500 and int(o2[r]) % 1024 == 900 and e[r] >= 10
        assert np.abs(np.diff(e.astype(np.int64))).max() == 24  # (0 next to 24)
        return d2, o2, e, 300, None
    elif name == "W_hand_slice":
        d2, o2, e, _, _ = _make_input(native, "W_hand")
        k = 1200  # (past the first 4096-aligned start)
        return d2[:int(o2[k])], o2[:k], e[:k], 40, None
    elif name == "W_two":
        d2, o2, e = two_letter_weighted(1_000_000, 19)
        assert int(e.min()) >= 8
        return d2, o2, e, 8, None
    else:
        raise KeyError(name)
    d2, o2, e, _ = native.dedup_chunks(data, offs)
    assert len(o2) < len(offs) and int(e.max()) >= 2
    if name == "W_runs":
        lens = np.diff(np.append(o2, len(d2)).astype(np.int64))
        assert ((lens > 1024) & (e >= 3)).sum() >= 4 and ((lens > 4096) & (e >= 3)).sum() >= 1
    return d2, o2, e, nm, (data, offs)


def _ref(native, name):
    """the input and its references, computed once per session"""
    if name in _REF:
        return _REF[name]
    d2, o2, e, nm, full = _make_input(native, name)
    if e is None:  # a corpus the sharded tests de-duplicate rank by rank: R1 only
        r1 = oracle.train(d2, nm, o2, raise_on_empty=False)
        _REF[name] = dict(chunks=full, nm=nm, r1=r1)
        return _REF[name]
    # no count can reach 2^31: the text the chunks stand for is shorter than that
    assert stands_for_bytes(o2, e, len(d2)) < 2**31
    assert len(set(e.tolist())) >= 6 or name == "W_two"  # (W_two: exponents 8 and 9 by design)
    r2 = oracle.train(d2, nm, o2, raise_on_empty=False, weights=_weights(e))
    r1 = None
    if full is not None:
        r1 = oracle.train(full[0], nm, full[1], raise_on_empty=False)
        assert r1[0] == r2[0] and r1[1] == r2[1] and r1[2] == r2[2]
    ids, starts, res_lens, full_lens = _replay(d2, o2, e, r2[0])
    assert full_lens == r2[2]  # R3's replay re-derives R2's lengths
    _REF[name] = dict(d2=d2, o2=o2, e=e, nm=nm, r1=r1, r2=r2, ids=ids, starts=starts, lens=res_lens, full=full)
    return _REF[name]


def _train(engine, nm, n_full):
    """train(nm); where the oracle ran out of pairs after n_full < nm merges, so must the engine"""
    if n_full < nm:
        with pytest.raises(ValueError):
            engine.train(nm)
        return engine.last_train
    return engine.train(nm)


def _check_result(res, ref, tag=None):
    pairs, counts, _ = ref["r2"]
    if res["pairs"] != pairs or res["counts"] != counts:
        k = next((i for i in range(min(len(pairs), len(res["pairs"])))
                  if res["pairs"][i] != pairs[i] or res["counts"][i] != counts[i]), min(len(pairs), len(res["pairs"])))
        pytest.fail(f"{tag}: first difference at merge {k}: got {res['pairs'][k:k + 3]} {res['counts'][k:k + 3]}, "
                    f"want {pairs[k:k + 3]} {counts[k:k + 3]}; {len(res['pairs'])} of {len(pairs)} merges")
    if ref["r1"] is not None:
        assert res["pairs"] == ref["r1"][0] and res["counts"] == ref["r1"][1], tag
    assert res["lens"] == ref["lens"], tag


def _check_stream(engine, ref, tag=None):
    got = engine.read_ids()
    assert int(got.max()) < (1 << 26), tag  # (the weight bits stay inside the library)
    assert np.array_equal(got, ref["ids"]), tag
    assert engine.read_chunk_starts().tolist() == ref["starts"], tag


def _load_train_check(engine, ref, tag=None):
    """load the weighted stream and train: pairs, counts, lens; then -- after a train that ran to the end -- the
    resident stream, its chunk starts, a re-run from the resident bytes and a depth-0 run.  Returns (train_stats of
    the first run that ran to the end, the number of merges it did)."""
    nm, n_full = ref["nm"], len(ref["r2"][0])
    engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
    res = _train(engine, nm, n_full)
    _check_result(res, ref, tag)
    if n_full < nm:
        # the table ran empty: n_full merges can be done, and that train runs to the end
        res = engine.train(n_full)
        _check_result(res, ref, tag)
    stats = engine.train_stats()
    _check_stream(engine, ref, tag)
    assert engine.train(n_full)["pairs"] == ref["r2"][0], tag
    engine.set_option("depth", 0)
    try:
        res = engine.train(n_full)
    finally:
        engine.set_option("depth", 8)
    assert res["pairs"] == ref["r2"][0], tag
    _check_stream(engine, ref, tag)
    return stats, n_full


# ---------------------------------------------------------------------------
# 1. every engine variant

@pytest.mark.parametrize("mode,mimpl,slots,sparse,lean", VARIANTS)
@pytest.mark.parametrize("name", ["W_regex", "W_ties", "W_runs"])
def test_weighted_train_variants_vs_oracle(engine, native, name, mode, mimpl, slots, sparse, lean):
    ref = _ref(native, name)
    set_variant(engine, mode, mimpl, slots, sparse, lean)
    try:
        stats, nm = _load_train_check(engine, ref, (name, mode, mimpl, slots, sparse, lean))
        print(name, (mode, mimpl, slots, sparse, lean), stats)
        # (the train_stats assertions of test_train_synth_2mb_vs_oracle: a variant that fell back to another path fails)
        if sparse == 2:
            # every a != b pass a sparse one; a chain step (k_chain.hip) is ONE pass for all the merges of its batch
            chain_merges = stats["chained"] + stats["selections"] if stats["steps"] else 0
            assert stats["sparse"] == nm - chain_merges + stats["steps"]
        if slots == 2 and mode == 1:
            n_same = sum(a == b for a, b in ref["r2"][0])
            if lean == 0:
                assert stats["lean"] == 0 and stats["deferred"] == 0
            elif lean in (2, 3, 4, 5, 7):
                assert stats["lean"] + stats["deferred"] == nm and stats["deferred"] >= n_same
                # (nothing but the a == b merges on the GPT-4-split text, as on the unweighted one; W_ties and W_runs
                # are made of ties, and a tie the lean selection cannot settle by itself is handed back as well)
                if sparse != 2 and lean != 7 and name == "W_regex":
                    assert stats["deferred"] == n_same
                if lean == 7:
                    assert stats["steps"] > 0 and stats["selections"] <= stats["steps"]
            else:
                assert stats["lean"] > 0
            if lean in (9, 10) and stats["index_builds"]:
                assert stats["slot_ids"] == 256, stats
            if lean in (9, 10):
                assert stats["index_builds"] > 0, stats  # (the 256-id geometry was reached)
        if (mode, mimpl, slots, sparse, lean) == (1, 0, 2, 1, 1):
            # the default engine: dense sweeps, then the index, then chain steps -- each with weighted words
            assert stats["dense"] > 0 and stats["index_builds"] > 0 and stats["steps"] > 0, stats
    finally:
        reset_variant(engine)


# ---------------------------------------------------------------------------
# 2. every option of the chain steps

@pytest.mark.parametrize("opts", CHAIN_OPTIONS)
@pytest.mark.parametrize("name", ["W_regex", "W_ties"])
def test_weighted_chain_step_options_vs_oracle(engine, native, name, opts):
    ref = _ref(native, name)
    set_variant(engine, 1, 0, 2, 2, 7)
    try:
        for k, v in opts:
            engine.set_option(k, v)
        st, _ = _load_train_check(engine, ref, (name, opts))
        print(name, opts, st)
        assert st["steps"] > 0
        if ("fuse_step", 1) in opts:
            assert st["fused_steps"] > 0
        else:
            assert st["fused_steps"] == 0
        if ("small_slots", 2) in opts and st["index_builds"]:
            assert st["slot_ids"] == 256
        if ("small_slots", 2) in opts:
            assert st["index_builds"] > 0
        if ("small_slots", 0) in opts:
            assert st["slot_ids"] == 1024
    finally:
        for k, _ in opts:
            engine.set_option(k, CHAIN_DEFAULTS[k])
        reset_variant(engine)


# ---------------------------------------------------------------------------
# 3. re-pack policy of the dense phase

@pytest.mark.parametrize("acc", [0, 5, 200, 10000])
def test_weighted_repack_policy_vs_oracle(engine, native, acc):
    ref = _ref(native, "W_regex")
    reset_variant(engine)
    engine.set_option("repack_acc", acc)
    try:
        engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
        res = engine.train(ref["nm"])
        _check_result(res, ref, acc)
        assert engine.train_stats()["dense"] > 0
    finally:
        engine.set_option("repack_acc", 200)


# ---------------------------------------------------------------------------
# 4. the literal path (mode = 0: the pairs are re-counted at every iteration)

@pytest.mark.parametrize("k1", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["W_regex", "W_hand", "W_two"])
def test_weighted_literal_path_histograms_vs_oracle(native, name, k1):
    """k1 = 0: one atomic per position; 1: the LDS hash cache (k_pair_count_lds); 2 and 3 are forms for unweighted
    streams and fall back for weighted ones -- exact all the same.  W_two: two letters, every position weighs 256 or
    512: each workgroup's LDS table passes 2^14 per pair (its drain) by weight, not by occurrence."""
    ref = _ref(native, name)
    eng = native.Engine(0)
    try:
        eng.set_option("mode", 0)
        eng.set_option("k1", k1)
        eng.load_bytes(ref["d2"], ref["o2"], ref["e"])
        res = _train(eng, ref["nm"], len(ref["r2"][0]))
        _check_result(res, ref, (name, k1))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 5. exponents set by hand; refusals

HAND_ENGINES = {
    "default": (1, 0, 2, 1, 1), "small_slots2": (1, 0, 2, 1, 9), "sparse2_chain": (1, 0, 2, 2, 7),
    "slots0": (1, 0, 0, 1, 1), "merge1": (1, 1, 0, 1, 1),
}


@pytest.mark.parametrize("which", list(HAND_ENGINES))
def test_hand_weighted_train_vs_oracle(engine, native, which):
    ref = _ref(native, "W_hand")
    variant = HAND_ENGINES[which]
    set_variant(engine, *variant)
    try:
        stats, _ = _load_train_check(engine, ref, which)
        print(which, stats)
        if which == "small_slots2":
            assert stats["index_builds"] > 0 and stats["slot_ids"] == 256, stats
        if which == "sparse2_chain":
            assert stats["steps"] > 0 and stats["sparse"] > 0, stats
    finally:
        reset_variant(engine)


def test_weighted_load_refusals_leave_the_engine_usable(engine, native):
    ties = _ref(native, "W_ties")
    ref = _ref(native, "W_hand")
    d2, o2, e = ref["d2"], ref["o2"], ref["e"]

    def usable():
        engine.load_bytes(ties["d2"], ties["o2"], ties["e"])
        _check_result(_train(engine, ties["nm"], len(ties["r2"][0])), ties, "after a refusal")

    reset_variant(engine)
    usable()
    # an exponent that does not fit the five bits: refused, the chunk is named
    bad = e.copy()
    bad[1234] = 32
    with pytest.raises(ValueError, match=r"exponent 32 of chunk 1234\b"):
        engine.load_bytes(d2, o2, bad)
    usable()
    # chunks that stand for 2^32 bytes or more: pair counts are 32-bit
    big = np.full(len(o2), 18, np.uint8)
    assert 2**32 <= stands_for_bytes(o2, big, len(d2))
    with pytest.raises(RuntimeError, match=rf"error {native.BPE_E_LIMIT}: .*2\^32"):
        engine.load_bytes(d2, o2, big)
    usable()
    # weights without chunk offsets: in the binding and in the library
    with pytest.raises(ValueError):
        engine.load_bytes(d2, None, e)
    buf = np.frombuffer(d2, dtype=np.uint8)
    rc = native._lib.bpe_load_bytes_weighted(engine._h, buf.ctypes.data, len(buf), None, 0, e.ctypes.data)
    assert rc == native.BPE_E_ARG and b"offsets" in native._lib.bpe_last_error(engine._h)
    usable()


# ---------------------------------------------------------------------------
# 6. the literal loop by hand: get_stats -> argmax -> merge on a weighted stream

def _weighted_stats(ids, o, e):
    """the oracle's statistics of a weighted stream: pairs in first-appearance order (oracle.get_stats of the stream)
    with counts = sum over the exponents k of 2^k x (oracle.get_stats count over the chunks that carry k)"""
    off_full = np.append(o, np.uint64(len(ids))).astype(np.int64)
    order = [p for p, _, _ in oracle.get_stats(ids, o)]
    total = dict.fromkeys(order, 0)
    for k in sorted(set(e.tolist())):
        sel = np.flatnonzero(e == k)
        parts = [ids[off_full[c]:off_full[c + 1]] for c in sel]
        sub = np.concatenate(parts) if parts else np.empty(0, np.int32)
        for p, cnt, _ in oracle.get_stats(sub, chunk_offsets(parts)) if len(sub) else []:
            total[p] += cnt << int(k)
    return [(p, total[p]) for p in order]


@pytest.mark.parametrize("name", ["W_ties", "W_hand_slice"])
def test_weighted_literal_loop_by_hand(engine, native, name):
    ref = _ref(native, name)
    steps = 40
    pairs, counts, _ = ref["r2"]
    assert len(pairs) >= steps
    reset_variant(engine)
    engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
    ids = np.frombuffer(ref["d2"], dtype=np.uint8).astype(np.int32)
    o = ref["o2"]
    for i in range(steps):
        want = _weighted_stats(ids, o, ref["e"])
        got = engine.get_stats()
        assert [(p, c) for p, c, _ in got] == want, i
        assert engine.argmax() == (pairs[i], counts[i]), i
        engine.merge(pairs[i], 256 + i)
        assert len(engine) == ref["lens"][i], i
        ids, off_full = oracle.merge_chunks(ids, o, pairs[i], 256 + i)
        o = off_full[:-1]
    got = engine.read_ids()
    assert int(got.max()) < (1 << 26)
    assert np.array_equal(got, ids)
    if len(pairs) == steps:
        assert np.array_equal(ids, ref["ids"]) and engine.read_chunk_starts().tolist() == ref["starts"]


# ---------------------------------------------------------------------------
# 7. nothing of a weighted load stays behind

def test_no_state_leaks_out_of_a_weighted_load(engine, native):
    ref = _ref(native, "W_regex")
    data, offs = ref["full"]
    reset_variant(engine)
    engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
    _check_result(engine.train(ref["nm"]), ref, "weighted")
    # ids loaded from the host: plain statistics
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 40, size=200_000, dtype=np.int32)
    ioffs = np.unique(np.concatenate([[0], rng.integers(0, len(ids), size=30_000)])).astype(np.uint64)
    engine.load_ids(ids, ioffs)
    assert engine.get_stats() == oracle.get_stats(ids, ioffs)
    # encoding a regex-split text
    engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
    engine.train(50)
    pairs = ref["r2"][0]
    text, toffs = split_chunks(native.synth_text(150_000, 22).decode())
    exp_ids, exp_off = oracle.encode(pairs, text, toffs)
    got_ids, got_off = engine.encode_batch(np.array(pairs, np.int32), None, text, toffs)
    assert np.array_equal(got_ids, exp_ids) and np.array_equal(got_off, exp_off)
    # an unweighted train: R1, lengths of the unweighted stream included
    engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
    engine.train(50)
    engine.load_bytes(data, offs)
    res = engine.train(ref["nm"])
    assert res["pairs"] == ref["r1"][0] and res["counts"] == ref["r1"][1] and res["lens"] == ref["r1"][2]
    assert int(engine.read_ids().max()) < 256 + ref["nm"]
    # and a weighted one straight after
    engine.load_bytes(ref["d2"], ref["o2"], ref["e"])
    _check_result(engine.train(ref["nm"]), ref, "weighted again")
    _check_stream(engine, ref)


# ---------------------------------------------------------------------------
# 8. sharded: every rank de-duplicates its own shard

@pytest.mark.parametrize("opts", [(), (("dp_kcap", 1),), (("dp_kcap", 8), ("sparse", 2)), (("sparse", 0),)])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name", ["W_shard", "W_shard_ties"])
def test_weighted_shards_chain_steps_vs_oracle(native, name, world, opts):
    pytest.importorskip("torch")
    from test_gpu_parity import _chain_ranks
    ref = _ref(native, name)
    pairs, counts, _ = ref["r1"]
    out, errs, _ = _chain_ranks(native, ref["chunks"], ref["nm"], world, opts, dedup=True)
    if len(pairs) < ref["nm"]:
        assert all(isinstance(err, ValueError) for err in errs)
    else:
        assert not any(errs)
    for res in out:
        assert res["pairs"] == pairs and res["counts"] == counts, (name, world, opts)


@pytest.mark.parametrize("slots,sparse", [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_weighted_shards_lockstep_vs_oracle(native, world, slots, sparse):
    pytest.importorskip("torch")
    from test_gpu_parity import _lockstep
    ref = _ref(native, "W_shard")
    nm = 200
    got = _lockstep(native, ref["chunks"], nm, world, slots, dedup=True, sparse=sparse)
    assert got[0] == ref["r1"][0][:nm] and got[1] == ref["r1"][1][:nm]
