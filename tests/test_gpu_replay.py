"""GPU: encode as a replay of training (api_encode.hip: one chunk of 1 MiB or more, a merge list of the shape training
makes) on the hand-built lists of replay_cases.py -- counts that rise from 0 to a quarter of the text, runs of 31
token-disjoint merges, cuts at lane 30, lists that end inside a run, streams that collapse to one id -- at the defaults,
at every batch width, through the engine's variants, on either side of the host's gate, and what the ctx is left with.
Every comparison is exact: ids and out_off against oracle.encode (pinned on these very lists, small, to a plain replay and
to the reference's loop by tests/test_replay_cases_cpu.py).  Each test also reads engine.train_stats() to see that the
replay did take the path the test is about: a parity test that ran every merge through the general path would prove
nothing about batches."""
import numpy as np
import pytest

import helpers
import oracle
import replay_cases as rc
from test_gpu_big import FULL_VARIANTS

pytestmark = pytest.mark.gpu

N = rc.REPLAY_MIN_BYTES
# the options these tests touch, at the ctx's defaults (api_ctx.hip); helpers.reset_variant restores the variant's
DEFAULTS = {"enc_replay": 1, "chain_kcap": rc.CH_KSWEEP, "chain_dense": 1, "count_is_removed": 1, "chain_hash_kmin": 0}
_EXPECTED = {}


def expected(name):
    """oracle.encode of a case at full size: computed once, shared by every test and left unchanged"""
    if name not in _EXPECTED:
        pairs, data = rc.CASES[name](N)
        ids, off = oracle.encode(pairs, data, None)
        ids.setflags(write=False)
        _EXPECTED[name] = (ids, off)
    return _EXPECTED[name]


def restore(engine):
    helpers.reset_variant(engine)
    for k, v in DEFAULTS.items():
        engine.set_option(k, v)


def same(ids, out_off, exp, what):
    exp_ids, exp_off = exp
    assert list(out_off) == list(exp_off) == [0, len(exp_ids)], f"{what}: offsets {list(out_off)} for {list(exp_off)}"
    assert len(ids) == len(exp_ids), what
    if not np.array_equal(ids, exp_ids):
        p = int(np.flatnonzero(ids != exp_ids)[0])
        raise AssertionError(f"{what}: first difference at token {p}: {ids[max(p - 4, 0):p + 8].tolist()} for "
                             f"{exp_ids[max(p - 4, 0):p + 8].tolist()}")


def replay(engine, name, options=(), variant=None, chain_steps=True):
    """the case through engine.encode_batch under a variant (helpers.set_variant's arguments) and options; equal to the
    oracle; returns train_stats() of the replay, printed"""
    pairs, data = rc.CASES[name](N)
    restore(engine)
    try:
        if variant is not None:
            helpers.set_variant(engine, *variant)
        for k, v in options:
            engine.set_option(k, v)
        ids, out_off = engine.encode_batch(pairs, None, data, None)
        st = engine.train_stats()
    finally:
        restore(engine)
    what = f"replay {name} variant={variant} options={dict(options)}"
    print(f"{what}: {st}")
    same(ids, out_off, expected(name), what)
    if chain_steps and rc.has_chain_merges(pairs):
        assert st["steps"] > 0, what   # it did go through the training engine's chain steps
    return st


# ---------------------------------------------------------------------------
# every case: the defaults, the stream-wide rounds, every batch width

@pytest.mark.parametrize("name", list(rc.CASES))
def test_defaults_and_rounds(engine, name):
    st = replay(engine, name)
    pairs, data = rc.CASES[name](N)
    aa = sum(1 for a, b in pairs[1:].tolist() if a == b)
    # merges that chain steps did + merges the general path took (the first one, and whatever was handed back)
    assert st["lean"] <= len(pairs) - 1 and st["deferred"] <= len(pairs) - 1
    if not rc.has_chain_merges(pairs):   # short_m1, the collapse family: nothing a chain step can take
        assert st["lean"] == 0 and st["chained"] == 0
    if name.startswith("collapse"):
        # every a == b merge that heads a chain step is handed back (k_forced_sel: K == 0), the general path takes one
        # merge and the next step meets the next rung: the deferrals account for every merge but the first
        assert st["deferred"] == aa == len(pairs) - 1, st
    if name == "shuffled_trained":
        return   # (the rounds sweep the stream once per rank present, ~2100 sweeps with two host round trips each: left out)
    engine.set_option("enc_replay", 0)
    try:
        ids, out_off = engine.encode_batch(pairs, None, data, None)
    finally:
        engine.set_option("enc_replay", 1)
    same(ids, out_off, expected(name), f"rounds {name}")


@pytest.mark.parametrize("kcap", rc.KCAPS)
@pytest.mark.parametrize("name", list(rc.CASES))
def test_batch_widths(engine, name, kcap):
    st = replay(engine, name, (("chain_kcap", kcap),))
    if name.startswith("short_tail"):
        # merge 0 is the general path's; the step that meets the barrier hands it back, which drains the queue: from
        # there on the host has seen a count (<= lean_count at this size), the index is built and every step is an
        # indexed one of up to chain_kcap merges -- the tail takes exactly the runs of k_forced_sel's rule
        pairs, _ = rc.CASES[name](N)
        runs = rc.forced_runs(pairs, 2, kcap)
        assert st["steps"] == len(runs) and st["lean"] == st["chained"] == sum(k for _, k in runs) == len(pairs) - 2, st
        assert st["deferred"] == 1, st


# ---------------------------------------------------------------------------
# the engine's variants

# on top of the default variant (mode, merge, slots, sparse, lean) = (1, 0, 2, 1, 1)
EXTRA_OPTIONS = [(("chain_dense", 0),), (("count_is_removed", 0),), (("chain_hash_kmin", 32),), (("small_slots", 0),),
                 (("small_slots", 2),), (("sparse", 0),), (("sparse", 2),), (("chain", 0),),
                 (("chain_dense", 0), ("small_slots", 2), ("chain_kcap", 15))]
# the first slotted form, no slots at all, the look-back merge: the general path alone
OLD_FORMS = [(1, 0, 1, 1, 1), (1, 0, 0, 1, 1), (1, 1, 0, 1, 1)]
VARIANT_CASES = ["disjoint_run", "cold_then_hot", "shared_token_cut", "shuffled_trained"]


def _chain_on(lean):
    return lean in (1, 7, 9, 10)   # helpers.set_variant: option chain


@pytest.mark.parametrize("sparse,lean", FULL_VARIANTS)
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_full_variants(engine, name, sparse, lean):
    """test_gpu_big.FULL_VARIANTS through helpers.set_variant (lean 6 there: the default engine without the back-off)"""
    options = (("lean_backoff", 0),) if lean == 6 else ()
    replay(engine, name, options, variant=(1, 0, 2, sparse, 1 if lean == 6 else lean),
           chain_steps=_chain_on(1 if lean == 6 else lean))


@pytest.mark.parametrize("options", EXTRA_OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o))
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_option_variants(engine, name, options):
    # (sparse = 0: no index, so no chain step once the host has seen a count and the iterations are lean ones -- a list
    # whose first steps all meet a barrier then counts none)
    replay(engine, name, options, chain_steps=("chain", 0) not in options and ("sparse", 0) not in options)


@pytest.mark.parametrize("variant", OLD_FORMS)
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_old_forms(engine, name, variant):
    replay(engine, name, variant=variant, chain_steps=False)


# ---------------------------------------------------------------------------
# what the stats must show

def test_disjoint_run_reaches_wide_indexed_batches(engine):
    """kcap = 31 on 40 token-disjoint merges: with dense steps off (their batches end at CH_KDENSE = 6) every chain step
    is an indexed one, and `chained` -- the merges that chain steps took off a given list, summed over the steps -- exceeds
    6 per step: some batch was wider than any dense step's."""
    for options in ((("chain_dense", 0),), (("chain_dense", 0), ("sparse", 2))):
        st = replay(engine, "disjoint_run", options + (("chain_kcap", 31),))
        assert st["chained"] > rc.CH_KDENSE * st["steps"], st
        assert st["sparse"] > 0 and st["index_builds"] > 0, st


# ---------------------------------------------------------------------------
# the gate

def _encode(eng, pairs, mids, data, offs=None):
    return eng.encode_batch(np.asarray(pairs, np.int32), mids, data, offs)


def test_gate_at_one_mebibyte(native):
    """2^20 - 1 bytes: the stream-wide rounds (a fresh engine has no train() behind it: no chain step counted);
    2^20 bytes: the replay"""
    pairs, data = rc.CASES["disjoint_run"](N)
    with native.Engine(0) as eng:
        for n, replays in ((N - 1, False), (N, True)):
            ids, out_off = _encode(eng, pairs, None, data[:n])
            same(ids, out_off, oracle.encode(pairs, data[:n], None), f"{n} bytes")
            st = eng.train_stats()
            print(f"gate {n} bytes: {st}")
            assert (st["steps"] > 0) == replays and (st["lean"] > 0) == replays, (n, st)


@pytest.mark.parametrize("label", ["pair_twice", "forward_reference", "merge_ids_identity", "merge_ids_sparse"])
def test_gate_keeps_other_lists_off_the_replay(native, label):
    pairs, mids = rc.gate_lists(N)[label]
    _, data = rc.CASES["disjoint_run"](N)
    exp = oracle.encode(pairs, data, None, merge_ids=mids)
    with native.Engine(0) as eng:
        ids, out_off = _encode(eng, pairs, mids, data)
        same(ids, out_off, exp, label)
        st = eng.train_stats()
        assert st["steps"] == 0 and st["lean"] == 0 and st["dense"] == 0 and st["sparse"] == 0, st


def test_gate_one_chunk_that_does_not_start_at_zero(native):
    pairs, data = rc.CASES["disjoint_run"](N)
    data = data[:5] + data   # (the chunk itself is still more than 1 MiB)
    exp_ids, exp_off = oracle.encode(pairs, data, np.array([5], np.uint64))
    assert np.array_equal(exp_ids, oracle.encode(pairs, data[5:], None)[0])
    with native.Engine(0) as eng:
        ids, out_off = _encode(eng, pairs, None, data, np.array([5], np.uint64))
        same(ids, out_off, (exp_ids, exp_off), "offsets = [5]")
        assert eng.train_stats()["steps"] == 0


# ---------------------------------------------------------------------------
# the ctx afterwards

def _refusal(eng):
    with pytest.raises(Exception) as e:
        eng.get_stats()
    return type(e.value), str(e.value)


def test_ctx_after_a_replay(native):
    pairs, data = rc.CASES["disjoint_run"](N)
    big_pairs, big_data = rc.CASES["shuffled_trained"](N)
    small_pairs, small_data = rc.CASES["short_m2"](N)
    rng = np.random.default_rng(5)
    text = bytes(97 + rng.integers(0, 4, size=150_000).astype(np.uint8))
    with native.Engine(0) as eng:
        # what the rounds path leaves: no ids to count
        _encode(eng, pairs, None, data[:N - 1])
        rounds_refusal = _refusal(eng)
        eng.set_option("mode", 0)
        ids, out_off = _encode(eng, pairs, None, data)
        same(ids, out_off, expected("disjoint_run"), "replay under mode 0")
        assert eng.train_stats()["steps"] > 0   # (the replay itself ran in mode 1)
        assert _refusal(eng) == rounds_refusal and "no ids loaded" in rounds_refusal[1]
        # mode 0 is back: the literal loop (clear, count, arg-max, merge) -- no chain steps, the oracle's merges
        eng.load_bytes(text)
        got = eng.train(40)
        want = oracle.train(text, 40)
        assert (got["pairs"], got["counts"], got["lens"]) == want
        eng.set_option("mode", 1)
        # a weighted load, then a replay: the weights must not outlive the load
        chunks = helpers.ties_chunks(4000, 9)
        wdata, woffs = b"".join(chunks), helpers.chunk_offsets(chunks)
        exps = rng.integers(0, 4, size=len(chunks)).astype(np.uint8)
        eng.load_bytes(wdata, woffs, weight_exp=exps)
        got = eng.train(30)
        want = oracle.train(wdata, 30, woffs, weights=np.uint64(1) << exps.astype(np.uint64))
        assert (got["pairs"], got["counts"]) == want[:2]
        res, roff = np.frombuffer(wdata, np.uint8).astype(np.int32), woffs
        for r, pair in enumerate(want[0]):   # (the engine's lens are those of the resident stream: every chunk once)
            res, roff = oracle.merge_chunks(res, roff, pair, 256 + r)
            assert got["lens"][r] == len(res)
        ids, out_off = _encode(eng, pairs, None, data)
        same(ids, out_off, expected("disjoint_run"), "replay after a weighted train")
        assert _refusal(eng) == rounds_refusal
        # two replays back to back, 2100 merges and then 2: the merge list's device buffer keeps its capacity
        ids, out_off = _encode(eng, big_pairs, None, big_data)
        same(ids, out_off, expected("shuffled_trained"), "M = 2100")
        ids, out_off = _encode(eng, small_pairs, None, small_data)
        same(ids, out_off, expected("short_m2"), "M = 2 after M = 2100")
        ids, out_off = _encode(eng, big_pairs, None, big_data)
        same(ids, out_off, expected("shuffled_trained"), "M = 2100 again")
