"""Training across the token ids at which the engine changes what it runs -- 1024, 1920 and 2048 -- under every variant.

The seams (merge i makes id 256 + i, so they are crossed by merges 768, 1664 and 1792):
  id 1024  CH_DCAP (k_chain.hip): dense chain steps are enqueued while 256 + hi_dense + 1 <= CH_DCAP (chain_dense in
           api_train.hip, want_dense in api_rccl.hip); after that the general path's single merges.  It is also where
           every kernel that gives a token to a thread of a 1024-thread workgroup goes from one workgroup to two: the
           table update of a one-launch step (gapply in launch_chain_step), the per-wave records of k_sel_lean, the
           pool's scans.
  id 1920  LDSD_CAP (bpe_device.h): launch_passes2 picks k_merge_ab_sparse<true> / k_merge_ab_dense_early<...> (delta in
           LDS tables) while newid + 1 <= LDSD_CAP, k_merge_ab_sparse<false> / k_merge_ab_dense<...> (global replicas of
           the delta, delta_layout) beyond.
  id 2048  a third 1024-thread workgroup of tokens.
  vcap     ensure_table rounds 256 + num_merges up to 64 and never shrinks: 768, 1664 and 1792 merges on a FRESH ctx give a
           table whose last row is exactly id 1023, 1919, 2047; a re-used ctx keeps the stride of an earlier, larger run.

One corpus, native.synth_text(600_000, 71), in two forms (GPT-4-split chunks; one stream), trained to 2200 merges: the
oracle's lists (oracle.train_fast, pinned to oracle.train by test_fast_oracle.py) and the stream after 767 .. 2200 merges
(oracle.merge_chunks replayed once per form) are computed once per module.  Integer work: every comparison is exact --
pairs, counts, lens and the resident stream.  The tests without the gpu mark assert, with the oracle alone, the facts about
the corpus that the GPU cases rely on: every seam is crossed inside a tie level or exactly at a level's edge."""
import contextlib

import numpy as np
import pytest

import oracle
from helpers import CHAIN_DEFAULTS, CHAIN_OPTIONS, VARIANTS, reset_variant, set_variant
from test_gpu_parity import _chain_ranks, _lockstep

gpu = pytest.mark.gpu
NM = 2200
SEAM_MERGES = (768, 1664, 1792)  # the merges that make ids 1024 (CH_DCAP, a second token workgroup), 1920 (LDSD_CAP), 2048
SEAM_NMS = tuple(m + d for m in SEAM_MERGES for d in (-1, 0, 1))
NM_PER_MERGE = 1700  # the per-merge protocol all-reduces on the host at every merge: 1700 crosses ids 1024 and 1920
KEEP = tuple(sorted(set(SEAM_NMS) | {NM_PER_MERGE, NM}))  # the stream is kept after these many merges
FORMS = ("chunked", "stream")
TIE_CAP = 96   # bpe_device.h
CH_KSWEEP = 31  # bpe_device.h: most pairs of one chain step
CH_KDENSE = 6   # k_chain.hip: most pairs of a dense chain step
LAST_DENSE_STEP_MERGE = 766  # a dense chain step makes ids up to 1022 = CH_DCAP - 2 (256 + hi_dense + 1 <= CH_DCAP)
DEPTH = 8  # api_ctx.hip's default, what reset_variant sets
WAIT = 30  # seconds a rank waits at a barrier for its peers
DEFAULT = (1, 0, 2, 1, 1)  # set_variant's arguments for the default engine
_REF = {}

# what every option a case may set goes back to (api_ctx.hip); mode, merge, slots, sparse, lean, chain, small_slots, lean_sum,
# lean_chain, aa_sparse, lean_backoff and depth are restored by reset_variant
DEFAULTS = dict(CHAIN_DEFAULTS, lean_count=1 << 20, chain_dense=1, lds_delta=1, rep_min=4, rep_max=8, tie_index=1,
                lean_select=1, sparse_ratio=1, lean_scan=31)
BY_RESET = {"mode", "merge", "slots", "sparse", "lean", "chain", "lean_sum", "lean_chain", "aa_sparse", "lean_backoff", "depth"}


# ---------------------------------------------------------------------------
# the corpus and its reference

def _ref(native, form):
    """dict(data, offs, pairs, counts, lens, ids = {k: the stream after k merges, k in KEEP}) -- once per form"""
    if form in _REF:
        return _REF[form]
    data = native.synth_text(600_000, 71)
    offs = native.split_offsets(data, 4) if form == "chunked" else None
    pairs, counts, lens = oracle.train_fast(data, NM, offs, raise_on_empty=False)
    ids = np.frombuffer(data, dtype=np.uint8).astype(np.int32)
    kept, o = {}, offs
    for i, p in enumerate(pairs):
        ids, off_full = oracle.merge_chunks(ids, o, p, 256 + i)
        o = off_full[:-1]
        if i + 1 in KEEP:
            kept[i + 1] = ids.copy()
            kept[i + 1].flags.writeable = False
    _REF[form] = dict(form=form, data=data, offs=offs, pairs=pairs, counts=counts, lens=lens, ids=kept)
    return _REF[form]


def _first_at_most(counts, threshold):
    """the first merge whose count is <= threshold: from the merge after it on the host may have seen such a count"""
    return next(i for i, c in enumerate(counts) if c <= threshold)


def _count_at_899(ref):
    return ref["counts"][899]


def _count_at_1799(ref):
    return ref["counts"][1799]


def _level(counts, i):
    """(first merge, last merge, count) of the run of equal counts that holds merge i"""
    lo = hi = i
    while lo > 0 and counts[lo - 1] == counts[i]:
        lo -= 1
    while hi + 1 < len(counts) and counts[hi + 1] == counts[i]:
        hi += 1
    return lo, hi, counts[i]


def _first_diff(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"first difference at merge {k} (id {256 + k}): got {got[k:k + 3]}, want {want[k:k + 3]} ({len(got)} of {len(want)})"


def _check(eng, res, ref, nm, tag):
    """pairs, counts, lens and the resident stream against the first nm entries of the reference"""
    assert res["n_done"] == nm, (tag, res["n_done"])
    for name in ("pairs", "counts", "lens"):
        assert res[name] == ref[name][:nm], (tag, name, _first_diff(res[name], ref[name][:nm]))
    got = eng.read_ids()
    assert len(eng) == len(got) == ref["lens"][nm - 1], tag
    assert np.array_equal(got, ref["ids"][nm]), tag


@contextlib.contextmanager
def _options(eng, variant, opts):
    """set_variant, then the options -- and back to the defaults whatever happens in between"""
    set_variant(eng, *variant)
    try:
        for k, v in opts:
            eng.set_option(k, v)
        yield
    finally:
        for k, _ in opts:
            if k not in BY_RESET:
                eng.set_option(k, DEFAULTS[k])
        reset_variant(eng)


def _resolve(opts, ref):
    """option values given as functions of the reference (a count the oracle reports) -> numbers"""
    return tuple((k, v(ref) if callable(v) else v) for k, v in opts)


def _train_and_check(eng, ref, nm, tag):
    eng.load_bytes(ref["data"], ref["offs"])
    res = eng.train(nm)
    st = eng.train_stats()
    print(tag, st)
    _check(eng, res, ref, nm, tag)
    return st


# ---------------------------------------------------------------------------
# the corpus is what the cases below take it to be (CPU: the oracle alone)

TABLE = {  # the oracle on this corpus
    "chunked": dict(counts={0: 23371, 899: 45, 1799: 19, 2199: 14},
                    levels={767: (759, 767, 55), 768: (768, 776, 54), 1663: (1608, 1665, 21), 1664: (1608, 1665, 21),
                            1791: (1742, 1807, 19), 1792: (1742, 1807, 19)},
                    same=(829, 1655, 1858), first=(884, 1742)),
    "stream": dict(counts={0: 23371, 899: 50, 1799: 21, 2199: 16},
                   levels={767: (764, 774, 62), 768: (764, 774, 62), 1663: (1642, 1698, 23), 1664: (1642, 1698, 23),
                           1791: (1751, 1824, 21), 1792: (1751, 1824, 21)},
                   same=(758, 1668, 1689, 1765, 1771, 1809), first=(895, 1751)),
}


@pytest.mark.parametrize("form", FORMS)
def test_corpus_gives_2200_merges_and_the_stated_counts(native, form):
    ref = _ref(native, form)
    assert len(ref["pairs"]) == len(ref["counts"]) == len(ref["lens"]) == NM
    assert sorted(ref["ids"]) == list(KEEP)
    assert all(len(ref["ids"][k]) == ref["lens"][k - 1] for k in KEEP)
    if form == "chunked":
        assert len(ref["offs"]) == 102_368
    assert {i: ref["counts"][i] for i in TABLE[form]["counts"]} == TABLE[form]["counts"]
    assert all(x >= y for x, y in zip(ref["counts"], ref["counts"][1:]))  # (the levels below are runs of equal counts)


@pytest.mark.parametrize("form", FORMS)
def test_every_seam_is_crossed_inside_a_tie_level_or_at_its_edge(native, form):
    """The merge that makes a seam's id and the merge before it tie with their neighbours: the seam lies inside a level
    of equal counts, or a level ends exactly on it (chunked, id 1024).  Some of these levels hold more pairs than a
    chain step's batch (CH_KSWEEP) and fewer than TIE_CAP: the step that crosses the seam is one of several of its level."""
    counts = _ref(native, form)["counts"]
    got = {i: _level(counts, i) for i in TABLE[form]["levels"]}
    assert got == TABLE[form]["levels"]
    sizes = []
    for m in SEAM_MERGES:
        before, at = got[m - 1], got[m]
        assert before[1] - before[0] >= 1 and at[1] - at[0] >= 1  # (both tie with a neighbour)
        assert before == at or (before[1] == m - 1 and at[0] == m)
        sizes += [before[1] - before[0] + 1, at[1] - at[0] + 1]
    assert any(CH_KSWEEP < s < TIE_CAP for s in sizes), sizes
    assert max(sizes) < TIE_CAP


def test_same_token_merges_lie_near_the_seams(native):
    """a == b merges (the a == b pass, a chain step's own or the general path's) near every seam; in the stream form
    within 12 merges of ids 1024 and 1920"""
    for form in FORMS:
        pairs = _ref(native, form)["pairs"]
        same = [i for i, (a, b) in enumerate(pairs) if a == b]
        assert set(TABLE[form]["same"]) <= set(same), (form, same)
    same = [i for i, (a, b) in enumerate(_ref(native, "stream")["pairs"]) if a == b]
    for m in (768, 1664):
        assert any(abs(i - m) <= 12 for i in same), (m, same)


@pytest.mark.parametrize("form", FORMS)
def test_count_thresholds_fall_between_and_after_the_seams(native, form):
    """lean_count = counts[899] brings the index up between ids 1024 and 1920, lean_count = counts[1799] after id 1920:
    the first merge with such a count lies after the seam's merge, and so far before the run's end (and, for the first,
    before merge 1664) that the units in flight -- depth + 1 at the most -- cannot carry the switch past it."""
    ref = _ref(native, form)
    mid, late = _first_at_most(ref["counts"], _count_at_899(ref)), _first_at_most(ref["counts"], _count_at_1799(ref))
    assert (mid, late) == TABLE[form]["first"]
    assert 768 < mid <= 899 and mid + 64 < 1664
    assert 1664 < late <= 1799 and late + 64 < NM
    assert LAST_DENSE_STEP_MERGE < mid  # (the dense chain steps end before the index comes up)


# ---------------------------------------------------------------------------
# 1. every variant

@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode,mimpl,slots,sparse,lean", VARIANTS)
def test_every_variant_across_the_seams(engine, native, form, mode, mimpl, slots, sparse, lean):
    """All 21 VARIANTS, default options otherwise, 2200 merges (mode = 0 recounts 2200 times: 600 KB each)."""
    ref = _ref(native, form)
    with _options(engine, (mode, mimpl, slots, sparse, lean), ()):
        _train_and_check(engine, ref, NM, (form, mode, mimpl, slots, sparse, lean))


# ---------------------------------------------------------------------------
# 2. option sets that pin a path on both sides of the seams
#
# Every set: the default variant + the options; a function of (stats, reference) that fails if the path was not taken.
# Read off bpe_train (api_train.hip), plan_pass2 and launch_passes2 (api_ctx.hip); the stream has 586 slots of 1024 ids,
# "small" for plan_pass2 (T <= 16 * SPARSE_GRID): a pass is sparse once the host has seen a count <= lean_count.

def _general_dense_passes(ref, lean_count):
    """A lower bound of the dense passes of a run with this lean_count: merges 767 .. F, F the first merge whose count
    is <= lean_count, are single merges of the general path through a dense kernel.  Dense chain steps end at merge 766
    (LAST_DENSE_STEP_MERGE); what the host knows when it enqueues merge i <= F is the count of a merge before F, which is
    > lean_count: plan_pass2 says "not sparse", lean_wanted says no."""
    last = NM - 1 if lean_count == 0 else _first_at_most(ref["counts"], lean_count)
    return last - LAST_DENSE_STEP_MERGE


def _dense_for_ever(st, ref):
    # no count is ever <= 0: no sparse pass, no index, no lean iteration; chain_dense holds from merge 1 to id 1022, then
    # k_merge_ab_dense_early<false> to id 1919, then k_merge_ab_dense<false> -- one dense pass per merge from 767 on
    assert st["sparse"] == 0 and st["index_builds"] == 0 and st["steps"] > 0, st
    assert st["dense"] > 1400 and st["dense"] >= _general_dense_passes(ref, 0), st
    assert st["fused_steps"] == 0, st


def _dense_no_steps(st, ref):
    # ... and without chain_dense every merge is one general iteration, one dense pass
    assert st["steps"] == 0 and st["sparse"] == 0 and st["index_builds"] == 0 and st["lean"] == 0, st
    assert st["dense"] == NM, st


def _index_comes_up(threshold):
    def fact(st, ref):
        # dense chain steps, general dense passes up to the first count <= lean_count at least, then the index and
        # sparse chain steps
        assert st["dense"] >= _general_dense_passes(ref, threshold(ref)) > 0, st
        assert st["sparse"] > 0 and st["index_builds"] > 0 and st["steps"] > 0, st
    return fact


def _general_through_the_index(st, ref):
    # sparse = 2: plan_pass2 says "sparse" from merge 0 on; lean = 0: no lean iteration, and chain_dense needs c->lean
    assert st["lean"] == 0 and st["steps"] == 0 and st["dense"] == 0, st
    assert st["sparse"] == NM and st["index_builds"] > 0, st


def _default_engine_runs(st, ref):
    # lds_delta = 0 takes the dense chain steps away (chain_dense needs c->lds_delta), not the indexed ones
    assert st["steps"] > 0 and st["index_builds"] > 0 and st["lean"] > 0, st


def _few_steps(st, ref):
    # tie_index = 0 / lean_select = 0 switch the INDEXED chain steps off (`chain` in bpe_train needs both); the issue's
    # table expected steps == 0, but chain_dense does not ask for them: while the host knows no count yet -- merge 0 is in
    # flight, at most `depth` units behind it -- merges 1 .. are dense chain steps.  What the code guarantees: at most
    # `depth` steps (a run with chain steps has hundreds), lean iterations after them.
    assert st["steps"] <= DEPTH and st["fused_steps"] == 0 and st["lean"] > 0, st


def _no_steps(st, ref):
    assert st["steps"] == 0 and st["lean"] > 0, st


def _lean(st, ref):
    assert st["lean"] > 0, st


def _nothing(st, ref):
    pass


OPTION_SETS = {
    "dense_for_ever": ((("lean_count", 0),), _dense_for_ever),
    "dense_no_steps": ((("lean_count", 0), ("chain_dense", 0)), _dense_no_steps),
    "index_between_1024_and_1920": ((("lean_count", _count_at_899),), _index_comes_up(_count_at_899)),
    "index_after_1920": ((("lean_count", _count_at_1799),), _index_comes_up(_count_at_1799)),
    "general_through_the_index": ((("sparse", 2), ("lean", 0)), _general_through_the_index),
    # global replicas of the delta from the first merge on, counts of 23 k included
    "no_lds_tables": ((("lds_delta", 0),), _default_engine_runs),
    "no_lds_tables_dense": ((("lds_delta", 0), ("lean_count", 0)), _dense_no_steps),
    # delta_layout: min(min(shift, max(want, rep_min)), rep_max) -- one replica | `want` alone | the most the buffer holds
    "one_replica": ((("lds_delta", 0), ("lean_count", 0), ("rep_min", 0), ("rep_max", 0)), _dense_no_steps),
    "replicas_by_count": ((("lds_delta", 0), ("lean_count", 0), ("rep_min", 0), ("rep_max", 8)), _dense_no_steps),
    "most_replicas": ((("lds_delta", 0), ("lean_count", 0), ("rep_min", 7), ("rep_max", 8)), _dense_no_steps),
    # ties swept / pairs selected the general way at a vocabulary of more than 1024
    "ties_swept": ((("tie_index", 0),), _few_steps),
    "ties_swept_no_dense_steps": ((("tie_index", 0), ("chain_dense", 0)), _no_steps),
    "general_selection": ((("lean_select", 0),), _few_steps),
    "general_selection_no_dense_steps": ((("lean_select", 0), ("chain_dense", 0)), _no_steps),
    # (586 slots: plan_pass2 reads sparse_ratio for streams of more than 16 * SPARSE_GRID slots only -- this pins that the
    # largest value is harmless here, nothing more)
    "sparse_ratio_64": ((("sparse_ratio", 64),), _nothing),
    # workgroups of k_rowmax_lean / k_rowsel_lean / k_sel_lean: one, and the most the option takes -- there with lean
    # iterations on every merge, which launch one of them each
    "lean_scan_1": ((("lean_scan", 1),), _lean),
    "lean_scan_1024": ((("lean_scan", 1024), ("lean", 2), ("chain", 0)), _lean),
}


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_option_sets_pin_a_path_across_the_seams(engine, native, form, name):
    ref = _ref(native, form)
    opts, fact = OPTION_SETS[name]
    with _options(engine, DEFAULT, _resolve(opts, ref)):
        st = _train_and_check(engine, ref, NM, (form, name))
        fact(st, ref)


# ---------------------------------------------------------------------------
# 3. chain-step options across the seams

def _chain_option_facts(st, opts):
    assert st["steps"] > 0, st
    # the step is ONE launch (k_step.hip) wherever its selection is the pool and the option stands
    if ("fuse_step", 1) in opts:
        assert st["fused_steps"] > 0, st
    else:
        assert st["fused_steps"] == 0, st
    if ("small_slots", 2) in opts and st["index_builds"]:
        assert st["slot_ids"] == 256, st
    if ("small_slots", 0) in opts:
        assert st["slot_ids"] == 1024, st


@gpu
@pytest.mark.parametrize("form,opts", [("chunked", o) for o in CHAIN_OPTIONS] +
                         [("stream", o) for o in CHAIN_OPTIONS if ("fuse_step", 1) in o])
def test_chain_step_options_across_the_seams(engine, native, form, opts):
    """Every CHAIN_OPTIONS entry with every merge a chain step through the index (sparse = 2, lean = 2 with chain steps),
    as test_chain_step_options_cross_check runs them to id 755.  The one-launch entries (fuse_step = 1) are the point: the
    table update of k_step takes a token per thread, gapply = (zhi + 1 + 1023) / 1024 workgroups -- two from id 1024, three
    from id 2048 (zhi is the bound the host knows, so three are launched for the last few hundred merges) -- and with
    lean_grid = 8 the grid is sized from max(lean_grid, gapply)."""
    ref = _ref(native, form)
    with _options(engine, (1, 0, 2, 2, 7), opts):
        st = _train_and_check(engine, ref, NM, (form, opts))
        _chain_option_facts(st, opts)


# ---------------------------------------------------------------------------
# 4. runs that end on a seam, on fresh contexts

FRESH = {
    "default": (DEFAULT, ()),
    "dense": (DEFAULT, (("lean_count", 0),)),
    # the hand-over from dense chain steps to single merges at id 1024 happens with that many units in flight
    "dense_depth_0": (DEFAULT, (("lean_count", 0), ("depth", 0))),
    "dense_depth_64": (DEFAULT, (("lean_count", 0), ("depth", 64))),
    "one_launch_steps": ((1, 0, 2, 2, 7), (("fuse_step", 1),)),
}


def _fresh_facts(st, setting):
    if setting.startswith("dense"):
        assert st["sparse"] == 0 and st["index_builds"] == 0 and st["steps"] > 0, st
    if setting == "one_launch_steps":
        assert st["fused_steps"] > 0, st


@gpu
@pytest.mark.parametrize("nm", SEAM_NMS)
@pytest.mark.parametrize("setting", list(FRESH))
def test_runs_that_end_on_a_seam_on_a_fresh_ctx(native, setting, nm):
    """A ctx of its own, so that the table's stride is exactly round64(256 + nm): its last row is id 1023, 1919 or 2047
    for nm = 768, 1664, 1792.  The stream form; the result is the first nm entries of the reference."""
    ref = _ref(native, "stream")
    variant, opts = FRESH[setting]
    eng = native.Engine(0)
    try:
        set_variant(eng, *variant)
        for k, v in opts:
            eng.set_option(k, v)
        st = _train_and_check(eng, ref, nm, (setting, nm))
        _fresh_facts(st, setting)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("setting", list(FRESH))
def test_table_grows_and_stays_large_on_one_ctx(native, setting):
    """768, then 2200, then 768 merges on one fresh ctx, the bytes loaded once: the table, the record array and the delta
    buffer grow and then stay large -- the third run works at a stride of 2496 on ids that end at 1023."""
    ref = _ref(native, "stream")
    variant, opts = FRESH[setting]
    eng = native.Engine(0)
    try:
        set_variant(eng, *variant)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_bytes(ref["data"], ref["offs"])
        for turn, nm in enumerate((768, NM, 768)):
            res = eng.train(nm)
            st = eng.train_stats()
            print(setting, turn, nm, st)
            _check(eng, res, ref, nm, (setting, turn, nm))
            _fresh_facts(st, setting)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 5. the sharded loop of chain steps (bpe_dp_train_cb), ranks emulated on one GPU

def _chunks(ref):
    ends = np.append(ref["offs"][1:], np.uint64(len(ref["data"]))).astype(np.int64)
    return [ref["data"][int(a):int(b)] for a, b in zip(ref["offs"].astype(np.int64), ends)]


def _dp_default(stats, ref):
    assert all(s["steps"] > 0 and s["lean"] > NM // 2 for s in stats), stats


def _dp_dense(stats, ref):
    # want_dense (api_rccl.hip) to id 1022, then the per-merge schedule for more than 1400 merges, every pass a dense one
    assert all(s["sparse"] == 0 and s["steps"] > 0 for s in stats), stats
    assert all(s["dense"] > 1400 and s["dense"] >= _general_dense_passes(ref, 0) for s in stats), stats


def _dp_index_between(stats, ref):
    # dense steps, the per-merge schedule from id 1023 on, indexed steps once a count <= lean_count has been seen
    floor = _general_dense_passes(ref, _count_at_899(ref))
    assert all(s["dense"] >= floor > 0 and s["sparse"] > 0 and s["steps"] > 0 for s in stats), stats


def _dp_kcap_1(stats, ref):
    assert all(s["steps"] > 0 and s["lean"] <= s["steps"] for s in stats), stats  # (a step is one merge at the most)


def _dp_kcap_15(stats, ref):
    assert all(0 < s["steps"] < s["lean"] for s in stats), stats


DP_SETS = {
    "default": ((), _dp_default),
    "dense": ((("lean_count", 0),), _dp_dense),             # SUM payload of the per-merge schedule: vcap * 4 + 64 words
    "index_between_1024_and_1920": ((("lean_count", _count_at_899),), _dp_index_between),
    "dp_kcap_15": ((("dp_kcap", 15),), _dp_kcap_15),        # SUM payload 2 K S + 64 words, S up to 2496 ids
    "dp_kcap_1": ((("dp_kcap", 1),), _dp_kcap_1),
}


@gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(DP_SETS))
def test_sharded_chain_steps_across_the_seams(native, name, world):
    pytest.importorskip("torch")
    ref = _ref(native, "chunked")
    opts, fact = DP_SETS[name]
    out, errs, stats = _chain_ranks(native, _chunks(ref), NM, world, _resolve(opts, ref), timeout=WAIT)
    assert not any(errs), errs
    for r, res in enumerate(out):
        print(name, world, "rank", r, stats[r])
        assert res["n_done"] == NM, (r, res["n_done"])
        for key in ("pairs", "counts", "lens"):
            assert res[key] == ref[key], (name, world, r, key, _first_diff(res[key], ref[key]))
    assert len({s["steps"] for s in stats}) == 1, stats  # (the step records are replicas)
    fact(stats, ref)


@gpu
def test_sharded_chain_steps_with_per_rank_dedup_across_the_seams(native):
    """every rank de-duplicates its own shard (weights in the id words, counts still global): the plain list's merges and
    counts (the lengths are those of the de-duplicated shards)"""
    pytest.importorskip("torch")
    ref = _ref(native, "chunked")
    out, errs, stats = _chain_ranks(native, _chunks(ref), NM, 2, dedup=True, timeout=WAIT)
    assert not any(errs), errs
    for r, res in enumerate(out):
        assert res["n_done"] == NM, (r, res["n_done"])
        for key in ("pairs", "counts"):
            assert res[key] == ref[key], (r, key, _first_diff(res[key], ref[key]))
    assert out[0]["lens"] == out[1]["lens"] and all(x < y for x, y in zip(out[0]["lens"], ref["lens"]))
    _dp_default(stats, ref)


# ---------------------------------------------------------------------------
# 6. the per-merge protocol (GpuShard)

@gpu
@pytest.mark.parametrize("slots,sparse", [(1, 1), (2, 1), (2, 2)])
def test_per_merge_protocol_across_the_seams(native, slots, sparse):
    """1700 merges (the host all-reduces at every one): ids 1024 and 1920 are crossed.  slots = 2: by k_merge_ab_sparse<true>
    then <false> (sparse = 1 goes through the index as soon as a count is known: these shards are small ones for
    plan_pass2); slots = 1: by the first slotted form's pass.  The dense kernels of this protocol are what the sharded loop
    runs after its dense steps (DP_SETS["dense"])."""
    pytest.importorskip("torch")
    ref = _ref(native, "chunked")
    pairs, counts, lens = _lockstep(native, _chunks(ref), NM_PER_MERGE, 2, slots, sparse=sparse)
    for key, got in (("pairs", pairs), ("counts", counts), ("lens", lens)):
        assert got == ref[key][:NM_PER_MERGE], (slots, sparse, key, _first_diff(got, ref[key][:NM_PER_MERGE]))
