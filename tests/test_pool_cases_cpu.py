"""Every case of pool_cases.py has the property it is named for (oracle only, no GPU).

Each assertion here is a condition a case must meet, not a measurement: a case that misses its branch is rebuilt.  The
capacities the cases are built around are pinned against the source text: whoever changes one moves the cases with it."""
import os
import re

import numpy as np
import pytest

import oracle
import pool_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minbpe_amd", "csrc")
ALL = [(n, f) for n in pc.CASES for f in pc.FORMS]


def _src(*path):
    with open(os.path.join(CSRC, *path), encoding="utf-8") as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, name
    return int(m.group(1))


def test_constants_match_the_sources():
    pool = _src("kernels", "k_pool.hip")
    dev = _src("bpe_device.h")
    assert pc.PL_CAP == _const(pool, "PL_CAP")
    assert pc.PL_ROWS == _const(pool, "PL_ROWS")
    assert pc.PL_GATHER == _const(pool, "PL_GATHER")
    assert pc.TIE_CAP == _const(dev, "TIE_CAP")
    assert pc.CHAIN_KCAP == _const(dev, "CH_KSWEEP")
    assert "DP_KEY_WORDS = TIE_CAP + 2;" in dev  # (the sharded MIN payload: tied_96 fills it to its last word)
    # where each capacity decides
    assert "if (s_cnt[k] <= PL_ROWS) ks = k;" in pool
    assert "if (ng > PL_GATHER || ng == 0)" in pool and "if (s < PL_GATHER)" in pool
    assert "if (n1 > PL_CAP)" in pool and "uint32_t cut = PL_CAP;" in pool
    # the round below reach, and TIE_CAP anywhere
    m = re.search(r"\(tid >= reach && P \+ size > (\d+)u\) \|\| P \+ size > \(uint32_t\)TIE_CAP", pool)
    assert m and int(m.group(1)) == pc.BELOW_REACH
    # eight thresholds: M - (M >> (2 + k)) for k = 0 .. 6, then M
    assert "th[k] = k < 7 ? M - (M >> (2 + k)) : M;" in pool and "uint32_t th[8], cn[8];" in pool
    assert pc.SHIFTS == tuple(2 + k for k in range(7))
    # the gather's loop over the rows handed out, and the default number of scanning workgroups
    assert "for (uint32_t j = blk - 1; j < n; j += nblk - 1)" in pool
    m = re.search(r"int chain_scan = (\d+);", _src("api", "api_ctx.hip"))
    assert m and int(m.group(1)) == pc.CHAIN_SCAN and pc.CHAIN_SCAN < pc.PL_ROWS
    # merge 0 is the general path's: the head pair of every stream
    assert "bool full_rowmax = (i == 0);" in _src("api", "api_train.hip")


def test_rebuild_view_on_small_tables():
    st = [((1, 2), 8, 0), ((1, 3), 5, 1), ((2, 3), 6, 2), ((4, 5), 8, 3), ((6, 7), 7, 9)]
    v = pc.rebuild_view(st)
    assert v.M == 8 and v.thresholds == (6, 7, 8, 8, 8, 8, 8, 8) and v.rows == (4, 3, 2, 2, 2, 2, 2, 2)
    assert (v.picked, v.theta, v.pairs, v.levels, v.kept) == (0, 6, 4, (2, 1, 1), 4)
    v = pc.rebuild_view(st, n_rows=3)
    assert (v.picked, v.theta, v.pairs, v.levels) == (1, 7, 3, (2, 1))
    v = pc.rebuild_view(st, n_rows=1)
    assert (v.picked, v.theta, v.pairs, v.levels) == (None, None, 2, (2,))
    assert pc.rebuild_view([]).M == 0
    many = [((i, 300), 5, i) for i in range(257)]
    assert pc.rebuild_view(many, n_rows=300).kept == 0
    assert pc.rebuild_view(many + [((0, 301), 6, 999)], n_rows=300).kept == 1


@pytest.mark.parametrize("name,form", ALL)
def test_case_is_what_it_says(name, form):
    case = pc.CASES[name]
    data, offs = pc.stream(name, form)
    assert len(data) <= (2_000_000 if pc.is_big(name) else 500_000 if case.M >= 256 else 10_000), len(data)
    st = pc.case_stats(name, form)
    v = pc.rebuild_view(st)
    for field, want in pc.PROPERTY[name].items():
        got = getattr(v, field)
        assert (got[:len(want)] if field == "levels" else got) == want, (field, got, want)
    # the designed pairs: a != b, no first token is a second token, every count as designed
    designed = case.designed()
    firsts, seconds = {a for a, _ in designed}, {b for _, b in designed}
    assert not firsts & seconds and all(a != b for a, b in designed)
    table = {p: c for p, c, _ in st}
    assert [table[p] for p in designed] == case.counts.tolist()
    # everything else: the tail below the deepest threshold, the noise far below what is picked (at M = 2 and 8: once)
    tail = {tuple(p) for p in case.tail_pairs.tolist()} if case.has_tail(form) else set()
    assert not ({a for a, _ in tail} & seconds) and not ({b for _, b in tail} & firsts)
    if tail:
        assert max(table[p] for p in tail) < v.thresholds[0] and len(tail) == pc.TAIL
    noise = max([c for p, c, _ in st if p not in tail and p not in set(designed)], default=0)
    floor = v.theta if v.theta is not None else v.M
    print(name, form, len(data), "bytes; noise", noise, "tail", sorted({table[p] for p in tail}, reverse=True)[:3], v)
    assert noise <= max(1, floor // 3) and noise < floor
    if form == "bare":
        assert noise == 0
    if tail and form == "body":
        low = min(table[p] for p in tail)
        assert noise < low - (low >> 2)  # (a rebuild inside the tail picks a threshold above the noise)


@pytest.mark.parametrize("name,form", ALL)
def test_oracle_run_passes_the_seam(name, form):
    case = pc.CASES[name]
    nm = case.num_merges(form)
    pairs, counts, lens, ids, starts = pc.expected(name, form)
    assert len(pairs) == nm == 1 + len(case.pairs) + (pc.TAIL if case.has_tail(form) else 0)
    assert pairs[0] == pc.HEAD and counts[0] == case.M + 1
    assert all(a != b for a, b in pairs)  # (`deferred` on the device then counts capacity hand-backs only)
    designed = case.designed()
    assert sorted(pairs[1:1 + len(designed)]) == sorted(designed)
    assert len(ids) == lens[-1] and starts[0] == 0
    # inside the seam's level -- the top one -- the reference's order is not the order by pair value
    top = [p for p, c in zip(pairs[1:], counts[1:]) if c == case.M]
    assert len(top) == pc.PROPERTY[name].get("levels", (len(top),))[0] or pc.is_big(name)
    assert len(top) >= 2 and top != sorted(top), top[:8]


def test_training_ends_inside_the_first_batch():
    name, nm = pc.MID_BATCH
    full = pc.expected(name, "bare")
    cut = pc.expected(name, "bare", nm)
    assert 1 < nm - 1 < pc.CHAIN_KCAP < len(pc.CASES[name].pairs)
    assert cut[0] == full[0][:nm] and cut[1] == full[1][:nm] and set(cut[1][1:]) == {pc.CASES[name].M}


@pytest.mark.parametrize("small,large,field", pc.NEIGHBOURS)
def test_neighbours_differ_in_one_pair(small, large, field):
    """the larger case is the smaller one plus ONE designed pair: the quantity named moves by one, and nothing else that
    rebuild_view reports moves but what that pair moves with it"""
    a = {p: c for p, c, _ in pc.case_stats(small, "bare")}
    b = {p: c for p, c, _ in pc.case_stats(large, "bare")}
    extra = set(b) - set(a)
    assert len(extra) == 1 and not set(a) - set(b)
    assert all(b[p] == a[p] for p in a)
    va, vb = pc.rebuild_view(pc.case_stats(small, "bare")), pc.rebuild_view(pc.case_stats(large, "bare"))
    assert va.M == vb.M and va.thresholds == vb.thresholds
    assert vb.pairs == va.pairs + 1
    if field == "rows":
        assert vb.rows == tuple(r + 1 for r in va.rows)
    else:
        assert vb.rows[0] - va.rows[0] in (0, 1) and va.picked == vb.picked == 0 and va.theta == vb.theta
    if field == "levels":
        assert sum(vb.levels) == sum(va.levels) + 1 and len(vb.levels) == len(va.levels)
    # the designed pairs of the body forms are the same ones
    ca, cb = pc.CASES[small], pc.CASES[large]
    assert cb.designed()[:len(ca.pairs)] == ca.designed() and cb.counts[:len(ca.pairs)].tolist() == ca.counts.tolist()


def test_the_sides_of_every_limit():
    view = lambda n: pc.rebuild_view(pc.case_stats(n, "bare"))
    assert view("rows_128").rows[7] == pc.PL_ROWS and view("rows_129").picked is None
    assert view("rows_128_m2").thresholds == (2,) * 8 and len(set(view("rows_128").thresholds)) == 8
    assert view("rows_depth").rows[2] == pc.PL_ROWS and view("rows_depth").rows[1] == pc.PL_ROWS + 1
    assert view("rows_depth_all").rows[0] == pc.PL_ROWS and view("rows_depth_all").levels[0] <= pc.TIE_CAP
    assert view("gather_1024").pairs == pc.PL_GATHER and max(view("gather_1025").levels) <= 8
    assert view("cap_256").pairs == pc.PL_CAP and view("cap_257").kept == 255 and view("cap_257_l4").kept == pc.PL_CAP
    assert view("cap_300_l3").kept == 255 and view("cap_one_level_257").kept == 0
    assert view("tied_96").levels[0] == pc.TIE_CAP and view("tied_97").rows[0] <= pc.TIE_CAP
    assert sum(view("tied_two_levels").levels) == pc.TIE_CAP + 1
    assert sum(view("below_reach_16").levels) == pc.BELOW_REACH
    # the top level of the below-reach cases shares its first token: it ends the reach where first tokens are not shared
    for n in ("below_reach_16", "below_reach_17"):
        top = [p for p, c, _ in pc.case_stats(n, "bare") if c == pc.CASES[n].M]
        assert len(top) == 2 and top[0][0] == top[1][0] and ("chain_share_first", 0) in pc.CASES[n].opts


@pytest.mark.parametrize("form", pc.FORMS)
def test_fast_oracle_and_encode_are_the_plain_ones_on_the_gather_streams(form):
    """the gather cases' expectations come from oracle.train_fast and oracle.encode (pool_cases.expected)"""
    name = "gather_1025"
    data, offs = pc.stream(name, form)
    pairs, counts, lens, ids, starts = pc.expected(name, form)
    assert (pairs, counts, lens) == oracle.train(data, len(pairs), offs)
    if form == "bare":
        ids2, starts2 = pc.replay(data, offs, pairs)
        assert np.array_equal(ids, ids2) and starts == starts2
    for small in ("cap_257", "tied_97"):
        d, o = pc.stream(small, form)
        e = pc.expected(small, form)
        ids3, starts3 = pc.replay_by_encode(d, o, e[0])
        assert np.array_equal(e[3], ids3) and e[4] == starts3
