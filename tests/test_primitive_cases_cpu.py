"""Every case of primitive_cases.py has the property it is named for (oracle only, no GPU).

Each assertion here is a condition a case must meet, not a measurement: a case that misses its regime is rebuilt."""
import os
import re

import numpy as np
import pytest

import oracle
import primitive_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minbpe_amd", "csrc")


def _src(*path):
    with open(os.path.join(CSRC, *path), encoding="utf-8") as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, name
    return int(m.group(1))


def test_constants_match_the_sources():
    dev = _src("bpe_device.h")
    sel = _src("kernels", "k_select.hip")
    # the contiguous view's tile: view_tile(SlotRef) returns TILE = (MT / 64) * MJ * 256 of the geometry the host code
    # names (bpe_g4), and k_select<SlotRef> is launched from that namespace
    assert re.search(r"view_tile\(const SlotRef &\)\s*\{\s*return TILE;", sel)
    assert "TILE = (MT / 64) * WAVE_SPAN" in dev and "WAVE_SPAN = MJ * 256" in dev
    mj = int(re.search(r"BPE_GEOMETRY\(bpe_g4,\s*(\d+),", dev).group(1))
    assert "using namespace bpe::bpe_g4;" in _src("bpe_api.hip")
    assert "k_select<SlotRef>, dim3(blocks)" in _src("api", "api_ctx.hip")  # (not GK(...): always bpe_g4)
    assert pc.TILE == (_const(dev, "MT") // 64) * mj * 256 == 4096
    assert pc.TIE_CAP == _const(dev, "TIE_CAP")
    assert pc.ARGMAX_ROWS == _const(dev, "ARGMAX_ROWS")
    assert pc.TIE_BLOCKS == _const(dev, "TIE_BLOCKS")
    assert pc.SEL_ROWS == _const(sel, "SEL_RPT") * 1024 == 20480
    assert pc.TIE_WIN == _const(sel, "TIE_WIN")
    assert _const(dev, "LDSD_CAP") == 1920 and {1919, 1920, 1921, 2048, 2049} <= set(pc.WIDTHS)


# ---------------------------------------------------------------------------
# classify() against a dictionary restatement of get_stats + max

def _restate(ids, offsets):
    ids = [int(x) for x in ids]
    cuts = set(int(o) for o in offsets) if offsets is not None else set()
    counts, first = {}, {}
    for p in range(len(ids) - 1):
        if p + 1 in cuts:
            continue
        pair = (ids[p], ids[p + 1])
        counts[pair] = counts.get(pair, 0) + 1
        first.setdefault(pair, p)
    if not counts:
        return pc.Regime(0, 0, 0, 0, None, None)
    best = max(counts, key=counts.get)  # the first maximum in insertion order
    M = counts[best]
    rows = {}
    for (a, _b), c in counts.items():
        if c == M:
            rows[a] = rows.get(a, 0) + 1
    return pc.Regime(M, sum(v == 1 for v in rows.values()), sum(v > 1 for v in rows.values()), sum(rows.values()),
                     first[best], best)


SMALL = ["unique", "tied_2", "tied_97", "multi_1", "multi_1_single_94", "multi_1_single_95", "side_hi", "side_lo",
         "pos0_5", "tail_120", "tile0_last_word_5", "astride_5", "astride_120"]


@pytest.mark.parametrize("name", SMALL)
def test_classify_vs_dictionary(name):
    ids, off, reg = pc.argmax_case(name)
    assert reg == _restate(ids, off)


def test_classify_small_streams():
    assert pc.classify([5]) == pc.Regime(0, 0, 0, 0, None, None)
    assert pc.classify([1, 2, 3, 1, 2]) == pc.Regime(2, 1, 0, 1, 0, (1, 2))
    assert pc.classify([1, 2, 1, 3, 4, 5, 4, 5]) == pc.Regime(2, 1, 0, 1, 4, (4, 5))
    assert pc.classify([1, 2, 1, 3, 9, 1, 2, 1, 3]) == pc.Regime(2, 1, 1, 3, 0, (1, 2))
    assert pc.classify([1, 2, 1, 2], [0, 2]) == _restate([1, 2, 1, 2], [0, 2]) == pc.Regime(2, 1, 0, 1, 0, (1, 2))
    rng = np.random.default_rng(3)
    for k in (2, 3, 6):
        ids = rng.integers(250, 250 + k, size=400)
        off = np.unique(np.concatenate([[0], rng.integers(0, 400, size=9)])).astype(np.uint64)
        assert pc.classify(ids, off) == _restate(ids, off)


def test_filler_holds_every_pair_once():
    ids = pc._filler(20000)
    st = oracle.get_stats(ids)
    assert len(st) == len(ids) - 1 and all(c == 1 for _, c, _ in st)
    assert ids.min() >= pc.FILL_BASE and ids.max() < pc.TIED_BASE
    # ... to its full length (the streams that reach tile 256)
    ids = pc._filler(pc.FILL_MAX)
    key = ids[:-1].astype(np.int64) * 65536 + ids[1:]
    assert len(np.unique(key)) == len(key) and pc.FILL_MAX > pc.TIE_BLOCKS * pc.TILE + 37 + 777


# ---------------------------------------------------------------------------
# table width

@pytest.mark.parametrize("V", pc.WIDTHS)
def test_width_cases(V):
    for variant in pc.WIDTH_VARIANTS:
        ids, off = pc.width_case(V, variant)
        assert ids.dtype == np.int32 and int(ids.max()) + 1 == V and int(ids.min()) == 0
        assert {0, 255, 256, V - 2, V - 1} <= set(ids.tolist()) and len(set(ids.tolist())) <= 6
        assert 4500 <= len(ids) <= 5500 and len(ids) % 4 != 0
        assert len(off) >= 2 and off[0] == 0 and np.all(np.diff(off.astype(np.int64)) > 0)
        reg = pc.classify(ids, off)
        assert reg.tied == 1 and reg.pair == pc.WIDTH_PAIR[variant](V)
        assert (reg.pair[0] == V - 1, reg.pair[1] == V - 1) == {"row": (True, False), "col": (False, True),
                                                                 "run": (True, True)}[variant]
        if variant == "run":  # a chunk start inside the run
            inside = [int(o) for o in off if 0 < o < len(ids) and ids[int(o) - 1] == V - 1 == ids[int(o)]]
            assert inside


# ---------------------------------------------------------------------------
# selection regimes

@pytest.mark.parametrize("name", list(pc.SELECTION))
def test_selection_cases(name):
    ids, off, reg = pc.argmax_case(name)
    assert len(ids) <= 25000
    assert (reg.tied, reg.single_rows, reg.multi_rows) == pc.SELECTION_REGIME[name]
    st = oracle.get_stats(ids, off)
    tied = [p for p, c, _ in st if c == reg.M]
    if reg.tied > 1:
        assert reg.pair != min(tied)
    if len(set(p[0] for p in tied)) > 100 or name.startswith("tied_"):  # (not the cases whose point is ONE multi row)
        assert reg.pair[0] != min(p[0] for p in tied)
    assert reg.pos > 0 and np.any(off == reg.pos)


def test_selection_bounds_are_straddled():
    tied = sorted(pc.SELECTION_REGIME[f"tied_{T}"][0] for T in (2, 95, 96, 97))
    assert tied == [2, pc.TIE_CAP - 1, pc.TIE_CAP, pc.TIE_CAP + 1]
    multi = sorted(pc.SELECTION_REGIME[f"multi_{R}"][2] for R in (1, 2047, 2048, 2049))
    assert multi == [1, pc.ARGMAX_ROWS - 1, pc.ARGMAX_ROWS, pc.ARGMAX_ROWS + 1]
    for R in (2047, 2048, 2049):  # about 8 ids per row, V a little above R
        ids, _, _ = pc.argmax_case(f"multi_{R}")
        assert len(ids) <= 8 * R + 128 and R < int(ids.max()) + 1 <= R + pc.TIED_BASE + 2
    assert pc.SELECTION_REGIME["multi_1_single_94"][0] == pc.TIE_CAP
    assert pc.SELECTION_REGIME["multi_1_single_95"][:2] == (pc.TIE_CAP + 1, pc.TIE_CAP - 1)
    assert pc.SELECTION_REGIME["multi_1_single_96"][1:] == (pc.TIE_CAP, 1)
    assert pc.argmax_case("multi_1_single_96")[2].pair[0] == pc.TIED_BASE  # the winner is in the multi-column row
    assert pc.SELECTION_REGIME["multi_2048_single_97"][1:] == (pc.TIE_CAP + 1, pc.ARGMAX_ROWS)


def test_side_cases():
    for name, hi in (("side_hi", True), ("side_lo", False)):
        ids, off, reg = pc.argmax_case(name)
        assert int(ids.max()) + 1 == pc.SEL_ROWS + 1
        rows = set(p[0] for p, c, _ in oracle.get_stats(ids, off) if c == reg.M)
        assert any(r >= pc.SEL_ROWS for r in rows) and any(r < pc.SEL_ROWS for r in rows)
        assert (reg.pair[0] >= pc.SEL_ROWS) == hi
        assert reg.pair[0] == (pc.SEL_ROWS if hi else pc.SEL_ROWS - 1)


# ---------------------------------------------------------------------------
# first occurrences

@pytest.mark.parametrize("T", pc.FIRST_T)
def test_first_occurrence_cases(T):
    assert min(pc.FIRST_T) <= pc.TIE_CAP < max(pc.FIRST_T)
    want = {"pos0": 0, "tile0_last_word": pc.TILE - 1, "tile256": pc.TIE_BLOCKS * pc.TILE + 37}
    for kind, where in want.items():
        ids, off, stated = pc.FIRST[f"{kind}_{T}"]()
        _, _, reg = pc.argmax_case(f"{kind}_{T}")
        assert stated == where == reg.pos and reg.tied == T and reg.single_rows == T
        assert (int(ids[where]), int(ids[where + 1])) == reg.pair
        assert (len(ids) > 100000) == (kind == "tile256")
    # the last word of tile 0: the pair's second word is tile 1's first
    assert want["tile0_last_word"] % pc.TILE == pc.TILE - 1 and want["tile0_last_word"] // pc.TILE == 0
    # a tile the sweep's first round does not reach
    ids, _, reg = pc.argmax_case(f"tile256_{T}")
    assert reg.pos // pc.TILE >= pc.TIE_BLOCKS and (len(ids) + pc.TILE - 1) // pc.TILE > pc.TIE_BLOCKS
    assert len(ids) < (pc.TIE_BLOCKS + 2) * pc.TILE


@pytest.mark.parametrize("T", pc.FIRST_T)
def test_tail_case(T):
    ids, off, stated = pc.FIRST[f"tail_{T}"]()
    reg = pc.classify(ids, off)
    n = len(ids)
    assert reg.tied == T and reg.pos == stated and stated // pc.TILE == 1
    assert (int(ids[n - 2]), int(ids[n - 1])) == reg.pair and not np.any(off == n - 1)
    # without the pair at n - 2 the winner is out of the tie
    cut = pc.classify(ids[:-1], off)
    assert cut.M == reg.M and cut.tied == T - 1 and cut.pair != reg.pair


@pytest.mark.parametrize("T", pc.FIRST_T)
def test_astride_case(T):
    ids, off, p = pc.FIRST[f"astride_{T}"]()
    reg = pc.classify(ids, off)
    assert reg.tied == T and reg.pos == p and np.any(off == p)
    spelled = (int(ids[p - 1]), int(ids[p]))
    st = {pair: (c, f) for pair, c, f in oracle.get_stats(ids, off)}
    assert st[spelled][0] == reg.M and spelled != reg.pair  # a tied pair is spelled astride the chunk start ...
    assert p - 1 < reg.pos < st[spelled][1]                   # ... ahead of the winner; it really occurs only later
    # ignoring chunk starts, that pair would win
    assert pc.classify(ids, None).pair == spelled


@pytest.mark.parametrize("T", pc.FIRST_T)
def test_tie_window_cases(T):
    want = {"tile7_last_word": pc.TIE_WIN * pc.TILE - 1, "tile8_first_word": pc.TIE_WIN * pc.TILE,
            "tile12": 12 * pc.TILE + 123}
    for kind, where in want.items():
        ids, off, reg = pc.argmax_case(f"{kind}_{T}")
        assert reg.pos == where and reg.tied == T and len(ids) < 100000
        assert (int(ids[where]), int(ids[where + 1])) == reg.pair
    assert want["tile7_last_word"] // pc.TILE == pc.TIE_WIN - 1 and want["tile8_first_word"] // pc.TILE == pc.TIE_WIN
    assert want["tile8_first_word"] % pc.TILE == 0 and want["tile12"] // pc.TILE > pc.TIE_WIN


# ---------------------------------------------------------------------------
# merges, the loop by hand

@pytest.mark.parametrize("V", pc.MERGE_V)
def test_merge_cases(V):
    ids, off = pc.merge_stream(V)
    assert int(ids.max()) + 1 == V and pc.MERGE_IDX_BELOW < V and pc.MERGE_IDX_BELOW not in set(ids.tolist())
    cases = pc.merge_cases(V)
    assert sorted(set(i for _, i in cases)) == [pc.MERGE_IDX_BELOW, V + 1000]
    assert set(p for p, _ in cases) == {(V - 2, V - 1), (V - 1, V - 1)}
    run = ids == V - 1
    for lo, hi, cut in ((4090, 4101, None), (8186, 8198, None), (6000, 6007, 6003), (7000, 7008, 7004)):
        assert run[lo:hi].all() and not run[lo - 1] and not run[hi]
        if cut is None:
            assert lo // pc.TILE != (hi - 1) // pc.TILE and not np.any((off > lo) & (off < hi))
        else:
            assert np.any(off == cut)
    assert {(4101 - 4090) % 2, (8198 - 8186) % 2} == {0, 1} and {(6003 - 6000) % 2, (6007 - 6003) % 2} == {0, 1}
    assert (ids[5000], ids[5001]) == (V - 2, V - 1) and np.any(off == 5001)
    assert (ids[12287], ids[12288]) == (V - 2, V - 1) and 12288 % pc.TILE == 0
    st = dict((p, c) for p, c, _ in oracle.get_stats(ids, off))
    for pair, idx in cases:
        assert st[pair] > 100
        out, _ = oracle.merge_chunks(ids, off, pair, idx)
        assert len(out) < len(ids) and idx in set(out.tolist())


def test_hand_loop_case():
    ids, off = pc.hand_stream()
    assert 15000 <= len(ids) <= 25000 and len(off) > 10
    assert ids.min() >= 250 and ids.max() <= 2100 and 35 <= len(set(ids.tolist())) <= 45
    loop = pc.hand_loop()
    assert len(loop) == pc.HAND_ITERS == 40
    assert any(tied > 1 for _, _, tied, _ in loop)
    assert any(a == b for (a, b), _, _, _ in loop)
    # ties on both sides of the list's capacity, and merged ids that are merged again
    assert any(tied > pc.TIE_CAP for _, _, tied, _ in loop) and any(1 < tied <= pc.TIE_CAP for _, _, tied, _ in loop)
    assert any(a >= pc.HAND_NEW for (a, _b), _, _, _ in loop)
    lens = [n for _, _, _, n in loop]
    assert all(x > y for x, y in zip([len(ids)] + lens, lens))
