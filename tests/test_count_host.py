"""CPU: bpe_count_fold -- from one histogram of token ids to the histogram at any smaller vocabulary and to the token count
at every vocabulary size -- against count_model (the fold in plain Python, and the curve by expanding every id, which does
not use the fold), and the Tokenizer methods on top of it against what the truncated tokenizer itself encodes, through
the oracle-backed engine double.  bpe_count_resident is declared, exported and bound; counting itself needs a GPU
(test_gpu_count.py).

The hand-made merge list is test_gpu_project.py's: at vocab_size 256 its ids expand to 1, 2, 3, 4, 5, 63, 64, 65 and (a
doubling chain) 4,096 ids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import count_model
import project_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_LIMIT = -2, -6

# id: length at vocab_size 256
MERGES = [(97, 98),      # 256: 2
          (256, 99),     # 257: 3
          (256, 256),    # 258: 4
          (258, 100),    # 259: 5
          (101, 101)]    # 260: 2, then the doubling chain 261: 4 ... 265: 64 ... 271: 4096
MERGES += [(259 + j, 259 + j) for j in range(1, 12)]
MERGES += [(264, 263),   # 272: 48
           (272, 262),   # 273: 56
           (273, 261),   # 274: 60
           (274, 260),   # 275: 62
           (275, 102),   # 276: 63
           (265, 103)]   # 277: 65
M = len(MERGES)
TOP = 256 + M
PASS = [-7, 300000, 2**31 - 1]
LEN_256 = {65: 1, 256: 2, 257: 3, 258: 4, 259: 5, 276: 63, 265: 64, 277: 65, 271: 4096}


def hand_ids(n=3000, seed=5):
    """ids over every bin of the hand list, every one of them present"""
    rng = np.random.default_rng(seed)
    pool = np.array(list(range(TOP)) + PASS, dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), size=n)]
    ids[:len(pool)] = pool
    return ids


def raw_fold(native, pairs, counts, vocab_size, want_folded=True, want_curve=True, n_bins=None):
    """the C call itself: (rc, folded, curve) as uint64 arrays (None where not asked for)"""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    n_bins = len(counts) if n_bins is None else n_bins
    folded = np.full(len(counts), 0xA5A5A5A5, np.uint64) if want_folded else None
    curve = np.full(len(pairs) + 1, 0xA5A5A5A5, np.uint64) if want_curve else None
    ptr = lambda a: None if a is None or not len(a) else a.ctypes.data_as(C.c_void_p)
    rc = native._lib.bpe_count_fold(ptr(pairs), len(pairs), ptr(counts), n_bins, vocab_size, ptr(folded), ptr(curve))
    return rc, folded, curve


def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "DESIGN 4.7" in hdr
    lib = C.CDLL(native.LIB_PATH)
    for name, nargs in (("bpe_count_resident", 8), ("bpe_count_fold", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, code)
        assert hasattr(lib, name)
        assert name in native.exported_symbols()
        assert len(getattr(native._lib, name).argtypes) == nargs
    assert callable(native.Engine.count_resident) and callable(native.count_fold)
    import minbpe_amd.tokenizer as T
    for cls in (T.BasicTokenizer, T.RegexTokenizer, T.GPT4Tokenizer):   # one implementation, on the base class
        for method in ("count_bins", "token_counts_resident", "token_counts", "counts_at_vocab", "compression_curve"):
            assert getattr(cls, method) is getattr(T.Tokenizer, method)


def test_the_model_is_what_the_docstring_says():
    lens = count_model.expansion_lengths(MERGES)
    for t, L in LEN_256.items():
        assert len(project_model.expand(t, MERGES, 256)) == L == lens[t, 0]
    for t in range(TOP):           # the lengths are project_model's recursion at every size
        for k in (0, 1, 5, 10, M - 1, M):
            assert lens[t, k] == len(project_model.expand(t, MERGES, 256 + k))
    ids = hand_ids(400)
    by_expand = [sum(len(project_model.expand(int(t), MERGES, 256 + k, PASS)) for t in ids) for k in range(M + 1)]
    assert count_model.curve_by_expansion(ids, MERGES, PASS) == by_expand
    assert count_model.bins(M, PASS).tolist() == list(range(TOP)) + PASS
    assert count_model.count([5, -7, 277, 5, 2**31 - 1], M, PASS).nonzero()[0].tolist() == [5, 277, TOP, TOP + 2]
    for bad, where in (([1, TOP], 1), ([-1, 5], 0), ([5, 5, 2**32 + 5], 2), ([300000, 299999, -8], 1)):
        with pytest.raises(count_model.BadId) as e:
            count_model.count(bad, M, PASS)
        assert e.value.args[0] == where


def test_hand_list_at_every_vocab_size(native):
    ids = hand_ids()
    counts = count_model.count(ids, M, PASS)
    assert counts.min() >= 1 and counts.sum() == len(ids)
    want_curve = count_model.curve_by_expansion(ids, MERGES, PASS)
    n_pass = int(counts[TOP:].sum())
    n_bytes = sum(int(c) * L for c, L in zip(counts[:TOP], count_model.expansion_lengths(MERGES)[:, 0]))
    for vs in range(256, TOP + 1):
        rc, folded, curve = raw_fold(native, MERGES, counts, vs)
        assert rc == 0
        assert folded.tolist() == count_model.fold(counts, MERGES, vs)
        assert curve.tolist() == want_curve
        assert curve[M] == len(ids)
        assert curve[0] == n_bytes + n_pass                      # bytes plus pass ids
        assert not folded[vs:TOP].any()
        assert folded[TOP:].tolist() == counts[TOP:].tolist()    # pass bins unchanged
        assert int(folded.sum()) == curve[vs - 256]
        # the binding: the same arrays, uint64 and int64
        f2, c2 = native.count_fold(MERGES, counts, vs)
        assert f2.dtype == np.uint64 and c2.dtype == np.int64
        assert np.array_equal(f2, folded) and c2.tolist() == want_curve
    # the projection of the ids, counted, is the folded histogram
    for vs in (256, 266, TOP - 1, TOP):
        projected = count_model.count(project_model.project(ids, MERGES, vs, PASS), M, PASS)
        assert raw_fold(native, MERGES, counts, vs)[1].tolist() == projected.tolist()


def test_null_outputs(native):
    counts = count_model.count(hand_ids(), M, PASS)
    rc, folded, curve = raw_fold(native, MERGES, counts, 266)
    assert rc == 0 and raw_fold(native, MERGES, counts, 266, want_curve=False)[0] == 0
    assert np.array_equal(raw_fold(native, MERGES, counts, 266, want_curve=False)[1], folded)
    assert np.array_equal(raw_fold(native, MERGES, counts, 266, want_folded=False)[2], curve)
    assert raw_fold(native, MERGES, counts, 266, want_folded=False, want_curve=False)[0] == 0
    for vs in (256, TOP):          # the two ends, folded alone
        assert raw_fold(native, MERGES, counts, vs, want_curve=False)[1].tolist() == count_model.fold(counts, MERGES, vs)
    f, c = native.count_fold(MERGES, counts, 266, want_curve=False)
    assert c is None and np.array_equal(f, folded)
    f, c = native.count_fold(MERGES, counts)
    assert f is None and np.array_equal(c, curve.astype(np.int64))
    # no merges: one size, one point
    rc, f, c = raw_fold(native, [], np.arange(256), 256)
    assert rc == 0 and f.tolist() == list(range(256)) and c.tolist() == [255 * 128]
    # bins past 256 + M are pass bins, however many
    more = np.concatenate([counts, [7, 8, 9]])
    rc, f, c = raw_fold(native, MERGES, more, 256)
    assert rc == 0 and f[TOP:].tolist() == more[TOP:].tolist() and c[M] == more.sum()


def random_list(rng):
    """1..300 merges of the shape training makes (no pair twice), and counts over all bins with a few pass bins"""
    m = int(rng.integers(1, 301))
    merges, seen = [], set()
    while len(merges) < m:
        r = len(merges)
        lo = 0 if rng.random() < 0.9 else max(0, 256 + r - 40)      # one in ten near the top: deep trees
        p = (int(rng.integers(lo, 256 + r)), int(rng.integers(lo, 256 + r)))
        if p not in seen:
            seen.add(p)
            merges.append(p)
    pas = sorted(set([-int(x) - 1 for x in rng.integers(0, 50, size=int(rng.integers(0, 4)))]
                     + [256 + m + int(x) for x in rng.integers(0, 1000, size=int(rng.integers(0, 4)))]))
    return merges, pas


def test_random_lists(native):
    rng = np.random.default_rng(20240)
    for _ in range(200):
        merges, pas = random_list(rng)
        m = len(merges)
        layout = count_model.bins(m, pas)
        ids = layout[rng.integers(0, len(layout), size=int(rng.integers(0, 400)))]
        ids = np.concatenate([ids, layout[-(len(pas) + 3):]])        # the top ids and every pass id are there
        counts = count_model.count(ids, m, pas)
        want_curve = count_model.curve_by_expansion(ids, merges, pas)
        assert max(want_curve) < 2**62
        for vs in sorted({256, 256 + m, 256 + int(rng.integers(0, m + 1)), 256 + m - 1}):
            rc, folded, curve = raw_fold(native, merges, counts, vs)
            assert rc == 0
            assert folded.tolist() == count_model.fold(counts, merges, vs), (m, vs)
            assert curve.tolist() == want_curve, (m, vs)
            assert int(folded.sum()) == want_curve[vs - 256]


def test_contracts(native):
    counts = count_model.count(hand_ids(), M, PASS)
    for vs in (255, 257 + M, 0, -1):
        assert raw_fold(native, MERGES, counts, vs)[0] == E_ARG
    for bad in ([(97, 256)], [(97, 98), (257, 99)], [(97, 98), (97, 98)], [(-1, 5)], MERGES[:10] + [(300, 5)]):
        assert raw_fold(native, bad, np.ones(256 + len(bad) + 2), 256)[0] == E_ARG
    assert raw_fold(native, MERGES, counts[:TOP], TOP)[0] == 0           # exactly 256 + M bins: no pass ids
    assert raw_fold(native, MERGES, counts, TOP, n_bins=TOP - 1)[0] == E_ARG
    assert native._lib.bpe_count_fold(None, 0, None, 256, 256, None, None) == E_ARG      # no counts
    for call in (lambda: native.count_fold(MERGES, counts, 255), lambda: native.count_fold([(97, 256)], np.ones(257, np.int64), 256),
                 lambda: native.count_fold(MERGES, counts[:TOP - 1]), lambda: native.count_fold(MERGES, -counts.astype(np.int64))):
        with pytest.raises(ValueError):
            call()
    for wrong in (counts.astype(np.float64), counts.reshape(1, -1), ["a"] * len(counts)):
        with pytest.raises(TypeError):
            native.count_fold(MERGES, wrong)


def test_overflow_is_a_limit(native):
    """a 40-merge doubling chain with 2^62 on its top id: two merges undone make 2^64 tokens"""
    chain = [(97, 97)] + [(255 + r, 255 + r) for r in range(1, 40)]
    counts = np.zeros(256 + 40, np.uint64)
    counts[295] = 2**62
    assert raw_fold(native, chain, counts, 256)[0] == E_LIMIT
    assert raw_fold(native, chain, counts, 256, want_curve=False)[0] == E_LIMIT
    assert raw_fold(native, chain, counts, 256, want_folded=False)[0] == E_LIMIT
    with pytest.raises(OverflowError):
        native.count_fold(chain, counts, 256)
    # one merge undone still fits: 2^63 tokens, 2^63 in bin 294 -- as uint64 (the binding's int64 curve refuses it)
    rc, folded, _ = raw_fold(native, chain, counts, 295, want_curve=False)
    assert rc == 0 and int(folded[294]) == 2**63 and not folded[295]
    # the sum of all bins is an add like any other
    full = np.full(256 + 40, 2**63, np.uint64)
    assert raw_fold(native, chain, full, 296, want_folded=False)[0] == E_LIMIT
    small = np.zeros(256 + 40, np.uint64)
    small[295] = 3
    rc, folded, curve = raw_fold(native, chain, small, 256)
    assert rc == 0 and int(folded[97]) == 3 * 2**40 and curve.tolist() == [3 * 2**(40 - k) for k in range(41)]


# ---------------------------------------------------------------------------
# the Tokenizer methods, over the oracle-backed engine double

@pytest.fixture(scope="module")
def T(native):
    import minbpe_amd.tokenizer as T
    from fake_engine import OracleEngine
    eng = OracleEngine()
    mp = pytest.MonkeyPatch()
    mp.setattr(T, "engine", lambda device=None: eng)
    yield T
    mp.undo()


@pytest.fixture(scope="module")
def taylor():
    with open(os.path.join(ROOT, "tests", "golden", "taylorswift.txt"), encoding="utf-8") as f:
        return f.read()[:60_000]


@pytest.fixture(scope="module")
def trained(T, taylor):
    """both classes trained to 256 + 400 on the first 60 kB, once"""
    toks = {}
    for name, cls in (("regex", T.RegexTokenizer), ("basic", T.BasicTokenizer)):
        tok = cls()
        tok.train(taylor, 256 + 400)
        assert len(tok.merges) == 400
        toks[name] = tok
    return toks


@pytest.mark.parametrize("kind", ["regex", "basic"])
def test_against_the_truncated_tokenizer(trained, taylor, kind):
    tok = trained[kind]
    assert tok.count_bins().tolist() == list(range(656)) and tok.count_bins().dtype == np.int64
    counts = np.bincount(tok.encode(taylor), minlength=656)
    curve = tok.compression_curve(counts)
    assert curve.dtype == np.int64 and curve.shape == (401,)
    for size in (256, 257, 300, 655, 656):
        small = tok.at_vocab(size).encode(taylor)
        got = tok.counts_at_vocab(counts, size)
        assert got.dtype == np.int64 and got.shape == (656,)
        assert np.array_equal(got, np.bincount(small, minlength=656)), (kind, size)
        assert curve[size - 256] == len(small), (kind, size)
    assert np.array_equal(tok.counts_at_vocab(counts.tolist(), 300), tok.counts_at_vocab(counts, 300))
    try:
        import torch
    except ImportError:       # (the fold itself does not need it)
        return
    assert np.array_equal(tok.counts_at_vocab(torch.from_numpy(counts), 300), tok.counts_at_vocab(counts, 300))
    assert np.array_equal(tok.compression_curve(torch.from_numpy(counts)), curve)


def test_fold_methods_need_no_engine(native, monkeypatch):
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called by a host-only method")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.RegexTokenizer()
    tok.merges = {(97, 98): 256, (256, 99): 257, (257, 257): 258}
    tok.vocab = tok._build_vocab()
    tok.register_special_tokens({"<|b|>": 100257, "<|a|>": -3})
    assert tok.count_bins().tolist() == list(range(259)) + [-3, 100257]
    counts = np.zeros(261, np.int64)
    counts[[97, 258, 259, 260]] = [5, 2, 7, 1]
    assert tok.compression_curve(counts).tolist() == [5 + 12 + 8, 5 + 8 + 8, 5 + 4 + 8, 5 + 2 + 8]
    want = np.zeros(261, np.int64)
    want[[97, 98, 99, 259, 260]] = [5 + 4, 4, 4, 7, 1]
    assert np.array_equal(tok.counts_at_vocab(counts, 256), want)
    assert np.array_equal(tok.counts_at_vocab(counts, 259), counts)
    for size in (255, 260, 256.0, "300", None, True):
        with pytest.raises(ValueError, match="vocab_size"):
            tok.counts_at_vocab(counts, size)
    with pytest.raises(ValueError, match="261"):
        tok.counts_at_vocab(counts[:260], 256)
    with pytest.raises(ValueError, match="261"):
        tok.compression_curve(np.zeros(262, np.int64))
    for wrong in (counts.astype(np.float32), counts.reshape(1, -1)):
        with pytest.raises(TypeError):
            tok.counts_at_vocab(wrong, 256)
        with pytest.raises(TypeError):
            tok.compression_curve(wrong)
    # a special token inside [vocab_size, 256 + M): _project_args' error
    tok.register_special_tokens({"<|a|>": 258, "<|b|>": 100257})
    counts = np.zeros(260, np.int64)
    for size in (256, 257, 258):
        with pytest.raises(ValueError, match="special token id 258 lies in"):
            tok.counts_at_vocab(counts, size)
    with pytest.raises(ValueError, match="special token id 258 lies in"):
        tok.compression_curve(counts)
    assert np.array_equal(tok.counts_at_vocab(counts, 259), counts)
    # a merge list of another shape
    bad = T.BasicTokenizer()
    bad.merges = {(97, 98): 257}
    with pytest.raises(ValueError, match="shape"):
        bad.compression_curve(np.zeros(257, np.int64))
    with pytest.raises(ValueError, match="shape"):
        bad.count_bins()
    # the device methods check their arguments before an engine exists
    try:
        import torch
    except ImportError:
        return
    tok.register_special_tokens({})
    ids = torch.arange(10, dtype=torch.int64)
    for wrong in (ids, ids.tolist(), ids.to(torch.float32), torch.empty(4, dtype=torch.int64, device="meta")):
        with pytest.raises(TypeError):
            tok.token_counts_resident(wrong)
    for wrong in ([0.5, 1.0], ["a"], np.arange(6).reshape(2, 3)):
        with pytest.raises(TypeError):
            tok.token_counts(wrong)
