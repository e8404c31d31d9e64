"""CPU: repetition_model (the definition of the repetition statistics) against a second, all-pairs statement
of it on random small streams; the cases worked by hand; its invariants; equality at the full width; document
boundaries; the flag rule against its definition in fractions; the call is declared, exported, bound and documented;
every argument error of Tokenizer.repetition_resident / repetition / repetitive_docs_resident /
drop_repetitive_docs_resident that needs no device is raised before an engine exists."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import repetition_model as model
import select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the definition once more: every window of a key against every earlier one, id by id, no dict and no tuple

def all_pairs(ids, off, w, max_len=None, tail=False):
    ids, off = [int(x) for x in ids], [int(x) for x in off]
    n_docs = len(off) - 1
    cols = {name: [0] * n_docs for name in ("length", "windows", "distinct", "covered", "top_count", "top_pos")}
    marks = [0] * len(ids)
    for d in range(n_docs):
        m_ids, m_off = select_model.select(np.asarray(ids, np.int64), off, [d], max_len, tail)  # the slice selection emits
        key = [int(x) for x in m_ids]
        assert int(m_off[1]) == len(key)
        s = off[d + 1] - len(key) if tail else off[d]
        assert ids[s:s + len(key)] == key
        starts = [k for k in range(len(key)) if k + w <= len(key)]
        equal = lambda j, k: all(key[j + t] == key[k + t] for t in range(w))
        repeats = [k for k in starts if any(equal(j, k) for j in starts if j < k)]
        covered = [i for i in range(len(key)) if any(k <= i < k + w for k in repeats)]
        mult = {k: sum(equal(j, k) for j in starts) for k in starts}
        cols["length"][d], cols["windows"][d] = len(key), len(starts)
        cols["distinct"][d], cols["covered"][d] = len(starts) - len(repeats), len(covered)
        cols["top_count"][d] = max(mult.values(), default=0)
        # the lowest start among the windows of the largest multiplicity: the first start of the class that starts first
        cols["top_pos"][d] = (s - off[d]) + min(k for k in starts if mult[k] == cols["top_count"][d]) if starts else -1
        for k in repeats:
            marks[s + k] |= 1
        for i in covered:
            marks[s + i] |= 2
    return cols, marks, sum(x < y for x, y in zip(cols["distinct"], cols["windows"]))


def agree(ids, off, w, max_len=None, tail=False):
    got = model.stats(ids, off, w, max_len, tail)
    cols, marks, n_rep = all_pairs(ids, off, w, max_len, tail)
    for name, col in cols.items():
        assert getattr(got, name).tolist() == col, (name, list(ids), list(off), w, max_len, tail)
        assert getattr(got, name).dtype == np.int64
    assert got.marks.tolist() == marks and got.marks.dtype == np.uint8 and got.n_repeat_docs == n_rep
    return got


def random_case(rng):
    w = int(rng.integers(1, 6))
    vocab = int(rng.integers(2, 4))                                        # two or three values: repeats are dense
    docs = [rng.integers(0, vocab, size=int(rng.integers(0, 15))) for _ in range(int(rng.integers(0, 6)))]
    ids, off = model.stream(docs)
    lead, trail = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    ids = np.concatenate([rng.integers(0, vocab, size=lead), ids, rng.integers(0, vocab, size=trail)])
    return ids, off + lead, w


def test_model_agrees_with_all_pairs():
    rng = np.random.default_rng(12)
    for case in range(300):
        ids, off, w = random_case(rng)
        agree(ids, off, w)
        if case % 2:
            agree(ids, off, w, max_len=int(rng.integers(1, 12)), tail=bool(case % 4 == 1))


def test_hand_cases():
    one = lambda ids, w: [int(c[0]) for c in model.stats(ids, [0, len(ids)], w)[:6]]
    assert one([7] * 6, 2) == [6, 5, 1, 5, 5, 0]
    assert one([1, 2, 3, 1, 2, 3, 9], 3) == [7, 5, 4, 3, 2, 0]
    assert model.stats([1, 2, 3, 1, 2, 3, 9], [0, 7], 3).marks.tolist() == [0, 0, 0, 3, 2, 2, 0]
    assert one([1, 2, 1, 2, 3, 4, 3, 4], 2) == [8, 7, 5, 4, 2, 0]
    assert one([], 1) == [0, 0, 0, 0, 0, -1] and one([5, 5], 3) == [2, 0, 0, 0, 0, -1]
    # the top window of several with one multiplicity: the class that starts first, though it ends last
    assert one([1, 2, 9, 3, 4, 8, 3, 4, 7, 1, 2], 2)[4:] == [2, 0]
    assert one([9, 3, 4, 8, 3, 4, 7], 2)[4:] == [2, 1]
    # top_pos is a position of the uncut document; the cut removes the earlier occurrence
    st = model.stats([0, 1, 2, 5, 6, 1, 2, 8], [0, 8], 2, max_len=6, tail=True)
    assert [int(c[0]) for c in st[:6]] == [6, 5, 5, 0, 1, 2]
    st = model.stats([0, 1, 2, 5, 1, 2, 8, 8], [0, 8], 2, max_len=6, tail=False)
    assert [int(c[0]) for c in st[:6]] == [6, 5, 4, 2, 2, 1] and st.marks.tolist() == [0, 0, 0, 0, 3, 2, 0, 0]


def test_invariants():
    rng = np.random.default_rng(13)
    for case in range(200):
        ids, off, w = random_case(rng)
        max_len = int(rng.integers(1, 12)) if case % 3 == 0 else None
        st = model.stats(ids, off, w, max_len, tail=bool(case % 2))
        assert (st.distinct <= st.windows).all() and (st.covered <= st.length).all()
        assert ((st.covered == 0) == (st.distinct == st.windows)).all()
        assert ((st.top_count >= 1) == (st.windows >= 1)).all()
        assert ((st.top_count == 1) == ((st.windows >= 1) & (st.distinct == st.windows))).all()
        assert ((st.top_pos == -1) == (st.windows == 0)).all()
        assert not ((st.marks & 1) & ~(st.marks >> 1)).any()               # bit 0 implies bit 1
        for d in range(len(off) - 1):
            assert int((st.marks[off[d]:off[d + 1]] & 1).sum()) == st.windows[d] - st.distinct[d]
            assert int((st.marks[off[d]:off[d + 1]] >> 1).sum()) == st.covered[d]
        assert not st.marks[:off[0]].any() and not st.marks[off[-1]:].any()
        assert st.n_repeat_docs == int((st.distinct < st.windows).sum())


def test_equality_at_full_width_and_document_boundaries():
    lo = [5, -5, 0, 2**31 - 1, -2**31]
    hi = [x + (1 << 32) for x in lo]
    st = agree(np.array(lo + hi + lo, np.int64), [0, 15], 5)
    assert (st.distinct[0], st.top_count[0], st.covered[0]) == (10, 2, 5)  # only the third run repeats the first
    assert agree(np.array(lo + hi, np.int64), [0, 10], 1).n_repeat_docs == 0
    assert agree(np.array([-1, -1, -2, -1, -1], np.int32), [0, 5], 2).distinct[0] == 3
    # windows never join across a document boundary: two adjacent identical documents have no repeat
    a = [3, 1, 4, 7, 5, 9, 2, 6]
    for w in (1, 2, 8):
        st = agree(a + a, [0, 8, 16], w)
        assert st.n_repeat_docs == 0 and st.distinct[0] == st.distinct[1] == st.windows[0]
    assert agree(a + a, [0, 16], 2).distinct[0] == 8                       # (one document: every window of the copy repeats)
    assert agree([1, 2, 3, 1, 2, 3], [0, 5, 6], 3).n_repeat_docs == 0      # the repeat would run over the document's end


# ---------------------------------------------------------------------------
# the flag rule

def fraction_flags(ids, off, top, dup, max_len=None, tail=False):
    n_docs = len(off) - 1
    out = [False] * n_docs
    for rules, column in ((top, "top_count"), (dup, "covered")):
        for w, t in rules:
            st = model.stats(ids, off, w, max_len, tail)
            for d in range(n_docs):
                lhs = int(getattr(st, column)[d]) * (w if column == "top_count" else 1)
                if st.length[d] > 0 and Fraction(lhs) > Fraction(t) * int(st.length[d]):
                    out[d] = True
    return out


def flag_corpus(seed):
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(60):
        l = int(rng.integers(0, 60))
        d = rng.integers(0, 1000, size=l)
        if i % 3 == 0 and l:
            d = np.resize(rng.integers(0, 1000, size=int(rng.integers(1, 7))), l)
        docs.append(d)
    return model.stream(docs)


def test_flag_rule():
    torch = pytest.importorskip("torch")
    from minbpe_amd.tokenizer import RepetitionStats, Tokenizer

    def package_flags(ids, off, top, dup):
        stats = {}
        for w in sorted({w for w, _ in tuple(top) + tuple(dup)}):
            st = model.stats(ids, off, w)
            stats[w] = RepetitionStats(*[torch.from_numpy(c) for c in st[:6]], None)
        top, dup = Tokenizer._repetition_rules(top, dup)
        return Tokenizer._repetition_flags(stats, top, dup).tolist()

    ids, off = flag_corpus(14)
    # thresholds as Fractions of what float64 holds: away from equality both statements say the same
    for top, dup in ((model.GOPHER_TOP, model.GOPHER_DUP), (((1, 0.3),), ()), ((), ((2, 0.37), (5, 0.15))), (((3, 0),), ((4, 1.5),))):
        want = fraction_flags(ids, off, top, dup)
        assert model.flagged(ids, off, top, dup).tolist() == want
        assert package_flags(ids, off, top, dup) == want
    want = fraction_flags(ids, off, model.GOPHER_TOP, model.GOPHER_DUP)
    assert 5 < sum(want) < 55 and not any(w for w, l in zip(want, np.diff(off)) if l == 0)
    # dyadic thresholds exactly at equality: > holds strictly
    eq_ids, eq_off = model.stream([[1, 1, 2, 3], [1, 1, 1, 2], [4, 4, 5, 6, 4, 4, 7, 8], [4, 4, 5, 6, 4, 4, 4, 8], []])
    st1, st2 = model.stats(eq_ids, eq_off, 1), model.stats(eq_ids, eq_off, 2)
    assert st1.top_count.tolist() == [2, 3, 4, 5, 0] and st1.length.tolist() == [4, 4, 8, 8, 0]
    assert st2.covered.tolist() == [0, 2, 2, 3, 0]
    for flags in (model.flagged, package_flags):
        assert list(flags(eq_ids, eq_off, ((1, 0.5),), ())) == [False, True, False, True, False]    # 2 > 2 is not
        assert list(flags(eq_ids, eq_off, (), ((2, 0.25),))) == [False, True, False, True, False]   # 2 > 0.25 * 8 is not
        assert list(flags(eq_ids, eq_off, ((1, 0),), ())) == [True, True, True, True, False]        # length 0: never


# ---------------------------------------------------------------------------
# declared, exported, bound, documented

def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    name = "bpe_repeat_stats_resident"
    assert re.search(rf"\bint\s+{name}\s*\(", code)
    assert hasattr(lib, name) and name in native.exported_symbols()
    assert len(getattr(native._lib, name).argtypes) == 18
    assert callable(native.Engine.repeat_stats_resident)
    for text in ("DESIGN 4.12", "tests/repetition_model.py", "does not depend on scheduling", '"rp_tile"', '"rp_hash_bits"',
                 "16 bytes per slot", "n_repeat_docs"):
        assert text in hdr, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in ("rp_tile", "rp_hash_bits", name):
        assert text in integration, text
    for doc, texts in (("DESIGN.md", ("4.12", "rp_tile", "k_rp_cover")), ("README.md", ("repetition_resident", "test_gpu_repetition.py")),
                       (os.path.join("profiles", "README.md"), ("repeat_notes.md", "repeat_bench.jsonl", "repeat_kernel_resources.csv"))):
        body = open(os.path.join(ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)
    import minbpe_amd
    from minbpe_amd.tokenizer import RepetitionStats, Tokenizer
    assert minbpe_amd.RepetitionStats is RepetitionStats and "RepetitionStats" in minbpe_amd._EXPORTS
    assert RepetitionStats._fields == ("length", "windows", "distinct", "covered", "top_count", "top_pos", "marks")
    for method in ("repetition_resident", "repetition", "repetitive_docs_resident", "drop_repetitive_docs_resident"):
        assert callable(getattr(Tokenizer, method))
    assert isinstance(Tokenizer.n_repetitive_docs, property)
    # the two options have a row each, and the fields they set carry the defaults the header states
    options = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_options.hip")).read()
    assert 'OPT_NAMED("rp_tile", rp_tile, OPT_POW2, 64, RP_TILE_MAX, 1)' in options and "OPT(rp_hash_bits, 0, 64)" in options
    ctx = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")).read()
    tile = int(re.search(r"int rp_tile = (\d+);", ctx).group(1))
    assert f'"rp_tile" ({tile}:' in hdr and "int rp_hash_bits = 64;" in ctx
    assert f"`rp_tile` ({tile}:" in integration


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    assert tok.n_repetitive_docs is None
    resident = (tok.repetition_resident, tok.repetitive_docs_resident, tok.drop_repetitive_docs_resident)
    # the window
    for bad in (0, 65, -1, 2.0, True, "5", None):
        with pytest.raises(ValueError):
            tok.repetition_resident(ids, off, ngram=bad)
        with pytest.raises(ValueError):
            tok.repetition(ids.numpy(), off, ngram=bad)
    # max_len, keep
    for kw in (dict(keep="middle"), dict(max_len=0), dict(max_len=2.0), dict(max_len=True)):
        for call in resident:
            with pytest.raises(ValueError):
                call(ids, off, **kw)
        with pytest.raises(ValueError):
            tok.repetition(ids.numpy(), off, **kw)
    # the rules: pairs of a window in 1..64 and a real threshold >= 0, not both lists empty
    for kw in (dict(top=5), dict(top=(2, .2)), dict(dup=((5, .1, 1),)), dict(top=((0, .2),)), dict(top=((65, .2),)),
               dict(dup=((2.0, .2),)), dict(dup=((True, .2),)), dict(top=((2, -.1),)), dict(top=((2, "0.2"),)),
               dict(top=((2, float("nan")),)), dict(dup=((5, float("inf")),)), dict(dup=((5, None),)), dict(top=((2, True),)),
               dict(top=(), dup=()), dict(top=[], dup=[])):
        for call in resident[1:]:
            with pytest.raises(ValueError):
                call(ids, off, **kw)
    assert T.Tokenizer._repetition_rules([[2, 1]], ()) == (((2, 1.0),), ())
    # ids and offsets: dtype, contiguity, dimensions, where they live -- the last of them "not on a GPU"
    for f in resident:
        with pytest.raises(ValueError):
            f(ids, [])                                                       # n_docs + 1 entries: at least one
        for bad_off in (torch.tensor([0.0, 10.0]), np.array([0.0, 10.0]), torch.tensor([0, 10], device="meta")):
            with pytest.raises(TypeError):
                f(ids, bad_off)
        for bad_ids in (ids.tolist(), ids.numpy(), ids.to(torch.int16), ids.to(torch.float32), ids.reshape(2, 5),
                        torch.arange(20, dtype=torch.int32)[::2]):
            with pytest.raises(TypeError):
                f(bad_ids, off)
        with pytest.raises(TypeError, match="on the GPU"):
            f(ids, off)                                                      # everything else is right: not on a GPU
    for bad_out in (ids.numpy(), ids.to(torch.int64), ids.reshape(2, 5), torch.empty(10, dtype=torch.int32, device="meta")):
        with pytest.raises(TypeError, match="out"):
            tok.drop_repetitive_docs_resident(ids, off, out=bad_out)
    # the host form: integers, flat; offsets as above
    for bad_ids in (np.array([0.5, 1.0]), np.zeros((2, 2), np.int64), ["a"]):
        with pytest.raises(TypeError):
            tok.repetition(bad_ids, off)
    with pytest.raises(ValueError):
        tok.repetition(ids.numpy(), [])
    with pytest.raises(TypeError):
        tok.repetition(ids.numpy(), np.array([0.0, 10.0]))
    assert tok.n_repetitive_docs is None
