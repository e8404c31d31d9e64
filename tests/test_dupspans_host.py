"""CPU: dupspans_model (the definition of span de-duplication) against a second, all-pairs statement of it on
random small streams; its three consequences against repetition_model and ngram_model; the cases worked by hand; its
invariants; equality at the full width; document boundaries and max_len cuts; the keep rule; the two calls are declared,
exported, bound and documented; every argument error of the Tokenizer methods that needs no device is raised before an
engine exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import dupspans_model as model
import ngram_model
import repetition_model
import select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("length", "windows", "seen", "covered", "first", "src_pos")


# ---------------------------------------------------------------------------
# the definition once more: every window against every other, id by id, no dict and no tuple

def all_pairs(ids, off, w, max_len=None, tail=False, anywhere=False):
    ids, off = [int(x) for x in ids], [int(x) for x in off]
    n_docs = len(off) - 1
    keys = []
    for d in range(n_docs):
        m_ids, m_off = select_model.select(np.asarray(ids, np.int64), off, [d], max_len, tail)  # the slice selection emits
        l = int(m_off[1])
        s = off[d + 1] - l if tail else off[d]
        assert ids[s:s + l] == [int(x) for x in m_ids]
        keys.append((s, l))
    starts = [(p, d) for d, (s, l) in enumerate(keys) for p in range(s, s + l) if p + w <= s + l]
    equal = lambda p, q: all(ids[p + t] == ids[q + t] for t in range(w))
    low = {p: min(q for q, _ in starts if equal(p, q)) for p, _ in starts}
    cols = {name: [0] * n_docs for name in COLUMNS}
    marks = [0] * len(ids)
    for d, (s, l) in enumerate(keys):
        mine = [p for p, e in starts if e == d]
        seen = [p for p in mine if low[p] < (p if anywhere else s)]
        covered = [i for i in range(s, s + l) if any(k <= i < k + w for k in seen)]
        cols["length"][d], cols["windows"][d] = l, len(mine)
        cols["seen"][d], cols["covered"][d] = len(seen), len(covered)
        cols["first"][d] = seen[0] - off[d] if seen else -1
        cols["src_pos"][d] = low[seen[0]] if seen else -1
        for p in seen:
            marks[p] |= 1
        for i in covered:
            marks[i] |= 2
    distinct = sum(1 for p, _ in starts if low[p] == p)
    return cols, marks, sum(x > 0 for x in cols["seen"]), len(starts), distinct


def agree(ids, off, w, max_len=None, tail=False, anywhere=False):
    got = model.stats(ids, off, w, max_len, tail, anywhere)
    cols, marks, n_seen, n_windows, n_distinct = all_pairs(ids, off, w, max_len, tail, anywhere)
    for name, col in cols.items():
        assert getattr(got, name).tolist() == col, (name, list(ids), list(off), w, max_len, tail, anywhere)
        assert getattr(got, name).dtype == np.int64
    assert got.marks.tolist() == marks and got.marks.dtype == np.uint8
    assert (got.n_docs_seen, got.n_windows, got.n_distinct) == (n_seen, n_windows, n_distinct)
    return got


def random_case(rng, width=8):
    w = int(rng.integers(1, 6))
    vocab = int(rng.integers(2, 5))                                        # two to four values: windows collide
    dt = np.int32 if width == 4 else np.int64
    docs = [rng.integers(0, vocab, size=int(rng.integers(0, 15))) for _ in range(int(rng.integers(0, 6)))]
    ids, off = model.stream(docs)
    lead, trail = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    ids = np.concatenate([rng.integers(0, vocab, size=lead), ids, rng.integers(0, vocab, size=trail)]).astype(dt)
    return ids, off + lead, w


def test_model_agrees_with_all_pairs():
    rng = np.random.default_rng(21)
    for case in range(300):
        ids, off, w = random_case(rng, width=4 if case % 3 == 0 else 8)
        for anywhere in (False, True):
            agree(ids, off, w, anywhere=anywhere)
            if case % 2:
                agree(ids, off, w, max_len=int(rng.integers(1, 12)), tail=bool(case % 4 == 1), anywhere=anywhere)


# ---------------------------------------------------------------------------
# the three consequences, against the models the project already has

def test_one_document_anywhere_is_repetition():
    rng = np.random.default_rng(22)
    for case in range(150):
        w = int(rng.integers(1, 6))
        vocab = int(rng.integers(2, 5))
        body = rng.integers(0, vocab, size=int(rng.integers(0, 40)))
        lead, trail = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        ids = np.concatenate([rng.integers(0, vocab, size=lead), body, rng.integers(0, vocab, size=trail)])
        off = [lead, lead + len(body)]
        kw = dict(max_len=int(rng.integers(1, 30)), tail=bool(case % 4 == 1)) if case % 2 else {}
        got = model.stats(ids, off, w, anywhere=True, **kw)
        want = repetition_model.stats(ids, off, w, **kw)
        assert got.seen.tolist() == (want.windows - want.distinct).tolist()
        assert got.covered.tolist() == want.covered.tolist() and got.marks.tolist() == want.marks.tolist()
        assert got.length.tolist() == want.length.tolist() and got.windows.tolist() == want.windows.tolist()
        assert got.n_docs_seen == want.n_repeat_docs
        assert not model.stats(ids, off, w, **kw).seen.any()               # the default scope: no earlier document


def test_two_documents_are_overlap_with_a_reference():
    rng = np.random.default_rng(23)
    for case in range(150):
        w = int(rng.integers(1, 6))
        vocab = int(rng.integers(2, 5))
        r = rng.integers(0, vocab, size=int(rng.integers(0, 25)))
        c = rng.integers(0, vocab, size=int(rng.integers(0, 25)))
        ids, off = model.stream([r, c])
        got = model.stats(ids, off, w)
        hits, first, ref_pos, starts, n_hit, n_windows, n_distinct = ngram_model.run(r, [0, len(r)], w, c, [0, len(c)])
        assert got.seen[0] == 0 and got.first[0] == -1 and got.src_pos[0] == -1
        assert (got.seen[1], got.first[1], got.src_pos[1]) == (hits[0], first[0], ref_pos[0])
        assert (got.marks[len(r):] & 1).tolist() == starts.tolist() and not got.marks[:len(r)].any()
        assert got.n_docs_seen == n_hit


def test_anywhere_counts_every_occurrence_but_the_first():
    rng = np.random.default_rng(24)
    for case in range(150):
        ids, off, w = random_case(rng)
        got = model.stats(ids, off, w, anywhere=True)
        low, n_windows = ngram_model.index(ids, off, w)
        assert (got.n_windows, got.n_distinct) == (n_windows, len(low))
        assert int(got.seen.sum()) == got.n_windows - got.n_distinct
        default = model.stats(ids, off, w)
        assert (default.n_windows, default.n_distinct) == (n_windows, len(low))
        assert (default.seen <= got.seen).all() and not (default.marks & ~got.marks).any()


# ---------------------------------------------------------------------------
# by hand

def columns(st):
    return [getattr(st, name).tolist() for name in COLUMNS]


def test_hand_cases():
    # the block 1 2 3 of document 0 again in documents 1 and 2; 7 8 twice in document 2 only
    ids, off = model.stream([[1, 2, 3, 9], [5, 1, 2, 3], [7, 8, 1, 2, 3, 7, 8]])
    st = model.stats(ids, off, 2)
    assert columns(st) == [[4, 4, 7], [3, 3, 6], [0, 2, 2], [0, 3, 3], [-1, 1, 2], [-1, 0, 0]]
    assert st.marks.tolist() == [0, 0, 0, 0, 0, 3, 3, 2, 0, 0, 3, 3, 2, 0, 0]
    assert (st.n_docs_seen, st.n_windows, st.n_distinct) == (2, 12, 7)
    st = model.stats(ids, off, 2, anywhere=True)
    assert columns(st)[2:] == [[0, 2, 3], [0, 3, 5], [-1, 1, 2], [-1, 0, 0]]
    assert st.marks.tolist() == [0, 0, 0, 0, 0, 3, 3, 2, 0, 0, 3, 3, 2, 3, 2]
    assert int(st.seen.sum()) == 12 - 7
    # w = 3: only the whole block
    st = model.stats(ids, off, 3)
    assert columns(st)[2:] == [[0, 1, 1], [0, 3, 3], [-1, 1, 2], [-1, 0, 0]]
    # nothing long enough, nothing at all
    assert columns(model.stats([4, 4, 4], [0, 1, 3], 3)) == [[1, 2], [0, 0], [0, 0], [0, 0], [-1, -1], [-1, -1]]
    st = model.stats([], [0], 1)
    assert columns(st) == [[]] * 6 and st.marks.tolist() == [] and (st.n_docs_seen, st.n_windows, st.n_distinct) == (0, 0, 0)
    # first is a position of the uncut document; the cut removes the earlier occurrence
    ids, off = model.stream([[1, 2, 6, 6], [0, 0, 0, 1, 2]])
    assert columns(model.stats(ids, off, 2))[2:] == [[0, 1], [0, 2], [-1, 3], [-1, 0]]
    assert columns(model.stats(ids, off, 2, max_len=2, tail=True))[2:] == [[0, 0], [0, 0], [-1, -1], [-1, -1]]   # 1 2 is cut off document 0
    assert columns(model.stats(ids, off, 2, max_len=2))[2:] == [[0, 0], [0, 0], [-1, -1], [-1, -1]]              # and here off document 1
    assert columns(model.stats(ids, off, 2, max_len=3, tail=True)) == [[3, 3], [2, 2], [0, 0], [0, 0], [-1, -1], [-1, -1]]
    ids, off = model.stream([[6, 1, 2], [0, 0, 0, 1, 2]])
    assert columns(model.stats(ids, off, 2, max_len=2, tail=True)) == [[2, 2], [1, 1], [0, 1], [0, 2], [-1, 3], [-1, 1]]


def test_three_documents_tell_the_scopes_apart():
    # [A B, B C, C A] with blocks of w = 3 ids; A B = 1 2 1 2 1 2 repeats itself, which only "anywhere" counts
    A, B, C = [1, 2, 1], [2, 1, 2], [7, 8, 9]
    ids, off = model.stream([A + B, B + C, C + A])
    st = agree(ids, off, 3)
    assert columns(st) == [[6, 6, 6], [4, 4, 4], [0, 1, 2], [0, 3, 6], [-1, 0, 0], [-1, 1, 9]]
    assert st.marks.tolist() == [0] * 6 + [3, 2, 2, 0, 0, 0] + [3, 2, 2, 3, 2, 2]
    assert (st.n_docs_seen, st.n_windows, st.n_distinct) == (2, 12, 7)
    st = agree(ids, off, 3, anywhere=True)
    assert columns(st)[2:] == [[2, 1, 2], [4, 3, 6], [2, 0, 0], [0, 1, 9]]
    assert st.marks.tolist() == [0, 0, 3, 3, 2, 2] + [3, 2, 2, 0, 0, 0] + [3, 2, 2, 3, 2, 2]
    assert st.n_docs_seen == 3 and int(st.seen.sum()) == 12 - 7


def test_same_document_later_other_document_earlier():
    # 5 6 stands twice in document 1 and once in document 0: both are seen in both scopes, and the source is document 0
    ids, off = model.stream([[5, 6, 9], [1, 5, 6, 2, 5, 6]])
    for anywhere in (False, True):
        st = agree(ids, off, 2, anywhere=anywhere)
        assert (st.seen[1], st.first[1], st.src_pos[1], st.covered[1]) == (2, 1, 0, 4)
    # without document 0's copy the second one is an in-document repeat: the default scope does not see it
    ids, off = model.stream([[9, 9, 8], [1, 5, 6, 2, 5, 6]])
    assert agree(ids, off, 2).seen.tolist() == [0, 0]
    st = agree(ids, off, 2, anywhere=True)
    assert (st.seen.tolist(), st.first[1], st.src_pos[1]) == ([0, 1], 4, 4)
    # the earlier copy in a LATER document does not count in the default scope
    ids, off = model.stream([[1, 5, 6, 2, 5, 6], [5, 6, 9]])
    st = agree(ids, off, 2)
    assert (st.seen.tolist(), st.first.tolist(), st.src_pos.tolist()) == ([0, 1], [-1, 0], [-1, 1])


def test_invariants():
    rng = np.random.default_rng(25)
    for case in range(200):
        ids, off, w = random_case(rng)
        max_len = int(rng.integers(1, 12)) if case % 3 == 0 else None
        tail = bool(case % 2)
        for anywhere in (False, True):
            st = model.stats(ids, off, w, max_len, tail, anywhere)
            assert (st.seen <= st.windows).all() and (st.covered <= st.length).all()
            assert ((st.covered == 0) == (st.seen == 0)).all() and (st.covered[st.seen > 0] >= w).all()
            assert ((st.first == -1) == (st.seen == 0)).all() and ((st.src_pos == -1) == (st.seen == 0)).all()
            assert not ((st.marks & 1) & ~(st.marks >> 1)).any()           # bit 0 implies bit 1
            for d, (s, l) in enumerate(model.keys([int(x) for x in off], max_len, tail)):
                assert int((st.marks[off[d]:off[d + 1]] & 1).sum()) == st.seen[d]
                assert int((st.marks[off[d]:off[d + 1]] >> 1).sum()) == st.covered[d]
                assert not st.marks[off[d]:s].any() and not st.marks[s + l:off[d + 1]].any()
                if st.seen[d]:
                    p = int(off[d] + st.first[d])
                    assert st.marks[p] & 1 and not (st.marks[s:p] & 1).any()
                    assert st.src_pos[d] < (p if anywhere else s)
                    assert ids[st.src_pos[d]:st.src_pos[d] + w].tolist() == ids[p:p + w].tolist()
            assert not st.marks[:off[0]].any() and not st.marks[off[-1]:].any()
            assert st.n_docs_seen == int((st.seen > 0).sum()) and st.n_windows == int(st.windows.sum())
            assert st.n_distinct <= st.n_windows and (st.n_distinct == 0) == (st.n_windows == 0)


def test_equality_at_full_width_and_boundaries():
    lo = [5, -5, 0, 2**31 - 1, -2**31]
    hi = [x + (1 << 32) for x in lo]
    st = agree(np.array(lo + hi + lo, np.int64), [0, 5, 10, 15], 5)
    assert st.seen.tolist() == [0, 0, 1] and st.src_pos.tolist() == [-1, -1, 0]  # only the third run repeats the first
    assert agree(np.array(lo + hi, np.int64), [0, 5, 10], 1).n_docs_seen == 0
    assert agree(np.array([-1, -1, -2, -1, -1], np.int32), [0, 2, 5], 2).seen.tolist() == [0, 1]
    # identical neighbours: every window of the copy is seen, none of the first
    a = [3, 1, 4, 7, 5, 9, 2, 6]
    for w in (1, 2, 8):
        st = agree(a + a, [0, 8, 16], w)
        assert st.seen.tolist() == [0, 9 - w] and st.covered.tolist() == [0, 8] and st.src_pos[1] == 0
    # a window that exists only across two documents is no window: 4 7 | 5 9 is not seen in 7 5
    assert agree(a + [7, 5], [0, 4, 8, 10], 2).n_docs_seen == 0
    assert agree(a + [7, 5], [0, 8, 10], 2).seen.tolist() == [0, 1]
    # nor one across a max_len cut: 3 1 4 | 7 with max_len = 3
    assert agree(a + [4, 7], [0, 8, 10], 2, max_len=3).n_docs_seen == 0
    assert agree(a + [1, 4], [0, 8, 10], 2, max_len=3).seen.tolist() == [0, 1]
    # strays in front and behind are no document
    assert agree([1, 2] + a + [1, 2], [2, 6, 10], 2).n_docs_seen == 0


# ---------------------------------------------------------------------------
# keep

def test_keep():
    rng = np.random.default_rng(26)
    for case in range(200):
        ids, off, _ = random_case(rng, width=4 if case % 2 else 8)
        ids = ids + 100
        mask = rng.integers(0, 4, size=len(ids)).astype(np.uint8)
        for bits in (1, 2, 3, 0xFF):
            kept, ooff = model.keep(ids, off, mask, bits)
            dropped, doff = model.keep(ids, off, mask, bits, drop=True)
            assert kept.dtype == ids.dtype and ooff.dtype == np.int64 and len(ooff) == len(off)
            assert ooff[0] == 0 and (np.diff(ooff) >= 0).all() and ooff[-1] == len(kept)
            inside = mask[off[0]:off[-1]]
            assert len(kept) == int(((inside & bits) != 0).sum()) and len(kept) + len(dropped) == off[-1] - off[0]
            assert (ooff + doff).tolist() == (np.asarray(off) - off[0]).tolist()       # drop is the complement
            for d in range(len(off) - 1):
                sl = slice(off[d], off[d + 1])
                assert kept[ooff[d]:ooff[d + 1]].tolist() == ids[sl][(mask[sl] & bits) != 0].tolist()
    ids, off = model.stream([[1, 2], [3, 4, 5], [6]])
    kept, ooff = model.keep(ids, off, [1, 1, 0, 0, 0, 2], 1)
    assert kept.tolist() == [1, 2] and ooff.tolist() == [0, 2, 2, 2]                    # emptied documents stay, empty
    kept, ooff = model.keep(ids, off, [1, 1, 0, 0, 0, 2], 2)
    assert kept.tolist() == [6] and ooff.tolist() == [0, 0, 0, 1]
    kept, ooff = model.keep(ids, off, [1, 1, 0, 0, 0, 2], 3, drop=True)
    assert kept.tolist() == [3, 4, 5] and ooff.tolist() == [0, 0, 3, 3]
    kept, ooff = model.keep(ids, [1, 3, 5], [1] * 6)
    assert kept.tolist() == [2, 3, 4, 5] and ooff.tolist() == [0, 2, 4]                 # ids outside the documents go
    # marks of the model, bit 1 dropped: every seen window goes, its first occurrence stays
    ids, off = model.stream([[1, 2, 3, 9], [5, 1, 2, 3], [7, 8, 1, 2, 3, 7, 8]])
    kept, ooff = model.keep(ids, off, model.stats(ids, off, 3).marks, 2, drop=True)
    assert kept.tolist() == [1, 2, 3, 9, 5, 7, 8, 7, 8] and ooff.tolist() == [0, 4, 5, 9]


# ---------------------------------------------------------------------------
# declared, exported, bound, documented

def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, nargs, method in (("bpe_dup_spans_resident", 20, "dup_spans_resident"), ("bpe_keep_ids_resident", 14, "keep_ids_resident")):
        assert re.search(rf"\bint\s+{name}\s*\(", code)
        assert hasattr(lib, name) and name in native.exported_symbols()
        assert len(getattr(native._lib, name).argtypes) == nargs
        assert callable(getattr(native.Engine, method))
    assert "#define BPE_SPANS_ANYWHERE 2u" in hdr and "#define BPE_KEEP_DROP 1u" in hdr
    assert (native.SPANS_ANYWHERE, native.KEEP_DROP, native.SELECT_TAIL) == (2, 1, 1)
    for text in ("DESIGN 4.13", "tests/dupspans_model.py", "does not depend on scheduling", '"ds_tile"', '"ds_hash_bits"',
                 "16 bytes per slot", "n_docs_seen", "BPE_E_INTERNAL"):
        assert text in hdr, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in ("ds_tile", "ds_hash_bits", "bpe_dup_spans_resident", "bpe_keep_ids_resident"):
        assert text in integration, text
    for doc, texts in (("DESIGN.md", ("4.13", "ds_tile", "k_ds_pass", "k_rp_cover", "bpe_keep_ids_resident")),
                       ("README.md", ("duplicate_spans_resident", "keep_ids_resident", "test_gpu_dupspans.py")),
                       (os.path.join("profiles", "README.md"), ("dupspans_notes.md", "dupspans_bench.jsonl",
                                                                "dupspans_kernel_resources.csv"))):
        body = open(os.path.join(ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)
    import minbpe_amd
    from minbpe_amd.tokenizer import SpanDupStats, Tokenizer
    assert minbpe_amd.SpanDupStats is SpanDupStats and "SpanDupStats" in minbpe_amd._EXPORTS
    assert SpanDupStats._fields == ("length", "windows", "seen", "covered", "first", "src_pos", "marks")
    for method in ("duplicate_spans_resident", "duplicate_spans", "keep_ids_resident", "keep_ids", "drop_duplicate_spans_resident"):
        assert callable(getattr(Tokenizer, method))
    for prop in ("n_docs_with_duplicate_spans", "n_span_windows", "n_distinct_span_windows"):
        assert isinstance(getattr(Tokenizer, prop), property)
    # the two options have a row each, and the fields they set carry the defaults the header states
    options = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_options.hip")).read()
    assert 'OPT_NAMED("ds_tile", ds_tile, OPT_POW2, 64, DS_TILE_MAX, 1)' in options and "OPT(ds_hash_bits, 0, 64)" in options
    ctx = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")).read()
    tile = int(re.search(r"int ds_tile = (\d+);", ctx).group(1))
    assert f'"ds_tile" ({tile}:' in hdr and "int ds_hash_bits = 64;" in ctx
    assert f"`ds_tile` ({tile}:" in integration
    kernels = open(os.path.join(ROOT, "minbpe_amd", "csrc", "kernels", "k_dupspans.hip")).read()
    assert "DS_TILE_MAX = 65536" in kernels


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    mask = torch.ones(10, dtype=torch.uint8)
    counters = lambda: (tok.n_docs_with_duplicate_spans, tok.n_span_windows, tok.n_distinct_span_windows)
    assert counters() == (None, None, None)
    spans = (tok.duplicate_spans_resident, tok.drop_duplicate_spans_resident)
    keep = lambda i, o, **kw: tok.keep_ids_resident(i, o, kw.pop("mask", mask), **kw)
    resident = spans + (keep,)
    # the window and the scope
    for bad in (0, 65, -1, 2.0, True, "5", None):
        for call in spans:
            with pytest.raises(ValueError):
                call(ids, off, ngram=bad)
        with pytest.raises(ValueError):
            tok.duplicate_spans(ids.numpy(), off, ngram=bad)
    for bad in ("later_doc", "", None, 0, True, b"anywhere"):
        for call in spans:
            with pytest.raises(ValueError):
                call(ids, off, scope=bad)
        with pytest.raises(ValueError):
            tok.duplicate_spans(ids.numpy(), off, scope=bad)
    # max_len, keep
    for kw in (dict(keep="middle"), dict(max_len=0), dict(max_len=2.0), dict(max_len=True)):
        with pytest.raises(ValueError):
            tok.duplicate_spans_resident(ids, off, **kw)
        with pytest.raises(ValueError):
            tok.duplicate_spans(ids.numpy(), off, **kw)
    # bits, drop
    for kw in (dict(bits=0), dict(bits=256), dict(bits=-1), dict(bits=1.0), dict(bits=True), dict(bits=None), dict(drop=1),
               dict(drop=None), dict(drop="yes")):
        with pytest.raises(ValueError):
            keep(ids, off, **kw)
        with pytest.raises(ValueError):
            tok.keep_ids(ids.numpy(), off, mask.numpy(), **kw)
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
        for f in (tok.drop_duplicate_spans_resident, keep):
            with pytest.raises(TypeError, match="out"):
                f(ids, off, out=bad_out)
    # the mask: a uint8 or bool tensor of len(ids) entries where the ids are
    for bad_mask in (mask.numpy(), mask.tolist(), mask.to(torch.int32), mask.to(torch.float32), mask.reshape(2, 5),
                     torch.ones(20, dtype=torch.uint8)[::2], torch.ones(10, dtype=torch.uint8, device="meta"), None):
        with pytest.raises(TypeError, match="mask"):
            keep(ids, off, mask=bad_mask)
    for bad_mask in (mask[:9], torch.ones(11, dtype=torch.bool), torch.ones(0, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask"):
            keep(ids, off, mask=bad_mask)
    # the host forms: integers, flat; offsets as above; the mask uint8 or bool, flat, of len(ids) entries
    for bad_ids in (np.array([0.5, 1.0]), np.zeros((2, 2), np.int64), ["a"]):
        with pytest.raises(TypeError):
            tok.duplicate_spans(bad_ids, off)
        with pytest.raises(TypeError):
            tok.keep_ids(bad_ids, off, mask.numpy())
    with pytest.raises(ValueError):
        tok.duplicate_spans(ids.numpy(), [])
    with pytest.raises(TypeError):
        tok.duplicate_spans(ids.numpy(), np.array([0.0, 10.0]))
    for bad_mask in (np.ones(10, np.int64), np.ones(10, np.float32), np.ones((2, 5), np.uint8)):
        with pytest.raises(TypeError, match="mask"):
            tok.keep_ids(ids.numpy(), off, bad_mask)
    with pytest.raises(ValueError, match="mask"):
        tok.keep_ids(ids.numpy(), off, np.ones(9, np.uint8))
    with pytest.raises(TypeError, match="out"):
        tok.keep_ids(ids.numpy(), off, mask.numpy(), out=ids)
    assert counters() == (None, None, None)
