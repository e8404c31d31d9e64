"""CPU: segments_model (the definition of segments) against a second statement of it -- itertools.groupby on
the boundaries -- on random small streams; the cases worked by hand; its invariants; the class rule against text, through
RegexTokenizers of both split patterns trained with the oracle-backed test double; the line statistics against
collections.Counter and the flag rule against fractions.Fraction; the two calls are declared, exported, bound and
documented; every argument error of the Tokenizer methods that needs no device is raised before an engine exists."""
import collections
import ctypes
import fractions
import itertools
import os
import re

import numpy as np
import pytest

import segments_model as model
from segments_model import BREAK, SKIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL, SP, END = 0, 1, 2                                             # a newline, a blank, content that ends its line; 3.. content
TABLE = np.array([BREAK | SKIP, SKIP, BREAK] + [0] * 5, np.uint8)


# ---------------------------------------------------------------------------
# the definition once more: the positions of a document grouped by the number of boundaries in front of them

def by_groups(ids, off, classes, tag=False):
    ids, off = [int(x) for x in ids], [int(x) for x in off]
    cols = {name: [] for name in ("out", "seg_offsets", "seg_doc", "src_start", "src_end")}
    doc_seg = [0]
    for d in range(len(off) - 1):
        pairs = [(p, model.class_of(ids[p], classes)) for p in range(off[d], off[d + 1])]
        line_of = {}
        for i, (p, c) in enumerate(pairs):                        # a boundary lies BEHIND its id
            line_of[p] = sum(1 for _, c2 in pairs[:i] if c2 & BREAK)
        firsts = []
        for _, group in itertools.groupby(pairs, key=lambda pc: line_of[pc[0]]):
            content = [p for p, c in group if not c & SKIP]
            if not content:
                continue
            cols["seg_offsets"].append(len(cols["out"]))
            cols["seg_doc"].append(d)
            cols["out"] += ([d] if tag else []) + [ids[p] for p in content]
            firsts.append(content[0])
        starts = [off[d]] + firsts[1:] if firsts else []
        cols["src_start"] += starts
        cols["src_end"] += starts[1:] + [off[d + 1]] if firsts else []
        doc_seg.append(len(cols["seg_doc"]))
    cols["seg_offsets"].append(len(cols["out"]))
    cols["doc_seg_offsets"] = doc_seg
    return cols


def agree(ids, off, classes, tag=False):
    got = model.segment_docs(ids, off, classes, tag)
    want = by_groups(ids, off, classes, tag)
    for name in got._fields:
        assert getattr(got, name).tolist() == want[name], (name, list(ids), list(off), tag)
        assert getattr(got, name).dtype == (np.asarray(ids).dtype if name == "out" else np.int64)
    return got


def random_case(rng, width=8):
    dt = np.int32 if width == 4 else np.int64
    p = rng.dirichlet(np.ones(len(TABLE)))
    docs = [rng.choice(len(TABLE), size=int(rng.integers(0, 25)), p=p) for _ in range(int(rng.integers(0, 6)))]
    lead, trail = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    ids = np.concatenate([rng.integers(0, 3, size=lead)] + docs + [rng.integers(0, 3, size=trail)]).astype(dt)
    off = lead + np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    if width == 8 and len(ids):                                   # ids outside the table are content that ends nothing
        far = rng.random(len(ids))
        ids[far < .1] += 1 << 32
        ids[far > .9] = -1 - ids[far > .9]
    return ids, off


def test_model_agrees_with_groups():
    rng = np.random.default_rng(31)
    for case in range(400):
        ids, off = random_case(rng, width=4 if case % 3 == 0 else 8)
        for tag in (False, True):
            agree(ids, off, TABLE, tag)
        agree(ids, off, TABLE[:int(rng.integers(0, 4))])


# ---------------------------------------------------------------------------
# the cases worked by hand

def test_by_hand():
    seg = lambda ids, off, **kw: agree(np.asarray(ids, np.int64), off, TABLE, **kw)
    # leading and trailing separators: they go with the first segment and trail the last
    s = seg([NL, SP, 5, 6, NL, SP, 7, SP, NL, NL], [0, 10])
    assert s.out.tolist() == [5, 6, 7] and s.seg_offsets.tolist() == [0, 2, 3]
    assert s.src_start.tolist() == [0, 6] and s.src_end.tolist() == [6, 10] and s.doc_seg_offsets.tolist() == [0, 2]
    # a document of separators only has no segment, and takes no part in anyone's ranges
    s = seg([5, NL, SP, NL, 6], [0, 1, 4, 5])
    assert s.seg_doc.tolist() == [0, 2] and s.src_start.tolist() == [0, 4] and s.src_end.tolist() == [1, 5]
    assert s.doc_seg_offsets.tolist() == [0, 1, 1, 2]
    # BREAK on the last id: no empty segment behind it; BREAK on content: the id belongs to the line it ends
    s = seg([5, 6, END], [0, 3])
    assert s.out.tolist() == [5, 6, END] and s.seg_offsets.tolist() == [0, 3] and s.src_end.tolist() == [3]
    s = seg([5, NL], [0, 2])
    assert s.out.tolist() == [5] and s.src_end.tolist() == [2]
    # consecutive one-id segments
    s = seg([END, END, END, 5], [0, 4])
    assert s.seg_offsets.tolist() == [0, 1, 2, 3, 4] and s.src_start.tolist() == [0, 1, 2, 3] and s.src_end.tolist() == [1, 2, 3, 4]
    # SKIP alone neither ends a segment nor starts one, in any number
    s = seg([5] + [SP] * 9 + [6, NL] + [SP] * 9 + [7], [0, 22])
    assert s.out.tolist() == [5, 6, 7] and s.seg_offsets.tolist() == [0, 2, 3] and s.src_start.tolist() == [0, 21]
    # an open segment does not reach into the next document; tags; strays that carry BREAK change nothing
    s = seg([END, 5, 6, SP, 7, NL, 8, END], [1, 3, 7], tag=True)
    assert s.out.tolist() == [0, 5, 6, 1, 7, 1, 8] and s.seg_offsets.tolist() == [0, 3, 5, 7] and s.seg_doc.tolist() == [0, 1, 1]
    assert s.src_start.tolist() == [1, 3, 6] and s.src_end.tolist() == [3, 6, 7]
    # ids outside the table: negative, beyond it, an int64 whose low 32 bits index it -- class 0, at the full width
    s = seg([-1, NL + (1 << 32), 8, NL, SP - (1 << 32)], [0, 5])
    assert s.out.tolist() == [-1, NL + (1 << 32), 8, SP - (1 << 32)] and s.seg_offsets.tolist() == [0, 3, 4]
    assert model.segment_docs(np.asarray([NL, 5, NL, 6]), [0, 4], ()).seg_offsets.tolist() == [0, 4]    # no table: one segment
    # nothing at all
    s = seg([], [0])
    assert s.seg_offsets.tolist() == [0] and s.doc_seg_offsets.tolist() == [0] and len(s.out) == 0
    # marks
    marks, bad = model.segment_marks([0, 3, 3, 6], [2, 3, 5, 8], [1, 2, 3, 4], 9)
    assert bad is None and marks.tolist() == [1, 1, 0, 3, 3, 0, 4, 4, 0]
    for start, end, first_bad in (([-1], [2], 0), ([0, 3], [2, 2], 1), ([0, 1], [2, 3], 1), ([0, 3], [2, 10], 1), ([2, 1], [2, 1], 1)):
        assert model.segment_marks(start, end, [1] * len(start), 9) == (None, first_bad)
    assert model.segment_marks([], [], [], 3)[0].tolist() == [0, 0, 0]


def test_invariants():
    rng = np.random.default_rng(32)
    for case in range(200):
        ids, off = random_case(rng)
        classes = TABLE[:int(rng.integers(0, len(TABLE) + 1))]
        plain, tagged = model.segment_docs(ids, off, classes), model.segment_docs(ids, off, classes, True)
        content = [int(ids[p]) for p in range(off[0], off[-1]) if not model.class_of(ids[p], classes) & SKIP]
        assert plain.out.tolist() == content                                     # the content ids, in order
        assert np.delete(tagged.out, tagged.seg_offsets[:-1]).tolist() == content
        assert tagged.out[tagged.seg_offsets[:-1]].tolist() == tagged.seg_doc.tolist()
        assert (np.diff(plain.seg_offsets) >= 1).all() and (np.diff(plain.seg_doc) >= 0).all()
        for name in ("seg_doc", "doc_seg_offsets", "src_start", "src_end"):
            assert getattr(plain, name).tolist() == getattr(tagged, name).tolist()
        for d in range(len(off) - 1):
            a, b = plain.doc_seg_offsets[d], plain.doc_seg_offsets[d + 1]
            assert (plain.seg_doc[a:b] == d).all()
            if b > a:                                                             # the ranges tile the document
                assert plain.src_start[a] == off[d] and plain.src_end[b - 1] == off[d + 1]
                assert plain.src_end[a:b - 1].tolist() == plain.src_start[a + 1:b].tolist()
                assert (plain.src_end[a:b] > plain.src_start[a:b]).all()
        assert plain.doc_seg_offsets[-1] == len(plain.seg_doc)
        marks, bad = model.segment_marks(plain.src_start, plain.src_end, np.ones(len(plain.seg_doc)), len(ids))
        assert bad is None and marks[:off[0]].sum() == 0 and marks[off[-1]:].sum() == 0


# ---------------------------------------------------------------------------
# the class rule against text

TEXTS = (
    "first line\nsecond line\n\n\nfourth,  with a comma.\n  indented\tand tabbed \r\nlast without a newline",
    "\n\n  \n leading blank lines\nx\ny\n\nz.\n.\n...\n\n",
    "one line only",
    " \t\r\n\x0b\x0c\n",
    "a\rb\x0bc\x0cd\ne f\n",
    "Hello, World!\nHello, World!\n\"quoted\"\n(1) 22 333 4444\n#!/bin/sh\nend.\n\n\nend.",
    "".join(f"line {i} of many: the quick brown fox jumps over the lazy dog.\n" + " " * (i % 4) + "\n" * (i % 3) for i in range(40)),
)


@pytest.fixture()
def classes(native, monkeypatch):
    import minbpe_amd.tokenizer as T
    from fake_engine import OracleEngine
    eng = OracleEngine()
    monkeypatch.setattr(T, "engine", lambda device=None: eng)
    return T


def squeeze(s):
    return "".join(s.split())


@pytest.mark.parametrize("pattern", ("gpt2", "gpt4"))
def test_class_rule_against_text(classes, pattern):
    split = classes.GPT2_SPLIT_PATTERN if pattern == "gpt2" else classes.GPT4_SPLIT_PATTERN
    rng = np.random.default_rng(35)
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, size=int(rng.integers(2, 9)))) for _ in range(300)]
    more = "".join(" ".join(rng.choice(words, size=int(rng.integers(1, 9)))) + rng.choice([".\n", "\n", "!\n\n", " \n", "\r\n"])
                   for _ in range(200))
    train_text = "\n".join(TEXTS) + "\n" + more
    for merges in (0, 10, 60, 200):
        tok = classes.RegexTokenizer(split)
        tok.train(train_text, 256 + merges)
        assert len(tok.merges) == merges
        cls = tok.segment_classes()
        assert cls.dtype == np.uint8 and len(cls) == 256 + merges
        assert cls.tolist() == model.token_classes([tok.vocab[i] for i in range(256 + merges)]).tolist()
        assert merges < 200 or (cls[256:] & BREAK).any()                          # (a merged token that ends a line exists)
        for text in TEXTS:
            ids = np.asarray(tok.encode_ordinary(text), np.int64)
            seg = model.segment_docs(ids, [0, len(ids)], cls)
            got = [squeeze(tok.decode([int(x) for x in seg.out[a:b]])) for a, b in zip(seg.seg_offsets, seg.seg_offsets[1:])]
            want = [squeeze(line) for line in text.split("\n") if squeeze(line)]
            assert got == want, (pattern, merges, text[:40])
            # and the source ranges decode to the document, piece by piece
            pieces = [tok.decode([int(x) for x in ids[a:b]]) for a, b in zip(seg.src_start, seg.src_end)]
            assert "".join(pieces) == (text if want else "")


def test_class_rule_is_token_granular(classes):
    """BasicTokenizer merges across newlines: a token with a newline in its middle belongs, whole, to the line it ends"""
    tok = classes.BasicTokenizer()
    tok.train("ab\ncd ab\ncd ab\ncd ab\ncd", 256 + 4)
    inner = [i for i in range(256, 260) if b"\n" in tok.vocab[i].strip(b"\n") and tok.vocab[i].strip()]
    assert inner, [tok.vocab[i] for i in range(256, 260)]
    cls = tok.segment_classes()
    assert cls.tolist() == model.token_classes([tok.vocab[i] for i in range(260)]).tolist()
    assert all(cls[i] == BREAK for i in inner)
    assert cls[10] == BREAK | SKIP and cls[32] == cls[9] == cls[13] == cls[11] == cls[12] == SKIP and cls[ord("a")] == 0
    assert cls[0] == 0 and cls[0x1c] == 0 and cls[0x85] == 0 and cls[0xa0] == 0   # only the six ASCII bytes are blank
    ids = np.asarray(tok.encode("ab\ncd ab\ncd"), np.int64)
    seg = model.segment_docs(ids, [0, len(ids)], cls)
    for a, b in zip(seg.seg_offsets, seg.seg_offsets[1:]):
        assert all(not cls[t] & BREAK for t in seg.out[a:b - 1])                  # a boundary lies behind a segment's last id only
    with pytest.raises(ValueError):
        tok.segment_classes("paragraph")
    first = tok.segment_classes()
    first[:] = 7                                                                  # the caller's copy
    assert tok.segment_classes().tolist() == cls.tolist()
    tok.train("xyxyxy", 257)                                                      # a new vocabulary: a new table
    assert len(tok.segment_classes()) == 257


# ---------------------------------------------------------------------------
# the line statistics and the flag rule

def test_line_statistics_against_counter():
    rng = np.random.default_rng(33)
    for case in range(150):
        ids, off = random_case(rng, width=4 if case % 2 else 8)
        min_len = int(rng.integers(1, 4))
        seg = model.segment_docs(ids, off, TABLE)
        bodies = [tuple(seg.out[a:b].tolist()) for a, b in zip(seg.seg_offsets, seg.seg_offsets[1:])]
        n_docs = len(off) - 1
        for scope in ("in_doc", "stream"):
            got, dup = model.line_stats(ids, off, TABLE, scope, min_len)
            assert got.length.tolist() == np.diff(off).tolist() and got.lines.tolist() == np.diff(seg.doc_seg_offsets).tolist()
            want_dup = [0] * n_docs
            want_content, want_dup_content = [0] * n_docs, [0] * n_docs
            if scope == "in_doc":
                for d in range(n_docs):
                    mine = bodies[seg.doc_seg_offsets[d]:seg.doc_seg_offsets[d + 1]]
                    count = collections.Counter(mine)
                    want_dup[d] = sum(c - 1 for b, c in count.items() if len(b) >= min_len)
                    want_dup_content[d] = sum((c - 1) * len(b) for b, c in count.items() if len(b) >= min_len)
                    want_content[d] = sum(len(b) for b in mine)
            else:
                count = collections.Counter(bodies)
                assert int(dup.sum()) == sum(c - 1 for b, c in count.items() if len(b) >= min_len)
                seen = collections.Counter()
                for s, b in enumerate(bodies):
                    d = int(seg.seg_doc[s])
                    want_content[d] += len(b)
                    if seen[b] and len(b) >= min_len:
                        want_dup[d] += 1
                        want_dup_content[d] += len(b)
                    seen[b] += 1
            assert got.dup_lines.tolist() == want_dup and got.content.tolist() == want_content
            assert got.dup_content.tolist() == want_dup_content
            want_marks = np.zeros(len(ids), np.uint8)
            for s in np.flatnonzero(dup):
                want_marks[seg.src_start[s]:seg.src_end[s]] = 1
            assert got.marks.tolist() == want_marks.tolist() and all(c.dtype == np.int64 for c in got[:5])


def test_flag_rule_against_fractions():
    F = fractions.Fraction
    rng = np.random.default_rng(34)
    for case in range(300):
        n = 8
        lines = rng.integers(0, 12, size=n)
        dup_lines = np.array([int(rng.integers(0, max(l, 1))) for l in lines])
        content = lines * rng.integers(1, 9, size=n)
        dup_content = np.array([int(rng.integers(0, c + 1)) if d else 0 for c, d in zip(content, dup_lines)])
        stats = model.LineStats(lines, lines, dup_lines, content, dup_content, None)
        # thresholds that are exact in binary, so that the rational statement and the float64 one must agree
        lf, cf = F(int(rng.integers(0, 65)), 64), F(int(rng.integers(0, 65)), 64)
        want = [F(int(dl)) > lf * int(l) or F(int(dc)) > cf * int(c) for l, dl, c, dc in zip(lines, dup_lines, content, dup_content)]
        assert model.flagged(stats, float(lf), float(cf)).tolist() == want
        assert not model.flagged(stats, float(lf), float(cf))[lines == 0].any()  # no line: never flagged
    one = lambda l, dl, c, dc: model.flagged(model.LineStats(*[np.array([x]) for x in (l, l, dl, c, dc)], None))[0]
    assert not one(10, 3, 100, 20) and one(10, 4, 100, 0) and one(10, 0, 100, 21) and not one(0, 0, 0, 0)   # Gopher's: > 30 %, > 20 %


# ---------------------------------------------------------------------------
# declared, exported, bound, documented

def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, nargs, method in (("bpe_segment_docs_resident", 20, "segment_docs_resident"),
                                ("bpe_segment_marks_resident", 8, "segment_marks_resident")):
        assert re.search(rf"\bint\s+{name}\s*\(", code)
        assert hasattr(lib, name) and name in native.exported_symbols()
        assert len(getattr(native._lib, name).argtypes) == nargs
        assert callable(getattr(native.Engine, method))
    for text in ("#define BPE_SEG_BREAK 1u", "#define BPE_SEG_SKIP 2u", "#define BPE_SEG_TAG_DOC 1u"):
        assert text in hdr
    assert (native.SEG_BREAK, native.SEG_SKIP, native.SEG_TAG_DOC) == (1, 2, 1) == (model.BREAK, model.SKIP, model.TAG_DOC)
    for text in ("DESIGN 4.14", "tests/segments_model.py", "does not depend on scheduling", '"seg_tile"', '"seg_stage"',
                 "No workgroup waits for another inside a launch", "launch of its own", "drops", "BPE_E_CAP", "2^26"):
        assert text in hdr, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in ("seg_tile", "seg_stage", "bpe_segment_docs_resident", "bpe_segment_marks_resident"):
        assert text in integration, text
    for doc, texts in (("DESIGN.md", ("4.14", "seg_tile", "k_seg_carry", "k_seg_mark", "k_segmarks_fill", "paragraph")),
                       ("README.md", ("segments_resident", "duplicate_lines_resident", "test_gpu_segments.py", "segments_model.py",
                                      "repeat, dupspans, keep, segment")),
                       (os.path.join("profiles", "README.md"), ("segments_notes.md",))):
        body = open(os.path.join(ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)
    assert os.path.exists(os.path.join(ROOT, "tools", "segments_bench.py"))
    import minbpe_amd
    from minbpe_amd.tokenizer import LineDupStats, Segments, Tokenizer
    assert minbpe_amd.Segments is Segments and minbpe_amd.LineDupStats is LineDupStats
    assert "Segments" in minbpe_amd._EXPORTS and "LineDupStats" in minbpe_amd._EXPORTS
    assert Segments._fields == ("ids", "seg_offsets", "seg_doc", "doc_seg_offsets", "src_start", "src_end")
    assert LineDupStats._fields == ("length", "lines", "dup_lines", "content", "dup_content", "marks")
    for method in ("segment_classes", "segments_resident", "segment_marks_resident", "duplicate_lines_resident",
                   "repetitive_line_docs_resident", "drop_duplicate_lines_resident", "segments", "duplicate_lines",
                   "drop_duplicate_lines"):
        assert callable(getattr(Tokenizer, method))
    for prop in ("n_segments", "n_segment_ids", "n_duplicate_lines", "n_docs_with_duplicate_lines"):
        assert isinstance(getattr(Tokenizer, prop), property)
    # the two options have a row each, and the fields they set carry the defaults the header states
    options = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_options.hip")).read()
    assert "OPT_STEP(seg_tile, 64, SEG_TILE_MAX, 64)" in options and "OPT(seg_stage, 0, SEG_STAGE_MAX)" in options
    ctx = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")).read()
    tile = int(re.search(r"int seg_tile = (\d+);", ctx).group(1))
    stage = int(re.search(r"int seg_stage = (\d+);", ctx).group(1))
    assert f'"seg_tile" ({tile}:' in hdr and f'"seg_stage" ({stage},' in hdr
    assert f"`seg_tile` ({tile}:" in integration and f"`seg_stage` ({stage}" in integration
    kernels = open(os.path.join(ROOT, "minbpe_amd", "csrc", "kernels", "k_segment.hip")).read()
    assert "SEG_TILE_MAX = 65536" in kernels and "SEG_STAGE_MAX = 4096" in kernels
    for part, agg in (("kernels/k_segment.hip", "bpe_kernels.hip"), ("api/api_segment.hip", "bpe_api.hip")):
        assert f'#include "{part}"' in open(os.path.join(ROOT, "minbpe_amd", "csrc", agg)).read()


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    counters = lambda: (tok.n_segments, tok.n_segment_ids, tok.n_duplicate_lines, tok.n_docs_with_duplicate_lines)
    assert counters() == (None,) * 4
    resident = (tok.segments_resident, tok.duplicate_lines_resident, tok.repetitive_line_docs_resident,
                tok.drop_duplicate_lines_resident)
    host = (tok.segments, tok.duplicate_lines, tok.drop_duplicate_lines)
    # the unit and the classes
    for bad in ("paragraph", "", None, 0, b"line"):
        for f in resident:
            with pytest.raises(ValueError):
                f(ids, off, unit=bad)
        for f in host:
            with pytest.raises(ValueError):
                f(ids.numpy(), off, unit=bad)
        with pytest.raises(ValueError):
            tok.segment_classes(bad)
    for bad in (np.zeros(4, np.int32), np.zeros((2, 2), np.uint8), [0.5], torch.zeros(4, dtype=torch.int64),
                torch.zeros((2, 2), dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)[::2], "line"):
        for f in resident:
            with pytest.raises(TypeError, match="classes"):
                f(ids, off, classes=bad)
        for f in host:
            with pytest.raises(TypeError, match="classes"):
                f(ids.numpy(), off, classes=bad)
    with pytest.raises(TypeError, match="classes"):
        tok.segments_resident(ids, off, classes=torch.zeros(4, dtype=torch.uint8, device="meta"))
    # tag_docs, scope, min_len, the fractions
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            tok.segments_resident(ids, off, tag_docs=bad)
        with pytest.raises(ValueError):
            tok.segments(ids.numpy(), off, tag_docs=bad)
    for bad in ("doc", "", None, 0, True, b"stream", "earlier_doc"):
        for f in (tok.duplicate_lines_resident, tok.drop_duplicate_lines_resident):
            with pytest.raises(ValueError):
                f(ids, off, scope=bad)
        for f in (tok.duplicate_lines, tok.drop_duplicate_lines):
            with pytest.raises(ValueError):
                f(ids.numpy(), off, scope=bad)
    for bad in (0, -1, 2.0, True, "1", None):
        for f in resident[1:]:
            with pytest.raises(ValueError):
                f(ids, off, min_len=bad)
        for f in host[1:]:
            with pytest.raises(ValueError):
                f(ids.numpy(), off, min_len=bad)
    for kw in (dict(line_frac=-.1), dict(line_frac=1.5), dict(content_frac="0.2"), dict(content_frac=None), dict(line_frac=True),
               dict(content_frac=float("nan"))):
        with pytest.raises(ValueError):
            tok.repetitive_line_docs_resident(ids, off, **kw)
    # ids and offsets: dtype, contiguity, dimensions, where they live -- the last of them "not on a GPU"
    for f in resident:
        with pytest.raises(ValueError):
            f(ids, [])
        for bad_off in (torch.tensor([0.0, 10.0]), np.array([0.0, 10.0]), torch.tensor([0, 10], device="meta")):
            with pytest.raises(TypeError):
                f(ids, bad_off)
        for bad_ids in (ids.tolist(), ids.numpy(), ids.to(torch.int16), ids.to(torch.float32), ids.reshape(2, 5),
                        torch.arange(20, dtype=torch.int32)[::2]):
            with pytest.raises(TypeError):
                f(bad_ids, off)
        with pytest.raises(TypeError, match="on the GPU"):
            f(ids, off)
    for bad_out in (ids.numpy(), ids.to(torch.int64), ids.reshape(2, 5), torch.empty(10, dtype=torch.int32, device="meta")):
        for f in (tok.segments_resident, tok.drop_duplicate_lines_resident):
            with pytest.raises(TypeError, match="out"):
                f(ids, off, out=bad_out)
    # the marks: a Segments, values of its length where it lives, n
    seg = T.Segments(*[torch.zeros(k, dtype=torch.int64) for k in (5, 3, 2, 3, 2, 2)])
    values = torch.ones(2, dtype=torch.uint8)
    for bad in (None, tuple(seg), [1, 2]):
        with pytest.raises(TypeError, match="segments"):
            tok.segment_marks_resident(bad, values, 10)
    for bad in (-1, 2.0, None, True, "10"):
        with pytest.raises(ValueError):
            tok.segment_marks_resident(seg, values, bad)
    with pytest.raises(TypeError, match="GPU"):
        tok.segment_marks_resident(seg, values, 10)
    # the host forms: integers, flat; offsets as above; no out
    for f in host:
        for bad_ids in (np.array([0.5, 1.0]), np.zeros((2, 2), np.int64), ["a"]):
            with pytest.raises(TypeError):
                f(bad_ids, off)
        with pytest.raises(ValueError):
            f(ids.numpy(), [])
        with pytest.raises(TypeError):
            f(ids.numpy(), np.array([0.0, 10.0]))
        with pytest.raises(TypeError, match="out"):
            f(ids.numpy(), off, out=ids)
    assert counters() == (None,) * 4
