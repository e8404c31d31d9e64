"""CPU: bpe_token_spans_resident is declared, exported and bound; the NumPy model of its definition (spans_model) agrees
with Python's own str on what a byte span and a character span are; every argument error of token_spans_resident /
token_spans is raised before an engine exists."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import spans_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+bpe_token_spans_resident\s*\(", code)
    assert re.search(r"#define\s+BPE_PROF_NKINDS\s+7\b", code)
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "bpe_token_spans_resident")
    assert "bpe_token_spans_resident" in native.exported_symbols()
    assert len(native._lib.bpe_token_spans_resident.argtypes) == 12
    assert callable(native.Engine.token_spans_resident)
    import minbpe_amd.tokenizer as T
    assert callable(T.Tokenizer.token_spans_resident) and callable(T.Tokenizer.token_spans)
    assert callable(T.RegexTokenizer.encode_ordinary_with_offsets) and callable(T.BasicTokenizer.encode_with_offsets)
    for cls in (T.BasicTokenizer, T.RegexTokenizer, T.GPT4Tokenizer):   # one implementation, on the base class
        assert cls.token_spans_resident is T.Tokenizer.token_spans_resident
        assert cls.token_spans is T.Tokenizer.token_spans


# ASCII, 2-, 3- and 4-byte characters and a combining mark
TEXTS = ["", "a", "\u00e9", "a\u00e9", "\u65e5", "\U0001f609", "e\u0301", "a\u00e9\u65e5\U0001f609e\u0301z",
         "\u00fcn\u00ef \U0001f609 \u65e5\u672c\u8a9e e\u0301!"]


def cuts_to_pieces(enc, cuts):
    """enc cut at the byte positions `cuts` (ascending, repeats make empty tokens)"""
    edges = [0] + list(cuts) + [len(enc)]
    return [enc[a:b] for a, b in zip(edges, edges[1:])]


def check_document(s, pieces):
    table = sorted(set(pieces))
    tidx = [table.index(p) for p in pieces]
    bs, cs = spans_model.spans(table, tidx)
    spans_model.check_against_str(s, pieces, bs, cs)
    return bs, cs


def test_model_against_str_exhaustive():
    """every subset of the byte boundaries of short texts (tokens that are pure continuation bytes, a lead without its
    tail, several characters), and every single boundary doubled (an empty token there)"""
    n_cases = 0
    for s in TEXTS:
        enc = s.encode("utf-8")
        inner = list(range(1, len(enc)))
        if len(inner) > 11:   # the longest text: every pattern over its first 11 boundaries, the rest cut everywhere
            subsets = (list(c) + inner[11:] for k in range(12) for c in itertools.combinations(inner[:11], k))
        else:
            subsets = (list(c) for k in range(len(inner) + 1) for c in itertools.combinations(inner, k))
        for cuts in subsets:
            pieces = cuts_to_pieces(enc, cuts)
            bs, cs = check_document(s, pieces)
            n_cases += 1
            if len(enc) <= 6:   # ... and against the definition in words, by brute force
                for i, p in enumerate(pieces):
                    if p:
                        assert tuple(cs[i]) == spans_model.shortest_cover(s, int(bs[i][0]), int(bs[i][1]))
        for pos in range(len(enc) + 1):   # empty tokens: at the ends, between and inside characters
            check_document(s, cuts_to_pieces(enc, [pos, pos]))
            check_document(s, cuts_to_pieces(enc, sorted(inner + [pos])))   # (a boundary doubled, or one at an end)
    assert n_cases > 4000
    # the example of the definition: two byte tokens that split one two-byte character both get (k, k + 1)
    bs, cs = check_document("a\u00e9", [b"a", b"\xc3", b"\xa9"])
    assert cs.tolist() == [[0, 1], [1, 2], [1, 2]] and bs.tolist() == [[0, 1], [1, 2], [2, 3]]


def test_model_against_str_random_documents():
    """seeded random cuts of longer texts, as several documents of one batch: empty documents, tokens before the first
    and after the last offset, offsets that cut in the middle of a character's tokens never (a document is a text)"""
    rng = np.random.default_rng(2024)
    alphabet = list("abc xyz,.") + ["\u00e9", "\u00fc", "\u00df", "\u65e5", "\u672c", "\u8a9e", "\u20ac", "\U0001f609",
                                    "\U0001f642", "e\u0301", "a\u0323\u0308"]
    for trial in range(60):
        docs = []
        for _ in range(int(rng.integers(1, 6))):
            s = "".join(alphabet[k] for k in rng.integers(0, len(alphabet), int(rng.integers(0, 25))))
            enc = s.encode("utf-8")
            cuts = sorted(rng.integers(0, len(enc) + 1, int(rng.integers(0, len(enc) + 3))).tolist())
            docs.append((s, cuts_to_pieces(enc, cuts)))
            if rng.random() < 0.3:
                docs.append(("", []))        # an empty document
        before = [b"zz"] * int(rng.integers(0, 3))   # tokens that belong to no document
        after = [b"\x80"] * int(rng.integers(0, 3))
        pieces = before + [p for _, ps in docs for p in ps] + after
        table = sorted(set(pieces))
        tidx = [table.index(p) for p in pieces]
        off = [len(before)]
        for _, ps in docs:
            off.append(off[-1] + len(ps))
        bs, cs = spans_model.spans(table, tidx, off)
        assert (bs[:off[0]] == -1).all() and (cs[:off[0]] == -1).all()
        assert (bs[off[-1]:] == -1).all() and (cs[off[-1]:] == -1).all()
        for d, (s, ps) in enumerate(docs):
            spans_model.check_against_str(s, ps, bs[off[d]:off[d + 1]], cs[off[d]:off[d + 1]])
        assert spans_model.totals(table, tidx) == (sum(map(len, pieces)),
                                                   sum(1 for p in pieces for b in p if (b & 0xC0) != 0x80))


def test_model_on_invalid_utf8():
    """the numbers are defined by the rule also where nothing decodes: the clamp at 0, lone continuation bytes"""
    table = [b"\x80", b"\xc3", b"", b"\x80\x80\x80", b"a\x80"]
    bs, cs = spans_model.spans(table, [0, 3, 1, 2, 4, 0])
    assert bs.tolist() == [[0, 1], [1, 4], [4, 5], [5, 5], [5, 7], [7, 8]]
    assert cs.tolist() == [[0, 0], [0, 0], [0, 1], [1, 1], [1, 2], [1, 2]]
    assert [spans_model.entry_meta(e) for e in table] == [(1, 0, 1), (1, 1, 0), (0, 0, 0), (3, 0, 1), (2, 1, 0)]


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.RegexTokenizer()
    ids = torch.arange(10, dtype=torch.int64)
    for unit in ("chars", "", None, "BYTE", 1):
        with pytest.raises(ValueError):
            tok.token_spans_resident(ids, unit=unit)
        with pytest.raises(ValueError):
            tok.token_spans(list(range(10)), unit=unit)
        with pytest.raises(ValueError):
            tok.encode_ordinary_with_offsets("some text", unit=unit)
        with pytest.raises(ValueError):
            T.BasicTokenizer().encode_with_offsets("some text", unit=unit)
    for wrong in (ids.tolist(), ids.numpy(), ids.to(torch.float32), ids.to(torch.int16), ids.reshape(2, 5),
                  torch.arange(20, dtype=torch.int64)[::2]):
        with pytest.raises(TypeError):
            tok.token_spans_resident(wrong)
    for unit in ("char", "byte", "both"):   # a CPU tensor is refused whatever else is in order
        with pytest.raises(TypeError, match="GPU"):
            tok.token_spans_resident(ids, [0, 4, 10], unit=unit)
        with pytest.raises(TypeError, match="GPU"):
            tok.token_spans_resident(ids.to(torch.int32), torch.tensor([0, 10]), unit=unit)
    for wrong_off in (torch.tensor([0.0, 10.0]), np.array([0.0, 10.0]), [0.5, 10],
                      torch.empty(2, dtype=torch.int64, device="meta"), torch.tensor([0, 10], dtype=torch.int16)):
        with pytest.raises(TypeError, match="doc_offsets"):
            tok.token_spans_resident(ids, wrong_off)
    with pytest.raises(ValueError):
        tok.token_spans_resident(ids, [])                       # n_docs + 1 entries: at least one
    # the host form: what it objects to before it asks for a device
    for wrong in ([0.5, 1.0], np.array([1.0, 2.0]), ["a"], np.arange(6).reshape(2, 3)):
        with pytest.raises(TypeError):
            tok.token_spans(wrong)
    with pytest.raises(TypeError):
        tok.token_spans([1, 2, 3], doc_offsets=[0.0, 3.0])
    with pytest.raises(ValueError):
        tok.token_spans([1, 2, 3], device="cpu")
