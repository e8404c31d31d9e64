"""CPU: bpe_project_set_merges / bpe_project_resident are declared, exported and bound; the plain-Python model of the
projection (project_model) agrees with what the truncated tokenizer itself encodes, through the oracle-backed engine
double; at_vocab(); every argument error is raised before an engine exists.
The limit check (BPE_E_LIMIT for a 40-merge doubling chain) is made on the host before any device work, but it needs a
ctx, and a ctx needs a GPU: it is with the GPU tests (test_gpu_project.py::test_limits_from_the_merge_list)."""
import ctypes
import os
import re

import numpy as np
import pytest

import project_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [256, 257, 300, 400, 655, 656]
FOREIGN = ("Grüße aus Köln, 日本語のテキスト \U0001f609\U0001f642 and Taylor "
           + "a" * 40 + " € 1989 songwriter\n\nété " + "the album " * 3)


def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+BPE_PROF_NKINDS\s+7\b", code)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, nargs in (("bpe_project_set_merges", 5), ("bpe_project_resident", 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, code)
        assert hasattr(lib, name)
        assert name in native.exported_symbols()
        assert len(getattr(native._lib, name).argtypes) == nargs
    assert callable(native.Engine.project_set_merges) and callable(native.Engine.project_resident)
    import minbpe_amd.tokenizer as T
    for cls in (T.BasicTokenizer, T.RegexTokenizer, T.GPT4Tokenizer):   # one implementation, on the base class
        for method in ("project_resident", "project", "projected_count"):
            assert getattr(cls, method) is getattr(T.Tokenizer, method)
    assert T.BasicTokenizer.at_vocab is T.Tokenizer.at_vocab and T.RegexTokenizer.at_vocab is T.Tokenizer.at_vocab
    assert T.GPT4Tokenizer.at_vocab is not T.Tokenizer.at_vocab


@pytest.fixture(scope="module")
def T(native):
    """minbpe_amd.tokenizer with the oracle-backed engine double in place of the device"""
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


def merge_list(tok):
    return [p for p, _ in sorted(tok.merges.items(), key=lambda kv: kv[1])]


def encode_of(tok):
    return tok.encode_ordinary if hasattr(tok, "encode_ordinary") else tok.encode


@pytest.mark.parametrize("kind", ["regex", "basic"])
def test_model_against_truncated_tokenizer(trained, taylor, kind):
    tok = trained[kind]
    merges = merge_list(tok)
    for text in (taylor[5_000:9_000], FOREIGN):
        ids = encode_of(tok)(text)
        assert max(ids) >= 300   # (the text uses the upper merges: something is there to expand)
        for size in SIZES:
            small = tok.at_vocab(size)
            assert encode_of(small)(text) == project_model.project(ids, merges, size), (kind, size)
            assert small.decode(encode_of(small)(text)) == text


def test_model_against_truncated_tokenizer_doubling_chain(T):
    tok = T.BasicTokenizer()
    tok.train("a" * 5000, 256 + 12)
    merges = merge_list(tok)
    assert merges == [(97, 97)] + [(255 + r, 255 + r) for r in range(1, 12)]
    ids = tok.encode("a" * 5000)
    assert ids == [267, 264, 263, 262, 258]
    assert len(project_model.project([267], merges, 256)) == 4096
    for size in range(256, 269):
        got = project_model.project(ids, merges, size)
        assert tok.at_vocab(size).encode("a" * 5000) == got
        assert got == [t for i in ids for t in project_model.expand(i, merges, size)]
        assert project_model.doc_offsets(ids, merges, size, [0, 1, 5]).tolist() == \
            [0, len(project_model.expand(267, merges, size)), len(got)]


def test_model_pass_ids_and_bad_ids():
    merges = [(97, 98), (256, 99), (257, 257)]
    assert project_model.project([258, -7, 5, 300000], merges, 256, pass_ids=[-7, 300000]) == [97, 98, 99] * 2 + [-7, 5, 300000]
    assert project_model.project([258, 257], merges, 258) == [257, 257, 257]
    for bad, where in (([1, 259], 1), ([-1, 259], 0), ([258, 2**32 + 5], 1)):
        with pytest.raises(project_model.BadId) as e:
            project_model.project(bad, merges, 256, pass_ids=[-7])
        assert e.value.args[0] == where


def test_at_vocab(trained, T, tmp_path):
    tok = trained["regex"]
    tok.register_special_tokens({"<|endoftext|>": 100257, "<|pad|>": 700})
    try:
        small = tok.at_vocab(300)
        assert type(small) is T.RegexTokenizer
        assert list(small.merges.items()) == list(tok.merges.items())[:44]
        assert small.vocab == {i: tok.vocab[i] for i in range(300)}
        assert small.pattern == tok.pattern and small.compiled_pattern.pattern == tok.pattern
        assert small.special_tokens == tok.special_tokens and small.special_tokens is not tok.special_tokens
        assert small.inverse_special_tokens == {100257: "<|endoftext|>", 700: "<|pad|>"}
        small.save(str(tmp_path / "small"))
        again = T.RegexTokenizer()
        again.load(str(tmp_path / "small.model"))
        assert again.merges == small.merges and again.special_tokens == small.special_tokens
        assert again.pattern == small.pattern
        assert {i: b for i, b in again.vocab.items() if i < 300} == small.vocab
        text = "Taylor Swift<|endoftext|> songs"
        assert again.encode(text, allowed_special="all") == small.encode(text, allowed_special="all")
        full = tok.at_vocab(656)
        assert full.merges == tok.merges and full.vocab == tok.vocab and full.special_tokens == tok.special_tokens
        assert full.encode_ordinary(FOREIGN) == tok.encode_ordinary(FOREIGN)
    finally:
        tok.register_special_tokens({})
    basic = trained["basic"]
    b300 = basic.at_vocab(300)
    assert type(b300) is T.BasicTokenizer and b300.pattern == "" and b300.special_tokens == {}
    assert list(b300.merges.items()) == list(basic.merges.items())[:44]
    assert b300.vocab == {i: basic.vocab[i] for i in range(300)}
    assert basic.at_vocab(256).merges == {} and basic.at_vocab(256).encode("hi") == [104, 105]
    gpt4 = T.GPT4Tokenizer.__new__(T.GPT4Tokenizer)   # (no ranks offline: the method itself)
    with pytest.raises(NotImplementedError):
        gpt4.at_vocab(300)


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.RegexTokenizer()
    tok.merges = {(97, 98): 256, (256, 99): 257, (257, 257): 258}
    tok.vocab = tok._build_vocab()
    gpu_like = torch.empty(4, dtype=torch.int64, device="meta")   # (not on the GPU either)
    ids = torch.arange(10, dtype=torch.int64)
    # vocab_size outside [256, 256 + M]
    for size in (255, 260, 0, -1, 2**40, 256.0, "300", None, True):
        with pytest.raises(ValueError, match="vocab_size"):
            tok.at_vocab(size)
        with pytest.raises(ValueError, match="vocab_size"):
            tok.project([1, 2, 3], size)
        with pytest.raises(ValueError, match="vocab_size"):
            tok.projected_count([1, 2, 3], size)
    # a merge list that does not have the training shape
    for merges in ({(97, 98): 256, (256, 99): 258}, {(97, 98): 257}, {(97, 256): 256}, {(97, 98): 256, (258, 99): 257},
                   {(-1, 98): 256}):
        bad = T.BasicTokenizer()
        bad.merges = merges
        with pytest.raises(ValueError, match="shape"):
            bad.at_vocab(256)
        with pytest.raises(ValueError, match="shape"):
            bad.project([1, 2, 3], 256)
    # a special token inside [vocab_size, 256 + M)
    tok.register_special_tokens({"<|a|>": 258, "<|b|>": 100257})
    for size in (256, 257, 258):
        with pytest.raises(ValueError, match="special token id 258"):
            tok.at_vocab(size)
        with pytest.raises(ValueError, match="special token id 258"):
            tok.project([1, 2, 3], size)
    assert tok.at_vocab(259).special_tokens == {"<|a|>": 258, "<|b|>": 100257}
    tok.register_special_tokens({"<|big|>": 2**31})
    with pytest.raises(ValueError, match="int32"):
        tok.project([1, 2, 3], 256)
    tok.register_special_tokens({})
    # tensors of another dtype, or not on the GPU
    for wrong in (ids, ids.to(torch.int32), gpu_like, ids.tolist(), ids.numpy(), ids.to(torch.float32)):
        with pytest.raises(TypeError):
            tok.project_resident(wrong, 256)
    with pytest.raises(TypeError):
        tok.projected_count(ids, 256)
    for wrong in ([0.5, 1.0], np.array([1.0, 2.0]), ["a"], np.arange(6).reshape(2, 3)):
        with pytest.raises(TypeError):
            tok.project(wrong, 256)
        with pytest.raises(TypeError):
            tok.projected_count(wrong, 256)
