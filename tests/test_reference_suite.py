"""CPU: the checks of the reference's OWN test module (tests/test_tokenizer.py) restated on its data -- test
strings, the Wikipedia example, save/load with and without special tokens -- with `minbpe` resolving to this
package, and compared with what the reference itself answered on the same data (tests/golden/live_reference.json
<- tests/golden/gen_live_reference.py).  The device engine is the oracle-backed test double
(tests/fake_engine.py), so this exercises the drop-in surface -- names, signatures, results, exceptions,
save/load -- not the kernels; the two tiktoken-equality tests are left out (no cl100k ranks offline)."""
import json
import os
import sys

import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def live_ref():
    with open(os.path.join(GOLDEN_DIR, "live_reference.json"), encoding="utf-8") as f:
        return json.load(f)


def test_reference_test_module_passes_against_this_package(native, monkeypatch, tmp_path, live_ref):
    import minbpe_amd
    import minbpe_amd.tokenizer as T
    from fake_engine import OracleEngine
    eng = OracleEngine()
    monkeypatch.setattr(T, "engine", lambda device=None: eng)
    monkeypatch.setitem(sys.modules, "minbpe", minbpe_amd)  # `from minbpe import BasicTokenizer, ...`
    from minbpe import BasicTokenizer, RegexTokenizer
    assert BasicTokenizer is minbpe_amd.BasicTokenizer and RegexTokenizer is minbpe_amd.RegexTokenizer
    suite = live_ref["suite"]
    texts = list(suite["test_strings"])
    for name in suite["test_files"]:  # the module's FILE: strings, resolved next to its test file
        texts.append(open(os.path.join(GOLDEN_DIR, name), encoding="utf-8").read())
    assert len(texts) == 4
    ran = 0
    for name, factory in (("basic", BasicTokenizer), ("regex", RegexTokenizer)):
        for text in texts:  # test_encode_decode_identity
            tok = factory()
            assert tok.decode(tok.encode(text)) == text
            ran += 1
        tok = factory()  # test_wikipedia_example
        tok.train("aaabdaaabac", 256 + 3)
        ids = tok.encode("aaabdaaabac")
        assert ids == [258, 100, 258, 97, 99] == suite["wikipedia"][name]
        assert tok.decode(tok.encode("aaabdaaabac")) == "aaabdaaabac"
        ran += 1
    monkeypatch.chdir(tmp_path)  # test_save_load writes its files into the working directory
    text = suite["llama_text"]
    for rec in suite["save_load"]:  # test_save_load
        specials = rec["special_tokens"]
        tok = RegexTokenizer()
        tok.train(text, 256 + 64)
        tok.register_special_tokens(specials)
        assert tok.decode(tok.encode(text, "all")) == text
        ids = tok.encode(text, "all")
        assert ids == rec["ids"]  # the reference's own encoding
        tok.save("test_tokenizer_tmp")
        assert open("test_tokenizer_tmp.model", encoding="utf-8").read() == rec["model"]
        tok = RegexTokenizer()
        tok.load("test_tokenizer_tmp.model")
        assert tok.decode(ids) == text
        assert tok.decode(tok.encode(text, "all")) == text
        assert tok.encode(text, "all") == ids
        for f in ("test_tokenizer_tmp.model", "test_tokenizer_tmp.vocab"):
            os.remove(f)
        ran += 1
    assert [r["special_tokens"] for r in suite["save_load"]][0] == {} and len(suite["save_load"]) == 2
    assert ran == 12 and os.listdir(tmp_path) == []


def test_saved_files_are_byte_identical_to_the_reference(native, monkeypatch, tmp_path, live_ref):
    """train.py's flow (train, register specials, save) on a slice of the reference's own sample
    text: the .model and .vocab files written by this package are the bytes the reference wrote."""
    import minbpe_amd.tokenizer as T
    from fake_engine import OracleEngine
    from helpers import saved_files_text, sha256_text
    eng = OracleEngine()
    monkeypatch.setattr(T, "engine", lambda device=None: eng)
    text = saved_files_text(GOLDEN_DIR)
    saved = live_ref["saved_files"]
    assert sha256_text(text) == saved["sha256"]
    for name, ours in (("basic", T.BasicTokenizer), ("regex", T.RegexTokenizer)):
        theirs = saved[name]
        a = ours()
        a.train(text, 256 + 80)
        assert [list(p) for p in a.merges] == theirs["merges"]
        if name == "regex":
            a.register_special_tokens({"<|endoftext|>": 100257, "<|pad|>": 100258})
        a.save(str(tmp_path / f"ours_{name}"))
        for ext, key in ((".model", "model"), (".vocab", "vocab")):
            assert open(tmp_path / f"ours_{name}{ext}", "rb").read() == theirs[key].encode("utf-8")
        # and this package loads the reference's file
        with open(tmp_path / f"ref_{name}.model", "wb") as f:
            f.write(theirs["model"].encode("utf-8"))
        c = ours()
        c.load(str(tmp_path / f"ref_{name}.model"))
        assert c.merges == a.merges and c.special_tokens == a.special_tokens and c.pattern == a.pattern
        probe = text[1000:3000]
        assert c.encode(probe) == theirs["probe_ids"] and c.decode(c.encode(probe)) == probe
