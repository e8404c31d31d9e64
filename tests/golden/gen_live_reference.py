"""Generate tests/golden/live_reference.json by RUNNING THE REFERENCE (karpathy/minbpe) on the inputs of the
comparisons in tests/test_oracle_golden.py and tests/test_reference_suite.py, so that those tests need nothing
outside this repository.

    python tests/golden/gen_live_reference.py PATH_TO_MINBPE_CHECKOUT

The inputs are rebuilt by tests/helpers.py (random.Random, synth_text, the committed taylorswift.txt) and pinned
here by sha256; what is stored is the reference's answer: merge lists (null where train() raises ValueError on an
empty pair table), encoded ids, and the bytes of the files save() writes.  The test strings and texts of the
reference's own test module (tests/test_tokenizer.py) are stored as data.  tiktoken is not needed: a stub module
satisfies minbpe/__init__.py's import; GPT4Tokenizer is never constructed.
"""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main(ref_root):
    sys.modules.setdefault("tiktoken", types.ModuleType("tiktoken"))
    sys.path.insert(0, ref_root)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(HERE))
    import importlib.util
    import numpy as np
    from minbpe import BasicTokenizer, RegexTokenizer  # noqa: E402  (the reference)
    from minbpe_amd import _native as native
    import helpers as H

    def train_or_none(tok, text, vocab_size):
        try:
            tok.train(text, vocab_size)
            return [list(p) for p in tok.merges]
        except ValueError:
            return None

    out = {"generated_by": "tests/golden/gen_live_reference.py, running karpathy/minbpe"}

    # test_oracle_golden.test_against_live_reference_random
    rows = []
    for text in H.random_texts(native):
        for nm in (5, 40):
            row = {"sha256": H.sha256_text(text), "num_merges": nm}
            ref = BasicTokenizer()
            row["basic"] = train_or_none(ref, text, 256 + nm)
            if row["basic"] is not None:
                row["basic_probe_ids"] = ref.encode(text[: len(text) // 3] + text[::-1][:50])
            ref = RegexTokenizer()
            row["regex"] = train_or_none(ref, text, 256 + nm)
            if row["regex"] is not None:
                row["regex_probe_ids"] = ref.encode_ordinary(text[: len(text) // 3])
            rows.append(row)
    out["random"] = rows

    # test_oracle_golden.test_weighted_oracle_against_live_reference
    out["weighted"] = [{"sha256": H.sha256_text(text), "num_merges": nm, "regex": train_or_none(RegexTokenizer(), text, 256 + nm)}
                       for text in H.weighted_texts(native) for nm in (8, 60)]

    # test_oracle_golden.test_oracle_encode_with_a_cl100k_sized_table_against_live_reference
    base = H.cl100k_base_pairs(native)
    probe = H.cl100k_probe(native)
    cl = {"probe_sha256": H.sha256_text(probe), "base_pairs_sha256": H.sha256_text(repr([tuple(p) for p in base]))}
    for kind in ("rank", "sparse"):
        pairs, mids = H.cl100k_shaped_table(base, 100_000, 5, kind)
        ref = RegexTokenizer()
        vals = mids if mids is not None else 256 + np.arange(len(pairs))
        ref.merges = {(int(a), int(b)): int(v) for (a, b), v in zip(pairs, vals)}
        assert len(ref.merges) == len(pairs)
        cl[kind] = ref.encode_ordinary(probe)
    out["cl100k_encode"] = cl

    # test_reference_suite.test_reference_test_module_passes_against_this_package: the reference's test module's
    # data, and what the reference itself answers on it
    spec = importlib.util.spec_from_file_location("ref_test_tokenizer", os.path.join(ref_root, "tests", "test_tokenizer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    strings = [s for s in mod.test_strings if not s.startswith("FILE:")]
    files = [s[5:] for s in mod.test_strings if s.startswith("FILE:")]
    for f in files:  # the module's FILE: strings are this fixture's taylorswift.txt
        with open(os.path.join(ref_root, "tests", f), "rb") as a, open(os.path.join(HERE, f), "rb") as b:
            assert a.read() == b.read(), f
    suite = {"test_strings": strings, "test_files": files, "llama_text": mod.llama_text,
             "special_tokens": mod.special_tokens, "wikipedia": {}, "save_load": []}
    for name, cls in (("basic", BasicTokenizer), ("regex", RegexTokenizer)):
        tok = cls()
        tok.train("aaabdaaabac", 256 + 3)
        suite["wikipedia"][name] = tok.encode("aaabdaaabac")
    for specials in ({}, mod.special_tokens):
        tok = RegexTokenizer()
        tok.train(mod.llama_text, 256 + 64)
        tok.register_special_tokens(specials)
        with tempfile.TemporaryDirectory() as d:
            tok.save(os.path.join(d, "t"))
            model = open(os.path.join(d, "t.model"), encoding="utf-8").read()
        suite["save_load"].append({"special_tokens": specials, "ids": tok.encode(mod.llama_text, "all"), "model": model})
    out["suite"] = suite

    # test_reference_suite.test_saved_files_are_byte_identical_to_the_reference
    text = H.saved_files_text(HERE)
    saved = {"sha256": H.sha256_text(text)}
    for name, cls in (("basic", BasicTokenizer), ("regex", RegexTokenizer)):
        tok = cls()
        tok.train(text, 256 + 80)
        if name == "regex":
            tok.register_special_tokens({"<|endoftext|>": 100257, "<|pad|>": 100258})
        with tempfile.TemporaryDirectory() as d:
            tok.save(os.path.join(d, "t"))
            files = {ext: open(os.path.join(d, "t" + ext), "rb").read().decode("utf-8") for ext in (".model", ".vocab")}
        saved[name] = {"merges": [list(p) for p in tok.merges], "model": files[".model"], "vocab": files[".vocab"],
                       "probe_ids": tok.encode(text[1000:3000])}
    out["saved_files"] = saved

    path = os.path.join(HERE, "live_reference.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, separators=(",", ":"), ensure_ascii=False)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
