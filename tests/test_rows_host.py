"""CPU: bpe_rows_resident is declared, exported and bound; rows_count is the number of rows the definition produces;
every argument error of Tokenizer.rows_resident is raised before an engine exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import rows_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+bpe_rows_resident\s*\(", code)
    for name, value in (("BPE_ROWS_PACK", "0"), ("BPE_ROWS_PER_DOC", "1"), ("BPE_ROWS_HAS_SEP", "1u"),
                        ("BPE_ROWS_TRUNC_LEFT", "2u"), ("BPE_ROWS_PAD_LEFT", "4u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert re.search(r"#define\s+BPE_PROF_NKINDS\s+7\b", code)
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "bpe_rows_resident")
    assert "bpe_rows_resident" in native.exported_symbols()
    assert len(native._lib.bpe_rows_resident.argtypes) == 19
    assert callable(native.Engine.rows_resident)
    assert (native.ROWS_PACK, native.ROWS_PER_DOC) == (0, 1)
    assert (native.ROWS_HAS_SEP, native.ROWS_TRUNC_LEFT, native.ROWS_PAD_LEFT) == (1, 2, 4)


def test_rows_count_is_the_models_count():
    from minbpe_amd.tokenizer import rows_count
    for L in range(1, 13):
        for S in range(1, L + 1):
            for T in range(0, 201):
                assert rows_count(T, L, S) == rows_model.brute_rows(T, L, S), (T, L, S)
    # ... and the model's rows have that shape, with only the last one partial
    rows, _, _ = rows_model.pack(np.arange(24), [0, 24], 5, 3, None, -1)
    assert rows.shape == (rows_count(24, 5, 3), 5) == (8, 5)
    assert not (rows[:-1] == -1).any() and (rows[-1] == -1).any()
    for bad in ((10, 0, 1), (10, 4, 0), (10, 4, 5), (-1, 4, 4)):
        with pytest.raises(ValueError):
            rows_count(*bad)


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.RegexTokenizer()
    tok.register_special_tokens({"<|endoftext|>": 100257})
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    value_errors = [
        dict(row_len=0), dict(row_len=-3), dict(row_len=2.0), dict(row_len=True),
        dict(stride=0), dict(stride=5), dict(stride=-1), dict(stride=1.5),
        dict(mode="rows"), dict(truncate="middle"), dict(pad_side="both"),
        dict(truncate="left"), dict(pad_side="left"),                      # per-document matters in pack mode
        dict(mode="per_doc", stride=2), dict(mode="per_doc", drop_last=True),
        dict(mode="per_doc", return_doc_index=True), dict(mode="per_doc", return_positions=True),
        dict(sep=2**31), dict(sep=-2**31 - 1), dict(sep=1.0), dict(pad=2**31), dict(pad=None), dict(pad="x"),
        dict(dtype=torch.int16), dict(dtype=torch.float32), dict(dtype="int64"),
    ]
    for kw in value_errors:
        kw = dict(kw)
        row_len = kw.pop("row_len", 4)
        with pytest.raises(ValueError):
            tok.rows_resident(ids, off, row_len, **kw)
    with pytest.raises(ValueError):
        tok.rows_resident(ids, [], 4)                                       # n_docs + 1 entries: at least one
    with pytest.raises(KeyError):
        tok.rows_resident(ids, off, 4, sep="<|nope|>")
    with pytest.raises(KeyError):
        T.BasicTokenizer().rows_resident(ids, off, 4, sep="<|endoftext|>")  # nothing is registered there
    type_errors = [
        dict(ids=ids.tolist()), dict(ids=ids.numpy()), dict(ids=ids.to(torch.int64)), dict(ids=ids.to(torch.float32)),
        dict(ids=ids.reshape(2, 5)), dict(ids=torch.arange(20, dtype=torch.int32)[::2]),
        dict(doc_offsets=torch.tensor([0.0, 10.0])), dict(doc_offsets=np.array([0.0, 10.0])),
        dict(out=np.zeros((3, 4), np.int64)), dict(out=torch.zeros((3, 4), dtype=torch.int32)),
        dict(out=torch.zeros((3, 8), dtype=torch.int64)[:, ::2]),
    ]
    for kw in type_errors:
        args = dict(ids=ids, doc_offsets=off)
        args.update(kw)
        with pytest.raises(TypeError):
            tok.rows_resident(args.pop("ids"), args.pop("doc_offsets"), 4, **args)
    # everything else in order: what is left to object to is that the ids are not on a GPU
    for kw in (dict(), dict(sep="<|endoftext|>", stride=3, pad=-100, dtype=torch.int32, drop_last=True,
                            return_doc_index=True, return_positions=True),
               dict(mode="per_doc", truncate="left", pad_side="left", sep=7)):
        with pytest.raises(TypeError, match="GPU"):
            tok.rows_resident(ids, off, 4, **kw)
