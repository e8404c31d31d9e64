"""CPU: the host side of the resident batch decode -- the two C-ABI entry points are declared, exported and bound, and
the tables the classes hand to the device (dense part, sorted sparse ids, GPT-4 byte map applied to the table) are what
bpe_decode_set_vocab / bpe_decode_set_sparse expect.  The kernels behind them: test_gpu_decode_resident.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import toy_rank_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bpe_decode_set_sparse", "bpe_decode_batch_resident")


def test_entry_points_declared_exported_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/bpe_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in native.exported_symbols()
    assert hasattr(native.Engine, "decode_set_sparse") and hasattr(native.Engine, "decode_batch_resident")


@pytest.fixture()
def classes(native, monkeypatch):
    import minbpe_amd.tokenizer as T
    from fake_engine import OracleEngine
    eng = OracleEngine()
    monkeypatch.setattr(T, "engine", lambda device=None: eng)
    return T


def _entries(blob, offs):
    return [blob[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


def test_resident_tables(classes, native):
    text = native.synth_text(30_000, 77).decode()
    tok = classes.RegexTokenizer()
    tok.train(text, 256 + 40)
    # registered out of order, with a gap above the dense range and the largest int32
    specials = {"<|endofprompt|>": 100276, "<|gap|>": 300, "<|endoftext|>": 100257, "<|max|>": 2**31 - 1}
    tok.register_special_tokens(specials)
    blob, offs, v_dense, sparse_ids = tok._decode_table_resident()
    assert v_dense == 296 and len(offs) == v_dense + len(specials) + 1
    assert sparse_ids.dtype == np.int32
    assert sparse_ids.tolist() == [300, 100257, 100276, 2**31 - 1]
    assert np.all(np.diff(sparse_ids.astype(np.int64)) > 0)
    assert np.all((sparse_ids < 0) | (sparse_ids >= v_dense))
    table = _entries(blob, offs)
    assert table[:v_dense] == [tok.vocab[i] for i in range(v_dense)]
    inv = {i: t.encode() for t, i in specials.items()}
    assert table[v_dense:] == [inv[int(i)] for i in sparse_ids]
    # the host form goes through the same table: it still decodes specials
    ids = tok.encode("<|gap|>ab<|max|>", allowed_special="all")
    assert tok.decode_batch(ids) == b"<|gap|>ab<|max|>"
    # an id that no int32 list can hold is refused here, not wrapped
    tok.register_special_tokens({"<|big|>": 2**31})
    with pytest.raises(ValueError):
        tok._decode_table_resident()

    # GPT-4: the resident table is the plain one passed through the inverse byte shuffle
    base = classes.RegexTokenizer()
    base.train(text, 256 + 120)
    _perm, ranks = toy_rank_table(base, 5)
    g = classes.GPT4Tokenizer(ranks)
    plain, poffs, pv, _sparse = g._decode_table()
    rblob, roffs, rv, rsparse = g._decode_table_resident()
    assert rblob == plain.translate(g._unshuffle_lut) and rblob != plain
    assert np.array_equal(roffs, poffs) and rv == pv == 376 and len(rsparse) == 0  # (gpt4.py:89: specials do not decode)
    probe = text[:500]
    want = g.encode_ordinary(probe)
    assert b"".join(_entries(rblob, roffs)[i] for i in want) == probe.encode("utf-8")
