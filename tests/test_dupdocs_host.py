"""CPU: dupdocs_model (the definition of exact document de-duplication) against a naive all-pairs comparison and its
invariants; bpe_dup_docs_resident is declared, exported and bound; every argument error of
Tokenizer.duplicate_docs_resident / unique_docs_resident / duplicate_docs / unique_docs that needs no device is raised
before an engine exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import dupdocs_model
import select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_pairs(ids, off, max_len=None, tail=False):
    """the definition once more, in plain Python: every document against every earlier one"""
    docs = []
    for a, b in zip(off, off[1:]):
        doc = list(ids[a:b])
        if max_len is not None:
            doc = doc[len(doc) - min(len(doc), max_len):] if tail else doc[:max_len]
        docs.append(doc)
    first = [next(e for e in range(d + 1) if docs[e] == docs[d]) for d in range(len(docs))]
    counts = [sum(1 for f in first if f == d) if first[d] == d else 0 for d in range(len(docs))]
    return first, counts


def random_case(seed):
    rng = np.random.default_rng(seed)
    n_docs = int(rng.integers(0, 61))
    lens = rng.integers(0, 7, size=n_docs)
    lens[rng.random(n_docs) < 0.2] = 0                          # empty documents
    lead, trail = (int(x) for x in rng.integers(0, 4, size=2))  # off[0] > 0 and off[-1] < n in most cases
    off = [lead + int(x) for x in np.concatenate([[0], np.cumsum(lens)])]
    alphabet = int(rng.integers(2, 4))                          # 2 - 3 values: duplicates are common
    ids = rng.integers(0, alphabet, size=off[-1] + trail).tolist()
    return ids, off


@pytest.mark.parametrize("seed", range(40))
def test_model_is_the_all_pairs_comparison(seed):
    ids, off = random_case(seed)
    n_docs = len(off) - 1
    for max_len in (None, 1, 2, 3, 6, 50):
        for tail in (False, True):
            if tail and max_len is None:
                continue
            first, counts, n_distinct = dupdocs_model.duplicates(ids, off, max_len, tail)
            want_first, want_counts = all_pairs(ids, off, max_len, tail)
            assert first.tolist() == want_first and counts.tolist() == want_counts, (seed, max_len, tail)
            assert first.dtype == np.int64 and counts.dtype == np.int64
            # the invariants
            arange = np.arange(n_docs)
            assert np.array_equal(first[first], first) and (first <= arange).all()
            assert counts.sum() == n_docs and n_distinct == int((first == arange).sum())
            assert ((counts > 0) == (first == arange)).all()


def test_model_small_cases_by_hand():
    ids = [9, 1, 2, 1, 2, 3, 1, 2, 9]
    off = [1, 3, 5, 5, 6, 8, 8]                       # [1 2] [1 2] [] [3] [1 2] [];  the 9s are strays
    dup = lambda *a, **k: tuple(x.tolist() if hasattr(x, "tolist") else x for x in dupdocs_model.duplicates(ids, off, *a, **k))
    assert dup() == ([0, 0, 2, 3, 0, 2], [3, 0, 2, 1, 0, 0], 3)
    assert dup(max_len=1) == ([0, 0, 2, 3, 0, 2], [3, 0, 2, 1, 0, 0], 3)
    assert dupdocs_model.duplicates([1, 2, 1, 3], [0, 2, 4], max_len=1)[0].tolist() == [0, 0]     # equal heads
    assert dupdocs_model.duplicates([1, 2, 1, 3], [0, 2, 4], max_len=1, tail=True)[0].tolist() == [0, 1]
    assert dupdocs_model.duplicates([1, 2, 3, 2], [0, 2, 4], max_len=1, tail=True)[0].tolist() == [0, 0]  # equal tails
    assert dupdocs_model.duplicates([], [0])[2] == 0 and dupdocs_model.duplicates([], [0, 0, 0])[0].tolist() == [0, 0]
    # a proper prefix is another document; ids are compared at their full width
    assert dupdocs_model.duplicates([1, 2, 1, 2, 3], [0, 2, 5])[0].tolist() == [0, 1]
    assert dupdocs_model.duplicates(np.array([5, 5 + 2**32], np.int64), [0, 1, 2])[0].tolist() == [0, 1]
    assert dupdocs_model.duplicates(np.array([5, 5 + 2**32], np.int64).astype(np.int32), [0, 1, 2])[0].tolist() == [0, 0]
    with pytest.raises(select_model.BadOffsets) as e:
        dupdocs_model.duplicates(ids, [0, 5, 4])
    assert e.value.index == 2 and dupdocs_model.BadOffsets is select_model.BadOffsets


def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+bpe_dup_docs_resident\s*\(", code)
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "bpe_dup_docs_resident")
    assert "bpe_dup_docs_resident" in native.exported_symbols()
    assert len(native._lib.bpe_dup_docs_resident.argtypes) == 12
    assert callable(native.Engine.dup_docs_resident)
    # the definition and the options stand in the header's comments
    for text in ("the lowest e with key(e) == key(d)", "differ only above bit 32", "empty keys are equal to each other",
                 "comparing the ids themselves", '"dup_tile"', '"dup_wave_len"', '"dup_hash_bits"'):
        assert text in hdr, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("dup_tile", "dup_wave_len", "dup_hash_bits", "bpe_dup_docs_resident"):
        assert name in integration, name


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    assert tok.n_distinct_docs is None
    with pytest.raises(AttributeError):
        tok.n_distinct_docs = 3                                               # read-only
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    methods = (tok.duplicate_docs_resident, tok.unique_docs_resident)
    host_methods = (tok.duplicate_docs, tok.unique_docs)
    for kw in (dict(keep="middle"), dict(keep=None), dict(keep="Head"), dict(max_len=0), dict(max_len=-1),
               dict(max_len=2.0), dict(max_len=True), dict(max_len="3")):
        for f in methods:
            with pytest.raises(ValueError):
                f(ids, off, **kw)
        for f in host_methods:
            with pytest.raises(ValueError):
                f(ids.numpy(), off, **kw)
    for f in methods:
        with pytest.raises(ValueError):
            f(ids, [])                                                        # n_docs + 1 entries: at least one
        for bad_off in (torch.tensor([0.0, 10.0]), np.array([0.0, 10.0]), torch.tensor([0, 10], device="meta")):
            with pytest.raises(TypeError):                                    # floats; offsets on another device
                f(ids, bad_off)
        for bad_ids in (ids.tolist(), ids.numpy(), ids.to(torch.int16), ids.to(torch.float32), ids.reshape(2, 5),
                        torch.arange(20, dtype=torch.int32)[::2]):
            with pytest.raises(TypeError):
                f(bad_ids, off)
    for f in host_methods:
        with pytest.raises(TypeError):
            f([0.5, 1.5], off)
        with pytest.raises(TypeError):
            f(ids.numpy(), np.array([0.0, 10.0]))
    with pytest.raises(TypeError):
        tok.unique_docs(ids.numpy(), off, out=np.zeros(10, np.int32))
    # everything else in order: what is left to object to is that the ids are not on a GPU
    for kw in (dict(), dict(max_len=3, keep="tail"), dict(max_len=2**40)):
        for f in methods:
            with pytest.raises(TypeError, match="GPU"):
                f(ids, off, **kw)
            with pytest.raises(TypeError, match="GPU"):
                f(ids.to(torch.int64), torch.tensor(off), **kw)
    with pytest.raises(TypeError, match="GPU"):
        tok.duplicate_docs_resident(ids, off, return_counts=True)
    assert tok.n_distinct_docs is None
