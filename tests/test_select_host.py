"""CPU: select_model (the definition of document selection in NumPy) against a restatement as a list of slices;
its error positions; bpe_select_docs_resident is declared, exported and bound; every argument error of
Tokenizer.select_docs_resident / select_docs that needs no device is raised before an engine exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slices(ids, off, index, max_len=None, tail=False):
    """the definition once more, in plain Python"""
    out, out_off = [], [0]
    for d in index:
        doc = list(ids[off[d]:off[d + 1]])
        if max_len is not None:
            doc = doc[len(doc) - min(len(doc), max_len):] if tail else doc[:max_len]
        out += doc
        out_off.append(len(out))
    return out, out_off


def random_case(seed):
    rng = np.random.default_rng(seed)
    n_docs = int(rng.integers(0, 40))
    lens = rng.integers(0, 30, size=n_docs)
    lens[rng.random(n_docs) < 0.3] = 0                       # empty documents
    lead, trail = (int(x) for x in rng.integers(0, 5, size=2))  # off[0] > 0 and off[-1] < n in most cases
    off = [lead + int(x) for x in np.concatenate([[0], np.cumsum(lens)])]
    n = off[-1] + trail
    ids = rng.integers(-2**31, 2**31, size=n).tolist()
    m = int(rng.integers(0, 3 * n_docs + 1)) if n_docs else 0
    index = rng.integers(0, n_docs, size=m).tolist() if n_docs else []   # repeats, any order, some left out
    return ids, off, index


@pytest.mark.parametrize("seed", range(40))
def test_model_is_the_list_of_slices(seed):
    ids, off, index = random_case(seed)
    longest = max([b - a for a, b in zip(off, off[1:])] + [1])
    for max_len in (None, 1, 2, 7, longest, longest + 5, 2**40):
        for tail in (False, True):
            if tail and max_len is None:
                continue
            out, out_off = select_model.select(ids, off, index, max_len, tail)
            want, want_off = slices(ids, off, index, max_len, tail)
            assert out.tolist() == want and out_off.tolist() == want_off, (seed, max_len, tail)
            assert out_off.dtype == np.int64


def test_model_small_cases_by_hand():
    ids = [10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
    off = [1, 4, 4, 9]                                       # documents [11 12 13], [], [14 .. 18]; 10 and 19 are strays
    sel = lambda *a, **k: tuple(x.tolist() for x in select_model.select(ids, off, *a, **k))
    assert sel([2, 0, 1, 0]) == ([14, 15, 16, 17, 18, 11, 12, 13, 11, 12, 13], [0, 5, 8, 8, 11])
    assert sel([]) == ([], [0])
    assert sel([1, 1]) == ([], [0, 0, 0])
    assert sel([0, 2], max_len=2) == ([11, 12, 14, 15], [0, 2, 4])
    assert sel([0, 2], max_len=2, tail=True) == ([12, 13, 17, 18], [0, 2, 4])
    assert sel([0, 1, 2], max_len=4, tail=True) == ([11, 12, 13, 15, 16, 17, 18], [0, 3, 3, 7])
    assert select_model.select(np.array(ids, np.int32), off, [0])[0].dtype == np.int32


def test_model_error_positions():
    ids = list(range(10))
    for off, bad in (([0, 5, 4, 10], 2), ([0, 5, 11], 2), ([11], 0), ([3, 2, 1], 1), ([0, 4, 12, 3], 2)):
        with pytest.raises(select_model.BadOffsets) as e:
            select_model.select(ids, off, [0])
        assert e.value.index == bad
    off = [0, 3, 10]
    for index, bad in (([0, 1, 2], 2), ([-1, 0], 0), ([0, 1, 1, 2**40, -1], 3), ([5, 7], 0)):
        with pytest.raises(select_model.BadSelection) as e:
            select_model.select(ids, off, index)
        assert e.value.index == bad
    with pytest.raises(select_model.BadOffsets):             # offsets are checked first
        select_model.select(ids, [0, 11], [9])
    assert isinstance(select_model.BadSelection(0), IndexError) and isinstance(select_model.BadOffsets(0), ValueError)


def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+bpe_select_docs_resident\s*\(", code)
    assert re.search(r"#define\s+BPE_SELECT_TAIL\s+1u\b", code)
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "bpe_select_docs_resident")
    assert "bpe_select_docs_resident" in native.exported_symbols()
    assert len(native._lib.bpe_select_docs_resident.argtypes) == 16
    assert callable(native.Engine.select_docs_resident)
    assert native.SELECT_TAIL == 1
    assert issubclass(native.BadSelection, IndexError)
    # the definition stands in the header's comment
    for text in ("len(d) = off[d + 1] - off[d]", "min(len(d), max_len)", "off[d + 1] - l_j with BPE_SELECT_TAIL",
                 "out_offsets[m] is the total"):
        assert text in hdr, text


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    value_errors = [
        dict(keep="middle"), dict(keep=None), dict(keep="Head"),
        dict(max_len=0), dict(max_len=-1), dict(max_len=2.0), dict(max_len=True), dict(max_len="3"),
        dict(index=torch.tensor([True, False, True])), dict(index=torch.tensor([True])),      # masks of the wrong length
        dict(index=np.array([True, False, True])), dict(index=torch.zeros(0, dtype=torch.bool)),
    ]
    for kw in value_errors:
        kw = dict(kw)
        index = kw.pop("index", [1, 0])
        with pytest.raises(ValueError):
            tok.select_docs_resident(ids, off, index, **kw)
        with pytest.raises(ValueError):
            tok.select_docs(ids.numpy(), off, index, **kw)
    with pytest.raises(ValueError):
        tok.select_docs_resident(ids, [], [0])                                 # n_docs + 1 entries: at least one
    type_errors = [
        dict(index=[0.0, 1.0]), dict(index=np.array([0.5])), dict(index=torch.tensor([0.0, 1.0])),   # a float index
        dict(index=[[0, 1], [1, 0]]), dict(index=torch.zeros((2, 2), dtype=torch.int64)),            # a 2-D index
        dict(index=torch.zeros((1, 2), dtype=torch.bool)), dict(index=torch.tensor([0, 1], dtype=torch.int16)),
        dict(index=["a"]),
        dict(doc_offsets=torch.tensor([0.0, 10.0])), dict(doc_offsets=np.array([0.0, 10.0])),
    ]
    for kw in type_errors:
        args = dict(ids=ids, doc_offsets=off, index=[1, 0])
        args.update(kw)
        with pytest.raises(TypeError):
            tok.select_docs_resident(args["ids"], args["doc_offsets"], args["index"])
        with pytest.raises(TypeError):
            tok.select_docs(args["ids"].numpy(), args["doc_offsets"], args["index"])
    for kw in (dict(ids=ids.tolist()), dict(ids=ids.numpy()), dict(ids=ids.to(torch.int16)), dict(ids=ids.to(torch.float32)),
               dict(ids=ids.reshape(2, 5)), dict(ids=torch.arange(20, dtype=torch.int32)[::2]),
               dict(out=np.zeros(10, np.int32)), dict(out=torch.zeros(10, dtype=torch.int64)),
               dict(out=torch.zeros((2, 5), dtype=torch.int32)), dict(out=torch.zeros(20, dtype=torch.int32)[::2])):
        args = dict(ids=ids, out=None)
        args.update(kw)
        with pytest.raises(TypeError):
            tok.select_docs_resident(args["ids"], off, [1, 0], out=args["out"])
    with pytest.raises(TypeError):
        tok.select_docs([0.5, 1.5], off, [0])
    with pytest.raises(TypeError):
        tok.select_docs(ids.numpy(), off, [0], out=np.zeros(10, np.int32))
    # everything else in order: what is left to object to is that the ids are not on a GPU
    for kw in (dict(), dict(max_len=3, keep="tail"), dict(max_len=2**40), dict(out=torch.zeros(10, dtype=torch.int32))):
        for index in ([1, 0, 1], np.array([1], np.int32), torch.tensor([0, 1]), torch.tensor([True, False]), [],
                      np.array([False, True])):
            with pytest.raises(TypeError, match="GPU"):
                tok.select_docs_resident(ids, off, index, **kw)
            with pytest.raises(TypeError, match="GPU"):
                tok.select_docs_resident(ids.to(torch.int64), torch.tensor(off), index, **{**kw, "out": None})
