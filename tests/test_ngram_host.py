"""CPU: ngram_model (the definition of n-gram overlap with a reference set) against a second, all-pairs
statement of it on random small streams; the rules of the definition by hand; its invariants; the two calls are declared,
exported, bound and documented; every argument error of Tokenizer.ngram_index_resident / ngram_index /
ngram_overlap_resident / ngram_overlap / decontaminate_docs_resident that needs no device is raised before an engine
exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import ngram_model
import select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the definition once more: every window of every key against every window of every reference document, no dict

def all_pairs(ref, roff, w, ids, off, max_len=None, tail=False):
    ref, ids = [int(x) for x in ref], [int(x) for x in ids]
    roff, off = [int(x) for x in roff], [int(x) for x in off]
    ref_windows = [i for r in range(len(roff) - 1) for i in range(roff[r], roff[r + 1]) if i + w <= roff[r + 1]]
    n_docs = len(off) - 1
    hits, first, ref_pos = [0] * n_docs, [-1] * n_docs, [-1] * n_docs
    starts = [0] * len(ids)
    for d in range(n_docs):
        m_ids, m_off = select_model.select(np.asarray(ids, np.int64), off, [d], max_len, tail)  # the slice selection emits
        key = [int(x) for x in m_ids]
        assert int(m_off[1]) == len(key)
        s = off[d + 1] - len(key) if tail else off[d]
        assert ids[s:s + len(key)] == key
        for k in range(len(key)):
            if k + w > len(key):
                continue
            equal = [i for i in ref_windows if all(ref[i + t] == key[k + t] for t in range(w))]
            if equal:
                if hits[d] == 0:
                    first[d], ref_pos[d] = (s - off[d]) + k, min(equal)
                hits[d] += 1
                starts[s + k] = 1
    distinct = {tuple(ref[i:i + w]) for i in ref_windows}
    return hits, first, ref_pos, starts, sum(h > 0 for h in hits), len(ref_windows), len(distinct)


def random_case(rng):
    w = int(rng.integers(1, 5))
    vocab = int(rng.integers(2, 5))                                        # few values: windows repeat and hit often
    ref_docs = [rng.integers(0, vocab, size=int(rng.integers(0, 9))) for _ in range(int(rng.integers(0, 5)))]
    docs = [rng.integers(0, vocab, size=int(rng.integers(0, 12))) for _ in range(int(rng.integers(0, 7)))]
    ref, roff = ngram_model.stream(ref_docs)
    ids, off = ngram_model.stream(docs)
    lead, trail = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    ref = np.concatenate([rng.integers(0, vocab, size=lead), ref, rng.integers(0, vocab, size=trail)])
    ids = np.concatenate([rng.integers(0, vocab, size=trail), ids, rng.integers(0, vocab, size=lead)])
    return ref, roff + lead, w, ids, off + trail


def test_model_against_all_pairs():
    rng = np.random.default_rng(1)
    some_hit = 0
    for _ in range(300):
        ref, roff, w, ids, off = random_case(rng)
        for max_len, tail in ((None, False), (3, False), (3, True), (1, True)):
            got = ngram_model.run(ref, roff, w, ids, off, max_len, tail)
            want = all_pairs(ref, roff, w, ids, off, max_len, tail)
            for g, x in zip(got, want):
                assert np.array_equal(np.asarray(g), np.asarray(x)), (ref, roff, w, ids, off, max_len, tail)
            some_hit += got[4] > 0
    assert some_hit > 100


# ---------------------------------------------------------------------------
# the rules by hand

def test_a_short_key_has_no_window_and_is_not_shortened():
    ref, roff = [1, 2, 3], [0, 3]
    hits, first, ref_pos, starts, n_hit, n_windows, n_distinct = ngram_model.run(ref, roff, 3, [1, 2, 1, 2, 3], [0, 2, 5])
    assert hits.tolist() == [0, 1] and first.tolist() == [-1, 0] and ref_pos.tolist() == [-1, 0]
    assert (n_hit, n_windows, n_distinct) == (1, 1, 1) and starts.tolist() == [0, 0, 1, 0, 0]
    # a reference document shorter than the window contributes nothing; an empty index hits nothing
    assert ngram_model.run([1, 2], [0, 2], 3, [1, 2, 3], [0, 3])[4:] == (0, 0, 0)
    assert ngram_model.run([], [0], 1, [1, 2, 3], [0, 3])[0].tolist() == [0]
    assert ngram_model.run([5], [0, 0, 1], 1, [], [0, 0])[0].tolist() == [0]


def test_windows_stop_at_document_ends_on_both_sides():
    # 2 3 straddles two corpus documents: no hit; 7 8 straddles two reference documents: no reference window
    ref, roff = [2, 3, 7, 8], [0, 3, 4]
    hits, first, ref_pos, starts, *_ = ngram_model.run(ref, roff, 2, [1, 2, 3, 4, 7, 8, 3, 7], [0, 2, 4, 6, 8])
    assert hits.tolist() == [0, 0, 0, 1] and first.tolist() == [-1, -1, -1, 0] and ref_pos.tolist() == [-1, -1, -1, 1]
    assert starts.tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    # ids in front of roff[0], behind roff[n], in front of off[0] and behind off[n] count for nothing
    hits, _, _, starts, _, n_windows, _ = ngram_model.run([9, 1, 2, 9], [1, 3], 1, [1, 9, 2, 9, 1], [1, 4])
    assert hits.tolist() == [1] and starts.tolist() == [0, 0, 1, 0, 0] and n_windows == 2


def test_max_len_and_tail_are_the_selection_slice_and_first_is_document_relative():
    ref, roff = [5, 6], [0, 2]
    ids, off = [0, 5, 6, 0, 0, 0, 5, 6], [0, 8]
    assert [x.tolist() for x in ngram_model.run(ref, roff, 2, ids, off)[:3]] == [[2], [1], [0]]
    assert [x.tolist() for x in ngram_model.run(ref, roff, 2, ids, off, 3)[:3]] == [[1], [1], [0]]          # a hit just inside
    assert [x.tolist() for x in ngram_model.run(ref, roff, 2, ids, off, 2)[:3]] == [[0], [-1], [-1]]        # ... just outside
    assert [x.tolist() for x in ngram_model.run(ref, roff, 2, ids, off, 2, True)[:3]] == [[1], [6], [0]]    # first: in the uncut document
    assert [x.tolist() for x in ngram_model.run(ref, roff, 2, ids, off, 1, True)[:3]] == [[0], [-1], [-1]]
    assert ngram_model.run(ref, roff, 2, ids, off, 7, True)[3].tolist() == [0, 1, 0, 0, 0, 0, 1, 0]
    assert ngram_model.run(ref, roff, 2, ids, off, 6, True)[3].tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    # a document that does not start the stream: first is relative to off[d], starts to the stream
    hits, first, ref_pos, starts, *_ = ngram_model.run(ref, roff, 2, [5, 6, 9, 5, 6], [2, 5])
    assert (hits.tolist(), first.tolist(), ref_pos.tolist(), starts.tolist()) == ([1], [1], [0], [0, 0, 0, 1, 0])


def test_ref_pos_is_the_lowest_repeat_and_every_start_counts():
    ref, roff = [4, 1, 2, 1, 2, 1, 2], [0, 3, 7]
    hits, first, ref_pos, starts, n_hit, n_windows, n_distinct = ngram_model.run(ref, roff, 2, [1, 2, 1, 2, 1], [0, 5])
    assert (n_windows, n_distinct) == (5, 3)                                # 41 12 | 12 21 12
    assert hits.tolist() == [4] and first.tolist() == [0] and ref_pos.tolist() == [1]
    assert starts.tolist() == [1, 1, 1, 1, 0] and n_hit == 1


def test_equality_is_by_value_at_the_full_width():
    ref32 = np.array([-1, 7, 2**31 - 1], np.int32)
    for ids in (ref32, ref32.astype(np.int64)):
        for ref in (ref32, ref32.astype(np.int64)):
            assert ngram_model.run(ref, [0, 3], 3, ids, [0, 3])[0].tolist() == [1]
    wide = ref32.astype(np.int64)
    wide[1] += 1 << 32                                                      # differs only above bit 32
    assert ngram_model.run(ref32, [0, 3], 3, wide, [0, 3])[0].tolist() == [0]
    assert ngram_model.run(wide, [0, 3], 3, wide, [0, 3])[0].tolist() == [1]
    assert ngram_model.run(np.array([2**32 - 1], np.int64), [0, 1], 1, np.array([-1], np.int32), [0, 1])[0].tolist() == [0]
    with pytest.raises(select_model.BadOffsets):
        ngram_model.run(ref32, [0, 4], 1, ref32, [0, 3])
    with pytest.raises(select_model.BadOffsets):
        ngram_model.run(ref32, [0, 3], 1, ref32, [2, 1])


def test_invariants():
    rng = np.random.default_rng(2)
    for _ in range(200):
        ref, roff, w, ids, off = random_case(rng)
        for max_len, tail in ((None, False), (4, False), (4, True)):
            hits, first, ref_pos, starts, n_hit, n_windows, n_distinct = ngram_model.run(ref, roff, w, ids, off, max_len, tail)
            L = np.diff(off)
            l = L if max_len is None else np.minimum(L, max_len)
            assert (hits <= np.maximum(l - w + 1, 0)).all() and (hits >= 0).all()
            assert np.array_equal(first == -1, hits == 0) and np.array_equal(ref_pos == -1, hits == 0)
            assert ((first < L) | (hits == 0)).all() and (ref_pos < len(ref)).all()
            assert [int(starts[a:b].sum()) for a, b in zip(off, off[1:])] == hits.tolist()
            assert int(starts.sum()) == int(hits.sum()) and n_hit == int((hits > 0).sum())
            assert n_distinct <= n_windows == int(np.maximum(np.diff(roff) - w + 1, 0).sum())
            for d in np.flatnonzero(hits):
                p = int(off[d] + first[d])
                assert starts[p] == 1 and list(ids[p:p + w]) == list(ref[ref_pos[d]:ref_pos[d] + w])


# ---------------------------------------------------------------------------
# declared, exported, bound, documented

def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, nargs in (("bpe_ngram_index_resident", 11), ("bpe_ngram_overlap_resident", 15)):
        assert re.search(rf"\bint\s+{name}\s*\(", code)
        assert hasattr(lib, name) and name in native.exported_symbols()
        assert len(getattr(native._lib, name).argtypes) == nargs
    assert callable(native.Engine.ngram_index_resident) and callable(native.Engine.ngram_overlap_resident)
    for text in ("DESIGN 4.11", "tests/ngram_model.py", "does not depend on scheduling", '"ng_tile"', '"ng_hash_bits"',
                 "BPE_E_STATE", "WITHOUT an index"):
        assert text in hdr, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("ng_tile", "ng_hash_bits", "bpe_ngram_index_resident", "bpe_ngram_overlap_resident"):
        assert name in integration, name
    for doc, texts in (("DESIGN.md", ("4.11", "ng_tile", "one index")), ("README.md", ("ngram_overlap_resident", "test_gpu_ngram.py")),
                       (os.path.join("profiles", "README.md"), ("ngram_notes.md",))):
        body = open(os.path.join(ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)
    import minbpe_amd
    from minbpe_amd.tokenizer import NgramIndex, Tokenizer
    assert minbpe_amd.NgramIndex is NgramIndex and "NgramIndex" in minbpe_amd._EXPORTS
    for method in ("ngram_index_resident", "ngram_index", "ngram_overlap_resident", "ngram_overlap", "decontaminate_docs_resident"):
        assert callable(getattr(Tokenizer, method))
    # the two options have a row each, and the fields they set carry the defaults the header states
    options = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_options.hip")).read()
    assert 'OPT_NAMED("ng_tile", ng_tile, OPT_POW2, 64, NG_TILE_MAX, 1)' in options and "OPT(ng_hash_bits, 0, 64)" in options
    ctx = open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")).read()
    tile = int(re.search(r"int ng_tile = (\d+);", ctx).group(1))
    assert f'"ng_tile" ({tile}:' in hdr and "int ng_hash_bits = 64;" in ctx


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    cpu = torch.device("cpu")
    index = T.NgramIndex(3, 8, 8, cpu, 1)                                    # (made by hand: no engine holds it)
    assert (index.ngram, index.n_windows, index.n_distinct, index.device, index.id) == (3, 8, 8, cpu, 1)
    assert "ngram=3" in repr(index)
    assert tok.n_overlapping_docs is None
    # the window
    for bad in (0, 65, -1, 2.0, True, "13", None):
        with pytest.raises(ValueError):
            tok.ngram_index_resident(ids, ngram=bad)
        with pytest.raises(ValueError):
            tok.ngram_index(ids.numpy(), ngram=bad)
        with pytest.raises(ValueError):
            tok.ngram_overlap(ids.numpy(), ids.numpy(), off, ngram=bad)
    # max_len, keep, min_hits
    for kw in (dict(keep="middle"), dict(max_len=0), dict(max_len=2.0), dict(max_len=True)):
        with pytest.raises(ValueError):
            tok.ngram_overlap_resident(index, ids, off, **kw)
        with pytest.raises(ValueError):
            tok.ngram_overlap(index, ids.numpy(), off, **kw)
        with pytest.raises(ValueError):
            tok.ngram_overlap(ids.numpy(), ids.numpy(), off, **kw)
        with pytest.raises(ValueError):
            tok.decontaminate_docs_resident(index, ids, off, **kw)
    for bad in (0, -1, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            tok.decontaminate_docs_resident(index, ids, off, min_hits=bad)
    # the index: its type, its device
    for bad in (None, 1, ids, (3, 8, 8)):
        with pytest.raises(TypeError):
            tok.ngram_overlap_resident(bad, ids, off)
        with pytest.raises(TypeError):
            tok.decontaminate_docs_resident(bad, ids, off)
    elsewhere = T.NgramIndex(3, 8, 8, torch.device("cuda", 1), 1)
    for call in (tok.ngram_overlap_resident, tok.decontaminate_docs_resident):
        with pytest.raises(ValueError, match="cuda:1"):
            call(elsewhere, ids, off)
    with pytest.raises(ValueError, match="cuda:1"):
        tok.ngram_overlap(elsewhere, ids.numpy(), off, device=0)
    # ids and offsets: dtype, contiguity, dimensions, where they live
    for f in (lambda i, o: tok.ngram_overlap_resident(index, i, o), lambda i, o: tok.decontaminate_docs_resident(index, i, o),
              lambda i, o: tok.ngram_index_resident(i, o)):
        with pytest.raises(ValueError):
            f(ids, [])                                                       # n_docs + 1 entries: at least one
        for bad_off in (torch.tensor([0.0, 10.0]), np.array([0.0, 10.0]), torch.tensor([0, 10], device="meta")):
            with pytest.raises(TypeError):
                f(ids, bad_off)
        for bad_ids in (ids.tolist(), ids.numpy(), ids.to(torch.int16), ids.to(torch.float32), ids.reshape(2, 5),
                        torch.arange(20, dtype=torch.int32)[::2]):
            with pytest.raises(TypeError):
                f(bad_ids, off)
    for f in (lambda i, o: tok.ngram_overlap(index, i, o), lambda i, o: tok.ngram_overlap(ids.numpy(), i, o),
              lambda i, o: tok.ngram_index(i, o), lambda i, o: tok.ngram_overlap(i, ids.numpy(), off, ref_doc_offsets=o)):
        with pytest.raises(TypeError):
            f([0.5, 1.5], off)
        with pytest.raises(TypeError):
            f(ids.numpy(), np.array([0.0, 10.0]))
    # out of decontaminate_docs_resident: dtype, device, contiguity
    for bad_out in (torch.zeros(10, dtype=torch.int64), np.zeros(10, np.int32), torch.zeros(20, dtype=torch.int32)[::2],
                    torch.zeros(10, dtype=torch.int32, device="meta"), torch.zeros((2, 5), dtype=torch.int32)):
        with pytest.raises(TypeError):
            tok.decontaminate_docs_resident(index, ids, off, out=bad_out)
    # everything else in order: what is left to object to is that the ids are not on a GPU
    with pytest.raises(TypeError, match="GPU"):
        tok.ngram_index_resident(ids)
    with pytest.raises(TypeError, match="GPU"):
        tok.ngram_index_resident(ids.to(torch.int64), torch.tensor(off), ngram=64)
    with pytest.raises(TypeError, match="GPU"):
        tok.ngram_overlap_resident(index, ids, off)
    with pytest.raises(TypeError, match="GPU"):
        tok.ngram_overlap_resident(index, ids.to(torch.int64), torch.tensor(off), max_len=3, keep="tail", return_first=True,
                                   return_starts=True)
    with pytest.raises(TypeError, match="GPU"):
        tok.decontaminate_docs_resident(index, ids, off, min_hits=2, max_len=5, out=torch.zeros(10, dtype=torch.int32))
    assert tok.n_overlapping_docs is None
