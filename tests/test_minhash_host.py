"""CPU: minhash_model (the definition of MinHash signatures and near-duplicate groups) against a second,
independent statement of it in Python integers and sets; the conditions the definition was chosen by -- the Jaccard
estimate, the recovery of planted families; the invariants of the groups; the two calls are declared, exported and bound;
every argument error of Tokenizer.minhash_resident / minhash / minhash_agreement_resident / near_duplicate_docs_resident /
near_duplicate_docs that needs no device is raised before an engine exists."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import dupdocs_model
import minhash_model
import select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


# ---------------------------------------------------------------------------
# the definition once more: Python integers, one shingle at a time

def py_fmix32(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ (h >> 16)


def py_tok(x):
    x = int(x) & M64                                            # two's complement of the value: the sign extension
    return py_fmix32((x & M32) ^ ((x >> 32) * 0x9E3779B1 & M32))


def py_shingle_set(key, w, seed):
    key = [int(x) for x in key]
    if not key:
        return set()
    ww = min(w, len(key))
    out = set()
    for i in range(len(key) - ww + 1):
        s = 0
        for x in key[i:i + ww]:
            s = (s * 0x01000193 + py_tok(x)) & M32
        out.add(py_fmix32(s ^ ((seed ^ ww) & M32)))
    return out


def py_params(seed, P):
    state = [seed & M64]

    def nxt():
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & M64
        r = state[0]
        r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9 & M64
        r = (r ^ (r >> 27)) * 0x94D049BB133111EB & M64
        return r ^ (r >> 31)

    ab = []
    for _ in range(P):
        a = nxt() | 1
        ab.append((a, nxt()))
    return ab


def py_signatures(ids, off, n_perm, ngram, seed, max_len=None, tail=False):
    ab = py_params(seed, n_perm)
    rows = []
    for o0, o1 in zip(off, off[1:]):
        doc = list(ids[o0:o1])
        if max_len is not None:
            doc = doc[len(doc) - min(len(doc), max_len):] if tail else doc[:max_len]
        S = py_shingle_set(doc, ngram, seed)
        rows.append([min(((a * s + b) & M64) >> 33 for s in S) if S else 0x7FFFFFFF for a, b in ab])
    return rows


def random_case(seed):
    rng = np.random.default_rng(seed)
    n_docs = int(rng.integers(0, 25))
    lens = rng.integers(0, 14, size=n_docs)
    lens[rng.random(n_docs) < 0.2] = 0
    lead, trail = (int(x) for x in rng.integers(0, 4, size=2))
    off = [lead + int(x) for x in np.concatenate([[0], np.cumsum(lens)])]
    if seed % 2:
        ids = rng.integers(-2**63, 2**63, size=off[-1] + trail, dtype=np.int64)
    else:
        ids = rng.integers(-2**31, 2**31, size=off[-1] + trail, dtype=np.int64).astype(np.int32)
    return ids, off


@pytest.mark.parametrize("seed", range(12))
def test_model_is_the_definition(seed):
    ids, off = random_case(seed)
    for n_perm, ngram, hseed in ((1, 1, 0), (7, 5, 1), (65, 3, 2**64 - 1), (16, 64, 12345 + 2**40)):
        for max_len, tail in ((None, False), (4, False), (4, True), (1, True), (50, True)):
            got = minhash_model.signatures(ids, off, n_perm, ngram, hseed, max_len, tail)
            assert got.dtype == np.int32 and got.shape == (len(off) - 1, n_perm) and (got >= 0).all()
            assert got.tolist() == py_signatures(ids.tolist(), off, n_perm, ngram, hseed, max_len, tail), (seed, n_perm, ngram)


def test_params_and_hashes_by_hand():
    A, B = minhash_model.params(0, 2)
    # splitmix64 from state 0: its first outputs are public test vectors
    assert [int(A[0]), int(B[0]), int(A[1])] == [0xE220A8397B1DCDAF | 1, 0x6E789E6AA1B965F4, 0x06C45D188009454F | 1]
    assert (A & np.uint64(1)).all()
    assert int(minhash_model.fmix32(0)) == 0 and int(minhash_model.fmix32(1)) == py_fmix32(1) == 0x514E28B7
    assert [(int(a), int(b)) for a, b in zip(*minhash_model.params(2**64 - 1, 5))] == py_params(2**64 - 1, 5)


def test_tok_takes_the_id_at_its_full_width():
    v = np.array([0, 1, -1, 2**31 - 1, -2**31, 77, -5], dtype=np.int64)
    assert np.array_equal(minhash_model.tok(v.astype(np.int32)), minhash_model.tok(v))
    off = [0, 3, 7]
    assert np.array_equal(minhash_model.signatures(v.astype(np.int32), off, 32, 2, 3), minhash_model.signatures(v, off, 32, 2, 3))
    # ids that differ only above bit 32 do not hash alike: int64 -1 and 2^32 - 1; the sign bit alone
    assert int(minhash_model.tok(np.array([-1], np.int64))[0]) != int(minhash_model.tok(np.array([2**32 - 1], np.int64))[0])
    a = np.array([5, 6, 7, 8], np.int64)
    for delta in (1 << 32, -2**63):
        b = a.copy()
        b[2] += np.int64(delta)
        assert np.array_equal(a.astype(np.int32), b.astype(np.int32))
        sa, sb = minhash_model.signatures(a, [0, 4], 64, 2), minhash_model.signatures(b, [0, 4], 64, 2)
        assert (sa != sb).any()


def test_short_and_empty_keys():
    ids = np.array([11, 12, 13, 14, 15, 16, 17], np.int32)
    sig = minhash_model.signatures(ids, [0, 3, 3, 7], 16, 5, 9)
    assert (sig[1] == 0x7FFFFFFF).all()                          # an empty key
    # a key shorter than the window is one shingle, all of it: the signature of the same key under the window of its length
    assert len(minhash_model.shingles(ids[:3], 5, 9)) == 1 and len(minhash_model.shingles(ids[3:], 5, 9)) == 1
    assert len(minhash_model.shingles(ids, 5, 9)) == 3
    assert np.array_equal(sig[0], minhash_model.signatures(ids[:3], [0, 3], 16, 3, 9)[0])
    # ... and no other: the length of the window is part of the shingle
    assert int(minhash_model.shingles(ids[:3], 5, 9)[0]) != int(minhash_model.shingles(ids[:3], 3, 8)[0])
    assert len(minhash_model.signatures([], [0], 4)) == 0


def test_max_len_is_the_selection_slice():
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1000, size=90).astype(np.int32)
    off = np.array([2, 2, 10, 30, 31, 85])
    for max_len, tail in ((1, False), (6, False), (6, True), (20, True), (1000, True)):
        cut, cut_off = select_model.select(ids, off, np.arange(5), max_len, tail)
        assert np.array_equal(minhash_model.signatures(ids, off, 32, 5, 4, max_len, tail),
                              minhash_model.signatures(cut, cut_off, 32, 5, 4))


# ---------------------------------------------------------------------------
# the conditions

def test_estimate_condition():
    """18 pairs of 400-id documents, w = 5, P = 256: |estimate - J| <= 0.10 (about three standard errors of the estimate
    at J = 0.5: 3 sqrt(0.25 / 256) = 0.094; every seed is fixed)"""
    cases = minhash_model.estimate_cases()
    assert len(cases) == 18
    worst = 0.0
    for a, b, seed in cases:
        ids, off = minhash_model.stream([a, b])
        sig = minhash_model.signatures(ids, off, 256, 5, seed)
        est = float((sig[0] == sig[1]).mean())
        sa, sb = py_shingle_set(a, 5, seed), py_shingle_set(b, 5, seed)
        J = len(sa & sb) / len(sa | sb)
        worst = max(worst, abs(est - J))
        assert abs(est - J) <= 0.10, (seed, J, est)
    print("largest |estimate - J|:", worst)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_family_condition(seed):
    docs, family = minhash_model.family_corpus()
    assert len(docs) == 107 and len(set(family.tolist())) == 40 and all(60 <= len(d) <= 300 for d in docs)
    ids, off = minhash_model.stream(docs)
    first = minhash_model.groups(ids, off, threshold=0.7, n_perm=128, bands=32, ngram=5, seed=seed)
    assert np.array_equal(first, family)


def test_shingle_collisions_at_the_birthday_rate():
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 2**31, size=200_004).astype(np.int32)
    S = minhash_model.shingles(ids, 5, 0)
    assert len(S) == 200_000
    expected = 200_000 ** 2 / 2 / 2**32                          # 4.7 colliding pairs
    assert 200_000 - len(np.unique(S)) <= 4 * expected + 5


@pytest.mark.parametrize("seed", range(6))
def test_group_invariants(seed):
    rng = np.random.default_rng(100 + seed)
    base = [rng.integers(0, 4, size=int(rng.integers(0, 12))).astype(np.int32) for _ in range(12)]
    docs = [base[i] for i in rng.integers(0, len(base), size=40)]          # exact copies, empty documents among them
    for i in range(0, 40, 7):
        d = docs[i].copy()
        if len(d):
            d[0] += 1
        docs[i] = d
    ids, off = minhash_model.stream(docs)
    for threshold, bands in ((0.5, 8), (1.0, 4), (0.8, 32)):
        first = minhash_model.groups(ids, off, threshold=threshold, n_perm=32, bands=bands, ngram=3, seed=seed)
        assert first.dtype == np.int64 and (first <= np.arange(40)).all() and np.array_equal(first[first], first)
        exact = dupdocs_model.duplicates(ids, off)[0]
        assert np.array_equal(first[exact], first), "an exact copy is outside its original's group"


def test_need_is_the_ceiling():
    assert minhash_model.need_of(0.7, 128) == math.ceil(0.7 * 128) == 90 and minhash_model.need_of(1.0, 128) == 128
    assert minhash_model.need_of(0.5, 128) == 64


# ---------------------------------------------------------------------------
# declared, exported, bound, documented

def test_declared_exported_bound(native):
    hdr = open(os.path.join(ROOT, "include", "bpe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, nargs in (("bpe_minhash_resident", 14), ("bpe_minhash_agree_resident", 9)):
        assert re.search(rf"\bint\s+{name}\s*\(", code)
        assert hasattr(lib, name) and name in native.exported_symbols()
        assert len(getattr(native._lib, name).argtypes) == nargs
    assert callable(native.Engine.minhash_resident) and callable(native.Engine.minhash_agree_resident)
    for text in ("DESIGN 4.10", "0x7FFFFFFF for every p", "does not depend on scheduling", '"mh_tile"'):
        assert text in hdr, text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mh_tile", "bpe_minhash_resident", "bpe_minhash_agree_resident"):
        assert name in integration, name


def test_argument_errors_need_no_engine(native, monkeypatch):
    torch = pytest.importorskip("torch")
    import minbpe_amd.tokenizer as T

    def no_engine(*a, **k):
        pytest.fail("engine() was called before the arguments were checked")

    monkeypatch.setattr(T, "engine", no_engine)
    tok = T.BasicTokenizer()
    ids = torch.arange(10, dtype=torch.int32)
    off = [0, 4, 10]
    resident = (tok.minhash_resident, tok.near_duplicate_docs_resident)
    host = (tok.minhash, tok.near_duplicate_docs)
    bad_values = [dict(keep="middle"), dict(max_len=0), dict(max_len=2.0), dict(max_len=True),
                  dict(n_perm=0), dict(n_perm=1025), dict(n_perm=64.0), dict(n_perm=True), dict(n_perm="128"),
                  dict(ngram=0), dict(ngram=65), dict(ngram=2.5), dict(seed=-1), dict(seed=2**64), dict(seed=1.5)]
    for kw in bad_values:
        for f in resident:
            with pytest.raises(ValueError):
                f(ids, off, **kw)
        for f in host:
            with pytest.raises(ValueError):
                f(ids.numpy(), off, **kw)
    for kw in (dict(bands=0), dict(bands=-4), dict(bands=3), dict(bands=256), dict(bands=2.0), dict(n_perm=100, bands=32),
               dict(threshold=0), dict(threshold=0.0), dict(threshold=-0.5), dict(threshold=1.01), dict(threshold="0.8"),
               dict(threshold=None), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            tok.near_duplicate_docs_resident(ids, off, **kw)
        with pytest.raises(ValueError):
            tok.near_duplicate_docs(ids.numpy(), off, **kw)
    for f in resident:
        with pytest.raises(ValueError):
            f(ids, [])                                                        # n_docs + 1 entries: at least one
        for bad_off in (torch.tensor([0.0, 10.0]), np.array([0.0, 10.0]), torch.tensor([0, 10], device="meta")):
            with pytest.raises(TypeError):
                f(ids, bad_off)
        for bad_ids in (ids.tolist(), ids.numpy(), ids.to(torch.int16), ids.to(torch.float32), ids.reshape(2, 5),
                        torch.arange(20, dtype=torch.int32)[::2]):
            with pytest.raises(TypeError):
                f(bad_ids, off)
    for f in host:
        with pytest.raises(TypeError):
            f([0.5, 1.5], off)
        with pytest.raises(TypeError):
            f(ids.numpy(), np.array([0.0, 10.0]))
    with pytest.raises(TypeError):
        tok.minhash(ids.numpy(), off, out=np.zeros(256, np.int32))
    # out: dtype, device, contiguity, size
    for bad_out in (torch.zeros(2 * 128, dtype=torch.int64), np.zeros(256, np.int32), torch.zeros(512, dtype=torch.int32)[::2],
                    torch.zeros(256, dtype=torch.int32, device="meta")):
        with pytest.raises(TypeError):
            tok.minhash_resident(ids, off, out=bad_out)
    for bad_out in (torch.zeros(2 * 128 - 1, dtype=torch.int32), torch.zeros((1, 128), dtype=torch.int32)):
        with pytest.raises(ValueError):
            tok.minhash_resident(ids, off, out=bad_out)
    # the signatures of the banding must stay below 2^32 words
    with pytest.raises(ValueError, match="2\\^32"):
        tok.near_duplicate_docs_resident(ids, torch.zeros(2**22 + 1, dtype=torch.int32), n_perm=1024)
    # agreement: a matrix, equally many a and b
    sig = torch.zeros((3, 8), dtype=torch.int32)
    for bad_sig in (sig.to(torch.int64), sig.reshape(-1), sig[:, ::2], sig.numpy()):
        with pytest.raises(TypeError):
            tok.minhash_agreement_resident(bad_sig, [0], [1])
    with pytest.raises(ValueError):
        tok.minhash_agreement_resident(sig, [0, 1], [1])
    with pytest.raises(TypeError):
        tok.minhash_agreement_resident(sig, [0.5], [1])
    with pytest.raises(TypeError):
        tok.minhash_agreement_resident(sig, torch.tensor([True, False, True]), [1, 2])
    # everything else in order: what is left to object to is that the ids are not on a GPU
    for f in resident:
        with pytest.raises(TypeError, match="GPU"):
            f(ids, off)
        with pytest.raises(TypeError, match="GPU"):
            f(ids.to(torch.int64), torch.tensor(off), max_len=3, keep="tail", n_perm=64, ngram=1, seed=2**64 - 1)
    with pytest.raises(TypeError, match="GPU"):
        tok.minhash_resident(ids, off, out=torch.zeros(256, dtype=torch.int32))
    with pytest.raises(TypeError, match="GPU"):
        tok.near_duplicate_docs_resident(ids, off, threshold=1, bands=128, return_signatures=True)
    with pytest.raises(TypeError, match="GPU"):
        tok.minhash_agreement_resident(sig, [0, 2], [1, 1])
    assert tok.n_distinct_docs is None
