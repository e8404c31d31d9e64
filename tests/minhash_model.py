"""The definition of MinHash signatures and near-duplicate groups in NumPy, uint64 arithmetic: the model
every minhash test compares with, element for element.  Not a test module.

    fmix32(h)   h ^= h >> 16; h = h * 0x85EBCA6B & M32; h ^= h >> 13; h = h * 0xC2B2AE35 & M32; h ^= h >> 16
    tok(x)      x sign-extended to 64 bits; lo = x & M32, hi = x >> 32; tok = fmix32(lo ^ (hi * 0x9E3779B1 & M32))
    key(d)      the slice select_model emits for document d (max_len, tail), length l
    shingles    l == 0: none.  ww = min(w, l); m = l - ww + 1; s = 0; s = (s * 0x01000193 + tok(key[i + k])) & M32 for k in
                [0, ww); S_i = fmix32(s ^ ((seed ^ ww) & M32))
    params      z = seed; A_p = next() | 1, B_p = next(), next() = splitmix64
    sig[d][p]   min_i ((A_p * S_i + B_p) mod 2^64) >> 33; no shingle: 0x7FFFFFFF
    groups      per band b the first document with the same band; an edge to it if the whole rows agree at
                need = ceil(threshold * P) positions or more; first[d] = the lowest document of d's component
"""
import math

import numpy as np

import select_model

M32 = np.uint64(0xFFFFFFFF)
EMPTY = 0x7FFFFFFF
U = np.uint64


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h = h ^ (h >> U(16))
    h = (h * U(0x85EBCA6B)) & M32
    h = h ^ (h >> U(13))
    h = (h * U(0xC2B2AE35)) & M32
    return h ^ (h >> U(16))


def tok(ids):
    """uint64 array of 32-bit token hashes; the ids at their own width, sign-extended"""
    x = np.asarray(ids)
    if x.dtype.kind not in "iu":
        x = x.astype(np.int64)
    x = x.astype(np.int64).view(np.uint64)                      # (an unsigned dtype never comes from the library's callers)
    lo, hi = x & M32, x >> U(32)
    return fmix32(lo ^ ((hi * U(0x9E3779B1)) & M32))


def shingles(key, w, seed):
    """uint64 array of the key's 32-bit shingle hashes"""
    l = len(key)
    if l == 0:
        return np.zeros(0, np.uint64)
    ww = min(int(w), l)
    m = l - ww + 1
    t = tok(key)
    s = np.zeros(m, np.uint64)
    for k in range(ww):
        s = (s * U(0x01000193) + t[k:k + m]) & M32
    return fmix32(s ^ U((int(seed) ^ ww) & 0xFFFFFFFF))


def params(seed, P):
    """(A, B): uint64 [P] each"""
    mask = (1 << 64) - 1
    z = int(seed) & mask
    out = []
    for _ in range(2 * P):
        z = (z + 0x9E3779B97F4A7C15) & mask
        r = z
        r = ((r ^ (r >> 30)) * 0xBF58476D1CE4E5B9) & mask
        r = ((r ^ (r >> 27)) * 0x94D049BB133111EB) & mask
        out.append(r ^ (r >> 31))
    A = np.array([x | 1 for x in out[0::2]], dtype=np.uint64)
    B = np.array(out[1::2], dtype=np.uint64)
    return A, B


def keys(ids, off, max_len=None, tail=False):
    """the documents' keys as arrays in the dtype of ids; BadOffsets as select_model raises it"""
    ids = np.asarray(ids)
    if ids.dtype.kind not in "iu":
        ids = ids.astype(np.int64)
    n_docs = len(off) - 1
    out, ooff = select_model.select(ids, off, np.arange(n_docs), max_len, tail)
    return [out[ooff[d]:ooff[d + 1]] for d in range(n_docs)]


def signatures(ids, off, n_perm=128, ngram=5, seed=0, max_len=None, tail=False):
    """int32 [n_docs, n_perm]"""
    A, B = params(seed, n_perm)
    ks = keys(ids, off, max_len, tail)
    sig = np.full((len(ks), n_perm), EMPTY, dtype=np.int32)
    with np.errstate(over="ignore"):
        for d, key in enumerate(ks):
            S = shingles(key, ngram, seed)
            if len(S):
                h = (A[None, :] * S[:, None] + B[None, :]) >> U(33)   # uint64 wraps: mod 2^64
                sig[d] = h.min(axis=0).astype(np.int32)
    return sig


def need_of(threshold, n_perm):
    return int(math.ceil(float(threshold) * n_perm))


def groups_of_signatures(sig, threshold=0.8, bands=32):
    """first int64 [n_docs] from a signature matrix, by a union-find"""
    n_docs, P = sig.shape
    assert P % bands == 0
    r = P // bands
    need = need_of(threshold, P)
    parent = list(range(n_docs))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for b in range(bands):
        seen = {}
        for d in range(n_docs):
            e = seen.setdefault(sig[d, b * r:(b + 1) * r].tobytes(), d)
            if e != d and int((sig[d] == sig[e]).sum()) >= need:
                x, y = find(d), find(e)
                if x != y:
                    parent[max(x, y)] = min(x, y)               # the root is the component's lowest document
    return np.array([find(d) for d in range(n_docs)], dtype=np.int64)


def groups(ids, off, threshold=0.8, n_perm=128, bands=32, ngram=5, seed=0, max_len=None, tail=False):
    return groups_of_signatures(signatures(ids, off, n_perm, ngram, seed, max_len, tail), threshold, bands)


# ---------------------------------------------------------------------------
# the corpora the conditions are stated on

def estimate_cases():
    """18 (doc_a, doc_b, seed): 400-id documents with 0 - 100 % of the ids of the second replaced"""
    out = []
    for seed in (0, 1, 12345):
        rng = np.random.default_rng(900 + seed)
        for frac in (0.0, 0.02, 0.1, 0.3, 0.6, 1.0):
            a = rng.integers(0, 50000, size=400).astype(np.int32)
            b = a.copy()
            where = rng.permutation(400)[:int(round(frac * 400))]
            b[where] = rng.integers(50000, 100000, size=len(where)).astype(np.int32)
            out.append((a, b, seed))
    return out


def family_corpus(seed=7):
    """(docs, family): 40 families, every document with 1 - 4 copies that differ from it in one id, 60 - 300 ids each,
    shuffled; family[d] = the lowest document number of d's family"""
    rng = np.random.default_rng(seed)
    copies = rng.integers(1, 5, size=40)
    for f in range(10 ** 6):                                    # 67 copies in all: 107 documents
        if copies.sum() == 67:
            break
        step = 1 if copies.sum() < 67 else -1
        if 1 <= copies[f % 40] + step <= 4:
            copies[f % 40] += step
    docs, fam = [], []
    for f in range(40):
        base = rng.integers(0, 30000, size=int(rng.integers(60, 301))).astype(np.int32)
        docs.append(base)
        fam.append(f)
        for _ in range(int(copies[f])):
            c = base.copy()
            c[int(rng.integers(0, len(c)))] = int(rng.integers(30000, 60000))
            docs.append(c)
            fam.append(f)
    order = rng.permutation(len(docs))
    docs = [docs[i] for i in order]
    fam = [fam[i] for i in order]
    lowest = {}
    for d, f in enumerate(fam):
        lowest.setdefault(f, d)
    return docs, np.array([lowest[f] for f in fam], dtype=np.int64)


def stream(docs, dtype=np.int32):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    ids = np.concatenate([np.asarray(d, dtype=dtype) for d in docs]) if docs else np.zeros(0, dtype)
    return ids.astype(dtype), off
