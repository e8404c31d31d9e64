"""GPU: bpe_minhash_resident -- the MinHash signature of every document of an id stream that lives in HBM -- and
bpe_minhash_agree_resident, through the raw C ABI, and the Tokenizer methods on top of them.  Every case is compared
element for element with minhash_model; nothing is sampled.  d_sig and d_agree are framed with canaries and prefilled
(d_sig with a small value, so that a row the kernel folds into without having prefilled it keeps that value); the inputs
are read back and must be as they were.  The shapes are the smallest at which the signature pass can go wrong: its tile
is 64 positions in most cases, so that a few hundred ids are many tiles, a strip of a wave is 16 positions, and a window
of 64 ids is as long as the tile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dupdocs_model
import minhash_model
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_CAP, E_LIMIT = -2, -5, -6
TAIL = 1
CANARY, PREFILL, PREFILL_AGREE = -0x5A5A5A5B, 5, -77
# the default is the field's initialiser (api_ctx.hip): the fixture puts it back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
DEFAULTS = {name: int(re.search(rf"int {name} = (\d+);", _CTX).group(1)) for name in ("mh_tile",)}
TILES = (64, DEFAULTS["mh_tile"], 65536)


def lengths(w):
    return [0, 1, w - 1, w, w + 1, 63, 64, 65, 64 + w - 1, 257, 0, 0, 1023]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture()
def eng(engine):
    yield engine
    for name, value in DEFAULTS.items():
        engine.set_option(name, value)


def make_ids(n, width, seed):
    """n ids that use the whole width: a 64-bit id differs from its neighbours above bit 32 too"""
    rng = np.random.default_rng(seed)
    if width == 4:
        return rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    return rng.integers(-2**63, 2**63, size=n, dtype=np.int64)


def stream_of(docs, width, lead=0, trail=0, seed=0):
    """(ids, off) of the documents laid back to back, `lead` stray ids in front (doc_offsets[0] > 0) and `trail` behind"""
    dt = np.int32 if width == 4 else np.int64
    parts = [make_ids(lead, width, seed + 1)] + [np.asarray(d, dtype=dt) for d in docs] + [make_ids(trail, width, seed + 2)]
    off = lead + np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return np.concatenate(parts).astype(dt), off


def lattice(width, w, seed):
    rng = np.random.default_rng(seed)
    docs = [make_ids(l, width, 1000 * seed + i) for i, l in enumerate(lengths(w))]
    return [docs[i] for i in rng.permutation(len(docs))]


def dev_array(torch, arr, shift=0):
    """arr on the device, `shift` elements past a 16-byte aligned address"""
    arr = np.ascontiguousarray(arr)
    per16 = 16 // arr.dtype.itemsize
    buf = torch.empty(len(arr) + per16 + shift, dtype=getattr(torch, arr.dtype.name), device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[per16 + shift:per16 + shift + len(arr)]
    view[:] = torch.from_numpy(arr).to("cuda")
    return view


class Frame:
    """room for `words` int32 words, prefilled, canaries before and after; the words begin `shift` words past 16 bytes"""

    def __init__(self, torch, words, prefill=PREFILL, shift=0):
        self.words, self.prefill, self.lead = words, prefill, 4 + shift
        self.buf = torch.full((self.lead + words + 4,), prefill, dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[:self.lead] = CANARY
        self.buf[self.lead + words:] = CANARY
        self.ptr = self.buf.data_ptr() + 4 * self.lead

    def read(self):
        host = self.buf.cpu().numpy()
        assert (host[:self.lead] == CANARY).all() and (host[self.lead + self.words:] == CANARY).all(), \
            "a word outside the output was written"
        return host[self.lead:self.lead + self.words]

    def untouched(self):
        assert (self.read() == self.prefill).all(), "the output was written"


def raw(native, engine, d_ids, width, n, d_off, n_docs, max_len, flags, ngram, n_perm, seed, d_sig, sig_cap):
    """the C call itself: (rc, bad_doc)"""
    bd = C.c_uint64(12345)
    rc = native._lib.bpe_minhash_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs, max_len, flags,
                                          ngram, n_perm, seed, C.c_void_p(d_sig), sig_cap, C.byref(bd))
    return rc, bd.value


def raw_agree(native, engine, d_sig, n_docs, n_perm, d_a, d_b, m, d_agree):
    bp = C.c_uint64(12345)
    rc = native._lib.bpe_minhash_agree_resident(engine._h, C.c_void_p(d_sig), n_docs, n_perm, C.c_void_p(d_a), C.c_void_p(d_b),
                                                m, C.c_void_p(d_agree), C.byref(bp))
    return rc, bp.value


_MODEL = {}


def model(ids, off, n_perm, ngram, seed, max_len, tail):
    """the model's signatures, computed once per case"""
    key = (ids.tobytes(), ids.dtype.str, np.asarray(off).tobytes(), n_perm, ngram, seed, max_len, tail)
    if key not in _MODEL:
        _MODEL[key] = minhash_model.signatures(ids, off, n_perm, ngram, seed, max_len, tail)
        _MODEL[key].setflags(write=False)
    return _MODEL[key]


def sig_checked(torch, native, engine, ids, off, ngram=5, n_perm=128, seed=0, max_len=None, tail=False, shift=0, sig_shift=0,
                extra_cap=0):
    """one call through the C ABI into a framed output, against the model; returns the signatures"""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    want = model(ids, off, n_perm, ngram, seed, max_len, tail)
    d_ids, d_off = dev_array(torch, ids, shift), dev_array(torch, off)
    assert d_ids.data_ptr() % 16 == (shift * width) % 16
    fr = Frame(torch, n_docs * n_perm + extra_cap, shift=sig_shift)
    got = raw(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(), n_docs,
              0 if max_len is None else max_len, TAIL if tail else 0, ngram, n_perm, seed, fr.ptr if n_docs else 0,
              n_docs * n_perm + extra_cap)
    assert got == (0, NONE), (native._lib.bpe_last_error(engine._h) or b"").decode()
    words = fr.read()
    sig = words[:n_docs * n_perm].reshape(n_docs, n_perm)
    assert (words[n_docs * n_perm:] == PREFILL).all(), "words beyond n_docs * n_perm were written"
    if not np.array_equal(sig, want):
        d, p = (int(x[0]) for x in np.nonzero(sig != want))
        pytest.fail(f"sig[{d}][{p}] = {sig[d, p]}, the model has {want[d, p]} (document of {off[d + 1] - off[d]} ids at {off[d]})")
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the ids were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    return sig


# ---------------------------------------------------------------------------
# the length lattice: both widths x the windows x the tile sizes x where the stream sits on its 16 bytes

@pytest.mark.parametrize("w", (1, 2, 5, 64))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (4, 8))
def test_lattice(torch, native, eng, width, tile, w):
    eng.set_option("mh_tile", tile)
    for shift in range(4):
        docs = lattice(width, w, 10 * shift + width)
        ids, off = stream_of(docs, width, lead=1 + shift, trail=shift, seed=shift)
        assert off[0] > 0
        sig = sig_checked(torch, native, eng, ids, off, ngram=w, n_perm=64 if shift % 2 else 70, seed=shift, shift=shift,
                          sig_shift=shift)
        empty = [i for i, d in enumerate(docs) if len(d) == 0]
        assert len(empty) >= 3 and (sig[empty] == 0x7FFFFFFF).all() and (sig >= 0).all()


@pytest.mark.parametrize("n_perm", (1, 63, 64, 65, 128, 256, 257, 1024))
def test_n_perm(torch, native, eng, n_perm):
    eng.set_option("mh_tile", 64)
    for width in (4, 8):
        ids, off = stream_of(lattice(width, 5, 20 + width), width, lead=3, trail=1)
        sig_checked(torch, native, eng, ids, off, n_perm=n_perm, seed=n_perm, shift=1, extra_cap=3)
    eng.set_option("mh_tile", DEFAULTS["mh_tile"])
    sig_checked(torch, native, eng, ids, off, n_perm=n_perm, seed=n_perm)


@pytest.mark.parametrize("seed", (0, 2**64 - 1, 2**32, 12345))
def test_seeds(torch, native, eng, seed):
    eng.set_option("mh_tile", 64)
    ids, off = stream_of(lattice(4, 5, 30), 4, lead=2)
    a = sig_checked(torch, native, eng, ids, off, seed=seed)
    b = sig_checked(torch, native, eng, ids, off, seed=seed ^ 1)         # (and the parameters on the device follow the seed)
    assert (a != b).any()
    assert np.array_equal(a, sig_checked(torch, native, eng, ids, off, seed=seed))


# ---------------------------------------------------------------------------
# the halo ends where the key ends

def seam_pair(width, w, seed):
    """two documents x, y such that the windows across the seam of x | y hold a shingle whose hash is below every
    minimum of x and of y in at least one permutation: including it would change a signature"""
    for attempt in range(50):
        x, y = make_ids(9, width, seed + 2 * attempt), make_ids(9, width, seed + 2 * attempt + 1)
        ids, off = stream_of([x, y], width)
        apart = minhash_model.signatures(ids, off, 128, w, 0)
        joined = minhash_model.signatures(ids, [0, len(ids)], 128, w, 0)
        if w > 1 and (joined[0] < np.minimum(apart[0], apart[1])).any():
            return x, y
    raise AssertionError("no pair found")


@pytest.mark.parametrize("width", (4, 8))
def test_halo_ends_at_the_document(torch, native, eng, width):
    eng.set_option("mh_tile", 64)
    w = 5
    x, y = seam_pair(width, w, 40)
    filler = make_ids(64, width, 41)
    # the seam at every position of a tile, the last and the first among them
    for lead in (0, 55, 54, 51, 50, 64 - 9 + 3):
        ids, off = stream_of([filler[:lead], x, y], width)
        sig_checked(torch, native, eng, ids, off, ngram=w)
    # a seam made by max_len: head (the ids beyond the cut are the next document's neighbours) and tail
    doc = np.concatenate([x, y])
    ids, off = stream_of([doc, doc, filler[:7], doc], width, lead=2, trail=6)
    sig_checked(torch, native, eng, ids, off, ngram=w, max_len=9)
    sig_checked(torch, native, eng, ids, off, ngram=w, max_len=9, tail=True)
    sig_checked(torch, native, eng, ids, off, ngram=w, max_len=3)        # (keys shorter than the window)
    sig_checked(torch, native, eng, ids, off, ngram=w, max_len=3, tail=True)
    # stray ids after off[n_docs] and before off[0]: x is the last document, y lies behind it; y in front of x
    ids, off = stream_of([filler[:50], x], width)
    ids = np.concatenate([ids, y])
    sig_checked(torch, native, eng, ids, off, ngram=w)
    ids, off = stream_of([y], width)
    sig_checked(torch, native, eng, np.concatenate([x, ids]), off + len(x), ngram=w)


# ---------------------------------------------------------------------------
# more documents in a tile than are staged in LDS (1,024), next to a tile that holds one document

@pytest.mark.parametrize("width", (4, 8))
def test_more_documents_in_a_tile_than_are_staged(torch, native, eng, width):
    eng.set_option("mh_tile", 4096)
    rng = np.random.default_rng(50 + width)
    dt = np.int32 if width == 4 else np.int64
    tiny = [rng.integers(0, 3, size=int(rng.integers(0, 3))).astype(dt) for _ in range(3000)]
    assert sum(len(d) for d in tiny) < 4096
    docs = tiny + [make_ids(9000, width, 51)] + tiny[:100]
    ids, off = stream_of(docs, width, lead=1, trail=2)
    for w in (1, 2):
        sig_checked(torch, native, eng, ids, off, ngram=w, n_perm=64, shift=1)


# ---------------------------------------------------------------------------
# contention: every tile folds into one row; thousands of equal rows

@pytest.mark.parametrize("tile", TILES)
def test_contention(torch, native, eng, tile):
    eng.set_option("mh_tile", tile)
    ids, off = stream_of([make_ids(20000, 4, 60)], 4, lead=3)
    sig_checked(torch, native, eng, ids, off, n_perm=128)
    hot = make_ids(7, 8, 61)
    ids, off = stream_of([hot] * 2000, 8)
    sig = sig_checked(torch, native, eng, ids, off, n_perm=64)
    assert (sig == sig[0]).all()
    # all empty: with and without ids around the documents
    for n_ids in (0, 5):
        sig = sig_checked(torch, native, eng, make_ids(n_ids, 4, 62), np.full(301, n_ids // 2), n_perm=65)
        assert (sig == 0x7FFFFFFF).all()


def test_equal_values_at_both_widths(torch, native, eng):
    eng.set_option("mh_tile", 64)
    docs = lattice(4, 5, 70)
    ids32, off = stream_of(docs, 4, lead=2)
    assert (ids32 < 0).any()
    a = sig_checked(torch, native, eng, ids32, off)
    b = sig_checked(torch, native, eng, ids32.astype(np.int64), off, shift=1)
    assert np.array_equal(a, b)
    # ... and ids that differ only above bit 32 are different ids
    wide = ids32.astype(np.int64)
    wide[off[3]:off[4]] += np.int64(1 << 32)
    c = sig_checked(torch, native, eng, wide, off)
    changed = [d for d in range(len(off) - 1) if not np.array_equal(a[d], c[d])]
    assert changed == ([3] if off[4] > off[3] else [])


def test_degenerate_sizes_and_growth(torch, native, eng):
    ids = make_ids(10, 4, 71)
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, np.array([4], np.int64))
    fr = Frame(torch, 8)
    assert raw(native, eng, d_ids.data_ptr(), 4, 10, d_off.data_ptr(), 0, 0, 0, 5, 8, 0, fr.ptr, 8) == (0, NONE)   # n_docs == 0
    fr.untouched()
    assert raw(native, eng, d_ids.data_ptr(), 4, 10, d_off.data_ptr(), 0, 0, 0, 5, 8, 0, 0, 0) == (0, NONE)
    for off in ([0, 10], [3, 3], [10, 10], [2, 9]):
        sig_checked(torch, native, eng, ids, off, n_perm=3)
    sig_checked(torch, native, eng, np.zeros(0, np.int64), [0, 0, 0, 0], n_perm=2)
    for n_perm in (16, 1024, 8):                                  # the parameters' scratch grows and is used again
        sig_checked(torch, native, eng, ids, [1, 8], n_perm=n_perm, seed=n_perm)


# ---------------------------------------------------------------------------
# agreement

def agree_checked(torch, native, engine, sig, a, b, shift=0):
    n_docs, n_perm = sig.shape
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    sf = Frame(torch, sig.size, shift=shift)
    sf.buf[sf.lead:sf.lead + sig.size] = torch.from_numpy(np.ascontiguousarray(sig).reshape(-1)).to("cuda")
    d_a, d_b = dev_array(torch, a), dev_array(torch, b)
    fr = Frame(torch, len(a), prefill=PREFILL_AGREE, shift=shift)
    got = raw_agree(native, engine, sf.ptr, n_docs, n_perm, d_a.data_ptr() if len(a) else 0, d_b.data_ptr() if len(a) else 0,
                    len(a), fr.ptr if len(a) else 0)
    assert got == (0, NONE), (native._lib.bpe_last_error(engine._h) or b"").decode()
    want = (sig[a] == sig[b]).sum(axis=1).astype(np.int32) if len(a) else np.zeros(0, np.int32)
    assert np.array_equal(fr.read(), want)
    assert np.array_equal(sf.read(), sig.reshape(-1)), "the signatures were written"
    assert np.array_equal(d_a.cpu().numpy(), a) and np.array_equal(d_b.cpu().numpy(), b), "the pairs were written"


@pytest.mark.parametrize("n_perm", (1, 5, 128, 1023))
def test_agreement(torch, native, eng, n_perm):
    rng = np.random.default_rng(80 + n_perm)
    sig = rng.integers(0, 3, size=(37, n_perm)).astype(np.int32)          # few values: rows agree at many positions
    sig[5] = sig[9]
    sig[11] = 0x7FFFFFFF
    a, b = rng.integers(0, 37, size=500), rng.integers(0, 37, size=500)
    a[:40] = b[:40]                                                       # a == b
    a[40:80], b[40:80] = a[80:120], b[80:120]                             # repeated pairs
    a[120], b[120] = 5, 9
    for shift in (0, 1):
        agree_checked(torch, native, eng, sig, a, b, shift=shift)
    agree_checked(torch, native, eng, sig, a[:1], b[:1])
    agree_checked(torch, native, eng, sig, [], [])                        # m == 0


def test_agreement_errors(torch, native, eng):
    sig = np.arange(40, dtype=np.int32).reshape(10, 4)
    sf = Frame(torch, sig.size)
    sf.buf[sf.lead:sf.lead + sig.size] = torch.from_numpy(sig.reshape(-1)).to("cuda")
    good_a, good_b = np.arange(10, dtype=np.int64), np.arange(10, dtype=np.int64)[::-1].copy()
    d_a, d_b = dev_array(torch, good_a), dev_array(torch, good_b)
    for side in (0, 1):
        for bad, where in (([(3, -1)], 3), ([(7, 10), (2, 10)], 2), ([(9, 2**32)], 9), ([(0, -2**63), (5, 11)], 0),
                           ([(4, 2**63 - 1)], 4)):
            pair = [good_a.copy(), good_b.copy()]
            for j, v in bad:
                pair[side][j] = v
            fr = Frame(torch, 10, prefill=PREFILL_AGREE)
            x, y = dev_array(torch, pair[0]), dev_array(torch, pair[1])
            assert raw_agree(native, eng, sf.ptr, 10, 4, x.data_ptr(), y.data_ptr(), 10, fr.ptr) == (E_ARG, where)
            fr.untouched()
    fr = Frame(torch, 10, prefill=PREFILL_AGREE)
    good = dict(d_sig=sf.ptr, n_docs=10, n_perm=4, d_a=d_a.data_ptr(), d_b=d_b.data_ptr(), m=10, d_agree=fr.ptr)
    for code, kw in ((E_ARG, dict(n_perm=0)), (E_ARG, dict(n_perm=1025)), (E_ARG, dict(d_a=0)), (E_ARG, dict(d_b=0)),
                     (E_ARG, dict(d_agree=0)), (E_ARG, dict(d_sig=0)), (E_ARG, dict(d_sig=sf.ptr + 2)),
                     (E_ARG, dict(d_agree=fr.ptr + 1)), (E_ARG, dict(d_a=d_a.data_ptr() + 4)), (E_ARG, dict(d_b=d_b.data_ptr() + 4)),
                     (E_LIMIT, dict(n_docs=2**32 - 1)), (E_LIMIT, dict(n_docs=2**38, n_perm=4))):
        assert raw_agree(native, eng, **dict(good, **kw)) == (code, NONE), kw
        fr.untouched()
    # no documents: every pair is out of range; and a good call follows
    assert raw_agree(native, eng, **dict(good, n_docs=0)) == (E_ARG, 0)
    fr.untouched()
    assert raw_agree(native, eng, **good) == (0, NONE)
    assert np.array_equal(fr.read(), (sig[good_a] == sig[good_b]).sum(axis=1))


# ---------------------------------------------------------------------------
# errors: one per line of the contract, the output untouched and the canaries whole

def test_bad_offsets(torch, native, eng):
    ids, off = stream_of(lattice(4, 5, 90), 4, lead=2)
    n, n_docs = len(ids), len(off) - 1
    d_ids = dev_array(torch, ids)
    descends = off.copy()
    descends[3] = descends[2] - 1
    beyond = off.copy()
    beyond[4:] += n
    for bad_off, where in ((descends, 3), (beyond, 4)):
        assert select_model.check_offsets(bad_off, n) == where
        fr = Frame(torch, n_docs * 8)
        d_off = dev_array(torch, bad_off)
        assert raw(native, eng, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, 5, 8, 0, fr.ptr, n_docs * 8) == (E_ARG, where)
        fr.untouched()
        assert f"doc_offsets[{where}]" in (native._lib.bpe_last_error(eng._h) or b"").decode()
        sig_checked(torch, native, eng, ids, off, n_perm=8)                   # a good call follows


def test_argument_errors(torch, native, eng):
    ids, off = stream_of(lattice(4, 5, 91), 4)
    n, n_docs = len(ids), len(off) - 1
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    cap = n_docs * 8
    good = dict(d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, max_len=0, flags=0, ngram=5,
                n_perm=8, seed=0, sig_cap=cap)
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)),
        (E_ARG, dict(flags=2)), (E_ARG, dict(flags=0x80000001)), (E_ARG, dict(flags=TAIL, max_len=0)),
        (E_ARG, dict(ngram=0)), (E_ARG, dict(ngram=65)), (E_ARG, dict(n_perm=0)), (E_ARG, dict(n_perm=1025, sig_cap=2**40)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(d_sig=0)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)), (E_ARG, dict(d_sig=2)),
        (E_CAP, dict(sig_cap=cap - 1)), (E_CAP, dict(sig_cap=0)),
        # the limits, on these tiny buffers: refused before anything is launched or allocated
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(n_docs=2**32 - 1)), (E_LIMIT, dict(n_docs=2**30, n_perm=1024, sig_cap=2**41)),
    ]
    for code, kw in refused:
        fr = Frame(torch, cap)
        args = dict(good, d_sig=fr.ptr)
        if kw.get("d_sig") == 2:                                             # misaligned by 2 bytes
            kw = dict(d_sig=fr.ptr + 2)
        args.update(kw)
        assert raw(native, eng, **args) == (code, NONE), kw
        fr.untouched()
    sig_checked(torch, native, eng, ids, off, n_perm=8)
    for bad in (32, 96, 63, 131072, 0, -64):                                 # the option's row: a power of two from 64 to 65536
        with pytest.raises(Exception):
            eng.set_option("mh_tile", bad)
    for ok in (64, 128, 65536):
        eng.set_option("mh_tile", ok)
    sig_checked(torch, native, eng, ids, off, n_perm=8)


# ---------------------------------------------------------------------------
# the Tokenizer methods, and the calls next to this one

@pytest.fixture(scope="module")
def families():
    docs, family = minhash_model.family_corpus()
    ids, off = minhash_model.stream(docs)
    return docs, family, ids, off


def test_minhash_methods(torch, native, families):
    from minbpe_amd import BasicTokenizer
    tok = BasicTokenizer()
    docs, family, h_ids, off = families
    want = minhash_model.signatures(h_ids, off, 128, 5, 0)
    for dt in (torch.int32, torch.int64):
        ids = torch.from_numpy(h_ids).to("cuda").to(dt)
        for form in (off, off.tolist(), torch.from_numpy(off).to("cuda"), torch.from_numpy(off.astype(np.int32)).to("cuda")):
            sig = tok.minhash_resident(ids, form)
            assert sig.dtype == torch.int32 and sig.device == ids.device and sig.shape == (107, 128)
            assert np.array_equal(sig.cpu().numpy(), want)
        out = torch.full((107 * 128 + 5,), -3, dtype=torch.int32, device="cuda")
        sig = tok.minhash_resident(ids, off, out=out)
        assert sig.data_ptr() == out.data_ptr() and np.array_equal(sig.cpu().numpy(), want) and (out[107 * 128:] == -3).all()
        sig = tok.minhash_resident(ids, off, n_perm=65, ngram=3, seed=2**64 - 1, max_len=50, keep="tail")
        assert np.array_equal(sig.cpu().numpy(), minhash_model.signatures(h_ids, off, 65, 3, 2**64 - 1, 50, True))
    # ids on the host: numpy in, numpy out
    got = tok.minhash(h_ids, off)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(tok.minhash(h_ids.tolist(), off.tolist(), n_perm=16, ngram=2, seed=3, max_len=70),
                          minhash_model.signatures(h_ids, off, 16, 2, 3, 70))
    # agreement, and the position of an index that names no document
    sig = tok.minhash_resident(torch.from_numpy(h_ids).to("cuda"), off)
    a, b = np.arange(107), family
    agree = tok.minhash_agreement_resident(sig, torch.from_numpy(a).to("cuda"), b.tolist())
    assert agree.dtype == torch.int32 and np.array_equal(agree.cpu().numpy(), (want[a] == want[b]).sum(axis=1))
    assert tok.minhash_agreement_resident(sig, [], []).numel() == 0
    for bad in (-1, 107, 2**40):
        with pytest.raises(IndexError) as e:
            tok.minhash_agreement_resident(sig, [0, 1, bad, 3, -5], [0, 1, 2, 3, 4])
        assert isinstance(e.value, native.BadPair) and e.value.index == 2
    bad_off = off.copy()
    bad_off[5] = bad_off[4] - 1
    for call in (lambda: tok.minhash_resident(sig.new_zeros(len(h_ids)), bad_off), lambda: tok.minhash(h_ids, bad_off),
                 lambda: tok.near_duplicate_docs(h_ids, bad_off)):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5
    assert tok.minhash_resident(sig.new_zeros(4), [3]).shape == (0, 128)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_near_duplicates_are_the_planted_families(torch, native, families, seed):
    from minbpe_amd import BasicTokenizer
    tok = BasicTokenizer()
    docs, family, h_ids, off = families
    ids = torch.from_numpy(h_ids).to("cuda")
    kw = dict(threshold=0.7, n_perm=128, bands=32, ngram=5, seed=seed)
    first, sig = tok.near_duplicate_docs_resident(ids, off, return_signatures=True, **kw)
    assert first.dtype == torch.int64 and first.device == ids.device
    assert np.array_equal(sig.cpu().numpy(), minhash_model.signatures(h_ids, off, 128, 5, seed))
    assert np.array_equal(first.cpu().numpy(), minhash_model.groups(h_ids, off, **kw))
    assert np.array_equal(first.cpu().numpy(), family) and tok.n_distinct_docs == 40
    assert np.array_equal(tok.near_duplicate_docs(h_ids, off, **kw), family)
    # first == arange is the mask selection takes: one document of every family, in the order of the stream
    arange = torch.arange(107, device="cuda")
    s_ids, s_off = tok.select_docs_resident(ids, off, first == arange)
    kept = np.flatnonzero(family == np.arange(107))
    m_ids, m_off = select_model.select(h_ids, off, kept)
    assert np.array_equal(s_ids.cpu().numpy(), m_ids) and np.array_equal(s_off.cpu().numpy(), m_off)


def test_near_duplicates_hold_the_exact_ones(torch, native):
    from minbpe_amd import BasicTokenizer
    tok = BasicTokenizer()
    rng = np.random.default_rng(95)
    base = [rng.integers(0, 50, size=int(rng.integers(0, 40))).astype(np.int64) for _ in range(30)]
    docs = [base[i] for i in rng.integers(0, 30, size=150)] + [np.zeros(0, np.int64)] * 3
    for i in range(0, 150, 9):
        d = docs[i].copy()
        if len(d):
            d[len(d) // 2] += 1000                                          # near copies among the exact ones
        docs[i] = d
    h_ids, off = minhash_model.stream(docs, np.int64)
    ids = torch.from_numpy(h_ids).to("cuda")
    for kw in (dict(threshold=0.5, n_perm=64, bands=16, ngram=3), dict(threshold=1.0, n_perm=32, bands=1, ngram=1, max_len=10),
               dict(threshold=0.3, n_perm=60, bands=60, ngram=2, max_len=10, keep="tail", seed=9)):
        first = tok.near_duplicate_docs_resident(ids, off, **kw).cpu().numpy()
        model_kw = {k: v for k, v in kw.items() if k != "keep"}
        assert np.array_equal(first, minhash_model.groups(h_ids, off, tail=kw.get("keep") == "tail", **model_kw))
        assert tok.n_distinct_docs == int((first == np.arange(len(docs))).sum())
        exact = dupdocs_model.duplicates(h_ids, off, kw.get("max_len"), kw.get("keep") == "tail")[0]
        assert np.array_equal(first[exact], first), "coarser than or equal to the exact de-duplication"
        assert np.array_equal(first[first], first) and (first <= np.arange(len(docs))).all()
        exact_dev = tok.duplicate_docs_resident(ids, off, max_len=kw.get("max_len"), keep=kw.get("keep", "head")).cpu().numpy()
        assert np.array_equal(exact_dev, exact)
    first = tok.near_duplicate_docs_resident(ids, [4])
    assert first.numel() == 0 and tok.n_distinct_docs == 0


def test_a_pending_decode_survives(torch, native):
    """a bpe_decode_batch result not yet read is as it was after the signatures were made on the same ctx"""
    import minbpe_amd.tokenizer as T
    from minbpe_amd import RegexTokenizer
    tok = RegexTokenizer()
    tok.train(native.synth_text(20_000, 61).decode(), 256 + 20)
    texts = [native.synth_text(300, 70 + i).decode() for i in range(12)]
    ids, doff = tok.encode_ordinary_batch_resident(texts)
    proc = T.engine(ids.device.index)
    h_ids = ids.cpu().numpy().astype(np.int32)
    tok.decode_batch_resident(ids, doff)                                     # (the decode table is on the ctx)
    nb, bad = C.c_uint64(0), C.c_uint64(0)
    assert native._lib.bpe_decode_batch(proc._h, h_ids.ctypes.data_as(C.c_void_p), len(h_ids), C.byref(nb), C.byref(bad)) == 0
    sig = tok.minhash_resident(ids, doff)
    tok.minhash_agreement_resident(sig, [0, 1], [1, 2])
    out = np.empty(max(nb.value, 1), np.uint8)
    assert native._lib.bpe_decode_read(proc._h, out.ctypes.data_as(C.c_void_p), len(out), None, 0, None) == 0
    assert out[:nb.value].tobytes() == "".join(texts).encode("utf-8")
    assert np.array_equal(sig.cpu().numpy(), minhash_model.signatures(h_ids, doff.cpu().numpy(), 128, 5, 0))
