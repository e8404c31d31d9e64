"""GPU: bpe_ngram_index_resident and bpe_ngram_overlap_resident -- which documents of an id stream in HBM hold a window of
w ids that also occurs in a reference stream -- through the raw C ABI, and the Tokenizer methods on top of them.  Every
case is compared element for element with ngram_model; nothing is sampled.  Every output column is framed with canaries
and prefilled with a value no result can be (d_starts with a non-zero byte, so that an unwritten byte shows); the inputs
are read back and must be as they were.  The shapes are the smallest at which the passes can go wrong: the tile is 64
positions in most cases, so that a few hundred ids are many tiles, a strip of a wave is 64 positions, a chunk 2048, and a
window of 64 ids is as long as the tile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ngram_model
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_STATE, E_LIMIT = -2, -4, -6
TAIL = 1
CANARY64, PREFILL64 = -0x5A5A5A5A5A5A5A5B, -777                  # (a count is never negative; first and ref_pos are -1 or more)
CANARY8, PREFILL8 = 0xA5, 0x5A                                   # (a start is 0 or 1)
UNSET = (111, 222, 333)                                          # index_id, n_windows, n_distinct before a call
# the defaults are the fields' initialisers (api_ctx.hip): the fixture puts them back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
DEFAULTS = {name: int(re.search(rf"int {name} = (\d+);", _CTX).group(1)) for name in ("ng_tile", "ng_hash_bits")}
TILES = (64, DEFAULTS["ng_tile"], 65536)


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


def dtype_of(width):
    return np.int32 if width == 4 else np.int64


def make_ids(n, width, seed):
    """n ids that use the whole width, negatives included: a 64-bit id differs from its neighbours above bit 32 too"""
    rng = np.random.default_rng(seed)
    if width == 4:
        return rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    return rng.integers(-2**63, 2**63, size=n, dtype=np.int64)


def stream_of(docs, width, lead=(), trail=()):
    """(ids, off) of the documents laid back to back, the stray ids `lead` in front (off[0] > 0) and `trail` behind"""
    dt = dtype_of(width)
    parts = [np.asarray(lead, dtype=dt)] + [np.asarray(d, dtype=dt) for d in docs] + [np.asarray(trail, dtype=dt)]
    off = len(lead) + np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return np.concatenate(parts).astype(dt), off


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
    """room for `count` elements of int64 or uint8, prefilled, canaries before and after; the elements begin `shift`
    elements past 16 bytes"""

    def __init__(self, torch, count, wide=True, shift=0):
        dt, self.canary, self.prefill = (torch.int64, CANARY64, PREFILL64) if wide else (torch.uint8, CANARY8, PREFILL8)
        self.count, self.lead = count, (2 if wide else 16) + shift
        self.buf = torch.full((self.lead + count + 16,), self.prefill, dtype=dt, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[:self.lead] = self.canary
        self.buf[self.lead + count:] = self.canary
        self.ptr = self.buf.data_ptr() + self.lead * (8 if wide else 1)

    def read(self):
        host = self.buf.cpu().numpy()
        canary = np.asarray(self.canary).astype(host.dtype)
        assert (host[:self.lead] == canary).all() and (host[self.lead + self.count:] == canary).all(), \
            "an element outside the output was written"
        return host[self.lead:self.lead + self.count]

    def untouched(self):
        assert (self.read() == np.asarray(self.prefill).astype(self.read().dtype)).all(), "the output was written"


def last_error(native, engine):
    return (native._lib.bpe_last_error(engine._h) or b"").decode()


def raw_index(native, engine, d_ref, width, n_ref, d_roff, n_ref_docs, ngram):
    """the C call itself: (rc, index_id, n_windows, n_distinct, bad_doc)"""
    iid, nw, nd, bd = C.c_uint64(UNSET[0]), C.c_uint64(UNSET[1]), C.c_uint64(UNSET[2]), C.c_uint64(12345)
    rc = native._lib.bpe_ngram_index_resident(engine._h, C.c_void_p(d_ref), width, n_ref, C.c_void_p(d_roff), n_ref_docs,
                                              ngram, C.byref(iid), C.byref(nw), C.byref(nd), C.byref(bd))
    return rc, iid.value, nw.value, nd.value, bd.value


def raw_overlap(native, engine, index_id, d_ids, width, n, d_off, n_docs, max_len, flags, d_hits, d_first, d_ref_pos,
                d_starts):
    """the C call itself: (rc, n_hit_docs, bad_doc)"""
    nh, bd = C.c_uint64(0), C.c_uint64(12345)
    rc = native._lib.bpe_ngram_overlap_resident(engine._h, index_id, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs,
                                                max_len, flags, C.c_void_p(d_hits), C.c_void_p(d_first),
                                                C.c_void_p(d_ref_pos), C.c_void_p(d_starts), C.byref(nh), C.byref(bd))
    return rc, nh.value, bd.value


_SERIAL = {}


def build_checked(torch, native, engine, ref, roff, w, shift=0):
    """one build through the C ABI, its counters against the model; returns (index_id, the model's dict)"""
    ref = np.asarray(ref)
    width = ref.dtype.itemsize
    roff = np.asarray(roff, dtype=np.int64)
    low, n_windows = ngram_model.index(ref, roff, w)
    d_ref, d_roff = dev_array(torch, ref, shift), dev_array(torch, roff)
    rc, iid, nw, nd, bad = raw_index(native, engine, d_ref.data_ptr() if len(ref) else 0, width, len(ref), d_roff.data_ptr(),
                                     len(roff) - 1, w)
    assert (rc, bad) == (0, NONE), last_error(native, engine)
    assert (nw, nd) == (n_windows, len(low))
    assert iid != 0 and iid > _SERIAL.get(id(engine), 0), "an index_id is new for every build"
    _SERIAL[id(engine)] = iid
    assert np.array_equal(d_ref.cpu().numpy(), ref) and np.array_equal(d_roff.cpu().numpy(), roff), "the reference was written"
    d_ref.fill_(0)                                               # (the ctx has its own copy: the caller's may go)
    return iid, low


def overlap_checked(torch, native, engine, iid, low, w, ids, off, max_len=None, tail=False, shift=0, out_shift=0,
                    columns=(True, True, True)):
    """one query through the C ABI into framed outputs, against the model; returns (hits, first, ref_pos, starts)"""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    want = ngram_model.overlap(low, w, ids, off, max_len, tail)
    d_ids, d_off = dev_array(torch, ids, shift), dev_array(torch, off)
    assert d_ids.data_ptr() % 16 == (shift * width) % 16
    frames = [Frame(torch, n_docs, shift=out_shift), Frame(torch, n_docs, shift=out_shift), Frame(torch, n_docs, shift=out_shift),
              Frame(torch, len(ids), wide=False, shift=out_shift)]
    use = (True,) + tuple(columns)
    rc, n_hit, bad = raw_overlap(native, engine, iid, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(),
                                 n_docs, 0 if max_len is None else max_len, TAIL if tail else 0,
                                 *[f.ptr if u and (f.count or f is frames[3]) else 0 for f, u in zip(frames, use)])
    assert (rc, bad) == (0, NONE), last_error(native, engine)
    assert n_hit == want[4]
    got = []
    for name, f, u, x in zip(("hits", "first", "ref_pos", "starts"), frames, use, want):
        if not u:
            f.untouched()
            got.append(None)
            continue
        col = f.read()
        if not np.array_equal(col, x):
            i = int(np.flatnonzero(col != x)[0])
            d = i if name != "starts" else int(np.searchsorted(off, i, side="right")) - 1
            pytest.fail(f"{name}[{i}] = {col[i]}, the model has {x[i]} (document {d} of {n_docs}, w = {w}, max_len = {max_len}, "
                        f"tail = {tail})")
        got.append(col)
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the ids were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    return got


def both_checked(torch, native, engine, ref, roff, w, ids, off, rshift=0, **kw):
    iid, low = build_checked(torch, native, engine, ref, roff, w, shift=rshift)
    return overlap_checked(torch, native, engine, iid, low, w, ids, off, **kw)


# ---------------------------------------------------------------------------
# the length lattice: both widths on each side x the windows x the tile sizes x where the streams sit on their 16 bytes

def planted(rng, ref, l, w, width, seed):
    """a document of l ids that use the whole width, with up to three runs of the reference copied in: runs shorter and
    longer than the window, at its ends and inside, from inside reference documents and across their ends"""
    d = make_ids(l, width, seed)
    for _ in range(3):
        m = int(rng.integers(1, min(l, 2 * w + 2) + 1)) if l else 0
        if m == 0 or len(ref) < m:
            continue
        src, dst = int(rng.integers(0, len(ref) - m + 1)), int(rng.choice([0, l - m, int(rng.integers(0, l - m + 1))]))
        d[dst:dst + m] = ref[src:src + m].astype(d.dtype)
    return d


def lattice(cw, rw, w, seed):
    """(ref, roff, ids, off): reference and corpus documents of the lattice's lengths, shuffled; the values of the
    reference fit the narrower side, so that equal values exist; strays in front and behind both that must not count"""
    rng = np.random.default_rng(seed)
    vw = min(cw, rw)
    ref_docs = [make_ids(l, vw, 1000 * seed + i) for i, l in enumerate(lengths(w))]
    ref_docs = [ref_docs[i] for i in rng.permutation(len(ref_docs))]
    body = np.concatenate(ref_docs)
    docs = [planted(rng, body, l, w, cw, 2000 * seed + i) for i, l in enumerate(lengths(w))]
    docs = [docs[i] for i in rng.permutation(len(docs))]
    only_corpus = make_ids(w + 2, vw, 3000 * seed)               # windows the reference holds outside its documents only
    longest = docs[int(np.argmax([len(d) for d in docs]))]
    longest[5:5 + w + 2] = only_corpus
    longest[100:100 + w + 3] = max(ref_docs, key=len)[10:10 + w + 3]  # (four hits at the least, whatever the runs above made)
    some = body[70:70 + w + 2]                                   # reference windows the corpus holds outside its documents too
    ref, roff = stream_of(ref_docs, rw, lead=only_corpus, trail=only_corpus[::-1])
    ids, off = stream_of(docs, cw, lead=some, trail=some)
    return ref, roff, ids, off


@pytest.mark.parametrize("w", (1, 2, 13, 64))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("cw,rw", ((4, 4), (4, 8), (8, 4), (8, 8)))
def test_lattice(torch, native, eng, cw, rw, tile, w):
    eng.set_option("ng_tile", tile)
    for shift in range(4):
        ref, roff, ids, off = lattice(cw, rw, w, 10 * shift + cw + rw // 8)
        assert off[0] > 0 and roff[0] > 0
        hits, first, ref_pos, starts = both_checked(torch, native, eng, ref, roff, w, ids, off, rshift=(shift + 1) % 4,
                                                    shift=shift, out_shift=shift)
        assert hits.sum() > 0 and (hits == 0).sum() >= 3
        assert starts[:off[0]].sum() == 0 and starts[off[-1]:].sum() == 0


# ---------------------------------------------------------------------------
# planted hits: a key's first and last window, the seams of tiles, chunks and strips, the ends of documents on both sides

@pytest.mark.parametrize("tile", (64, 256, 4096, 65536))
@pytest.mark.parametrize("width", (4, 8))
def test_planted_at_seams(torch, native, eng, width, tile):
    eng.set_option("ng_tile", tile)
    w = 13
    rng = np.random.default_rng(100 + width)
    ref_docs = [make_ids(40, width, 101), make_ids(w, width, 102), make_ids(w - 1, width, 103), make_ids(30, width, 104)]
    ref, roff = stream_of(ref_docs, width, lead=make_ids(3, width, 105))
    iid, low = build_checked(torch, native, eng, ref, roff, w)
    window = ref_docs[0][5:5 + w]
    across_ref = np.concatenate([ref_docs[0][-6:], ref_docs[1][:w - 6]])   # equal to ids that span two reference documents
    assert tuple(int(x) for x in across_ref) not in low and tuple(int(x) for x in window) in low
    n, seams = 4500, (64, 128, 192, 256, 2048, 4096)                      # strips of 64, tiles, the chunk of 2048
    # the window ends at the seam, straddles it (three ways), begins at it: j = where it starts, counted from the seam
    for case, j in enumerate((-w, -w + 1, -6, -1, 0)):
        lead = case % 3
        doc = make_ids(n, width, 110 + case)
        for seam in seams:                                                # (positions of the stream; the document begins at `lead`)
            doc[seam - lead + j:seam - lead + j + w] = window
            doc[seam - lead + 20:seam - lead + 20 + w] = across_ref
        doc[:w] = window                                                  # the key's first window
        doc[n - w:] = ref_docs[1]                                         # ... and its last, a whole reference document
        ids, off = stream_of([doc], width, lead=make_ids(lead, width, 120))
        hits, first, ref_pos, starts = overlap_checked(torch, native, eng, iid, low, w, ids, off)
        assert first[0] == 0 and starts[off[0]] == 1 and starts[off[1] - w] == 1 and hits[0] == len(seams) + 2
        assert all(starts[s + j] == 1 for s in seams)
        # a reference window split over two corpus documents: every planted window cut in two
        cuts = [lead] + [s + j + 6 for s in seams] + [lead + n]
        hits2 = overlap_checked(torch, native, eng, iid, low, w, ids, cuts)[0]
        assert hits2.sum() == 2
    # near misses: the window with its last id changed, and its first; found next to the window itself
    near_last, near_first = window.copy(), window.copy()
    near_last[-1] ^= 1
    near_first[0] ^= 1
    ids, off = stream_of([near_last, near_first, window, np.concatenate([near_first, window[-1:]])], width)
    hits = overlap_checked(torch, native, eng, iid, low, w, ids, off)[0]
    assert hits.tolist() == [0, 0, 1, 0]


def test_full_width_ids(torch, native, eng):
    """int64 ids that differ only above bit 32; the extremes of both widths; equal values at both widths"""
    eng.set_option("ng_tile", 64)
    w = 3
    base = np.array([-2**31, -1, 0, 1, 2**31 - 1, 7, -7], np.int64)
    for rw in (4, 8):
        ref, roff = stream_of([base], rw)
        iid, low = build_checked(torch, native, eng, ref, roff, w)
        same32, same64 = base.astype(np.int32), base.copy()
        high = base + (np.int64(1) << 32)                                 # every id differs above bit 32 only
        one_high = base.copy()
        one_high[3] += np.int64(1) << 32
        a = overlap_checked(torch, native, eng, iid, low, w, same32, [0, 7])[0]
        b = overlap_checked(torch, native, eng, iid, low, w, same64, [0, 7], shift=1)[0]
        assert a.tolist() == b.tolist() == [5]
        assert overlap_checked(torch, native, eng, iid, low, w, high, [0, 7])[0].tolist() == [0]
        assert overlap_checked(torch, native, eng, iid, low, w, one_high, [0, 7])[0].tolist() == [2]
    wide = np.array([-2**63, 2**63 - 1, -1, 2**32 - 1, 2**32, -2**32, 2**63 - 1, -2**63], np.int64)
    hits, first, ref_pos, _ = both_checked(torch, native, eng, wide, [0, 8], 2, np.concatenate([wide[2:], wide[:3]]), [0, 6, 9])
    assert hits.tolist() == [5, 2] and first.tolist() == [0, 0] and ref_pos.tolist() == [2, 0]
    # what an int32 corpus cannot hold is never equal to it
    narrow = np.array([-1, 0, -2**31], np.int32)
    assert both_checked(torch, native, eng, wide, [0, 8], 1, narrow, [0, 3])[0].tolist() == [1]


# ---------------------------------------------------------------------------
# repeats: ref_pos is the lowest of a repeated reference window; every start of a repeated corpus window counts

@pytest.mark.parametrize("tile", TILES)
def test_repeats(torch, native, eng, tile):
    eng.set_option("ng_tile", tile)
    w = 4
    a, b = make_ids(w, 4, 130), make_ids(w + 3, 4, 131)
    filler = make_ids(3000, 4, 132)
    # a at 2100 (another tile, another chunk), 700 and 90; b at 2500 and 300; in three documents
    ref = filler.copy()
    for at in (2100, 700, 90):
        ref[at:at + w] = a
    for at in (2500, 300):
        ref[at:at + w + 3] = b
    roff = np.array([0, 500, 1500, 3000])
    iid, low = build_checked(torch, native, eng, ref, roff, w)
    assert low[tuple(int(x) for x in a)] == 90 and low[tuple(int(x) for x in b[:w])] == 300
    doc = np.concatenate([make_ids(70, 4, 133), a, make_ids(5, 4, 134), a, a, b, make_ids(66, 4, 135), a])
    ids, off = stream_of([doc, b, a[1:], np.tile(a, 40)], 4, lead=a)
    hits, first, ref_pos, starts = overlap_checked(torch, native, eng, iid, low, w, ids, off)
    assert hits.tolist() == [4 + 4, 4, 0, 40] and first.tolist() == [70, 0, -1, 0] and ref_pos.tolist() == [90, 300, -1, 90]
    # a reference of one value: every window is the same one
    ones = np.full(700, 9, np.int64)
    hits, first, ref_pos, _ = both_checked(torch, native, eng, ones, [0, 300, 700], 5, ones[:200], [0, 4, 9, 200])
    assert hits.tolist() == [0, 1, 187] and ref_pos.tolist() == [-1, 0, 0]


# ---------------------------------------------------------------------------
# max_len with both keep values: a hit just inside and just outside the cut; first stays document-relative

@pytest.mark.parametrize("width", (4, 8))
def test_max_len(torch, native, eng, width):
    eng.set_option("ng_tile", 64)
    w = 5
    window = make_ids(w, width, 140)
    ref, roff = stream_of([window], width)
    iid, low = build_checked(torch, native, eng, ref, roff, w)
    docs = []
    for i, l in enumerate((3, 40, 64, 65, 200, 0, 5)):
        d = make_ids(l, width, 141 + i)
        for at in (0, l - w):                                               # its first and its last window
            if 0 <= at <= l - w:
                d[at:at + w] = window
        docs.append(d)
    inside, outside = make_ids(100, width, 150), make_ids(100, width, 151)  # of a cut of 20, at either end
    inside[15:20], inside[80:85] = window, window                           # the last window of the head, the first of the tail
    outside[16:21], outside[79:84] = window, window                         # one id beyond the cut, one id in front of it
    docs += [inside, outside]
    A, B = len(docs) - 2, len(docs) - 1
    ids, off = stream_of(docs, width, lead=window, trail=window)
    whole = overlap_checked(torch, native, eng, iid, low, w, ids, off)
    assert whole[0][A] == whole[0][B] == 2
    for max_len in (20, 19, w, w - 1, 1, 64, 10**6, 2**64 - 1):
        head = overlap_checked(torch, native, eng, iid, low, w, ids, off, max_len=max_len)
        tail = overlap_checked(torch, native, eng, iid, low, w, ids, off, max_len=max_len, tail=True, shift=1)
        if max_len >= 200:
            assert all(np.array_equal(x, y) for x, y in zip(whole, head)) and all(np.array_equal(x, y) for x, y in zip(whole, tail))
    head = overlap_checked(torch, native, eng, iid, low, w, ids, off, max_len=20)
    tail = overlap_checked(torch, native, eng, iid, low, w, ids, off, max_len=20, tail=True)
    assert (head[0][A], head[1][A], head[0][B], head[1][B]) == (1, 15, 0, -1)
    assert (tail[0][A], tail[1][A], tail[0][B], tail[1][B]) == (1, 80, 0, -1)  # first: a position of the uncut document


# ---------------------------------------------------------------------------
# more documents in a tile than are staged in LDS (1,024), next to tiles that stage

@pytest.mark.parametrize("width", (4, 8))
def test_more_documents_in_a_tile_than_are_staged(torch, native, eng, width):
    rng = np.random.default_rng(150 + width)
    dt = dtype_of(width)
    tiny = [rng.integers(0, 5, size=int(rng.integers(1, 4))).astype(dt) for _ in range(1100)]  # (4 is in no reference document)
    docs = tiny + [rng.integers(0, 5, size=3000).astype(dt)] + tiny[:50]
    ids, off = stream_of(docs, width, lead=[1], trail=[2, 3])
    ref_docs = [rng.integers(0, 3, size=int(rng.integers(0, 3))).astype(dt) for _ in range(1100)] + [np.array([0, 3, 3, 1], dt)]
    ref, roff = stream_of(ref_docs, width, lead=[3, 3])
    for tile in (65536, 64):
        eng.set_option("ng_tile", tile)
        for w in (1, 2):
            hits = both_checked(torch, native, eng, ref, roff, w, ids, off, shift=1)[0]
            assert 0 < (hits > 0).sum() < len(docs)


# ---------------------------------------------------------------------------
# contention: every tile folds into one row; thousands of equal rows

@pytest.mark.parametrize("tile", TILES)
def test_contention(torch, native, eng, tile):
    eng.set_option("ng_tile", tile)
    w = 5
    period = make_ids(7, 4, 160)
    ref, roff = stream_of([np.tile(period, 15)], 4)
    iid, low = build_checked(torch, native, eng, ref, roff, w)
    assert len(low) == 7
    ids, off = stream_of([np.tile(period, 715)[:5000]], 4, lead=make_ids(3, 4, 161))
    hits, first, ref_pos, starts = overlap_checked(torch, native, eng, iid, low, w, ids, off)
    assert hits.tolist() == [5000 - w + 1] and first.tolist() == [0] and ref_pos.tolist() == [0]
    hot = np.tile(period, 2)[2:2 + 8].astype(np.int64)
    ids, off = stream_of([hot] * 2000, 8)
    hits, first, ref_pos, _ = overlap_checked(torch, native, eng, iid, low, w, ids, off)
    assert (hits == 4).all() and (first == 0).all() and (ref_pos == 2).all()


# ---------------------------------------------------------------------------
# forced collisions: few bits of the hash, long probe runs, every probe a comparison

@pytest.mark.parametrize("bits", (0, 1, 3, 64))
@pytest.mark.parametrize("cw,rw", ((4, 8), (8, 4)))
def test_hash_bits(torch, native, eng, cw, rw, bits):
    eng.set_option("ng_hash_bits", bits)
    eng.set_option("ng_tile", 64)
    rng = np.random.default_rng(170 + bits)
    for w in (1, 3, 13):
        ref_docs = [rng.integers(-3, 40, size=l) for l in (0, w, 100, w - 1, 150, 30)]
        ref, roff = stream_of(ref_docs, rw, lead=[1, 2])
        assert ngram_model.index(ref, roff, w)[1] <= 300
        body = np.concatenate(ref_docs)
        docs = [planted(rng, body, l, w, cw, 171 + i) for i, l in enumerate((0, 1, w, 63, 64, 65, 300, 700, 2 * w, 500))]
        ids, off = stream_of(docs, cw, lead=body[:w])
        assert len(ids) <= 2000
        hits = both_checked(torch, native, eng, ref, roff, w, ids, off, shift=bits % 4)[0]
        assert hits.sum() > 0
    # the index keeps the bits it was built with: a change of the option between build and query is not its concern
    iid, low = build_checked(torch, native, eng, ref, roff, w)
    eng.set_option("ng_hash_bits", 64 - bits)
    overlap_checked(torch, native, eng, iid, low, w, ids, off)
    for bad in (-1, 65):
        with pytest.raises(Exception):
            eng.set_option("ng_hash_bits", bad)


# ---------------------------------------------------------------------------
# the life of the index

def test_empty_index_and_degenerate_sizes(torch, native, eng):
    ids, off = stream_of([make_ids(l, 4, 180 + l) for l in (5, 0, 70)], 4, lead=[1])
    some = make_ids(10, 8, 181)
    # no window: no reference document, every reference document shorter than the window, no ids at all
    for ref, roff, w in ((some, [4], 1), (some, [0, 3, 3, 7, 10], 5), (some[:0], [0, 0], 1), (some, [2, 2, 2], 1)):
        iid, low = build_checked(torch, native, eng, ref, roff, w)
        assert low == {}
        hits, first, ref_pos, starts = overlap_checked(torch, native, eng, iid, low, w, ids, off)
        assert (hits == 0).all() and (first == -1).all() and (ref_pos == -1).all() and (starts == 0).all()
    iid, low = build_checked(torch, native, eng, ids, off, 2)
    # n_docs == 0: the columns stay as they were, every byte of starts is written; n == 0; all documents empty
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, np.array([4], np.int64))
    col, st = Frame(torch, 4), Frame(torch, len(ids), wide=False)
    assert raw_overlap(native, eng, iid, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), 0, 0, 0, col.ptr, col.ptr, col.ptr,
                       st.ptr) == (0, 0, NONE)
    col.untouched()
    assert (st.read() == 0).all()
    assert raw_overlap(native, eng, iid, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), 0, 0, 0, 0, 0, 0, 0) == (0, 0, NONE)
    overlap_checked(torch, native, eng, iid, low, 2, ids[:0], [0, 0, 0])
    overlap_checked(torch, native, eng, iid, low, 2, ids, [3, 3, 3, 3])
    overlap_checked(torch, native, eng, iid, low, 2, ids, [len(ids)] * 2)
    for columns in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        overlap_checked(torch, native, eng, iid, low, 2, ids, off, columns=columns)
    assert overlap_checked(torch, native, eng, iid, low, 2, ids, off)[0].tolist() == [4, 0, 69]


def test_index_survives_other_calls(torch, native):
    with native.Engine(0) as own:                                            # (a ctx of its own: it gets a decode table)
        own.set_option("ng_tile", 64)
        survives(torch, native, own)


def survives(torch, native, eng):
    ref, roff, ids, off = lattice(4, 8, 2, 190)
    iid, low = build_checked(torch, native, eng, ref, roff, 2)
    before = overlap_checked(torch, native, eng, iid, low, 2, ids, off)
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    n_docs = len(off) - 1
    first = torch.empty(n_docs, dtype=torch.int64, device="cuda")
    sig = torch.empty(n_docs * 16, dtype=torch.int32, device="cuda")
    eng.dup_docs_resident(d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), n_docs, 0, 0, first.data_ptr(), 0)
    eng.minhash_resident(d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), n_docs, 0, 0, 5, 16, 0, sig.data_ptr(), sig.numel())
    eng.decode_set_vocab(bytes(range(256)), np.arange(257))
    assert eng.decode_batch(np.arange(65, 75)) == bytes(range(65, 75))
    after = overlap_checked(torch, native, eng, iid, low, 2, ids, off)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_rebuilds(torch, native, eng):
    eng.set_option("ng_tile", 64)
    ids, off = stream_of([make_ids(l, 4, 200 + l) for l in (50, 9, 300)], 4)
    n_docs = len(off) - 1
    small, large = ids[10:40].astype(np.int64), np.concatenate([make_ids(20000, 8, 201), ids[340:359].astype(np.int64)])
    first_id, low = build_checked(torch, native, eng, small, [0, 30], 4)
    assert overlap_checked(torch, native, eng, first_id, low, 4, ids, off)[0].tolist() == [27, 0, 0]
    # a larger reference (the scratch grows), then a smaller one again: each build replaces the one before
    second_id, low2 = build_checked(torch, native, eng, large, [0, 20000, len(large)], 4)
    assert overlap_checked(torch, native, eng, second_id, low2, 4, ids, off)[0].tolist() == [0, 0, 16]
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    frames = [Frame(torch, n_docs) for _ in range(3)] + [Frame(torch, len(ids), wide=False)]
    query = lambda index_id: raw_overlap(native, eng, index_id, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), n_docs, 0, 0,
                                         *[f.ptr for f in frames])
    for stale in (first_id, 0, second_id + 1, NONE):
        assert query(stale) == (E_STATE, 0, NONE)
        assert "index" in last_error(native, eng)
        for f in frames:
            f.untouched()
    third_id, low3 = build_checked(torch, native, eng, small, [0, 30], 4)
    assert query(second_id)[0] == E_STATE
    assert overlap_checked(torch, native, eng, third_id, low3, 4, ids, off)[0].tolist() == [27, 0, 0]
    # a rebuild that fails leaves no index: the id that was current is refused, and a good build follows
    d_ref, d_roff = dev_array(torch, small), dev_array(torch, np.array([0, 31], np.int64))
    assert raw_index(native, eng, d_ref.data_ptr(), 8, 30, d_roff.data_ptr(), 1, 4) == (E_ARG,) + UNSET + (1,)
    assert query(third_id) == (E_STATE, 0, NONE)
    for f in frames:
        f.untouched()
    fourth_id, low4 = build_checked(torch, native, eng, small, [0, 30], 4)
    assert fourth_id > third_id and query(fourth_id)[:2] == (0, 1)


# ---------------------------------------------------------------------------
# errors: one per line of the contract, the outputs untouched and the canaries whole

def test_bad_offsets(torch, native, eng):
    ref, roff, ids, off = lattice(4, 4, 5, 210)
    n, n_docs = len(ids), len(off) - 1
    iid, low = build_checked(torch, native, eng, ref, roff, 5)
    d_ids = dev_array(torch, ids)
    descends = off.copy()
    descends[3] = descends[2] - 1
    beyond = off.copy()
    beyond[4:] += n
    for bad_off, where in ((descends, 3), (beyond, 4)):
        assert select_model.check_offsets(bad_off, n) == where
        frames = [Frame(torch, n_docs) for _ in range(3)] + [Frame(torch, n, wide=False)]
        d_off = dev_array(torch, bad_off)
        assert raw_overlap(native, eng, iid, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0,
                           *[f.ptr for f in frames]) == (E_ARG, 0, where)
        for f in frames:
            f.untouched()
        assert f"doc_offsets[{where}]" in last_error(native, eng)
        overlap_checked(torch, native, eng, iid, low, 5, ids, off)           # the index stands; a good call follows
    # the same on the build, which then leaves no index
    d_ref = dev_array(torch, ref)
    for change, where in ((lambda o: o.__setitem__(3, o[2] - 1), 3), (lambda o: o.__setitem__(slice(4, None), o[4:] + len(ref)), 4)):
        bad_roff = roff.copy()
        change(bad_roff)
        assert select_model.check_offsets(bad_roff, len(ref)) == where
        iid, low = build_checked(torch, native, eng, ref, roff, 5)
        d_roff = dev_array(torch, bad_roff)
        assert raw_index(native, eng, d_ref.data_ptr(), 4, len(ref), d_roff.data_ptr(), len(roff) - 1, 5) == (E_ARG,) + UNSET + (where,)
        assert f"doc_offsets[{where}]" in last_error(native, eng)
        col = Frame(torch, n_docs)
        d_off = dev_array(torch, off)
        assert raw_overlap(native, eng, iid, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, col.ptr, 0, 0, 0)[0] == E_STATE
        col.untouched()


def test_argument_errors(torch, native, eng):
    ref, roff, ids, off = lattice(4, 4, 5, 211)
    n, n_docs = len(ids), len(off) - 1
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    d_ref, d_roff = dev_array(torch, ref), dev_array(torch, roff)
    good = dict(d_ref=d_ref.data_ptr(), width=4, n_ref=len(ref), d_roff=d_roff.data_ptr(), n_ref_docs=len(roff) - 1, ngram=5)
    for code, kw in ((E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)), (E_ARG, dict(ngram=0)),
                     (E_ARG, dict(ngram=65)), (E_ARG, dict(d_ref=0)), (E_ARG, dict(d_roff=0)),
                     (E_ARG, dict(d_ref=d_ref.data_ptr() + 2)), (E_ARG, dict(d_roff=d_roff.data_ptr() + 4)),
                     (E_ARG, dict(width=8, d_ref=d_ref.data_ptr() + 4)),
                     (E_LIMIT, dict(n_ref=2**32)), (E_LIMIT, dict(n_ref_docs=2**32 - 1))):
        assert raw_index(native, eng, **dict(good, **kw)) == (code,) + UNSET + (NONE,), kw
    assert native._lib.bpe_ngram_index_resident(eng._h, C.c_void_p(good["d_ref"]), 4, len(ref), C.c_void_p(good["d_roff"]),
                                                len(roff) - 1, 5, None, None, None, None) == E_ARG    # index_id is required
    iid, low = build_checked(torch, native, eng, ref, roff, 5)
    frames = [Frame(torch, n_docs) for _ in range(3)] + [Frame(torch, n, wide=False)]
    good = dict(index_id=iid, d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, max_len=0, flags=0,
                d_hits=frames[0].ptr, d_first=frames[1].ptr, d_ref_pos=frames[2].ptr, d_starts=frames[3].ptr)
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)),
        (E_ARG, dict(flags=2)), (E_ARG, dict(flags=0x80000001)), (E_ARG, dict(flags=TAIL, max_len=0)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(d_hits=0)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)),
        (E_ARG, dict(d_hits=frames[0].ptr + 4)), (E_ARG, dict(d_first=frames[1].ptr + 4)), (E_ARG, dict(d_ref_pos=frames[2].ptr + 2)),
        # the limits, on these tiny buffers: refused before anything is launched or allocated
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(n_docs=2**32 - 1)),
        (E_STATE, dict(index_id=0)), (E_STATE, dict(index_id=iid + 1)),
    ]
    for code, kw in refused:
        assert raw_overlap(native, eng, **dict(good, **kw)) == (code, 0, NONE), kw
        for f in frames:
            f.untouched()
    overlap_checked(torch, native, eng, iid, low, 5, ids, off)
    for bad in (32, 96, 63, 131072, 0, -64):                                 # the option's row: a power of two from 64 to 65536
        with pytest.raises(Exception):
            eng.set_option("ng_tile", bad)
    for ok in (64, 128, 65536):
        eng.set_option("ng_tile", ok)
    overlap_checked(torch, native, eng, iid, low, 5, ids, off)


# ---------------------------------------------------------------------------
# the Tokenizer methods

def test_methods(torch, native):
    from minbpe_amd import BasicTokenizer, NgramIndex
    tok = BasicTokenizer()
    assert tok.n_overlapping_docs is None
    h_ref, roff, h_ids, off = lattice(8, 8, 13, 220)
    want = ngram_model.run(h_ref, roff, 13, h_ids, off)
    assert want[4] > 0
    for dt in (torch.int32, torch.int64):
        np_dt = np.int32 if dt == torch.int32 else np.int64
        r32, i32 = h_ref.astype(np_dt), h_ids.astype(np_dt)                 # (int32: the values wrap, on both sides alike)
        want = ngram_model.run(r32, roff, 13, i32, off)
        ref, ids = torch.from_numpy(r32).to("cuda"), torch.from_numpy(i32).to("cuda")
        index = tok.ngram_index_resident(ref, roff)
        assert isinstance(index, NgramIndex) and index.device == ids.device and index.ngram == 13 and index.id != 0
        assert (index.n_windows, index.n_distinct) == want[5:]
        del ref
        for form in (off, off.tolist(), torch.from_numpy(off).to("cuda"), torch.from_numpy(off.astype(np.int32)).to("cuda")):
            hits = tok.ngram_overlap_resident(index, ids, form)
            assert hits.dtype == torch.int64 and hits.device == ids.device and np.array_equal(hits.cpu().numpy(), want[0])
            assert tok.n_overlapping_docs == want[4]
        hits, first, ref_pos, starts = tok.ngram_overlap_resident(index, ids, off, return_first=True, return_starts=True)
        assert starts.dtype == torch.uint8 and first.dtype == ref_pos.dtype == torch.int64
        for got, x in zip((hits, first, ref_pos, starts), want):
            assert np.array_equal(got.cpu().numpy(), x)
        hits, starts = tok.ngram_overlap_resident(index, ids, off, return_starts=True, max_len=50, keep="tail")
        cut = ngram_model.run(r32, roff, 13, i32, off, 50, True)
        assert np.array_equal(hits.cpu().numpy(), cut[0]) and np.array_equal(starts.cpu().numpy(), cut[3])
        at = ref_pos.cpu().numpy()[want[0] > 0]                               # searchsorted names the reference document
        r = np.searchsorted(roff, at, side="right") - 1
        assert (r >= 0).all() and (at + 13 <= roff[r + 1]).all()
        # decontamination: the model's mask applied by select_model
        for min_hits, max_len, keep in ((1, None, "head"), (2, None, "head"), (1, 50, "tail"), (10**6, 7, "head")):
            m = ngram_model.run(r32, roff, 13, i32, off, max_len, keep == "tail")
            kept = np.flatnonzero(m[0] < min_hits)
            m_ids, m_off = select_model.select(i32, off, kept, max_len, keep == "tail")
            s_ids, s_off, s_kept, s_hits = tok.decontaminate_docs_resident(index, ids, off, min_hits=min_hits, max_len=max_len,
                                                                           keep=keep)
            assert s_ids.dtype == ids.dtype and np.array_equal(s_ids.cpu().numpy(), m_ids)
            assert np.array_equal(s_off.cpu().numpy(), m_off) and np.array_equal(s_kept.cpu().numpy(), kept)
            assert np.array_equal(s_hits.cpu().numpy(), m[0]) and tok.n_overlapping_docs == m[4]
    # one document when no offsets come; ids on the host: numpy in, numpy out; an index or a reference
    want = ngram_model.run(h_ref, [0, len(h_ref)], 2, h_ids, off)
    index = tok.ngram_index(h_ref.tolist(), ngram=2)
    assert (index.n_windows, index.n_distinct) == want[5:] and index.n_windows == len(h_ref) - 1
    got = tok.ngram_overlap(index, h_ids, off, return_first=True)
    assert all(isinstance(g, np.ndarray) and np.array_equal(g, x) for g, x in zip(got, want[:3]))
    got = tok.ngram_overlap(h_ref, h_ids.tolist(), off.tolist(), ngram=2)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want[0])
    want = ngram_model.run(h_ref, roff, 3, h_ids, off, 40)
    got = tok.ngram_overlap(h_ref, h_ids, off, ngram=3, ref_doc_offsets=roff, max_len=40, return_starts=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[3])
    # an NgramIndex of a replaced build raises; bad offsets carry their entry, on both calls
    ids = torch.from_numpy(h_ids).to("cuda")
    with pytest.raises(RuntimeError, match="index"):
        tok.ngram_overlap_resident(index, ids, off)
    with pytest.raises(RuntimeError, match="index"):
        tok.decontaminate_docs_resident(index, ids, off)
    index = tok.ngram_index(h_ref, roff)
    bad_off = off.copy()
    bad_off[5] = bad_off[4] - 1
    for call in (lambda: tok.ngram_overlap_resident(index, ids, bad_off), lambda: tok.ngram_overlap(index, h_ids, bad_off),
                 lambda: tok.ngram_index_resident(ids, bad_off), lambda: tok.ngram_index(h_ids, bad_off)):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5
    assert tok.ngram_overlap_resident(tok.ngram_index(h_ref), ids, [3]).numel() == 0
