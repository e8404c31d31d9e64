"""GPU: bpe_dup_spans_resident -- which windows of w ids of a document an earlier document of the same stream already
holds -- and bpe_keep_ids_resident -- cutting marked ids out of a stream --, through the raw C ABI, and the Tokenizer
methods on top of them, on a ctx of its own.  Every case is compared element for element, every column, every mark byte
and every counter, with dupspans_model; nothing is sampled.  Every output is framed with canaries and prefilled with a
value no result can be (d_marks with a byte no mark can be, so that an unwritten byte shows); the inputs are read back
and must be as they were.  The shapes are the smallest at which the passes can go wrong: the tile is 64 positions in
most cases, so that a few hundred ids are many tiles, a strip of a wave is 64 positions, a chunk 2048, and a window of
64 ids is as long as the tile."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import dupspans_model as model
import ngram_model
import repetition_model
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_CAP, E_LIMIT = -2, -5, -6
TAIL, ANYWHERE, DROP = 1, 2, 1
CANARY64, PREFILL64 = -0x5A5A5A5A5A5A5A5B, -777                  # (no column goes below -1)
CANARY32, PREFILL32 = -0x5A5A5A5B, -777
CANARY8, PREFILL8 = 0xA5, 0x5A                                   # (a mark is 0 .. 3)
COLUMNS = ("length", "windows", "seen", "covered", "first", "src_pos", "marks")
# the defaults are the fields' initialisers (api_ctx.hip): the fixture puts them back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
DEFAULTS = {name: int(re.search(rf"int {name} = (\d+);", _CTX).group(1)) for name in ("ds_tile", "ds_hash_bits")}
TILE_MAX = 65536
TILES = tuple(sorted({64, 256, 4096, DEFAULTS["ds_tile"], TILE_MAX}))


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def own(native):
    with native.Engine(0) as eng:
        yield eng


@pytest.fixture()
def eng(own):
    yield own
    for name, value in DEFAULTS.items():
        own.set_option(name, value)


def dtype_of(width):
    return np.int32 if width == 4 else np.int64


def wide_ids(n, width, seed):
    """n ids that use the whole width, negatives included: no two alike but by accident"""
    rng = np.random.default_rng(seed)
    if width == 4:
        return rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    return rng.integers(-2**63, 2**63, size=n, dtype=np.int64)


def alphabet(width, seed, size):
    """`size` ids of the whole width; at 64 bits each comes with a twin that differs from it only above bit 32"""
    base = wide_ids(size, width, seed)
    if width == 8:
        base = np.concatenate([base[:(size + 1) // 2], base[:size // 2] ^ np.int64(1 << 40)])
    return base


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
    """room for `count` elements of int64, int32 or uint8, prefilled, canaries before and after"""

    def __init__(self, torch, count, size=8, shift=0):
        dt, self.canary, self.prefill = {8: (torch.int64, CANARY64, PREFILL64), 4: (torch.int32, CANARY32, PREFILL32),
                                         1: (torch.uint8, CANARY8, PREFILL8)}[size]
        self.count, self.lead, self.size = count, 16 // size + shift, size
        self.buf = torch.full((self.lead + count + 16,), self.prefill, dtype=dt, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[:self.lead] = self.canary
        self.buf[self.lead + count:] = self.canary
        self.ptr = self.buf.data_ptr() + self.lead * size

    def raw(self):
        return self.buf.cpu().numpy().tobytes()

    def read(self):
        host = self.buf.cpu().numpy()
        canary = np.asarray(self.canary).astype(host.dtype)
        assert (host[:self.lead] == canary).all() and (host[self.lead + self.count:] == canary).all(), \
            "an element outside the output was written"
        return host[self.lead:self.lead + self.count]

    def untouched(self):
        assert (self.read() == np.asarray(self.prefill).astype(self.read().dtype)).all(), "the output was written"


def frames_for(torch, n, n_docs, shift=0):
    return [Frame(torch, n_docs, shift=shift) for _ in range(6)] + [Frame(torch, n, size=1, shift=shift)]


def last_error(native, engine):
    return (native._lib.bpe_last_error(engine._h) or b"").decode()


def raw_call(native, engine, d_ids, width, n, d_off, n_docs, ngram, max_len, flags, ptrs):
    """the C call itself: (rc, n_docs_seen, n_windows, n_distinct, bad_doc)"""
    ns, nw, nd, bd = C.c_uint64(4242), C.c_uint64(4243), C.c_uint64(4244), C.c_uint64(12345)
    rc = native._lib.bpe_dup_spans_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs, ngram,
                                            max_len, flags, *[C.c_void_p(p) for p in ptrs], C.byref(ns), C.byref(nw),
                                            C.byref(nd), C.byref(bd))
    return rc, ns.value, nw.value, nd.value, bd.value


def checked(torch, native, engine, ids, off, w, max_len=None, tail=False, anywhere=False, shift=0, out_shift=0,
            use=(True,) * 7, want=None, frames_out=None):
    """one call through the C ABI into framed outputs, against the model; returns the model's Stats"""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    if want is None:
        want = model.stats(ids, off, w, max_len, tail, anywhere)
    d_ids, d_off = dev_array(torch, ids, shift), dev_array(torch, off)
    assert d_ids.data_ptr() % 16 == (shift * width) % 16
    frames = frames_for(torch, len(ids), n_docs, out_shift)
    rc, n_seen, n_win, n_dis, bad = raw_call(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids),
                                             d_off.data_ptr(), n_docs, w, 0 if max_len is None else max_len,
                                             (TAIL if tail else 0) | (ANYWHERE if anywhere else 0),
                                             [f.ptr if u else 0 for f, u in zip(frames, use)])
    assert (rc, bad) == (0, NONE), last_error(native, engine)
    assert (n_seen, n_win, n_dis) == (want.n_docs_seen, want.n_windows, want.n_distinct)
    for name, f, u, x in zip(COLUMNS, frames, use, want):
        if not u:
            f.untouched()
            continue
        col = f.read()
        if not np.array_equal(col, x):
            i = int(np.flatnonzero(col != x)[0])
            d = i if name != "marks" else int(np.searchsorted(off, i, side="right")) - 1
            pytest.fail(f"{name}[{i}] = {col[i]}, the model has {x[i]} (document {d} of {n_docs}, w = {w}, max_len = {max_len}, "
                        f"tail = {tail}, anywhere = {anywhere}, shift = {shift})")
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the ids were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    if frames_out is not None:
        frames_out.extend(frames)
    return want


# ---------------------------------------------------------------------------
# the length lattice: both widths x the windows x the tile sizes x where the stream sits on its 16 bytes x both scopes

def lengths(w):
    return [0, 1, w - 1, w, w + 1, 63, 64, 65, 127, 129]


def make_doc(rng, l, width, seed, w, earlier, kind):
    """a document of l ids, one of three kinds: two or three ids (windows collide everywhere), a block said over and over
    (the same block in every such document of the stream: seen across documents and, once l >= w + its length, inside
    them), ids of the whole width with a run of an earlier document and a run of itself copied in"""
    if kind == 0:
        return alphabet(width, 11, int(rng.integers(2, 4)))[rng.integers(0, 2, size=l)]
    if kind == 1:
        block = wide_ids(w // 2 + 1, width, 12)
        return np.resize(block, l) if l else block[:0]
    d = wide_ids(l, width, seed)
    pool = [e for e in earlier if len(e) >= 2]
    for source in (pool[int(rng.integers(0, len(pool)))] if pool else d, d):
        m = int(rng.integers(1, min(l, len(source), w + 6) + 1)) if l and len(source) else 0
        if m == 0 or (source is d and l < 2 * m):
            continue
        src = int(rng.integers(0, (l - 2 * m if source is d else len(source) - m) + 1))
        dst = int(rng.integers(src + m if source is d else 0, l - m + 1))
        d[dst:dst + m] = source[src:src + m].copy()
    return d


@functools.lru_cache(maxsize=None)
def lattice(width, w, seed=1):
    """(ids, off, the model's Stats of both scopes): three documents of every length of the lattice, shuffled; strays in
    front and behind that repeat windows of the first and the last document and must not count"""
    rng = np.random.default_rng(1000 * seed + 10 * w + width)
    todo = [(l, kind) for kind in range(3) for l in lengths(w)]
    docs = []
    for i in rng.permutation(len(todo)):
        docs.append(make_doc(rng, todo[i][0], width, 100 * seed + int(i), w, docs, todo[i][1]))
    body = np.concatenate(docs)
    ids, off = stream_of(docs, width, lead=body[-(w + 1):], trail=body[:w + 1])
    return ids, off, {a: model.stats(ids, off, w, anywhere=a) for a in (False, True)}


@pytest.mark.parametrize("w", (1, 2, 13, 50, 64))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (4, 8))
def test_lattice(torch, native, eng, width, tile, w):
    eng.set_option("ds_tile", tile)
    ids, off, want = lattice(width, w)
    assert want[False].n_docs_seen >= 2 and (want[False].seen == 0).sum() > 3
    assert (want[True].seen > want[False].seen).any() and want[True].n_distinct < want[True].n_windows
    for shift in range(4):
        for anywhere in (False, True):
            checked(torch, native, eng, ids, off, w, anywhere=anywhere, shift=shift, out_shift=shift % 2, want=want[anywhere])


@pytest.mark.parametrize("width", (4, 8))
def test_max_len_cuts(torch, native, eng, width):
    eng.set_option("ds_tile", 64)
    for w, max_len, tail in ((2, 1, False), (13, 40, False), (13, 40, True), (50, 64, True), (1, 3, True), (64, 100, False)):
        ids, off, _ = lattice(width, w)
        for anywhere in (False, True):
            checked(torch, native, eng, ids, off, w, max_len=max_len, tail=tail, anywhere=anywhere, shift=1)
    # a cut that removes the earlier occurrence: the later one is no longer seen
    p, filler = wide_ids(6, width, 402), wide_ids(200, width, 403)
    a, b = np.concatenate([p, filler[:50]]), np.concatenate([filler[60:100], p, filler[100:120]])
    ids, off = stream_of([a, b, np.concatenate([filler[120:150], p])], width)
    assert checked(torch, native, eng, ids, off, 6).seen.tolist() == [0, 1, 1]
    want = checked(torch, native, eng, ids, off, 6, max_len=50, tail=True)                              # p is cut off document 0:
    assert want.seen.tolist() == [0, 0, 1] and want.src_pos[2] == off[1] + 40                           # document 1 becomes the source
    assert checked(torch, native, eng, ids, off, 6, max_len=30, tail=False).n_docs_seen == 0            # no copy is left
    want = checked(torch, native, eng, ids, off, 5, max_len=55, tail=True)                              # p1 .. p5 survive in document 0
    assert want.seen.tolist() == [0, 1, 2] and want.src_pos[1] == 1 and want.first[1] == 41   # (p0 .. p4 of document 1 is new: 2 sees both)


# ---------------------------------------------------------------------------
# seams: the two occurrences on either side of a tile, chunk or strip seam, a window across it, a covered run across it

def seamed(width, n_src, n, w, seams, lead, seed):
    """two documents: the source of n_src ids, and one of n ids, no two alike but by accident, into which runs of the
    source are copied across every seam; a seam is a position of the stream, in front of which the second document
    has `lead` positions"""
    src = wide_ids(n_src, width, seed + 1)
    d = wide_ids(n, width, seed)
    for k, S in enumerate(seams):
        s = S - lead
        d[s - w // 2 - 1:s - w // 2 + w + 1] = src[3 * k * (w + 2):3 * k * (w + 2) + w + 2]   # a seen window and its cover across the seam
        d[s + 2 * w:s + 3 * w + 2] = d[s - 4 * w - 8:s - 3 * w - 6].copy()                   # in-document: earlier below, later above
    return src, d


@pytest.mark.parametrize("width", (4, 8))
def test_seams(torch, native, eng, width):
    for tile, n, w, seams in ((64, 700, 2, (320, 384, 448)), (64, 900, 5, (384, 448, 576)), (256, 1400, 5, (512, 576, 768, 1024)),
                              (4096, 4200, 5, (2048, 4096)), (4096, 4200, 13, (2048, 4096, 1216)),
                              (TILE_MAX, 4200, 13, (2048, 4096))):
        eng.set_option("ds_tile", tile)
        # the window passes count from the 16-byte boundary (position + shift), the cover pass from position 0
        for shift in (0, 3 if width == 4 else 1):
            for units in (0, shift):
                lead = n // 4 + 7
                src, d = seamed(width, n // 4, n - lead, w, [S - units for S in seams], lead, 300 + tile + w)
                ids, off = stream_of([src[:7], src, d], width)
                assert off[2] == lead and len(ids) == n
                for anywhere in (False, True):
                    want = checked(torch, native, eng, ids, off, w, anywhere=anywhere, shift=shift)
                    assert want.seen[2] >= (3 + 3 * anywhere) * len(seams)
                    assert want.covered[2] >= (w + 2) * len(seams)
                    s = seams[0] - units
                    assert want.marks[s - w // 2 - 1] == 3 and want.marks[s - 1] & 2 and want.marks[s] & 2
                # the source BEHIND the document: in the default scope nothing of it is seen in front
                ids, off = stream_of([d, src], width, lead=wide_ids(lead, width, 299))
                want = checked(torch, native, eng, ids, off, w, shift=shift)
                assert want.seen[0] == 0 and want.seen[1] >= 3 * len(seams)


# ---------------------------------------------------------------------------
# document boundaries

def test_document_boundaries(torch, native, eng):
    eng.set_option("ds_tile", 64)
    for width in (4, 8):
        a = wide_ids(40, width, 400)
        # identical neighbours: every window of a copy is seen, none of the first
        ids, off = stream_of([a, a, a, a[:5], a[:5]], width)
        for w in (1, 3, 40):
            want = checked(torch, native, eng, ids, off, w)
            assert want.seen.tolist() == [0, 41 - w, 41 - w, max(0, 6 - w), max(0, 6 - w)]
            assert want.src_pos.tolist()[:3] == [-1, 0, 0]
            assert checked(torch, native, eng, ids, off, w, anywhere=True).seen.tolist() == want.seen.tolist()
        # a window that exists only across two documents is not seen
        b = wide_ids(30, width, 401)
        ids, off = stream_of([b[:10], b[10:20], np.concatenate([b[20:25], b[8:12], b[25:]])], width)
        assert checked(torch, native, eng, ids, off, 3).n_docs_seen == 0
        assert checked(torch, native, eng, ids, off, 2).seen.tolist() == [0, 0, 2]    # (b8 b9 and b10 b11 do stand in one document)
        # the window stands twice in this document and once in an earlier one; then only in this one; then in a later one
        p = wide_ids(4, width, 402)
        twice = np.concatenate([b[:7], p, b[7:15], p, b[15:20]])
        for docs, seen_default, seen_anywhere in (([np.concatenate([b[20:25], p]), twice], [0, 2], [0, 2]),
                                                  ([b[20:29], twice], [0, 0], [0, 1]),
                                                  ([twice, np.concatenate([p, b[20:25]])], [0, 1], [1, 1])):
            ids, off = stream_of(docs, width, lead=p, trail=p)
            assert checked(torch, native, eng, ids, off, 4).seen.tolist() == seen_default
            assert checked(torch, native, eng, ids, off, 4, anywhere=True).seen.tolist() == seen_anywhere


@pytest.mark.parametrize("width", (4, 8))
def test_one_id_three_thousand_times(torch, native, eng, width):
    ids, off = stream_of([wide_ids(5, width, 500), np.full(1400, -7), wide_ids(70, width, 501), np.full(1600, -7)], width)
    for tile in (64, DEFAULTS["ds_tile"]):
        eng.set_option("ds_tile", tile)
        for w in (1, 64):
            want = checked(torch, native, eng, ids, off, w)
            assert (want.seen[1], want.seen[3], want.covered[3], want.first[3], want.src_pos[3]) == (0, 1601 - w, 1600, 0, 5)
            want = checked(torch, native, eng, ids, off, w, anywhere=True)
            assert (want.seen[1], want.covered[1], want.first[1], want.src_pos[1]) == (1400 - w, 1399, 1, 5)


@pytest.mark.parametrize("width", (4, 8))
def test_many_documents_in_a_tile_and_one_over_all(torch, native, eng, width):
    rng = np.random.default_rng(520)
    two = alphabet(width, 521, 2)
    small = [two[rng.integers(0, 2, size=int(rng.integers(1, 4)))] for _ in range(1800)]  # ~3,600 ids: the search unstaged
    long = wide_ids(3000, width, 522)
    long[1000:1040] = long[100:140]
    for tile in (4096, TILE_MAX):
        eng.set_option("ds_tile", tile)
        ids, off = stream_of(small + [long, long[2000:2100]], width, lead=two)
        for w in (1, 2):
            assert checked(torch, native, eng, ids, off, w, shift=1).n_docs_seen > 100
    for tile in (64, 256):
        eng.set_option("ds_tile", tile)
        ids, off = stream_of([long[140:200], long, long[2000:2100]], width, lead=long[:9], trail=long[:9])
        for anywhere in (False, True):
            want = checked(torch, native, eng, ids, off, 5, anywhere=anywhere, shift=2 if width == 4 else 1)
            assert want.seen.tolist() == [0, 56 + 36 * anywhere, 96]


# ---------------------------------------------------------------------------
# forced collisions, equality, scheduling

@pytest.mark.parametrize("width", (4, 8))
def test_forced_collisions(torch, native, eng, width):
    rng = np.random.default_rng(530)
    docs = []
    for i, l in enumerate((40, 0, 25, 45, 3, 30, 33, 40, 30)):
        docs.append(make_doc(rng, l, width, 532 + i, 3, docs, i % 3))
    ids, off = stream_of(docs + [docs[0]], width)
    assert len(ids) <= 300                                       # (one chain: the walk is quadratic)
    eng.set_option("ds_tile", 64)
    for bits in (0, 1, 5, 33):
        eng.set_option("ds_hash_bits", bits)
        for w in (1, 3):
            for anywhere in (False, True):
                want = checked(torch, native, eng, ids, off, w, anywhere=anywhere)
                assert want.seen[-1] == 41 - w and 0 < want.n_distinct < want.n_windows
    for bad in (-1, 65):
        with pytest.raises(Exception):
            eng.set_option("ds_hash_bits", bad)


def test_equality_at_full_width(torch, native, eng):
    eng.set_option("ds_tile", 64)
    lo = np.array([5, -5, 0, 2**31 - 1, -2**31, 7], np.int64)
    docs = [lo, lo + (1 << 32), lo, lo ^ np.int64(-2**63), lo + (1 << 33), np.array([-1, -1, -1, -2, -1, -1], np.int64)]
    ids, off = stream_of(docs, 8)
    for w in (1, 2, 6):
        for anywhere in (False, True):
            want = checked(torch, native, eng, ids, off, w, anywhere=anywhere)
            assert want.seen.tolist()[:5] == [0, 0, 7 - w, 0, 0]   # only the third run repeats the first
    assert checked(torch, native, eng, ids, off, 6).marks.tolist()[:24] == [0] * 12 + [3] + [2] * 5 + [0] * 6
    ids32, off = stream_of([np.array([-1, -1, -2, 2**31 - 1], np.int32), np.array([-1, -1, -2**31, 2**31 - 1, -1, -1], np.int32)], 4)
    assert checked(torch, native, eng, ids32, off, 2).seen.tolist() == [0, 2]


def test_scheduling_independence(torch, native, eng):
    ids, off, want = lattice(8, 13, seed=2)
    for tile in (64, DEFAULTS["ds_tile"]):
        eng.set_option("ds_tile", tile)
        for anywhere in (False, True):
            runs = []
            for _ in range(3):
                frames = []
                checked(torch, native, eng, ids, off, 13, anywhere=anywhere, want=want[anywhere], frames_out=frames)
                runs.append([f.raw() for f in frames])
            assert runs[0] == runs[1] == runs[2]


# ---------------------------------------------------------------------------
# contracts

def test_null_columns_and_degenerate_sizes(torch, native, eng):
    eng.set_option("ds_tile", 64)
    ids, off, want = lattice(4, 13)
    for subset in range(1, 128):                                 # every combination that leaves an output
        anywhere = bool(subset % 3 == 0)
        checked(torch, native, eng, ids, off, 13, anywhere=anywhere, use=tuple(bool(subset >> i & 1) for i in range(7)),
                want=want[anywhere])
    # n_docs == 0: the columns stay as they were, every byte of marks is zeroed; n == 0; empty documents only; no window
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, np.array([4], np.int64))
    frames = frames_for(torch, len(ids), 4)
    assert raw_call(native, eng, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), 0, 5, 0, 0, [f.ptr for f in frames]) == (0, 0, 0, 0, NONE)
    for f in frames[:6]:
        f.untouched()
    assert (frames[6].read() == 0).all()
    assert raw_call(native, eng, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), 0, 5, 0, 0, [0] * 7) == (0, 0, 0, 0, NONE)
    checked(torch, native, eng, ids[:0], [0, 0, 0], 2)
    checked(torch, native, eng, ids, [3, 3, 3, 3], 2)
    checked(torch, native, eng, ids, [len(ids)] * 2, 1)
    same = np.resize(ids[:4], 40)
    want = checked(torch, native, eng, same, [0, 4, 4, 8, 11], 5, anywhere=True)                     # every key shorter than w
    assert not want.windows.any() and (want.first == -1).all() and want.length.tolist() == [4, 0, 4, 3]
    assert (want.n_windows, want.n_distinct) == (0, 0)
    checked(torch, native, eng, same, [0, 4, 4, 8, 11], 4)                                           # one window each: the passes run


def test_bad_offsets(torch, native, eng):
    ids, off, want = lattice(4, 13)
    n, n_docs = len(ids), len(off) - 1
    d_ids = dev_array(torch, ids)
    descends = off.copy()
    descends[3] = descends[2] - 1
    beyond = off.copy()
    beyond[4:] += n
    for bad_off, where in ((descends, 3), (beyond, 4)):
        assert select_model.check_offsets(bad_off, n) == where
        frames = frames_for(torch, n, n_docs)
        d_off = dev_array(torch, bad_off)
        assert raw_call(native, eng, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 13, 0, 0,
                        [f.ptr for f in frames]) == (E_ARG, 0, 0, 0, where)
        for f in frames:
            f.untouched()
        assert f"doc_offsets[{where}]" in last_error(native, eng)
        checked(torch, native, eng, ids, off, 13, want=want[False])      # a good call follows


def test_argument_errors(torch, native, eng):
    ids, off, want = lattice(4, 13)
    n, n_docs = len(ids), len(off) - 1
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    frames = frames_for(torch, n, n_docs)
    ptrs = [f.ptr for f in frames]
    good = dict(d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, ngram=13, max_len=0, flags=0, ptrs=ptrs)
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)), (E_ARG, dict(ngram=0)), (E_ARG, dict(ngram=65)),
        (E_ARG, dict(flags=4)), (E_ARG, dict(flags=0x80000002)), (E_ARG, dict(flags=TAIL, max_len=0)),
        (E_ARG, dict(flags=TAIL | ANYWHERE, max_len=0)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(ptrs=[0] * 7)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)),
        (E_ARG, dict(width=8, d_ids=d_ids.data_ptr() + 4)),
    ] + [(E_ARG, dict(ptrs=[p + (4 if i == k else 0) for i, p in enumerate(ptrs)])) for k in range(6)] + [
        # the limits, on these tiny buffers: refused before anything is launched or allocated
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(n_docs=2**32 - 1)),
    ]
    for code, kw in refused:
        assert raw_call(native, eng, **dict(good, **kw)) == (code, 0, 0, 0, NONE), kw
        for f in frames:
            f.untouched()
    checked(torch, native, eng, ids, off, 13, want=want[False])
    for bad in (32, 96, 63, 2 * TILE_MAX, 0, -64):               # the option's row: a power of two from 64 to the maximum
        with pytest.raises(Exception):
            eng.set_option("ds_tile", bad)
    for ok in (64, 128, TILE_MAX):
        eng.set_option("ds_tile", ok)
    checked(torch, native, eng, ids, off, 13, anywhere=True, want=want[True])


def test_other_calls_keep_their_answers(torch, native):
    with native.Engine(0) as fresh:                              # (a ctx of its own: it gets an index and a merge list)
        for name in ("ds_tile", "rp_tile", "ng_tile"):
            fresh.set_option(name, 64)
        rng = np.random.default_rng(600)
        docs = [rng.integers(0, 4, size=int(l)).astype(np.int32) for l in rng.integers(0, 80, size=30)]
        docs[7] = docs[3].copy()
        ids, off = stream_of(docs, 4)
        n, n_docs = len(ids), len(off) - 1
        d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
        ref = ids[50:90].astype(np.int64)
        d_ref, d_roff = dev_array(torch, ref), dev_array(torch, np.array([0, len(ref)], np.int64))
        iid, _, _ = fresh.ngram_index_resident(d_ref.data_ptr(), 8, len(ref), d_roff.data_ptr(), 1, 3)   # BEFORE the calls below
        index = dev_array(torch, np.arange(n_docs - 1, -1, -1, dtype=np.int64))

        def others():
            hits, first, distinct = (torch.full((n_docs,), -9, dtype=torch.int64, device="cuda") for _ in range(3))
            marks = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            n_hit = fresh.ngram_overlap_resident(iid, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, hits.data_ptr())
            n_distinct = fresh.dup_docs_resident(d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, first.data_ptr(), 0)
            n_rep = fresh.repeat_stats_resident(d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 3, d_distinct=distinct.data_ptr(),
                                                d_marks=marks.data_ptr())
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            ooff = torch.zeros(n_docs + 1, dtype=torch.int64, device="cuda")
            total = fresh.select_docs_resident(d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, index.data_ptr(), n_docs, 0, 0,
                                               out.data_ptr(), n, ooff.data_ptr())
            return [n_hit, n_distinct, n_rep, total] + [t.cpu().numpy().tobytes() for t in (hits, first, distinct, marks, out, ooff)]

        before = others()
        assert before[0] > 0 and before[1] < n_docs and before[2] > 0 and before[3] == n
        low, _ = ngram_model.index(ref, [0, len(ref)], 3)
        assert before[4] == ngram_model.overlap(low, 3, ids, off)[0].tobytes()
        assert before[7] == repetition_model.stats(ids, off, 3).marks.tobytes()
        for w in (1, 3, 64):
            checked(torch, native, fresh, ids, off, w)
            checked(torch, native, fresh, ids, off, w, anywhere=True, use=(True,) * 6 + (False,))   # (marks in the scratch)
        big = np.resize(ids, 40000)                              # (the scratch grows past every other group's)
        checked(torch, native, fresh, big, [0, 20000, 40000], 3, want=model.stats(big, [0, 20000, 40000], 3))
        checked_keep(torch, native, fresh, big, [0, 20000, 40000], (big & 1).astype(np.uint8), 1)
        assert others() == before


# ---------------------------------------------------------------------------
# bpe_keep_ids_resident

def raw_keep(native, engine, d_ids, width, n, d_off, n_docs, d_mask, bits, flags, d_out, out_cap, d_ooff):
    """the C call itself: (rc, n_out, bad_doc)"""
    no, bd = C.c_uint64(4242), C.c_uint64(12345)
    rc = native._lib.bpe_keep_ids_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs, C.c_void_p(d_mask),
                                           bits, flags, C.c_void_p(d_out), out_cap, C.c_void_p(d_ooff), C.byref(no), C.byref(bd))
    return rc, no.value, bd.value


def checked_keep(torch, native, engine, ids, off, mask, bits, drop=False, shift=0, spare=0):
    """one call into framed outputs of exactly the room it needs (+ spare), and a count-only call, against the model"""
    ids, mask = np.asarray(ids), np.asarray(mask, np.uint8)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    want, want_off = model.keep(ids, off, mask, bits, drop)
    d_ids, d_off, d_mask = dev_array(torch, ids, shift), dev_array(torch, off), dev_array(torch, mask, shift)
    for count_only in (True, False):
        out, ooff = Frame(torch, len(want) + spare, size=width, shift=shift), Frame(torch, n_docs + 1)
        rc, n_out, bad = raw_keep(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(), n_docs,
                                  d_mask.data_ptr() if len(ids) else 0, bits, DROP if drop else 0,
                                  0 if count_only else out.ptr, 0 if count_only else out.count, ooff.ptr)
        assert (rc, n_out, bad) == (0, len(want), NONE), last_error(native, engine)
        assert np.array_equal(ooff.read(), want_off)
        if count_only:
            out.untouched()
        else:
            got = out.read()
            assert np.array_equal(got[:len(want)], want) and (got[len(want):] == out.prefill).all()
    assert np.array_equal(d_ids.cpu().numpy(), ids) and np.array_equal(d_mask.cpu().numpy(), mask), "the inputs were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    return want, want_off


@pytest.mark.parametrize("width", (4, 8))
def test_keep_ids(torch, native, eng, width):
    rng = np.random.default_rng(800 + width)
    docs = [wide_ids(int(l), width, 810 + i) for i, l in enumerate((70, 0, 300, 1, 64, 900, 0, 129, 2100, 5))]
    lead, trail = wide_ids(3, width, 801), wide_ids(5, width, 802)
    ids, off = stream_of(docs, width, lead=lead, trail=trail)
    n = len(ids)
    runs = np.zeros(n, np.uint8)                                  # runs across the seams of 64, 256 and 2048 positions
    for s in (60, 250, 500, 1000, 2040, 3000):
        runs[s:s + 9] = 1
        runs[s + 20:s + 300] |= 2
    emptied = np.full(n, 3, np.uint8)                             # the first, a middle and the last document lose everything
    for d in (0, 5, 9):
        emptied[off[d]:off[d + 1]] = 0
    masks = [np.full(n, 0xFF, np.uint8), np.zeros(n, np.uint8), (np.arange(n) & 1).astype(np.uint8),
             (np.arange(n) % 3).astype(np.uint8), runs, emptied, rng.integers(0, 4, size=n).astype(np.uint8)]
    for k, mask in enumerate(masks):
        for bits in (1, 2, 3):
            for drop in (False, True):
                want, want_off = checked_keep(torch, native, eng, ids, off, mask, bits, drop, shift=(k + bits) % 4, spare=k % 2)
                if k == 5 and not drop:
                    assert want_off[1] == 0 and want_off[5] == want_off[6] and want_off[9] == want_off[10] == len(want) > 0
    want, _ = checked_keep(torch, native, eng, ids, off, masks[0], 0xFF)
    assert np.array_equal(want, ids[3:n - 5])                     # all ones: the documents, without the strays
    assert len(checked_keep(torch, native, eng, ids, off, masks[0], 0x80, drop=True)[0]) == 0
    assert len(checked_keep(torch, native, eng, ids, off, masks[1], 0xFF)[0]) == 0
    # no documents, no ids, one document over everything
    checked_keep(torch, native, eng, ids, [7], masks[0], 1)
    checked_keep(torch, native, eng, ids[:0], [0, 0], masks[0][:0], 1)
    checked_keep(torch, native, eng, ids, [0, n], masks[6], 2)


def test_keep_ids_contracts(torch, native, eng):
    ids, off = stream_of([wide_ids(100, 4, 820), wide_ids(50, 4, 821)], 4, lead=[1, 2])
    n, n_docs = len(ids), 2
    mask = (np.arange(n) % 4 != 0).astype(np.uint8)
    want, want_off = model.keep(ids, off, mask, 1)
    d_ids, d_off, d_mask = dev_array(torch, ids), dev_array(torch, off), dev_array(torch, mask)
    out, ooff = Frame(torch, n, size=4), Frame(torch, n_docs + 1)
    good = dict(d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, d_mask=d_mask.data_ptr(), bits=1,
                flags=0, d_out=out.ptr, out_cap=n, d_ooff=ooff.ptr)
    # too little room: the total comes back, the offsets are written, the output is not
    assert raw_keep(native, eng, **dict(good, out_cap=len(want) - 1)) == (E_CAP, len(want), NONE)
    out.untouched()
    assert np.array_equal(ooff.read(), want_off)
    ooff = Frame(torch, n_docs + 1)
    good["d_ooff"] = ooff.ptr
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=16)), (E_ARG, dict(bits=0)), (E_ARG, dict(bits=256)), (E_ARG, dict(flags=2)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_mask=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(d_ooff=0)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_out=out.ptr + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)),
        (E_ARG, dict(d_ooff=ooff.ptr + 4)),
        # the output over the ids: at their start, inside them, ending in them
        (E_ARG, dict(d_out=d_ids.data_ptr())), (E_ARG, dict(d_out=d_ids.data_ptr() + 4 * (n - 1))),
        (E_ARG, dict(d_out=d_ids.data_ptr() - 4 * (n - 1))),
        (E_LIMIT, dict(n=2**32)),
    ]
    for code, kw in refused:
        assert raw_keep(native, eng, **dict(good, **kw)) == (code, 0, NONE), kw
        out.untouched()
        ooff.untouched()
    bad_off = off.copy()
    bad_off[1] = n + 1
    assert raw_keep(native, eng, **dict(good, d_off=dev_array(torch, bad_off).data_ptr())) == (E_ARG, 0, 1)
    out.untouched()
    ooff.untouched()
    assert raw_keep(native, eng, **good) == (0, len(want), NONE)
    assert np.array_equal(out.read()[:len(want)], want) and np.array_equal(ooff.read(), want_off)
    assert np.array_equal(d_ids.cpu().numpy(), ids)


# ---------------------------------------------------------------------------
# the Tokenizer methods

def planted(width, seed=700):
    """40 short documents of ids no two alike but by accident, a boilerplate block of 60 ids planted in 12 of them"""
    rng = np.random.default_rng(seed)
    block = wide_ids(60, width, seed + 1)
    docs = []
    for i in range(40):
        l = int(rng.integers(0, 5)) if i % 13 == 5 else int(rng.integers(20, 120))
        d = wide_ids(l, width, seed + 2 + i)
        if i % 10 in (2, 3, 7):
            at = int(rng.integers(0, l + 1))
            d = np.concatenate([d[:at], block, d[at:]])
        docs.append(d)
    assert sum(i % 10 in (2, 3, 7) for i in range(40)) == 12
    ids, off = stream_of(docs, width)
    return ids, off, block


def count_block(ids, block):
    ids, block = [int(x) for x in ids], [int(x) for x in block]
    return sum(ids[p:p + len(block)] == block for p in range(len(ids) - len(block) + 1))


def test_methods(torch, native):
    from minbpe_amd import BasicTokenizer, SpanDupStats
    tok = BasicTokenizer()
    assert tok.n_docs_with_duplicate_spans is None and tok.n_span_windows is None and tok.n_distinct_span_windows is None
    for width in (4, 8):
        h_ids, off, block = planted(width)
        ids = torch.from_numpy(h_ids).to("cuda")
        assert count_block(h_ids, block) == 12
        for w, scope, max_len, keep in ((50, "earlier_doc", None, "head"), (50, "anywhere", None, "head"),
                                        (13, "earlier_doc", 70, "tail"), (2, "anywhere", 70, "head")):
            want = model.stats(h_ids, off, w, max_len, keep == "tail", scope == "anywhere")
            counters = (want.n_docs_seen, want.n_windows, want.n_distinct)
            for form in (off, off.tolist(), torch.from_numpy(off).to("cuda")):
                got = tok.duplicate_spans_resident(ids, form, ngram=w, scope=scope, max_len=max_len, keep=keep, return_marks=True)
                assert isinstance(got, SpanDupStats) and got.marks.dtype == torch.uint8
                for name, g, x in zip(COLUMNS, got, want):
                    assert g.device == ids.device and np.array_equal(g.cpu().numpy(), x), name
                    assert name == "marks" or g.dtype == torch.int64
                assert (tok.n_docs_with_duplicate_spans, tok.n_span_windows, tok.n_distinct_span_windows) == counters
            assert tok.duplicate_spans_resident(ids, off, ngram=w, scope=scope, max_len=max_len, keep=keep).marks is None
            host = tok.duplicate_spans(h_ids if width == 4 else h_ids.tolist(), off, ngram=w, scope=scope, max_len=max_len,
                                       keep=keep, return_marks=True)
            assert isinstance(host, SpanDupStats)
            assert all(isinstance(g, np.ndarray) and np.array_equal(g, x) for g, x in zip(host, want))
        want = model.stats(h_ids, off, 50)
        got = tok.duplicate_spans_resident(ids, off)                       # ngram = 50, the earlier document
        assert np.array_equal(got.seen.cpu().numpy(), want.seen) and want.n_docs_seen == 11 and want.seen.sum() == 11 * 11
        src = np.searchsorted(off, want.src_pos[want.seen > 0], side="right") - 1
        assert (src == 2).all()                                            # the first planted document is the source
        # keep_ids: this call's marks, repetition's marks and the overlap's starts as they are; a bool mask; out
        marks = tok.duplicate_spans_resident(ids, off, return_marks=True).marks
        rep = tok.repetition_resident(ids, off, ngram=2, return_marks=True).marks
        index = tok.ngram_index_resident(torch.from_numpy(block).to("cuda"), ngram=13)
        starts = tok.ngram_overlap_resident(index, ids, off, return_starts=True)[-1]
        assert starts.dtype == torch.uint8 and int(starts.sum()) == 12 * 48
        for mask, kw in ((marks, dict(bits=2, drop=True)), (marks, dict(bits=1)), (marks, dict()), (rep, dict(bits=2)),
                         (starts, dict()), (marks.to(torch.bool), dict(drop=True)), (marks > 1, dict(bits=2))):
            h_mask = mask.cpu().numpy().astype(np.uint8)
            m_ids, m_off = model.keep(h_ids, off, h_mask, 1 if mask.dtype == torch.bool else kw.get("bits", 0xFF), kw.get("drop", False))
            k_ids, k_off = tok.keep_ids_resident(ids, off, mask, **kw)
            assert k_ids.dtype == ids.dtype and k_off.dtype == torch.int64 and k_ids.device == ids.device == k_off.device
            assert np.array_equal(k_ids.cpu().numpy(), m_ids) and np.array_equal(k_off.cpu().numpy(), m_off)
            room = torch.full((len(h_ids) + 3,), -1, dtype=ids.dtype, device="cuda")
            k_ids, k_off = tok.keep_ids_resident(ids, torch.from_numpy(off).to("cuda"), mask, out=room, **kw)
            assert np.array_equal(k_ids.cpu().numpy(), m_ids) and (len(m_ids) == 0 or k_ids.data_ptr() == room.data_ptr())
            assert (room[len(m_ids):] == -1).all()
            h_ids2, h_off2 = tok.keep_ids(h_ids if width == 4 else h_ids.tolist(), off, h_mask if mask.dtype != torch.bool
                                          else h_mask.astype(bool), **kw)
            assert isinstance(h_ids2, np.ndarray) and h_ids2.dtype == h_ids.dtype
            assert np.array_equal(h_ids2, m_ids) and np.array_equal(h_off2, m_off)
        if len(marks) > 1:
            with pytest.raises(ValueError, match="out holds"):
                tok.keep_ids_resident(ids, off, marks, out=torch.empty(1, dtype=ids.dtype, device="cuda"))
        # drop_duplicate_spans: the model's marks followed by the model's keep; the block survives exactly once
        for scope in ("earlier_doc", "anywhere"):
            want = model.stats(h_ids, off, 50, anywhere=scope == "anywhere")
            m_ids, m_off = model.keep(h_ids, off, want.marks, 2, drop=True)
            s_ids, s_off, s_stats = tok.drop_duplicate_spans_resident(ids, off, scope=scope)
            assert s_ids.dtype == ids.dtype and np.array_equal(s_ids.cpu().numpy(), m_ids) and np.array_equal(s_off.cpu().numpy(), m_off)
            assert isinstance(s_stats, SpanDupStats) and all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(s_stats, want))
            assert count_block(m_ids, block) == 1 and len(m_ids) == len(h_ids) - 11 * 60
            assert np.array_equal(np.diff(off) - np.diff(m_off), want.covered)         # covered: what each document lost
            assert (tok.n_docs_with_duplicate_spans, tok.n_span_windows, tok.n_distinct_span_windows) == \
                (want.n_docs_seen, want.n_windows, want.n_distinct) == (11, want.n_windows, want.n_windows - 11 * 11)
        s_ids, s_off, _ = tok.drop_duplicate_spans_resident(ids, off, ngram=13, out=torch.empty_like(ids))
        m_ids, m_off = model.keep(h_ids, off, model.stats(h_ids, off, 13).marks, 2, drop=True)
        assert np.array_equal(s_ids.cpu().numpy(), m_ids) and np.array_equal(s_off.cpu().numpy(), m_off)
    bad_off = off.copy()
    bad_off[5] = bad_off[4] - 1
    for call in (lambda: tok.duplicate_spans_resident(ids, bad_off), lambda: tok.duplicate_spans(h_ids, bad_off),
                 lambda: tok.keep_ids_resident(ids, bad_off, marks), lambda: tok.keep_ids(h_ids, bad_off, marks.cpu().numpy()),
                 lambda: tok.drop_duplicate_spans_resident(ids, bad_off)):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5
    assert tok.duplicate_spans_resident(ids, [3]).length.numel() == 0
    k_ids, k_off = tok.keep_ids_resident(ids, [3], marks)
    assert k_ids.numel() == 0 and k_off.tolist() == [0]
