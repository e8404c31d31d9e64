"""GPU: bpe_repeat_stats_resident -- how often the windows of w ids of a document occur again inside the same document --
through the raw C ABI, and the Tokenizer methods on top of it, on a ctx of its own.  Every case is compared element for
element, every column and every mark byte, with repetition_model; nothing is sampled.  Every output is framed with
canaries and prefilled with a value no result can be (d_marks with a byte no mark can be, so that an unwritten byte
shows); the inputs are read back and must be as they were.  The shapes are the smallest at which the passes can go
wrong: the tile is 64 positions in most cases, so that a few hundred ids are many tiles, a strip of a wave is 64
positions, a chunk 2048, and a window of 64 ids is as long as the tile."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import ngram_model
import repetition_model as model
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_LIMIT = -2, -6
TAIL = 1
CANARY64, PREFILL64 = -0x5A5A5A5A5A5A5A5B, -777                  # (no column goes below -1)
CANARY8, PREFILL8 = 0xA5, 0x5A                                   # (a mark is 0 .. 3)
COLUMNS = ("length", "windows", "distinct", "covered", "top_count", "top_pos", "marks")
# the defaults are the fields' initialisers (api_ctx.hip): the fixture puts them back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
DEFAULTS = {name: int(re.search(rf"int {name} = (\d+);", _CTX).group(1)) for name in ("rp_tile", "rp_hash_bits")}
TILE_MAX = 65536
TILES = tuple(sorted({64, 256, 4096, DEFAULTS["rp_tile"], TILE_MAX}))


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
    """room for `count` elements of int64 or uint8, prefilled, canaries before and after"""

    def __init__(self, torch, count, wide=True, shift=0):
        dt, self.canary, self.prefill = (torch.int64, CANARY64, PREFILL64) if wide else (torch.uint8, CANARY8, PREFILL8)
        self.count, self.lead = count, (2 if wide else 16) + shift
        self.buf = torch.full((self.lead + count + 16,), self.prefill, dtype=dt, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[:self.lead] = self.canary
        self.buf[self.lead + count:] = self.canary
        self.ptr = self.buf.data_ptr() + self.lead * (8 if wide else 1)

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
    return [Frame(torch, n_docs, shift=shift) for _ in range(6)] + [Frame(torch, n, wide=False, shift=shift)]


def last_error(native, engine):
    return (native._lib.bpe_last_error(engine._h) or b"").decode()


def raw_call(native, engine, d_ids, width, n, d_off, n_docs, ngram, max_len, flags, ptrs):
    """the C call itself: (rc, n_repeat_docs, bad_doc)"""
    nr, bd = C.c_uint64(4242), C.c_uint64(12345)
    rc = native._lib.bpe_repeat_stats_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs, ngram,
                                               max_len, flags, *[C.c_void_p(p) for p in ptrs], C.byref(nr), C.byref(bd))
    return rc, nr.value, bd.value


def checked(torch, native, engine, ids, off, w, max_len=None, tail=False, shift=0, out_shift=0, use=(True,) * 7, want=None,
            frames_out=None):
    """one call through the C ABI into framed outputs, against the model; returns the model's Stats"""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    if want is None:
        want = model.stats(ids, off, w, max_len, tail)
    d_ids, d_off = dev_array(torch, ids, shift), dev_array(torch, off)
    assert d_ids.data_ptr() % 16 == (shift * width) % 16
    frames = frames_for(torch, len(ids), n_docs, out_shift)
    rc, n_rep, bad = raw_call(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(), n_docs, w,
                              0 if max_len is None else max_len, TAIL if tail else 0,
                              [f.ptr if u else 0 for f, u in zip(frames, use)])
    assert (rc, bad) == (0, NONE), last_error(native, engine)
    assert n_rep == want.n_repeat_docs
    for name, f, u, x in zip(COLUMNS, frames, use, want):
        if not u:
            f.untouched()
            continue
        col = f.read()
        if not np.array_equal(col, x):
            i = int(np.flatnonzero(col != x)[0])
            d = i if name != "marks" else int(np.searchsorted(off, i, side="right")) - 1
            pytest.fail(f"{name}[{i}] = {col[i]}, the model has {x[i]} (document {d} of {n_docs}, w = {w}, max_len = {max_len}, "
                        f"tail = {tail}, shift = {shift})")
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the ids were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    if frames_out is not None:
        frames_out.extend(frames)
    return want


# ---------------------------------------------------------------------------
# the length lattice: both widths x the windows x the tile sizes x where the stream sits on its 16 bytes

def lengths(w):
    return [0, 1, w - 1, w, w + 1, 2 * w, 63, 64, 65, 257]


def make_doc(rng, l, width, seed, w):
    """a document of l ids, one of: two or three ids (repeats everywhere), a block said over and over, ids of the whole
    width with runs of itself copied further back"""
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return alphabet(width, seed, int(rng.integers(2, 4)))[rng.integers(0, 2, size=l)]
    if kind == 1:
        block = wide_ids(int(rng.integers(1, w + 3)), width, seed)
        return np.resize(block, l) if l else block[:0]
    d = wide_ids(l, width, seed)
    for _ in range(3):
        m = int(rng.integers(1, min(l, 2 * w + 2) + 1)) if l else 0
        if m == 0 or l < 2 * m:
            continue
        src = int(rng.integers(0, l - 2 * m + 1))
        dst = int(rng.integers(src + 1, l - m + 1))
        d[dst:dst + m] = d[src:src + m].copy()
    return d


@functools.lru_cache(maxsize=None)
def lattice(width, w, seed=1):
    """(ids, off, the model's Stats): three documents of every length of the lattice, shuffled; strays in front and
    behind that repeat windows of the first and the last document and must not count"""
    rng = np.random.default_rng(1000 * seed + 10 * w + width)
    docs = [make_doc(rng, l, width, 100 * seed + 7 * i + k, w) for k in range(3) for i, l in enumerate(lengths(w))]
    docs = [docs[i] for i in rng.permutation(len(docs))]
    body = np.concatenate(docs)
    ids, off = stream_of(docs, width, lead=body[:w + 1], trail=body[-(w + 1):])
    return ids, off, model.stats(ids, off, w)


@pytest.mark.parametrize("w", (1, 2, 5, 13, 64))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (4, 8))
def test_lattice(torch, native, eng, width, tile, w):
    eng.set_option("rp_tile", tile)
    ids, off, want = lattice(width, w)
    assert want.n_repeat_docs >= 2 and (want.distinct == want.windows).sum() > 3
    for shift in range(4):
        checked(torch, native, eng, ids, off, w, shift=shift, out_shift=shift % 2, want=want)


@pytest.mark.parametrize("width", (4, 8))
def test_lattice_cut(torch, native, eng, width):
    eng.set_option("rp_tile", 64)
    for w, max_len, tail in ((2, 1, False), (5, 40, False), (5, 40, True), (13, 64, True), (1, 3, True), (64, 200, False)):
        ids, off, _ = lattice(width, w)
        checked(torch, native, eng, ids, off, w, max_len=max_len, tail=tail, shift=1)


# ---------------------------------------------------------------------------
# seams: the two occurrences on either side of a tile, chunk or strip seam, a window across it, a covered run across it

def seamed(width, n, w, seams, lead, seed):
    """one document of n ids, no two alike but by accident, with runs copied across every seam; a seam is a position
    of the stream, in front of which the document has `lead` positions"""
    d = wide_ids(n, width, seed)
    for S in seams:
        s = S - lead
        d[s + w:s + 2 * w + 2] = d[s - 2 * w - 8:s - w - 6].copy()            # earlier below the seam, later above it
        d[s - w // 2 - 1:s - w // 2 + w + 1] = d[s - 3 * w - 14:s - 2 * w - 12].copy()  # the later window and its cover across it
    return d


@pytest.mark.parametrize("width", (4, 8))
def test_seams(torch, native, eng, width):
    for tile, n, w, seams in ((64, 400, 2, (64, 128, 256)), (64, 400, 5, (64, 192, 320)), (256, 700, 5, (64, 128, 256, 512)),
                              (4096, 5000, 5, (2048, 4096)), (4096, 5000, 13, (2048, 4096, 64)),
                              (TILE_MAX, 5000, 13, (2048, 4096))):
        eng.set_option("rp_tile", tile)
        # the window passes count from the 16-byte boundary (position + shift), the cover pass from position 0
        for shift in (0, 3 if width == 4 else 1):
            for units in (0, shift):
                d = seamed(width, n, w, [S - units for S in seams], 7, 300 + tile + w)
                ids, off = stream_of([d[:7], d, d[:9]], width)
                want = checked(torch, native, eng, ids, off, w, shift=shift)
                assert want.windows[1] - want.distinct[1] >= 2 * len(seams) and want.covered[1] >= (w + 2) * len(seams)
                s = seams[0] - units
                assert want.marks[s + w] == 3 and want.marks[s - 1] & 2 and want.marks[s] & 2


# ---------------------------------------------------------------------------
# document boundaries

def test_document_boundaries(torch, native, eng):
    eng.set_option("rp_tile", 64)
    for width in (4, 8):
        a = wide_ids(40, width, 400)
        # identical neighbours: no window of one is compared with a window of the other
        ids, off = stream_of([a, a, a, a[:5], a[:5]], width)
        for w in (1, 3, 40):
            want = checked(torch, native, eng, ids, off, w)
            assert (want.distinct == want.windows).all() and want.n_repeat_docs == 0 and not want.marks.any()
        # a window that would repeat only if it ran over its document's end
        b = wide_ids(30, width, 401)
        first = np.concatenate([b[:3], b[10:20], b[:2]])         # ... b0 b1 | b2: the next document begins with b2
        ids, off = stream_of([first, b[2:12]], width)
        want = checked(torch, native, eng, ids, off, 3)
        assert want.n_repeat_docs == 0
        assert checked(torch, native, eng, ids, off, 2).n_repeat_docs == 1   # (b0 b1 does repeat)
        # a cut that removes the earlier occurrence from the head or the later from the tail: no repeat is left
        p = wide_ids(6, width, 402)
        doc = np.concatenate([p, wide_ids(50, width, 403), p])
        ids, off = stream_of([b, doc, b], width)
        assert checked(torch, native, eng, ids, off, 6).distinct[1] == len(doc) - 6
        for max_len, tail in ((len(doc) - 1, True), (len(doc) - 1, False), (len(doc) - 6, True), (7, True), (7, False)):
            want = checked(torch, native, eng, ids, off, 6, max_len=max_len, tail=tail)
            assert want.n_repeat_docs == 0 and want.covered[1] == 0
        want = checked(torch, native, eng, ids, off, 5, max_len=len(doc) - 1, tail=True)
        assert want.distinct[1] == want.windows[1] - 1 and want.top_pos[1] == 1  # (p1 .. p5 survive the cut)


# ---------------------------------------------------------------------------
# multiplicity and ties

@pytest.mark.parametrize("width", (4, 8))
def test_one_id_three_thousand_times(torch, native, eng, width):
    ids, off = stream_of([wide_ids(5, width, 500), np.full(3000, -7), wide_ids(70, width, 501)], width)
    for tile in (64, DEFAULTS["rp_tile"]):
        eng.set_option("rp_tile", tile)
        for w in (1, 64):
            want = checked(torch, native, eng, ids, off, w)
            assert (want.top_count[1], want.distinct[1], want.covered[1], want.top_pos[1]) == (3001 - w, 1, 2999, 0)


def test_ties_pick_the_lower_first_start(torch, native, eng):
    eng.set_option("rp_tile", 64)
    x = wide_ids(300, 8, 510)
    doc = x[:200].copy()
    doc[150:153] = doc[20:23]                                    # the class of 20 and the class of 90 hold two each,
    doc[120:123] = doc[90:93]                                    # and the one that starts first ends last
    ids, off = stream_of([x[200:230], doc], 8)
    want = checked(torch, native, eng, ids, off, 3)
    assert (want.top_count[1], want.top_pos[1]) == (2, 20)
    want = checked(torch, native, eng, ids, off, 3, max_len=175, tail=True)
    assert (want.top_count[1], want.top_pos[1]) == (2, 90)       # (a position of the uncut document)
    assert (want.top_count[0], want.top_pos[0]) == (1, 0)


@pytest.mark.parametrize("width", (4, 8))
def test_many_documents_in_a_tile_and_one_over_all(torch, native, eng, width):
    rng = np.random.default_rng(520)
    two = alphabet(width, 521, 2)
    small = [two[rng.integers(0, 2, size=int(rng.integers(1, 4)))] for _ in range(1800)]  # ~3,600 ids: the search unstaged
    for tile in (4096, TILE_MAX):
        eng.set_option("rp_tile", tile)
        ids, off = stream_of(small, width, lead=two)
        for w in (1, 2):
            assert checked(torch, native, eng, ids, off, w, shift=1).n_repeat_docs > 100
    long = make_doc(rng, 3000, width, 522, 5)
    for tile in (64, 256):
        eng.set_option("rp_tile", tile)
        ids, off = stream_of([long], width, lead=long[:9], trail=long[:9])
        checked(torch, native, eng, ids, off, 5, shift=2 if width == 4 else 1)


# ---------------------------------------------------------------------------
# forced collisions, equality, scheduling

@pytest.mark.parametrize("width", (4, 8))
def test_forced_collisions(torch, native, eng, width):
    rng = np.random.default_rng(530)
    shared = make_doc(rng, 90, width, 531, 3)
    docs = [shared, shared.copy()] + [make_doc(rng, int(l), width, 532 + i, 3) for i, l in enumerate(rng.integers(0, 120, size=14))]
    ids, off = stream_of(docs + [shared], width)
    assert len(ids) <= 1500                                      # (one chain: the walk is quadratic)
    eng.set_option("rp_tile", 64)
    for bits in (0, 1, 5, 33):
        eng.set_option("rp_hash_bits", bits)
        for w in (1, 3):
            want = checked(torch, native, eng, ids, off, w)
            assert want.distinct[0] == want.distinct[1] == want.distinct[-1]  # equal windows in three documents stay apart
    for bad in (-1, 65):
        with pytest.raises(Exception):
            eng.set_option("rp_hash_bits", bad)


def test_equality_at_full_width(torch, native, eng):
    eng.set_option("rp_tile", 64)
    lo = np.array([5, -5, 0, 2**31 - 1, -2**31, 7], np.int64)
    docs = [np.concatenate([lo, lo + (1 << 32), lo, lo ^ np.int64(-2**63)]),      # only the third run repeats the first
            np.concatenate([lo + (1 << 32), lo, lo + (1 << 33)]),               # no repeat at all
            np.array([-1, -1, -1, -2, -1, -1], np.int64)]
    ids, off = stream_of(docs, 8)
    for w in (1, 2, 6):
        want = checked(torch, native, eng, ids, off, w)
        assert want.distinct[1] == want.windows[1]
    assert checked(torch, native, eng, ids, off, 6).marks.tolist()[:24] == [0] * 12 + [3] + [2] * 5 + [0] * 6
    ids32, off = stream_of([np.array([-1, -1, -2, -1, -1, 2**31 - 1, -2**31, 2**31 - 1], np.int32)], 4)
    assert checked(torch, native, eng, ids32, off, 2).distinct[0] == 6


def test_scheduling_independence(torch, native, eng):
    ids, off, want = lattice(8, 5, seed=2)
    for tile in (64, DEFAULTS["rp_tile"]):
        eng.set_option("rp_tile", tile)
        runs = []
        for _ in range(3):
            frames = []
            checked(torch, native, eng, ids, off, 5, want=want, frames_out=frames)
            runs.append([f.raw() for f in frames])
        assert runs[0] == runs[1] == runs[2]


# ---------------------------------------------------------------------------
# contracts

def test_null_columns_and_degenerate_sizes(torch, native, eng):
    eng.set_option("rp_tile", 64)
    ids, off, want = lattice(4, 5)
    for k in range(7):
        checked(torch, native, eng, ids, off, 5, use=tuple(i == k for i in range(7)), want=want)     # one alone
        checked(torch, native, eng, ids, off, 5, use=tuple(i != k for i in range(7)), want=want)     # one left out
    # n_docs == 0: the columns stay as they were, every byte of marks is zeroed; n == 0; empty documents only; no window
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, np.array([4], np.int64))
    frames = frames_for(torch, len(ids), 4)
    assert raw_call(native, eng, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), 0, 5, 0, 0, [f.ptr for f in frames]) == (0, 0, NONE)
    for f in frames[:6]:
        f.untouched()
    assert (frames[6].read() == 0).all()
    assert raw_call(native, eng, d_ids.data_ptr(), 4, len(ids), d_off.data_ptr(), 0, 5, 0, 0, [0] * 7) == (0, 0, NONE)
    checked(torch, native, eng, ids[:0], [0, 0, 0], 2)
    checked(torch, native, eng, ids, [3, 3, 3, 3], 2)
    checked(torch, native, eng, ids, [len(ids)] * 2, 1)
    want = checked(torch, native, eng, ids[:40], [0, 4, 4, 8, 11], 5)                                # every key shorter than w
    assert not want.windows.any() and (want.top_pos == -1).all() and want.length.tolist() == [4, 0, 4, 3]


def test_bad_offsets(torch, native, eng):
    ids, off, want = lattice(4, 5)
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
        assert raw_call(native, eng, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 5, 0, 0,
                        [f.ptr for f in frames]) == (E_ARG, 0, where)
        for f in frames:
            f.untouched()
        assert f"doc_offsets[{where}]" in last_error(native, eng)
        checked(torch, native, eng, ids, off, 5, want=want)      # a good call follows


def test_argument_errors(torch, native, eng):
    ids, off, want = lattice(4, 5)
    n, n_docs = len(ids), len(off) - 1
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    frames = frames_for(torch, n, n_docs)
    ptrs = [f.ptr for f in frames]
    good = dict(d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, ngram=5, max_len=0, flags=0, ptrs=ptrs)
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)), (E_ARG, dict(ngram=0)), (E_ARG, dict(ngram=65)),
        (E_ARG, dict(flags=2)), (E_ARG, dict(flags=0x80000001)), (E_ARG, dict(flags=TAIL, max_len=0)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(ptrs=[0] * 7)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)),
        (E_ARG, dict(width=8, d_ids=d_ids.data_ptr() + 4)),
    ] + [(E_ARG, dict(ptrs=[p + (4 if i == k else 0) for i, p in enumerate(ptrs)])) for k in range(6)] + [
        # the limits, on these tiny buffers: refused before anything is launched or allocated
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(n_docs=2**32 - 1)),
    ]
    for code, kw in refused:
        assert raw_call(native, eng, **dict(good, **kw)) == (code, 0, NONE), kw
        for f in frames:
            f.untouched()
    checked(torch, native, eng, ids, off, 5, want=want)
    for bad in (32, 96, 63, 2 * TILE_MAX, 0, -64):               # the option's row: a power of two from 64 to the maximum
        with pytest.raises(Exception):
            eng.set_option("rp_tile", bad)
    for ok in (64, 128, TILE_MAX):
        eng.set_option("rp_tile", ok)
    checked(torch, native, eng, ids, off, 5, want=want)


def test_other_calls_keep_their_answers(torch, native):
    with native.Engine(0) as fresh:                              # (a ctx of its own: it gets an index and a merge list)
        fresh.set_option("rp_tile", 64)
        fresh.set_option("ng_tile", 64)
        rng = np.random.default_rng(600)
        docs = [rng.integers(0, 4, size=int(l)).astype(np.int32) for l in rng.integers(0, 80, size=30)]
        docs[7] = docs[3].copy()
        ids, off = stream_of(docs, 4)
        n, n_docs = len(ids), len(off) - 1
        d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
        ref = ids[50:90].astype(np.int64)
        d_ref, d_roff = dev_array(torch, ref), dev_array(torch, np.array([0, len(ref)], np.int64))
        iid, _, _ = fresh.ngram_index_resident(d_ref.data_ptr(), 8, len(ref), d_roff.data_ptr(), 1, 3)
        fresh.project_set_merges(np.empty((0, 2), np.int32))
        index = dev_array(torch, np.arange(n_docs - 1, -1, -1, dtype=np.int64))

        def others():
            hits, first = (torch.full((n_docs,), -9, dtype=torch.int64, device="cuda") for _ in range(2))
            n_hit = fresh.ngram_overlap_resident(iid, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, hits.data_ptr())
            n_distinct = fresh.dup_docs_resident(d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, first.data_ptr(), 0)
            sig = torch.zeros(n_docs * 16, dtype=torch.int32, device="cuda")
            fresh.minhash_resident(d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, 5, 16, 0, sig.data_ptr(), sig.numel())
            counts = torch.zeros(256, dtype=torch.int64, device="cuda")
            fresh.count_resident(d_ids.data_ptr(), 4, n, counts.data_ptr(), 256)
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            ooff = torch.zeros(n_docs + 1, dtype=torch.int64, device="cuda")
            total = fresh.select_docs_resident(d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, index.data_ptr(), n_docs, 0, 0,
                                               out.data_ptr(), n, ooff.data_ptr())
            return [n_hit, n_distinct, total] + [t.cpu().numpy().tobytes() for t in (hits, first, sig, counts, out, ooff)]

        before = others()
        assert before[0] > 0 and before[1] < n_docs and before[2] == n
        low, _ = ngram_model.index(ref, [0, len(ref)], 3)
        assert before[3] == ngram_model.overlap(low, 3, ids, off)[0].tobytes()
        for w in (1, 3, 64):
            checked(torch, native, fresh, ids, off, w)
        big = np.resize(ids, 40000)                              # (the scratch grows past every other group's)
        checked(torch, native, fresh, big, [0, 40000], 3, want=model.stats(big, [0, 40000], 3))
        assert others() == before


# ---------------------------------------------------------------------------
# the Tokenizer methods

def corpus(width, seed=700):
    """a few hundred documents: random text, which no rule flags, and documents that say a boilerplate block over and over"""
    rng = np.random.default_rng(seed)
    dt = dtype_of(width)
    block = rng.integers(0, 50000, size=12).astype(dt)
    docs = []
    for i in range(300):
        l = int(rng.integers(0, 6)) if i % 23 == 0 else int(rng.integers(30, 150))  # (a short text is its own top window)
        d = rng.integers(0, 50000, size=l).astype(dt)
        if i % 5 == 0 and l >= 30:
            at = int(rng.integers(0, l - 24))
            d[at:at + 24] = np.resize(block, 24)
        if i % 17 == 0:
            d = np.resize(block[:int(rng.integers(1, 5))], l).astype(dt)
        docs.append(d)
    return stream_of(docs, width)


def test_methods(torch, native):
    from minbpe_amd import BasicTokenizer, RepetitionStats
    tok = BasicTokenizer()
    assert tok.n_repetitive_docs is None
    for width in (4, 8):
        h_ids, off = corpus(width)
        ids = torch.from_numpy(h_ids).to("cuda")
        for w, max_len, keep in ((5, None, "head"), (2, 50, "tail"), (10, 50, "head")):
            want = model.stats(h_ids, off, w, max_len, keep == "tail")
            for form in (off, off.tolist(), torch.from_numpy(off).to("cuda")):
                got = tok.repetition_resident(ids, form, ngram=w, max_len=max_len, keep=keep, return_marks=True)
                assert isinstance(got, RepetitionStats) and got.marks.dtype == torch.uint8
                for name, g, x in zip(COLUMNS, got, want):
                    assert g.device == ids.device and np.array_equal(g.cpu().numpy(), x), name
                    assert name == "marks" or g.dtype == torch.int64
            assert tok.repetition_resident(ids, off, ngram=w, max_len=max_len, keep=keep).marks is None
            host = tok.repetition(h_ids if width == 4 else h_ids.tolist(), off, ngram=w, max_len=max_len, keep=keep,
                                  return_marks=True)
            assert isinstance(host, RepetitionStats)
            assert all(isinstance(g, np.ndarray) and np.array_equal(g, x) for g, x in zip(host, want))
        assert tok.repetition_resident(ids, off).length.numel() == len(off) - 1   # ngram = 5
        # the flags: the default rules and custom ones, whole documents and cut ones
        for kw in (dict(), dict(top=((1, 0.5),), dup=()), dict(top=(), dup=[(3, 0.25), [4, 0.5]]),
                   dict(top=((2, 0),), dup=((5, .15),), max_len=40, keep="tail"), dict(max_len=30)):
            m_kw = dict(kw)
            m_kw["tail"] = m_kw.pop("keep", "head") == "tail"
            want = model.flagged(h_ids, off, **m_kw)
            got = tok.repetitive_docs_resident(ids, off, **kw)
            assert got.dtype == torch.bool and got.device == ids.device and np.array_equal(got.cpu().numpy(), want), kw
            assert tok.n_repetitive_docs == int(want.sum())
            kept = np.flatnonzero(~want)
            m_ids, m_off = select_model.select(h_ids, off, kept, m_kw.get("max_len"), m_kw["tail"])
            s_ids, s_off, s_kept, s_flag = tok.drop_repetitive_docs_resident(ids, off, **kw)
            assert s_ids.dtype == ids.dtype and np.array_equal(s_ids.cpu().numpy(), m_ids)
            assert np.array_equal(s_off.cpu().numpy(), m_off) and np.array_equal(s_kept.cpu().numpy(), kept)
            assert np.array_equal(s_flag.cpu().numpy(), want) and tok.n_repetitive_docs == int(want.sum())
        want = model.flagged(h_ids, off)
        planted = np.arange(len(off) - 1) % 17 == 0
        lens = np.diff(off)
        assert want[planted & (lens >= 12)].all() and 0 < want.sum() < len(want) // 2
        assert not want[(np.arange(len(want)) % 5 != 0) & ~planted & (lens >= 30)].any()     # random text is not flagged
        assert not want[lens == 0].any() and (lens == 0).any()
    bad_off = off.copy()
    bad_off[5] = bad_off[4] - 1
    for call in (lambda: tok.repetition_resident(ids, bad_off), lambda: tok.repetition(h_ids, bad_off),
                 lambda: tok.repetitive_docs_resident(ids, bad_off), lambda: tok.drop_repetitive_docs_resident(ids, bad_off)):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5
    assert tok.repetition_resident(ids, [3]).length.numel() == 0
