"""GPU: bpe_segment_docs_resident -- the segments (lines) of every document as an id stream of its own -- and
bpe_segment_marks_resident -- a verdict per segment back as a mark per id --, through the raw C ABI, and the Tokenizer
methods on top of them, on a ctx of its own.  Every case is compared element for element, every output, with
segments_model; nothing is sampled.  Every output is framed with canaries, sized to the element, and prefilled with a
value no result can be, so that an unwritten element and a write beyond a capacity both show; the inputs are read back
and must be as they were.  The shapes are the smallest at which the passes can go wrong: the tile is 64 positions in most
cases, so that a few hundred ids are many tiles and a run of 200 skipped ids covers whole tiles; a wave is 64 positions,
a round of a tile 256."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import dupspans_model
import minhash_model
import ngram_model
import segments_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_CAP, E_LIMIT = -2, -5, -6
BREAK, SKIP, TAG = 1, 2, 1
CANARY64, PREFILL64 = -0x5A5A5A5A5A5A5A5B, -777                  # (no offset, document or position is negative)
CANARY32, PREFILL32 = -0x5A5A5A5B, -777
CANARY8, PREFILL8 = 0xA5, 0x5A                                   # (the marks of the tests are 0 .. 9)
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
DEFAULTS = {name: int(re.search(rf"int {name} = (\d+);", _CTX).group(1)) for name in ("seg_tile", "seg_stage")}
TILES = tuple(sorted({64, 256, DEFAULTS["seg_tile"], 65536}))
LATTICE = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
# the small class table of most cases: 0 = a newline, 1 = a blank, 2 = content that ends its line, 3.. = content
NL, SP, END = 0, 1, 2
TABLE = np.array([BREAK | SKIP, SKIP, BREAK] + [0] * 13, np.uint8)


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


def stream_of(docs, width, lead=(), trail=()):
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


def last_error(native, engine):
    return (native._lib.bpe_last_error(engine._h) or b"").decode()


NAMES = ("out", "seg_offsets", "seg_doc", "src_start", "src_end", "doc_seg_offsets")   # the order of the C arguments


def raw_seg(native, engine, d_ids, width, n, d_off, n_docs, d_cls, n_cls, flags, d_out, out_cap, d_so, seg_cap, d_sd, d_ss, d_se,
            d_dso):
    """the C call itself: (rc, n_out, n_seg, bad_doc)"""
    no, ns, bd = C.c_uint64(4242), C.c_uint64(4243), C.c_uint64(12345)
    rc = native._lib.bpe_segment_docs_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs,
                                               C.c_void_p(d_cls), n_cls, flags, C.c_void_p(d_out), out_cap, C.c_void_p(d_so),
                                               seg_cap, C.c_void_p(d_sd), C.c_void_p(d_ss), C.c_void_p(d_se), C.c_void_p(d_dso),
                                               C.byref(no), C.byref(ns), C.byref(bd))
    return rc, no.value, ns.value, bd.value


def checked(torch, native, engine, ids, off, classes=TABLE, tag=False, shift=0, out_shift=0, use=(True,) * 4, want=None,
            spare=0, frames_out=None):
    """one call through the C ABI into framed outputs of exactly the needed size (+ spare), against the model.  use: which of
    seg_doc, src_start, src_end, doc_seg_offsets are given."""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    classes = np.asarray(classes, np.uint8)
    if want is None:
        want = model.segment_docs(ids, off, classes, tag)
    n_out, n_seg = len(want.out), len(want.seg_doc)
    d_ids, d_off, d_cls = dev_array(torch, ids, shift), dev_array(torch, off), dev_array(torch, classes)
    assert d_ids.data_ptr() % 16 == (shift * width) % 16
    out_cap = max(1, n_out + spare)                               # (no room at all would be a count-only call)
    frames = [Frame(torch, out_cap, size=width, shift=out_shift), Frame(torch, n_seg + spare + 1)] + \
        [Frame(torch, n_seg + spare) for _ in range(3)] + [Frame(torch, n_docs + 1)]
    ptrs = [f.ptr if u else 0 for f, u in zip(frames[2:], use)]
    rc, no, ns, bad = raw_seg(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(), n_docs,
                              d_cls.data_ptr() if len(classes) else 0, len(classes), TAG if tag else 0, frames[0].ptr, out_cap,
                              frames[1].ptr, n_seg + spare, *ptrs)
    assert (rc, bad) == (0, NONE), last_error(native, engine)
    assert (no, ns) == (n_out, n_seg)
    sizes = (n_out, n_seg + 1, n_seg, n_seg, n_seg, n_docs + 1)
    for name, f, u, m in zip(NAMES, frames, (True, True) + tuple(use), sizes):
        x = getattr(want, name)
        if not u:
            f.untouched()
            continue
        col = f.read()
        if not np.array_equal(col[:m], x):
            i = int(np.flatnonzero(col[:m] != x)[0])
            pytest.fail(f"{name}[{i}] = {col[i]}, the model has {x[i]} (n = {len(ids)}, {n_docs} documents, {n_seg} segments, "
                        f"tag = {tag}, shift = {shift})")
        assert (col[m:] == np.asarray(f.prefill).astype(col.dtype)).all(), f"{name}: written past its total"
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the ids were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    assert np.array_equal(d_cls.cpu().numpy(), classes), "the classes were written"
    if frames_out is not None:
        frames_out.extend(frames)
    return want


# ---------------------------------------------------------------------------
# the length lattice, for documents and for segments: both widths x the tile sizes x where the stream sits on its 16 bytes

def body(rng, l, width):
    """l content ids (3 .. 15; at 64 bits some lie far outside the table and some are twins of NL above bit 32)"""
    d = rng.integers(3, 16, size=l).astype(dtype_of(width))
    if width == 8 and l:
        far = rng.random(l)
        d[far < .1] = NL + (1 << 32)                              # class 0: compared at the full width
        d[far > .9] = -5
    return d


@functools.lru_cache(maxsize=None)
def lattice(width, seed=1):
    """(ids, off): a random document of every length of the lattice over the whole alphabet; a long document whose
    segments have every length of the lattice, separated by a newline and blanks in growing number; strays in front and
    behind that carry BREAK and must change nothing"""
    rng = np.random.default_rng(100 * seed + width)
    docs = []
    for l in LATTICE:
        d = rng.choice(np.arange(16), size=l, p=[.08, .25, .05] + [.62 / 13] * 13).astype(dtype_of(width))
        docs.append(d)
    parts = []
    for k, l in enumerate(rng.permutation(LATTICE)):
        ends = k % 3 == 0 and l > 0                               # the last id of the segment is the one that ends it
        parts += [body(rng, int(l) - ends, width), np.full(1, END if ends else NL), np.full(k * 7 % 40, SP)]
    docs.insert(5, np.concatenate(parts).astype(dtype_of(width)))
    order = rng.permutation(len(docs))
    return stream_of([docs[i] for i in order], width, lead=[7, NL, END], trail=[END, NL, 9, 9])


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (4, 8))
def test_lattice(torch, native, eng, width, tile):
    eng.set_option("seg_tile", tile)
    ids, off = lattice(width)
    for tag in (False, True):
        want = model.segment_docs(ids, off, TABLE, tag)
        lens = set(np.diff(want.seg_offsets) - tag)
        assert set(LATTICE) - {0} <= lens and set(np.diff(off)) >= set(LATTICE)
        for shift in range(4):
            checked(torch, native, eng, ids, off, tag=tag, shift=shift, out_shift=shift % 2, want=want)


# ---------------------------------------------------------------------------
# class patterns: a start is no neighbour predicate -- runs of skipped ids of any length

@pytest.mark.parametrize("width", (4, 8))
def test_class_patterns(torch, native, eng, width):
    eng.set_option("seg_tile", 64)
    n = 300
    for pattern in ([5] * n, [SP] * n, [NL] * n, [5, SP] * (n // 2), [5, NL] * (n // 2), [END] * n, [SP, END] * (n // 2),
                    [NL, SP] * (n // 2)):
        ids, off = stream_of([pattern[:130], pattern[130:131], pattern[131:]], width)
        want = checked(torch, native, eng, ids, off, tag=True)
        checked(torch, native, eng, ids, [0, n])
    assert len(want.seg_doc) == 0 and len(want.out) == 0          # (the last pattern: separators only)
    rng = np.random.default_rng(31)
    for run in (1, 63, 64, 65, 200, 1000):
        for pad in (0, 1, 63, 64, 100):                           # where the run begins in its tile of 64
            head, tail_ = body(rng, pad + 1, width), body(rng, 5, width)
            # behind a boundary the next content starts a segment, however far away; without one it does not
            for boundary, segs in (([NL], 2), ([END], 2), ([], 1)):
                doc = np.concatenate([head, boundary, np.full(run, SP), tail_]).astype(dtype_of(width))
                for tile in (64, 256) if run in (200, 1000) or pad == 63 else (64,):
                    eng.set_option("seg_tile", tile)
                    want = checked(torch, native, eng, *stream_of([doc], width), tag=bool(pad & 1))
                    assert len(want.seg_doc) == segs
                    assert want.src_end[0] == (len(doc) if segs == 1 else len(doc) - 5)
            eng.set_option("seg_tile", 64)


# ---------------------------------------------------------------------------
# document seams

@pytest.mark.parametrize("width", (4, 8))
def test_document_seams(torch, native, eng, width):
    rng = np.random.default_rng(41)
    blanks = lambda k: np.full(k, SP)
    for tile in (64, 256):
        eng.set_option("seg_tile", tile)
        for a_len in (1, 63, 64, 65, 128, 255, 256, 257):         # the seam on a wave seam, a tile seam, and off both
            for run in (0, 1, 64, 200):
                # an open segment at a's end, then blanks and content in b: b's content starts a segment of b's own
                a, b = body(rng, a_len, width), np.concatenate([blanks(run), body(rng, 3, width)])
                want = checked(torch, native, eng, *stream_of([a, b], width), tag=True)
                assert want.seg_doc.tolist() == [0, 1] and want.src_start.tolist() == [0, a_len]
                # ... with empty documents in between, and several documents starting where b starts
                want = checked(torch, native, eng, *stream_of([a, [], [], b, [], []], width))
                assert want.seg_doc.tolist() == [0, 3] and want.doc_seg_offsets.tolist() == [0, 1, 1, 1, 2, 2, 2]
    eng.set_option("seg_tile", 64)
    # documents without a segment between documents with one; strays that carry BREAK in front and behind
    docs = [body(rng, 70, width), blanks(90), [NL] * 3, body(rng, 2, width), [], blanks(1), body(rng, 130, width), [NL]]
    for lead, trail in (((), ()), ([5, END], [NL, 6]), ([NL] * 70, [END] * 70)):
        ids, off = stream_of(docs, width, lead=lead, trail=trail)
        want = checked(torch, native, eng, ids, off, tag=True)
        assert want.seg_doc.tolist() == [0, 3, 6]
        assert want.src_start.tolist() == [off[0], off[3], off[6]] and want.src_end.tolist() == [off[1], off[4], off[7]]
    # no documents, no ids, empty documents only, one document over everything, a stream inside strays only
    ids, off = stream_of(docs, width)
    checked(torch, native, eng, ids, [7])
    checked(torch, native, eng, ids[:0], [0, 0, 0])
    checked(torch, native, eng, ids, [5, 5, 5], tag=True)
    checked(torch, native, eng, ids, [len(ids)] * 2)
    checked(torch, native, eng, ids, [0, len(ids)], tag=True)


# ---------------------------------------------------------------------------
# ids outside the table, tables of other sizes

def test_ids_outside_the_table(torch, native, eng):
    eng.set_option("seg_tile", 64)
    rng = np.random.default_rng(51)
    base = rng.choice(np.arange(16), size=700, p=[.08, .25, .05] + [.62 / 13] * 13)
    for width in (4, 8):
        ids = base.astype(dtype_of(width))
        ids[::7] = -1 - ids[::7]                                  # negative: class 0
        ids[3::11] += 16                                          # beyond the table: class 0
        if width == 8:
            ids[5::13] += 1 << 32                                 # the low 32 bits index the table: class 0 all the same
            ids[6::17] = NL - (1 << 32)
        off = [0, 100, 100, 433, 700]
        for classes in (TABLE, TABLE[:0], TABLE[:2], TABLE[:1], np.full(16, BREAK | SKIP | 0xFC, np.uint8)):
            want = checked(torch, native, eng, ids, off, classes=classes, tag=True)
        assert len(want.seg_doc) > 4                              # (only the two low bits of a class are read)
    big = np.zeros(100_000, np.uint8)
    big[99_999], big[70_000], big[65_536] = BREAK | SKIP, SKIP, BREAK
    ids = rng.choice([99_999, 70_000, 65_536, 5, 99_998, 100_000], size=900).astype(np.int32)
    want = checked(torch, native, eng, ids, [0, 450, 900], classes=big)
    assert 20 < len(want.seg_doc) < 400
    eng.set_option("seg_tile", DEFAULTS["seg_tile"])
    checked(torch, native, eng, ids.astype(np.int64), [0, 450, 900], classes=big, tag=True)


def test_tags(torch, native, eng):
    eng.set_option("seg_tile", 64)
    for width in (4, 8):
        ids, off = lattice(width)
        frames = []
        want = checked(torch, native, eng, ids, off, tag=True, frames_out=frames)
        out, so = frames[0].read(), frames[1].read()
        assert np.array_equal(out[so[:-1]], want.seg_doc) and len(want.seg_doc) > 30
        assert np.array_equal(np.delete(out[:len(want.out)], so[:-1]), model.segment_docs(ids, off, TABLE).out)


# ---------------------------------------------------------------------------
# contracts

def test_contracts(torch, native, eng):
    eng.set_option("seg_tile", 64)
    ids, off = lattice(4)
    n, n_docs = len(ids), len(off) - 1
    want = model.segment_docs(ids, off, TABLE, True)
    n_out, n_seg = len(want.out), len(want.seg_doc)
    d_ids, d_off, d_cls = dev_array(torch, ids), dev_array(torch, off), dev_array(torch, TABLE)

    def fresh():
        return [Frame(torch, n_out, size=4), Frame(torch, n_seg + 1)] + [Frame(torch, n_seg) for _ in range(3)] + \
            [Frame(torch, n_docs + 1)]

    fr = fresh()
    good = dict(d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, d_cls=d_cls.data_ptr(),
                n_cls=len(TABLE), flags=TAG, d_out=fr[0].ptr, out_cap=n_out, d_so=fr[1].ptr, seg_cap=n_seg, d_sd=fr[2].ptr,
                d_ss=fr[3].ptr, d_se=fr[4].ptr, d_dso=fr[5].ptr)
    # count-only calls: no output, or no room; the totals and the documents' segment offsets come back, nothing else
    for kw in (dict(d_out=0), dict(out_cap=0), dict(d_out=0, d_so=0, d_sd=0, d_ss=0, d_se=0)):
        assert raw_seg(native, eng, **dict(good, **kw)) == (0, n_out, n_seg, NONE), kw
        for f in fr[:5]:
            f.untouched()
        assert np.array_equal(fr[5].read(), want.doc_seg_offsets)
        fr[5] = Frame(torch, n_docs + 1)
        good["d_dso"] = fr[5].ptr
    assert raw_seg(native, eng, **dict(good, d_out=0, d_dso=0)) == (0, n_out, n_seg, NONE)
    # too little room: for the ids alone, for the segments alone, for both -- both totals, and nothing per segment
    for kw in (dict(out_cap=n_out - 1), dict(seg_cap=n_seg - 1), dict(out_cap=1, seg_cap=0)):
        assert raw_seg(native, eng, **dict(good, **kw)) == (E_CAP, n_out, n_seg, NONE), kw
        for f in fr[:5]:
            f.untouched()
    fr[5] = Frame(torch, n_docs + 1)
    good["d_dso"] = fr[5].ptr
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=16)), (E_ARG, dict(flags=2)), (E_ARG, dict(flags=TAG | 4)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(d_so=0)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_out=fr[0].ptr + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)),
        (E_ARG, dict(d_so=fr[1].ptr + 4)), (E_ARG, dict(d_sd=fr[2].ptr + 4)), (E_ARG, dict(d_ss=fr[3].ptr + 4)),
        (E_ARG, dict(d_se=fr[4].ptr + 4)), (E_ARG, dict(d_dso=fr[5].ptr + 4)),
        # the output over the ids: at their start, inside them, ending in them
        (E_ARG, dict(d_out=d_ids.data_ptr())), (E_ARG, dict(d_out=d_ids.data_ptr() + 4 * (n - 1))),
        (E_ARG, dict(d_out=d_ids.data_ptr() - 4 * (n_out - 1))),
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(n_docs=2**32 - 1)), (E_LIMIT, dict(n_cls=2**26 + 1)),
        # decided before any device work: the sizes are made up, and nothing stands behind the pointers
        (E_LIMIT, dict(n_docs=2**31 + 1, n=2**32 - 1, d_ids=4096, d_off=4096, d_cls=4096, d_out=1 << 40, d_so=8192, d_sd=0,
                       d_ss=0, d_se=0, d_dso=0)),
    ]
    for code, kw in refused:
        assert raw_seg(native, eng, **dict(good, **kw)) == (code, 0, 0, NONE), kw
        for f in fr:
            f.untouched()
    for entry, value in ((1, n + 1), (3, int(off[2]) - 1), (n_docs, n + 7)):
        bad_off = off.copy()
        bad_off[entry] = value
        assert raw_seg(native, eng, **dict(good, d_off=dev_array(torch, bad_off).data_ptr())) == (E_ARG, 0, 0, entry)
        for f in fr:
            f.untouched()
    assert raw_seg(native, eng, **good) == (0, n_out, n_seg, NONE)
    for name, f in zip(NAMES, fr):
        assert np.array_equal(f.read(), getattr(want, name)), name
    assert np.array_equal(d_ids.cpu().numpy(), ids)


@pytest.mark.parametrize("width", (4, 8))
def test_nullable_columns_and_repeats(torch, native, eng, width):
    eng.set_option("seg_tile", 64)
    ids, off = lattice(width)
    for k in range(4):
        checked(torch, native, eng, ids, off, tag=bool(k & 1), use=tuple(j != k for j in range(4)), spare=k)
    checked(torch, native, eng, ids, off, use=(False,) * 4)
    # three runs, identical bytes
    raws = []
    for _ in range(3):
        frames = []
        checked(torch, native, eng, ids, off, tag=True, frames_out=frames)
        raws.append([f.raw() for f in frames])
    assert raws[0] == raws[1] == raws[2]


# ---------------------------------------------------------------------------
# bpe_segment_marks_resident

def raw_marks(native, engine, d_start, d_end, n_seg, d_val, n, d_marks):
    bad = C.c_uint64(12345)
    rc = native._lib.bpe_segment_marks_resident(engine._h, C.c_void_p(d_start), C.c_void_p(d_end), n_seg, C.c_void_p(d_val), n,
                                                C.c_void_p(d_marks), C.byref(bad))
    return rc, bad.value


def checked_marks(torch, native, engine, start, end, val, n, shift=0):
    start, end, val = np.asarray(start, np.int64), np.asarray(end, np.int64), np.asarray(val, np.uint8)
    want, want_bad = model.segment_marks(start, end, val, n)
    d_start, d_end, d_val = dev_array(torch, start), dev_array(torch, end), dev_array(torch, val, shift % 3)
    marks = Frame(torch, n, size=1, shift=shift)
    rc, bad = raw_marks(native, engine, d_start.data_ptr() if len(start) else 0, d_end.data_ptr() if len(start) else 0,
                        len(start), d_val.data_ptr() if len(start) else 0, n, marks.ptr)
    if want_bad is None:
        assert (rc, bad) == (0, NONE), last_error(native, engine)
        got = marks.read()
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            pytest.fail(f"marks[{i}] = {got[i]}, the model has {want[i]} (n = {n}, {len(start)} ranges, shift = {shift})")
    else:
        assert (rc, bad) == (E_ARG, want_bad)
        marks.untouched()
    for d, h in ((d_start, start), (d_end, end), (d_val, val)):
        assert np.array_equal(d.cpu().numpy(), h), "an input was written"
    return want


def test_marks(torch, native, eng):
    rng = np.random.default_rng(61)
    n = 1500
    cuts = np.sort(rng.choice(np.arange(1, n), size=60, replace=False))
    tiling = (np.concatenate([[0], cuts]), np.concatenate([cuts, [n]]))                 # ranges that tile [0, n)
    gaps = (tiling[0] + rng.integers(0, 3, size=61), tiling[1])                          # ... with gaps in front
    gaps = (np.minimum(gaps[0], gaps[1]), gaps[1])
    ones = (np.arange(5, 905), np.arange(6, 906))                                        # 900 ranges of one position
    empties = (np.repeat(np.arange(0, n, 25), 20), np.repeat(np.arange(0, n, 25), 20))   # 1,200 empty ranges, 20 at a place
    mixed = (np.sort(np.concatenate([empties[0], cuts])), None)
    mixed = (mixed[0], np.concatenate([mixed[0][1:], [n]]) - (np.arange(len(mixed[0])) % 2))
    mixed = (mixed[0], np.maximum(mixed[0], mixed[1]))
    cases = [tiling, gaps, ones, empties, mixed, ([0], [n]), ([64], [n - 64]), ([63], [65]), ([], []), ([n], [n]), ([0], [0]),
             ([0, 64, 128], [64, 128, 192])]
    for tile, stage in ((64, DEFAULTS["seg_stage"]), (64, 4), (64, 0), (256, 1), (DEFAULTS["seg_tile"], 16), (65536, 4096)):
        eng.set_option("seg_tile", tile)
        eng.set_option("seg_stage", stage)
        for k, (start, end) in enumerate(cases):
            val = rng.integers(1, 10, size=len(start))
            checked_marks(torch, native, eng, start, end, val, n, shift=k % 4)
    eng.set_option("seg_tile", 64)
    assert not checked_marks(torch, native, eng, [], [], [], 777).any()                  # no range: n zeros
    checked_marks(torch, native, eng, [], [], [], 0)
    checked_marks(torch, native, eng, [0, 0], [0, 0], [3, 4], 0)
    # every kind of bad range, the first one reported, nothing written
    for start, end in (([-1, 5], [3, 9]), ([0, 5], [3, 4]), ([0, 5], [3, n + 1]), ([0, 5], [6, 9]), ([0, 9, 5], [3, 9, 9]),
                       ([0, 5, 7, 8], [3, 6, 6, 9]), ([0], [n + 1]), ([2, 1], [2, 1])):
        want = checked_marks(torch, native, eng, start, end, [1] * len(start), n)
        assert want is None
    # the ranges of a segment call tile its documents
    ids, off = lattice(4)
    seg = model.segment_docs(ids, off, TABLE)
    want = checked_marks(torch, native, eng, seg.src_start, seg.src_end, np.arange(len(seg.seg_doc)) % 7 + 1, len(ids))
    covered = np.zeros(len(ids), bool)
    for d in range(len(off) - 1):
        if seg.doc_seg_offsets[d + 1] > seg.doc_seg_offsets[d]:
            covered[off[d]:off[d + 1]] = True
    assert np.array_equal(want != 0, covered)
    # refusals before any device work
    d = dev_array(torch, np.zeros(4, np.int64))
    v, m = dev_array(torch, np.ones(4, np.uint8)), Frame(torch, 10, size=1)
    for code, args in ((E_ARG, (0, d.data_ptr(), 4, v.data_ptr(), 10, m.ptr)), (E_ARG, (d.data_ptr(), 0, 4, v.data_ptr(), 10, m.ptr)),
                       (E_ARG, (d.data_ptr(), d.data_ptr(), 4, 0, 10, m.ptr)), (E_ARG, (d.data_ptr(), d.data_ptr(), 4, v.data_ptr(), 10, 0)),
                       (E_ARG, (d.data_ptr() + 4, d.data_ptr(), 3, v.data_ptr(), 10, m.ptr)),
                       (E_LIMIT, (d.data_ptr(), d.data_ptr(), 4, v.data_ptr(), 2**32, m.ptr)),
                       (E_LIMIT, (d.data_ptr(), d.data_ptr(), 2**32, v.data_ptr(), 10, m.ptr))):
        assert raw_marks(native, eng, *args) == (code, NONE), args
        m.untouched()


def test_options(native, eng):
    for name, good, bad in (("seg_tile", (64, 128, 4096, 65536), (0, 32, 96, 97, 65536 + 64, -64)),
                            ("seg_stage", (0, 1, 4096), (-1, 4097))):
        for v in bad:
            assert native._lib.bpe_set_option(eng._h, name.encode(), v) == E_ARG, (name, v)
            assert name in last_error(native, eng)
            with pytest.raises(ValueError, match=name):
                eng.set_option(name, v)
        for v in good:
            eng.set_option(name, v)


# ---------------------------------------------------------------------------
# the Tokenizer methods

PLANTED = "read more about our cookie policy here"


@functools.lru_cache(maxsize=None)
def corpus():
    """40 documents of lines no two of which are alike; PLANTED three times inside document 7 and once each in five others"""
    rng = np.random.default_rng(71)
    words = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau".split()
    docs, serial = [], 0
    for d in range(40):
        lines = []
        for _ in range(int(rng.integers(3, 9))):
            serial += 1
            lines.append(" ".join(rng.choice(words, size=int(rng.integers(2, 8)))) + f" item {serial}")
        if d == 7:
            for at in (1, 3, 6):
                lines.insert(at, PLANTED)
        elif d in (3, 11, 19, 23, 31):
            lines.insert(int(rng.integers(0, len(lines) + 1)), PLANTED + "   ")        # blanks behind it: the same line
        sep = "\n" if d % 3 else "\n\n"
        docs.append(sep.join(lines) + ("\n" if d % 2 else ""))
    return docs


@pytest.fixture(scope="module")
def trained(torch, native):
    from minbpe_amd import RegexTokenizer
    tok = RegexTokenizer()
    docs = corpus()
    tok.train("\n".join(docs), 256 + 80)
    id_lists = [tok.encode_ordinary(d) for d in docs]
    ids, off = stream_of(id_lists, 4)
    return tok, ids, off


def test_methods(torch, native, trained):
    from minbpe_amd import LineDupStats, Segments
    tok, h_ids, off = trained
    classes = tok.segment_classes()
    assert classes.dtype == np.uint8 and len(classes) == 256 + 80 and classes[10] == 3 and classes[32] == 2
    line = [t for t in tok.encode_ordinary(PLANTED) if not classes[t] & SKIP]   # (a blank that no merge took is a token of its own)
    L = len(line)
    for width in (4, 8):
        h = h_ids.astype(dtype_of(width))
        ids = torch.from_numpy(h).to("cuda")
        # the segments, in every form of the offsets and with room of the caller's
        for tag in (False, True):
            want = model.segment_docs(h, off, classes, tag)
            for form in (off, off.tolist(), torch.from_numpy(off).to("cuda")):
                got = tok.segments_resident(ids, form, tag_docs=tag)
                assert isinstance(got, Segments) and got.ids.dtype == ids.dtype
                for name, g, x in zip(model.Segs._fields, got, want):
                    assert g.device == ids.device and np.array_equal(g.cpu().numpy(), x), name
                    assert name == "out" or g.dtype == torch.int64
                assert (tok.n_segments, tok.n_segment_ids) == (len(want.seg_doc), len(want.out))
            room = torch.full((len(h) + 50,), -1, dtype=ids.dtype, device="cuda")
            got = tok.segments_resident(ids, off, tag_docs=tag, out=room, classes=torch.from_numpy(classes).to("cuda"))
            assert got.ids.data_ptr() == room.data_ptr() and np.array_equal(got.ids.cpu().numpy(), want.out)
            assert (room[len(want.out):] == -1).all()
            host = tok.segments(h if width == 4 else h.tolist(), off, tag_docs=tag, classes=classes)
            assert all(isinstance(g, np.ndarray) and np.array_equal(g, x) for g, x in zip(host, want))
        with pytest.raises(ValueError, match="out holds"):
            tok.segments_resident(ids, off, out=torch.empty(3, dtype=ids.dtype, device="cuda"))
        # the planted line is a segment of its own, six times and three times in document 7
        seg = model.segment_docs(h, off, classes)
        bodies = [seg.out[a:b].tolist() for a, b in zip(seg.seg_offsets, seg.seg_offsets[1:])]
        assert [int(seg.seg_doc[s]) for s, b in enumerate(bodies) if b == line] == [3, 7, 7, 7, 11, 19, 23, 31]
        # the statistics: in a document, over the stream, min_len on either side of the line's length
        for scope, min_len, dups in (("in_doc", 1, 2), ("stream", 1, 7), ("in_doc", L, 2), ("stream", L, 7), ("in_doc", L + 1, 0),
                                     ("stream", L + 1, 0)):
            want, want_dup = model.line_stats(h, off, classes, scope, min_len)
            assert int(want_dup.sum()) == dups == int(want.dup_lines.sum()) and want.dup_lines[7] == (dups and (2 if scope == "in_doc" else 3))
            got = tok.duplicate_lines_resident(ids, off, scope=scope, min_len=min_len, return_marks=True)
            assert isinstance(got, LineDupStats) and got.marks.dtype == torch.uint8
            for name, g, x in zip(LineDupStats._fields, got, want):
                assert g.device == ids.device and np.array_equal(g.cpu().numpy(), x), (name, scope, min_len)
            assert (tok.n_duplicate_lines, tok.n_docs_with_duplicate_lines) == (dups, int((want.dup_lines > 0).sum()))
            assert tok.duplicate_lines_resident(ids, off, scope=scope, min_len=min_len).marks is None
            host = tok.duplicate_lines(h if width == 4 else h.tolist(), off, scope=scope, min_len=min_len, return_marks=True)
            assert all(isinstance(g, np.ndarray) and np.array_equal(g, x) for g, x in zip(host, want))
        # the flags: document 7 has 2 duplicates among its lines -- thresholds on either side of that fraction
        want, _ = model.line_stats(h, off, classes, "in_doc", 1)
        frac = want.dup_lines[7] / want.lines[7]
        for line_frac, hit in ((frac - .01, True), (frac + .01, False)):
            flagged = tok.repetitive_line_docs_resident(ids, off, line_frac=line_frac, content_frac=1.0)
            assert flagged.dtype == torch.bool and flagged.device == ids.device
            assert np.array_equal(flagged.cpu().numpy(), model.flagged(want, line_frac, 1.0))
            assert flagged.cpu().numpy().tolist() == [d == 7 and hit for d in range(40)]
        cfrac = want.dup_content[7] / want.content[7]
        for content_frac, hit in ((cfrac - .01, True), (cfrac + .01, False)):
            flagged = tok.repetitive_line_docs_resident(ids, off, line_frac=1.0, content_frac=content_frac)
            assert flagged.cpu().numpy().tolist() == [d == 7 and hit for d in range(40)]
        assert np.array_equal(tok.repetitive_line_docs_resident(ids, off).cpu().numpy(), model.flagged(want))
        # dropping: the model's marks followed by the model's keep; the planted line survives exactly once
        for scope, left in (("stream", 1), ("in_doc", 6)):
            want, _ = model.line_stats(h, off, classes, scope, 1)
            m_ids, m_off = dupspans_model.keep(h, off, want.marks, 1, drop=True)
            for out in (None, torch.empty_like(ids)):
                s_ids, s_off, s_stats = tok.drop_duplicate_lines_resident(ids, off, scope=scope, out=out)
                assert s_ids.dtype == ids.dtype and np.array_equal(s_ids.cpu().numpy(), m_ids)
                assert np.array_equal(s_off.cpu().numpy(), m_off)
                assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(s_stats, want))
            assert tok.decode([int(x) for x in m_ids]).count(PLANTED) == left
            h_ids2, h_off2, h_stats = tok.drop_duplicate_lines(h if width == 4 else h.tolist(), off, scope=scope)
            assert h_ids2.dtype == h.dtype and np.array_equal(h_ids2, m_ids) and np.array_equal(h_off2, m_off)
        # the segment stream is an (ids, doc_offsets) pair of the per-document calls
        seg = tok.segments_resident(ids, off)
        m = model.segment_docs(h, off, classes)
        sig = tok.minhash_resident(seg.ids, seg.seg_offsets, n_perm=16, ngram=3)
        assert np.array_equal(sig.cpu().numpy().reshape(-1),
                              np.asarray(minhash_model.signatures(m.out, m.seg_offsets, n_perm=16, ngram=3)).reshape(-1))
        ref = np.asarray(line, np.int64)
        index = tok.ngram_index_resident(torch.from_numpy(ref.astype(h.dtype)).to("cuda"), ngram=3)
        hits = tok.ngram_overlap_resident(index, seg.ids, seg.seg_offsets)
        want_hits = ngram_model.run(ref, [0, len(ref)], 3, m.out, m.seg_offsets)[0]
        assert np.array_equal(hits.cpu().numpy(), want_hits)
        assert [int(x) for x, b in zip(want_hits, bodies) if b == line] == [L - 2] * 8
        first = tok.duplicate_docs_resident(seg.ids, seg.seg_offsets)
        _, dup = model.line_stats(h, off, classes, "stream", 1)
        assert np.array_equal(first.cpu().numpy() != np.arange(len(dup)), dup)
        # marks of the caller's own values
        values = torch.arange(len(m.seg_doc), device="cuda").to(torch.uint8) % 5 + 1
        marks = tok.segment_marks_resident(seg, values, len(h))
        assert np.array_equal(marks.cpu().numpy(), model.segment_marks(m.src_start, m.src_end, values.cpu().numpy(), len(h))[0])
        with pytest.raises(ValueError, match="segment"):
            tok.segment_marks_resident(seg, values, len(h) - 1)
    bad_off = off.copy()
    bad_off[5] = bad_off[4] - 1
    for call in (lambda: tok.segments_resident(ids, bad_off), lambda: tok.segments(h_ids, bad_off),
                 lambda: tok.duplicate_lines_resident(ids, bad_off), lambda: tok.drop_duplicate_lines_resident(ids, bad_off),
                 lambda: tok.repetitive_line_docs_resident(ids, bad_off)):
        with pytest.raises(ValueError) as e:
            call()
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5
    empty = tok.segments_resident(ids, [3])
    assert empty.ids.numel() == 0 and empty.seg_offsets.tolist() == [0] and empty.doc_seg_offsets.tolist() == [0]
    st = tok.duplicate_lines_resident(ids, [3, 3], return_marks=True)
    assert st.lines.tolist() == [0] and not st.marks.any() and tok.n_duplicate_lines == 0
    assert tok.repetitive_line_docs_resident(ids, [3, 3]).tolist() == [False]


def test_other_calls_keep_their_answers(torch, native, trained):
    """the decode scratch is shared: a segment call between two runs of the calls that use it changes none of their answers"""
    tok, h_ids, off = trained
    ids = torch.from_numpy(h_ids).to("cuda")
    mask = (torch.arange(len(h_ids), device="cuda") % 3 != 0).to(torch.uint8)

    def others():
        first = tok.duplicate_docs_resident(ids, off)
        kept, k_off = tok.keep_ids_resident(ids, off, mask)
        counts = tok.token_counts_resident(ids)
        raw, r_off = tok.decode_batch_resident(ids, off)
        return [t.cpu().numpy().tobytes() for t in (first, kept, k_off, counts, raw, r_off)]

    before = others()
    seg = tok.segments_resident(ids, off, tag_docs=True)
    tok.segment_marks_resident(seg, torch.ones(seg.seg_doc.numel(), dtype=torch.uint8, device="cuda"), len(h_ids))
    assert others() == before
    assert bytes(tok.decode_batch_resident(ids, off)[0].cpu().numpy()).decode() == "".join(corpus())
    tok.duplicate_lines_resident(ids, off, scope="stream", return_marks=True)
    assert others() == before
