"""GPU: bpe_select_docs_resident -- which documents of an id stream that lives in HBM go on, and in what order -- and the
Tokenizer methods on top of it.  Every case is compared element for element with select_model (the definition in
NumPy); nothing is sampled.  The output is framed with canaries: one element before d_out, one after out_cap, one word
after out_offsets[m]; the inputs are read back and must be as they were.  The shapes are the smallest at which the
placement kernel can go wrong: its tile is set to 64 elements in most cases, so that a few hundred ids are many tiles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rows_model
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_CAP, E_LIMIT = -2, -5, -6
TAIL = 1
CANARY = {4: -0x5A5A5A5B, 8: -0x5A5A5A5B5A5A5A5B}
PREFILL = {4: 0x3C3C3C3D, 8: 0x3C3C3C3D3C3C3C3D}          # what an output holds before a call
OFF_CANARY, OFF_PREFILL = -0x1234567812345679, 0x0F0F0F0F0F0F0F0F
# the defaults are the fields' initialisers (api_ctx.hip): the fixture puts them back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
TILE_DEFAULT = int(re.search(r"int sel_tile = (\d+);", _CTX).group(1))
STAGE_DEFAULT = int(re.search(r"int sel_stage = (\d+);", _CTX).group(1))
TILES = (64, TILE_DEFAULT, 65536)
STAGES = (0, 4, STAGE_DEFAULT)
MIX = [0, 1, 3, 4, 5, 63, 64, 65, 257, 0, 0, 1023]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture()
def eng(engine):
    yield engine
    engine.set_option("sel_tile", TILE_DEFAULT)
    engine.set_option("sel_stage", STAGE_DEFAULT)


def settings(engine, tile, stage):
    engine.set_option("sel_tile", tile)
    engine.set_option("sel_stage", stage)


def np_dtype(width):
    return np.int32 if width == 4 else np.int64


def offsets_of(lens, lead=0):
    return np.concatenate([[lead], lead + np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def make_ids(n, width, seed):
    """n distinct-looking ids that use the whole width: a 64-bit id differs from its neighbours above bit 32 too"""
    rng = np.random.default_rng(seed)
    if width == 4:
        return rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    return rng.integers(-2**63, 2**63, size=n, dtype=np.int64)


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
    """room for cap output ids `shift` elements past a 16-byte boundary and for m + 1 offsets, prefilled, with canaries"""

    def __init__(self, torch, width, cap, m, shift=0):
        dt = torch.int32 if width == 4 else torch.int64
        per16 = 16 // width
        self.width, self.cap, self.m, self.start = width, cap, m, per16 + shift
        self.buf = torch.full((self.start + cap + 1,), PREFILL[width], dtype=dt, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.start - 1] = CANARY[width]
        self.buf[self.start + cap] = CANARY[width]
        self.off = torch.full((m + 2,), OFF_PREFILL, dtype=torch.int64, device="cuda")
        self.off[m + 1] = OFF_CANARY
        self.d_out = self.buf.data_ptr() + self.start * width
        assert self.d_out % 16 == (shift * width) % 16
        self.d_off = self.off.data_ptr()

    def read(self):
        """(out [cap], out_offsets [m + 1]) on the host, the canaries checked"""
        host, off = self.buf.cpu().numpy(), self.off.cpu().numpy()
        assert host[self.start - 1] == CANARY[self.width], "the element before d_out was written"
        assert host[self.start + self.cap] == CANARY[self.width], "the element after out_cap was written"
        assert (host[:self.start - 1] == PREFILL[self.width]).all(), "elements before d_out were written"
        assert off[self.m + 1] == OFF_CANARY, "the word after out_offsets[m] was written"
        return host[self.start:self.start + self.cap], off[:self.m + 1]

    def untouched(self, ids=True, offsets=True):
        out, off = self.read()
        if ids:
            assert (out == PREFILL[self.width]).all(), "d_out was written"
        if offsets:
            assert (off == OFF_PREFILL).all(), "d_out_offsets was written"


def raw(native, engine, d_ids, width, n, d_off, n_docs, d_index, m, max_len, flags, d_out, cap, d_ooff):
    """the C call itself: (rc, n_out, bad_doc, bad_sel)"""
    no, bd, bs = C.c_uint64(12345), C.c_uint64(12345), C.c_uint64(12345)
    rc = native._lib.bpe_select_docs_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs,
                                              C.c_void_p(d_index), m, max_len, flags, C.c_void_p(d_out), cap,
                                              C.c_void_p(d_ooff), C.byref(no), C.byref(bd), C.byref(bs))
    return rc, no.value, bd.value, bs.value


def select_checked(torch, native, engine, ids, off, index, max_len=None, tail=False, in_shift=0, out_shift=0, slack=0):
    """one selection through the C call into a framed output of exactly the total (+ slack), against the model"""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    want, want_off = select_model.select(ids, off, index, max_len, tail)
    total, m = len(want), len(index)
    d_ids, d_off, d_idx = dev_array(torch, ids, in_shift), dev_array(torch, off), dev_array(torch, index)
    fr = Frame(torch, width, total + slack, m, out_shift)
    got = raw(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(), len(off) - 1,
              d_idx.data_ptr() if m else 0, m, 0 if max_len is None else max_len, TAIL if tail else 0, fr.d_out,
              total + slack, fr.d_off)
    assert got == (0, total, NONE, NONE)
    out, out_off = fr.read()
    assert np.array_equal(out_off, want_off), f"first offset difference at {int(np.flatnonzero(out_off != want_off)[0])}"
    assert np.array_equal(out[:total], want), f"first difference at element {int(np.flatnonzero(out[:total] != want)[0])}"
    assert (out[total:] == PREFILL[width]).all(), "elements beyond the total were written"
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the input was written"
    assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_idx.cpu().numpy(), index)
    return want, want_off


# ---------------------------------------------------------------------------
# the lattice: document-length patterns x selections, the other axes pruned so that every value meets every pattern

PATTERNS = {
    "ones": [1] * 300,
    "empty": [0] * 300,
    "mix": MIX,
    "long": [12293],
    "gap": [5] + [0] * 5000 + [5],          # more starts in one tile than sel_stage holds at its maximum (4096)
}
SELECTIONS = ("identity", "reverse", "perm", "thrice", "one_x1000", "mask", "none")


def selection(name, lens, seed):
    n_docs = len(lens)
    rng = np.random.default_rng(seed)
    if name == "identity":
        return np.arange(n_docs)
    if name == "reverse":
        return np.arange(n_docs)[::-1]
    if name == "perm":
        return rng.permutation(n_docs)
    if name == "thrice":
        return np.repeat(np.arange(n_docs), 3)
    if name == "one_x1000":
        return np.full(1000, int(np.argmax(lens)))               # the longest document
    if name == "mask":
        mask = rng.random(n_docs) < 0.5
        mask[int(np.argmax(lens))] = True
        return mask
    return np.zeros(0, np.int64)


@pytest.mark.parametrize("sel_i", range(len(SELECTIONS)), ids=SELECTIONS)
@pytest.mark.parametrize("pat_i", range(len(PATTERNS)), ids=list(PATTERNS))
def test_lattice(torch, native, eng, pat_i, sel_i):
    lens = PATTERNS[list(PATTERNS)[pat_i]]
    width = (4, 8)[(sel_i + pat_i) % 2]
    tile, stage = TILES[sel_i % 3], STAGES[(sel_i // 2 + pat_i) % 3]
    settings(eng, tile, stage)
    off = offsets_of(lens)
    ids = make_ids(int(off[-1]), width, 100 + pat_i)
    index = selection(SELECTIONS[sel_i], lens, 7 * pat_i + sel_i)
    if index.dtype == np.bool_:  # the mask as the Tokenizer resolves it: nonzero on the device
        d_mask = torch.from_numpy(index).to("cuda")
        index = torch.nonzero(d_mask).reshape(-1).cpu().numpy()
    select_checked(torch, native, eng, ids, off, index)


def test_lattice_covers_every_axis():
    """the pruning rule of test_lattice: every width, tile and stage meets every pattern"""
    for p in range(len(PATTERNS)):
        seen = [set(), set(), set()]
        for s in range(len(SELECTIONS)):
            seen[0].add((s + p) % 2)
            seen[1].add(s % 3)
            seen[2].add((s // 2 + p) % 3)
        assert [len(x) for x in seen] == [2, 3, 3]


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", (4, 8))
def test_alignment(torch, native, eng, width):
    """ids 0..3 elements past a 16-byte boundary, and d_out, independently"""
    settings(eng, 64, STAGE_DEFAULT)
    off = offsets_of(MIX)
    ids = make_ids(int(off[-1]), width, 3)
    index = np.random.default_rng(4).permutation(np.repeat(np.arange(len(MIX)), 2))
    for in_shift in range(4):
        for out_shift in range(4):
            select_checked(torch, native, eng, ids, off, index, in_shift=in_shift, out_shift=out_shift)


@pytest.mark.parametrize("width", (4, 8))
@pytest.mark.parametrize("total", [64 * k + d for k in (1, 2, 3) for d in (-1, 0, 1)])
def test_tile_seams(torch, native, eng, total, width):
    settings(eng, 64, STAGE_DEFAULT)
    ids = make_ids(total + 2, width, total)
    # one long document across every seam
    select_checked(torch, native, eng, ids, [1, 1 + total], [0])
    # documents of length 1
    select_checked(torch, native, eng, ids, offsets_of([1] * total, 2), np.arange(total)[::-1])
    # a document boundary exactly on each seam: seams lie at elements 64 k - a, a = the elements d_out is past 16 bytes
    for a in (0, 1):
        lens = [min(64 - a, total)]
        while total - sum(lens) >= 64:
            lens.append(64)
        lens.append(total - sum(lens))                  # (what is left after the last seam; may be empty)
        select_checked(torch, native, eng, ids, offsets_of(lens), np.arange(len(lens)), out_shift=a)


@pytest.mark.parametrize("tail", (False, True), ids=("head", "tail"))
@pytest.mark.parametrize("max_len", (1, 2, 64, 2**40))
def test_max_len(torch, native, eng, max_len, tail):
    settings(eng, 64, 4)
    off = offsets_of(MIX, 3)
    for width in (4, 8):
        ids = make_ids(int(off[-1]) + 5, width, 11)
        index = np.concatenate([np.arange(len(MIX)), np.random.default_rng(12).permutation(len(MIX))])
        _, out_off = select_checked(torch, native, eng, ids, off, index, max_len, tail)
        got_len = np.diff(out_off)
        assert np.array_equal(got_len, np.minimum(np.asarray(MIX)[index], max_len))
        assert (got_len[np.asarray(MIX)[index] == 0] == 0).all()     # empty documents stay empty


def test_strays(torch, native, eng):
    """ids before off[0] and after off[n_docs] belong to no document: they never reach an output"""
    settings(eng, 64, STAGE_DEFAULT)
    lens = [9, 0, 70, 1, 33]
    n = 7 + sum(lens) + 9
    off = offsets_of(lens, 7)
    assert off[0] == 7 and off[-1] == n - 9
    for width, poison in ((4, -77777), (8, -7777777777777)):
        ids = np.arange(1, n + 1, dtype=np_dtype(width))
        ids[:7] = poison
        ids[n - 9:] = poison
        for index, kw in ((np.arange(5)[::-1], {}), (np.repeat(np.arange(5), 3), {}),
                          (np.arange(5), dict(max_len=40, tail=True)), (np.arange(5), dict(max_len=40))):
            want, _ = select_checked(torch, native, eng, ids, off, index, **kw)
            assert poison not in want


def test_total_beyond_one_documents_range(torch, native, eng):
    """one document of 4097 ids selected 1100 times: about 4.5 M ids from a stream of 4097"""
    settings(eng, TILE_DEFAULT, STAGE_DEFAULT)
    ids = make_ids(4097 + 4, 4, 21)
    want, want_off = select_checked(torch, native, eng, ids, [2, 2 + 4097], np.zeros(1100, np.int64))
    assert len(want) == 4097 * 1100 and want_off.dtype == np.int64 and want_off[-1] == 4097 * 1100


# ---------------------------------------------------------------------------
# errors, through the raw C call

class Case:
    """a small good case on the device, the pieces of a raw call by name"""

    def __init__(self, torch, width=4):
        self.lens = [5, 0, 70, 3, 64]
        self.off = offsets_of(self.lens, 2)
        self.ids = make_ids(int(self.off[-1]) + 3, width, 31)
        self.index = np.array([4, 0, 2, 2, 1, 3], dtype=np.int64)
        self.width = width
        self.d_ids, self.d_off, self.d_idx = (dev_array(torch, x) for x in (self.ids, self.off, self.index))
        self.want, self.want_off = select_model.select(self.ids, self.off, self.index)

    def args(self, fr, **kw):
        a = dict(d_ids=self.d_ids.data_ptr(), width=self.width, n=len(self.ids), d_off=self.d_off.data_ptr(),
                 n_docs=len(self.lens), d_index=self.d_idx.data_ptr(), m=len(self.index), max_len=0, flags=0,
                 d_out=fr.d_out, cap=fr.cap, d_ooff=fr.d_off)
        a.update(kw)
        return a


def good_call_follows(torch, native, engine, case):
    select_checked(torch, native, engine, case.ids, case.off, case.index, slack=3)


def test_bad_offsets(torch, native, eng):
    settings(eng, 64, STAGE_DEFAULT)
    case = Case(torch)
    n = len(case.ids)
    descends = case.off.copy()
    descends[3] = descends[2] - 1                      # entry 3 descends
    beyond = case.off.copy()
    beyond[4:] += n                                    # entries 4 and 5 lie beyond n
    both = descends.copy()
    both[5] = n + 1
    for off, first in ((descends, 3), (beyond, 4), (both, 3)):
        fr = Frame(torch, 4, len(case.want), len(case.index))
        d_off = dev_array(torch, off)
        assert raw(native, eng, **case.args(fr, d_off=d_off.data_ptr())) == (E_ARG, 0, first, NONE)
        assert select_model.check_offsets(off, n) == first
        fr.untouched()
        assert f"doc_offsets[{first}]" in (native._lib.bpe_last_error(eng._h) or b"").decode()
        good_call_follows(torch, native, eng, case)
    # an offsets fault is reported before an index fault
    bad_idx = dev_array(torch, np.array([9, -1, 0, 0, 0, 0], dtype=np.int64))
    fr = Frame(torch, 4, len(case.want), len(case.index))
    d_off = dev_array(torch, descends)
    assert raw(native, eng, **case.args(fr, d_off=d_off.data_ptr(), d_index=bad_idx.data_ptr())) == (E_ARG, 0, 3, NONE)
    fr.untouched()
    good_call_follows(torch, native, eng, case)


def test_bad_selections(torch, native, eng):
    settings(eng, 64, STAGE_DEFAULT)
    case = Case(torch)
    n_docs, m = len(case.lens), 700                    # (several workgroups of the length pass)
    base = np.random.default_rng(41).integers(0, n_docs, size=m)
    for value in (-1, n_docs, 2**40, -2**63, 2**63 - 1, 2**32, -2**32 + 1):
        for places in ((0,), (m - 1,), (300, 20, 699), (256, 255), (511, 512, 64)):
            index = base.copy()
            index[list(places)] = value
            d_idx = dev_array(torch, index)
            fr = Frame(torch, 4, 20000, m)
            got = raw(native, eng, **case.args(fr, d_index=d_idx.data_ptr(), m=m))
            assert got == (E_ARG, 0, NONE, min(places)), (value, places)
            with pytest.raises(select_model.BadSelection) as e:
                select_model.select(case.ids, case.off, index)
            assert e.value.index == min(places)
            fr.untouched()
    assert f"index[{64}]" in (native._lib.bpe_last_error(eng._h) or b"").decode()
    good_call_follows(torch, native, eng, case)
    # a mixture: the lowest position wins whatever its value
    index = base.copy()
    index[[100, 50, 600]] = [2**40, n_docs, -1]
    d_idx = dev_array(torch, index)
    fr = Frame(torch, 4, 20000, m)
    assert raw(native, eng, **case.args(fr, d_index=d_idx.data_ptr(), m=m)) == (E_ARG, 0, NONE, 50)
    fr.untouched()
    good_call_follows(torch, native, eng, case)


@pytest.mark.parametrize("width", (4, 8))
def test_capacity_and_count_only(torch, native, eng, width):
    settings(eng, 64, STAGE_DEFAULT)
    case = Case(torch, width)
    total, m = len(case.want), len(case.index)
    # one element short: BPE_E_CAP, the total reported, d_out untouched, the offsets written
    fr = Frame(torch, width, total - 1, m)
    assert raw(native, eng, **case.args(fr)) == (E_CAP, total, NONE, NONE)
    fr.untouched(offsets=False)
    assert np.array_equal(fr.read()[1], case.want_off)
    assert str(total) in (native._lib.bpe_last_error(eng._h) or b"").decode()
    good_call_follows(torch, native, eng, case)
    # count-only: d_out = NULL, or no room at all
    for kw in (dict(d_out=0, cap=total), dict(d_out=0, cap=0), dict(cap=0)):
        fr = Frame(torch, width, total, m)
        assert raw(native, eng, **case.args(fr, **kw)) == (0, total, NONE, NONE)
        fr.untouched(offsets=False)
        assert np.array_equal(fr.read()[1], case.want_off)
    # the empty selection: nothing but out_offsets = [0]
    fr = Frame(torch, width, 4, 0)
    assert raw(native, eng, **case.args(fr, d_index=0, m=0)) == (0, 0, NONE, NONE)
    fr.untouched(offsets=False)
    assert fr.read()[1].tolist() == [0]
    # ... and a selection of empty documents only
    d_idx = dev_array(torch, np.array([1, 1, 1], dtype=np.int64))
    fr = Frame(torch, width, 4, 3)
    assert raw(native, eng, **case.args(fr, d_index=d_idx.data_ptr(), m=3)) == (0, 0, NONE, NONE)
    fr.untouched(offsets=False)
    assert fr.read()[1].tolist() == [0, 0, 0, 0]
    good_call_follows(torch, native, eng, case)


def test_argument_errors(torch, native, eng):
    settings(eng, 64, STAGE_DEFAULT)
    case = Case(torch)
    total, m = len(case.want), len(case.index)
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)),
        (E_ARG, dict(flags=2)), (E_ARG, dict(flags=0x80000001)),
        (E_ARG, dict(flags=TAIL, max_len=0)),
        (E_ARG, dict(d_index=0)), (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(d_ooff=0)),
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(m=2**32)), (E_LIMIT, dict(n_docs=2**48)),
    ]
    for code, kw in refused:
        fr = Frame(torch, 4, total, m)
        got = raw(native, eng, **case.args(fr, **kw))
        assert got == (code, 0, NONE, NONE), kw
        fr.untouched()
        good_call_follows(torch, native, eng, case)
    # what the refusals leave legal: no ids with no documents' ids, no index with no selection
    fr = Frame(torch, 4, 4, 0)
    d_off = dev_array(torch, np.zeros(3, np.int64))
    assert raw(native, eng, **case.args(fr, d_ids=0, n=0, d_off=d_off.data_ptr(), n_docs=2, d_index=0, m=0)) == (0, 0, NONE, NONE)
    assert fr.read()[1].tolist() == [0]
    # options: the rows of the table
    for name, bad in (("sel_tile", 32), ("sel_tile", 66), ("sel_tile", 65540), ("sel_stage", -1), ("sel_stage", 4097)):
        with pytest.raises(Exception):
            eng.set_option(name, bad)
    good_call_follows(torch, native, eng, case)


# ---------------------------------------------------------------------------
# composition with the calls the selection stands in front of, and the Tokenizer methods

@pytest.fixture(scope="module")
def trained(native):
    from minbpe_amd import RegexTokenizer
    tok = RegexTokenizer()
    tok.train(native.synth_text(30_000, 61).decode(), 256 + 40)
    src = native.synth_text(40_000, 62).decode()
    rng = np.random.default_rng(5)
    texts, p = [], 0
    for i in range(60):
        k = 0 if i % 17 == 3 else int(rng.integers(1, 400))
        texts.append(src[p:p + k])
        p += k
    texts.append(" don't  stop 12345 ünïcödé 😉")
    return tok, texts


def test_composition(torch, trained):
    tok, texts = trained
    ids, doff = tok.encode_ordinary_batch_resident(texts)
    h_ids, h_off = ids.cpu().numpy(), doff.cpu().numpy()
    n_docs = len(texts)
    before = tok.decode_batch_resident(ids, doff)
    index = np.random.default_rng(8).permutation(np.repeat(np.arange(n_docs), 2))[:90]
    sel, soff = tok.select_docs_resident(ids, doff, torch.from_numpy(index).to("cuda"))
    want, want_off = select_model.select(h_ids, h_off, index)
    assert sel.dtype == ids.dtype and sel.device == ids.device and soff.dtype == torch.int64 and soff.device == ids.device
    assert np.array_equal(sel.cpu().numpy(), want) and np.array_equal(soff.cpu().numpy(), want_off)
    # select, then rows: the model's rows of the model's selected stream
    rows = tok.rows_resident(sel, soff, 48, stride=47, sep=7, pad=-100)
    assert np.array_equal(rows.cpu().numpy(), rows_model.pack(want, want_off, 48, 47, 7, -100)[0])
    # select, then decode: the joined bytes of the chosen documents
    back, boff = tok.decode_batch_resident(sel, soff)
    chosen = [texts[d].encode("utf-8") for d in index]
    assert back.cpu().numpy().tobytes() == b"".join(chosen)
    assert boff.cpu().tolist() == np.concatenate([[0], np.cumsum([len(b) for b in chosen])]).tolist()
    # the identity selection returns the input's documents
    same, same_off = tok.select_docs_resident(ids, doff, torch.arange(n_docs, device="cuda"))
    assert np.array_equal(same.cpu().numpy(), h_ids[h_off[0]:h_off[-1]])
    assert np.array_equal(same_off.cpu().numpy(), h_off - h_off[0])
    # the decode table is untouched: the same bytes before and after the select calls on the same ctx
    after = tok.decode_batch_resident(ids, doff)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert before[0].cpu().numpy().tobytes() == "".join(texts).encode("utf-8")


def test_tokenizer_methods(torch, native):
    from minbpe_amd import BasicTokenizer
    tok = BasicTokenizer()
    lens = MIX + [7, 0, 31]
    off = offsets_of(lens, 4)
    n_docs = len(lens)
    for width, dt in ((4, torch.int32), (8, torch.int64)):
        h_ids = make_ids(int(off[-1]) + 6, width, 51)
        ids = torch.from_numpy(h_ids).to("cuda")
        mask = np.random.default_rng(52).random(n_docs) < 0.6
        index = np.flatnonzero(mask)
        want, want_off = select_model.select(h_ids, off, index)
        # the mask, the device index (int64 and int32) and the host sequences agree; offsets in every form
        forms = [torch.from_numpy(mask).to("cuda"), torch.from_numpy(index).to("cuda"),
                 torch.from_numpy(index.astype(np.int32)).to("cuda"), index.tolist(), index, index.astype(np.int32), mask]
        offs = [off, off.tolist(), torch.from_numpy(off).to("cuda"), torch.from_numpy(off.astype(np.int32)).to("cuda")]
        for i, form in enumerate(forms):
            got, got_off = tok.select_docs_resident(ids, offs[i % len(offs)], form)
            assert got.dtype == dt and got.device == ids.device and got.dim() == 1
            assert got_off.dtype == torch.int64 and got_off.device == ids.device
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_off.cpu().numpy(), want_off)
        # max_len and keep
        for max_len, keep in ((3, "head"), (3, "tail"), (2**40, "tail"), (np.int64(64), "head")):
            got, got_off = tok.select_docs_resident(ids, off, index[::-1].copy(), max_len=max_len, keep=keep)
            w, w_off = select_model.select(h_ids, off, index[::-1], int(max_len), keep == "tail")
            assert np.array_equal(got.cpu().numpy(), w) and np.array_equal(got_off.cpu().numpy(), w_off)
        # out=: the result is a view of its head, the ids beyond the total are untouched
        out = torch.full((len(want) + 5,), 123456, dtype=dt, device="cuda")
        got, _ = tok.select_docs_resident(ids, off, index, out=out)
        assert got.data_ptr() == out.data_ptr() and got.numel() == len(want)
        assert np.array_equal(out.cpu().numpy()[:len(want)], want) and (out[len(want):] == 123456).all()
        with pytest.raises(ValueError, match=str(len(want))):
            tok.select_docs_resident(ids, off, index, out=out[:len(want) - 1])
        assert (out[len(want):] == 123456).all()
        with pytest.raises(ValueError):
            tok.select_docs_resident(ids, off, index, out=out[:0])
        # the empty selection
        got, got_off = tok.select_docs_resident(ids, off, [])
        assert got.numel() == 0 and got.dtype == dt and got_off.cpu().tolist() == [0]
        # ids on the host: numpy in, numpy out
        got, got_off = tok.select_docs(h_ids, off, index.tolist())
        assert isinstance(got, np.ndarray) and got.dtype == h_ids.dtype
        assert np.array_equal(got, want) and np.array_equal(got_off, want_off) and got_off.dtype == np.int64
        got, got_off = tok.select_docs(h_ids.tolist(), off.tolist(), mask, max_len=5, keep="tail")
        w, w_off = select_model.select(h_ids, off, index, 5, True)
        assert got.dtype == np.int64 and np.array_equal(got, w) and np.array_equal(got_off, w_off)
        # the exceptions' types and positions
        for bad, pos in (([0, -1, 2], 1), ([n_docs], 0), (torch.tensor([1, 2, 3, 2**40], device="cuda"), 3),
                         (np.array([0, 1, -5, n_docs]), 2)):
            with pytest.raises(IndexError) as e:
                tok.select_docs_resident(ids, off, bad)
            assert isinstance(e.value, native.BadSelection) and e.value.index == pos and f"index[{pos}]" in str(e.value)
        with pytest.raises(IndexError) as e:
            tok.select_docs(h_ids, off, [0, n_docs + 3])
        assert e.value.index == 1
        bad_off = off.copy()
        bad_off[5] = bad_off[4] - 1
        with pytest.raises(ValueError) as e:
            tok.select_docs_resident(ids, bad_off, [0])
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5 and "doc_offsets[5]" in str(e.value)
        with pytest.raises(ValueError) as e:
            tok.select_docs_resident(ids, [0, len(h_ids) + 1], [0, 7])      # offsets first
        assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 1
