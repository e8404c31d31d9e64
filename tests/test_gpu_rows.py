"""GPU: bpe_rows_resident -- a flat id stream with document offsets in HBM to fixed-length rows in HBM -- and the
tokenizer methods on top of it.  Every element of every output is compared with the definition (rows_model.py); ids are
1000 + position, so any misplaced element shows.  Every engine-level call writes into a view that starts one element
into a sentinel-filled buffer (aligned to the element, not to 16 bytes) with rows_cap == R exactly, and everything
around the R * L elements is checked afterwards, for the rows and for the companions."""
import ctypes as C

import numpy as np
import pytest

import rows_model
from helpers import toy_rank_table

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_CAP, E_LIMIT = -2, -5, -6
PACK, PER_DOC = 0, 1
HAS_SEP, TRUNC_LEFT, PAD_LEFT = 1, 2, 4
SENTINEL = -77777
SEP, PAD = 7, -1

# the pack kernel as shipped; with a tile and a staging area so small that every case spans many tiles and overflows the
# staging; and with every lane searching global memory
ROWS_DEFAULTS = {"rows_tile": 4096, "rows_stage": 1024}
FORMS = {"default": {}, "small": {"rows_tile": 64, "rows_stage": 4}, "global": {"rows_stage": 0}}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture()
def eng(engine):
    yield engine
    for k, v in ROWS_DEFAULTS.items():
        engine.set_option(k, v)


def set_form(eng, form):
    for k, v in {**ROWS_DEFAULTS, **FORMS[form]}.items():
        eng.set_option(k, v)
    return {**ROWS_DEFAULTS, **FORMS[form]}["rows_tile"]


def raw(native, engine, d_ids, n, d_off, n_docs, mode, flags, L, S, sep, pad, d_rows, width, cap, d_di=0, d_pos=0, d_len=0):
    """the C call itself: (rc, n_rows, bad_doc)"""
    nr, bad = C.c_uint64(12345), C.c_uint64(12345)
    rc = native._lib.bpe_rows_resident(engine._h, C.c_void_p(d_ids), n, C.c_void_p(d_off), n_docs, mode, flags, L, S, sep,
                                       pad, C.c_void_p(d_rows), width, cap, C.c_void_p(d_di), C.c_void_p(d_pos),
                                       C.c_void_p(d_len), C.byref(nr), C.byref(bad))
    return rc, nr.value, bad.value


def offsets_of(lens, start=0):
    return np.concatenate([[start], start + np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def guarded(torch, count, dtype):
    """(buffer, device address of the view one element in): count elements wanted, 64 more behind them"""
    buf = torch.full((1 + count + 64,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + buf.element_size()


def inside(buf, count):
    """the view's first `count` elements on the host, after checking that nothing around them was written"""
    host = buf.cpu().numpy()
    assert host[0] == SENTINEL and np.all(host[1 + count:] == SENTINEL), "elements outside [0, R L) were written"
    return host[1:1 + count].astype(np.int64)


def run_pack(torch, native, eng, ids, off, L, S, sep, pad=PAD, width=8, companions=False):
    """count, then write with rows_cap == R into guarded buffers: (rows, doc_index, pos) as int64 [R, L] (None without
    companions), the ids unchanged"""
    n, n_docs = len(ids), len(off) - 1
    d_ids = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to("cuda")
    d_off = torch.from_numpy(np.asarray(off, dtype=np.int64)).to("cuda")
    keep = d_ids.clone()
    flags = HAS_SEP if sep is not None else 0
    sepv = 0 if sep is None else sep
    torch.cuda.synchronize()
    rc, R, bad = raw(native, eng, d_ids.data_ptr(), n, d_off.data_ptr(), n_docs, PACK, flags, L, S, sepv, pad, 0, width, 0)
    assert (rc, bad) == (0, NONE), native._lib.bpe_last_error(eng._h)
    dt = torch.int32 if width == 4 else torch.int64
    rows, p_rows = guarded(torch, R * L, dt)
    assert R == 0 or p_rows % 16 != 0
    di, p_di = guarded(torch, R * L, torch.int32) if companions else (None, 0)
    ps, p_ps = guarded(torch, R * L, torch.int32) if companions else (None, 0)
    torch.cuda.synchronize()
    rc, R2, bad = raw(native, eng, d_ids.data_ptr(), n, d_off.data_ptr(), n_docs, PACK, flags, L, S, sepv, pad, p_rows,
                      width, R, p_di, p_ps)
    assert (rc, R2, bad) == (0, R, NONE), native._lib.bpe_last_error(eng._h)
    assert torch.equal(d_ids, keep), "the ids were written"
    out = [inside(rows, R * L).reshape(R, L)]
    out += [inside(t, R * L).reshape(R, L) for t in (di, ps)] if companions else [None, None]
    return out


def check_pack(torch, native, eng, ids, off, L, S, sep, pad=PAD, width=8, companions=False):
    want = rows_model.pack(ids, off, L, S, sep, pad)
    got = run_pack(torch, native, eng, ids, off, L, S, sep, pad, width, companions)
    what = f"L={L} S={S} sep={sep} width={width}"
    assert got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), what
    if companions:
        assert np.array_equal(got[1], want[1]), what + " doc_index"
        assert np.array_equal(got[2], want[2]), what + " pos"
    return want[0]


def strides_of(L):
    return sorted({L, (L + 1) // 2} | ({L - 1} if L >= 2 else set()) | ({1} if L <= 7 else set()))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [1, 2, 7, 64, 1000])
def test_length_lattice(torch, native, eng, L, form):
    tile = set_form(eng, form)
    lens = [0, 0, 1, 2, 3, L - 1, L, L + 1, 2 * L, 5 * L + 3, tile - 1, tile, tile + 1]
    np.random.default_rng(L).shuffle(lens)
    off = offsets_of(lens)
    ids = 1000 + np.arange(off[-1])
    first = True
    for S in strides_of(L):
        for sep in (None, SEP):
            for width in (4, 8):
                check_pack(torch, native, eng, ids, off, L, S, sep, width=width, companions=first)
                first = False
    # ... the companions also without a separator (empty documents own no element)
    check_pack(torch, native, eng, ids, off, L, max(L - 1, 1), None, width=4, companions=True)


@pytest.mark.parametrize("form", list(FORMS))
def test_staging_overflow(torch, native, eng, form):
    """5,000 empty documents between two real ones: 5,000 separators in a row, or nothing at all"""
    set_form(eng, form)
    off = offsets_of([300] + [0] * 5000 + [500])
    ids = 1000 + np.arange(off[-1])
    for sep in (SEP, None):
        for L, S in ((64, 64), (64, 63), (1000, 500)):
            rows = check_pack(torch, native, eng, ids, off, L, S, sep, width=4, companions=True)
            assert (rows == SEP).sum() >= (5002 if sep is not None else 0)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_long_document(torch, native, eng, form):
    set_form(eng, form)
    ids = 1000 + np.arange(300_000)
    off = [0, 300_000]
    check_pack(torch, native, eng, ids, off, 1000, 999, SEP, width=8, companions=True)
    check_pack(torch, native, eng, ids, off, 64, 64, None, width=4)


@pytest.mark.parametrize("form", list(FORMS))
def test_boundaries_on_row_ends(torch, native, eng, form):
    set_form(eng, form)
    for L in (8, 100):
        off = offsets_of([L] * 64)
        ids = 1000 + np.arange(off[-1])
        rows = check_pack(torch, native, eng, ids, off, L, L, None, width=4, companions=True)
        assert rows.shape == (64, L) and not (rows == PAD).any()
        check_pack(torch, native, eng, ids, off, L, L, SEP, width=8, companions=True)
        off = offsets_of([L - 1] * 64)                  # with the separator every document is exactly a row
        rows = check_pack(torch, native, eng, ids[:off[-1]], off, L, L, SEP, width=4, companions=True)
        assert rows.shape == (64, L) and np.all(rows[:, -1] == SEP)


@pytest.mark.parametrize("form", list(FORMS))
def test_partial_coverage(torch, native, eng, form):
    """off[0] > 0 and off[n_docs] < n: the ids outside belong to no document"""
    set_form(eng, form)
    off = offsets_of([5, 0, 700, 1, 64, 0], start=333)
    ids = 1000 + np.arange(off[-1] + 444)
    ids[:333] = -5
    ids[off[-1]:] = -6
    for sep in (None, SEP):
        for L, S in ((64, 64), (7, 6), (1000, 999)):
            rows = check_pack(torch, native, eng, ids, off, L, S, sep, width=4, companions=True)
            assert not np.isin(rows, (-5, -6)).any()


@pytest.mark.parametrize("form", list(FORMS))
def test_empty_batches(torch, native, eng, form):
    set_form(eng, form)
    ids = 1000 + np.arange(10)
    for off in ([0], [4], [10]):                         # n_docs = 0
        for sep in (None, SEP):
            assert check_pack(torch, native, eng, ids, off, 8, 8, sep).shape == (0, 8)
    assert check_pack(torch, native, eng, ids[:0], [0], 8, 8, SEP).shape == (0, 8)      # ... and no ids at all
    off = [3] * 301                                       # 300 empty documents
    assert check_pack(torch, native, eng, ids, off, 8, 7, None, companions=True).shape == (0, 8)
    rows = check_pack(torch, native, eng, ids, off, 8, 8, SEP, width=4, companions=True)
    assert rows.shape == (38, 8) and (rows == SEP).sum() == 300 and (rows == PAD).sum() == 4


def test_capacity_and_bad_offsets(torch, native, eng):
    lens = [10, 0, 25, 3, 40]
    off = offsets_of(lens)
    n = int(off[-1])
    ids = 1000 + np.arange(n)
    want, _, _ = rows_model.pack(ids, off, 8, 7, SEP, PAD)
    R = want.shape[0]
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda")
    d_off = torch.from_numpy(off).to("cuda")
    bufs = [guarded(torch, R * 8, dt) for dt in (torch.int64, torch.int32, torch.int32)]
    untouched = lambda: all(bool((b == SENTINEL).all()) for b, _ in bufs)
    args = lambda o, cap: (native, eng, d_ids.data_ptr(), n, o.data_ptr(), len(lens), PACK, HAS_SEP, 8, 7, SEP, PAD,
                           bufs[0][1], 8, cap, bufs[1][1], bufs[2][1])
    torch.cuda.synchronize()
    # d_rows = NULL counts, whatever rows_cap says
    assert raw(native, eng, d_ids.data_ptr(), n, d_off.data_ptr(), len(lens), PACK, HAS_SEP, 8, 7, SEP, PAD, 0, 8,
               1 << 40) == (0, R, NONE)
    assert eng.rows_resident(d_ids.data_ptr(), n, d_off.data_ptr(), len(lens), PACK, HAS_SEP, 8, 7, SEP, PAD, 0, 8, 0) == R
    # one row short
    assert raw(*args(d_off, R - 1)) == (E_CAP, R, NONE) and untouched()
    with pytest.raises(native.RowsTooSmall) as e:
        eng.rows_resident(d_ids.data_ptr(), n, d_off.data_ptr(), len(lens), PACK, HAS_SEP, 8, 7, SEP, PAD, bufs[0][1], 8,
                          R - 1)
    assert e.value.needed == R and untouched()
    # offsets that descend at entry j; a last entry of n + 1
    for j in (1, 3, 5):
        bad = off.copy()
        bad[j] = bad[j - 1] - 1
        if j + 1 < len(bad):
            bad[j + 1:] = np.maximum(bad[j + 1:], bad[j])   # (entry j is the only one below its predecessor)
        d_bad = torch.from_numpy(bad).to("cuda")
        torch.cuda.synchronize()
        assert raw(*args(d_bad, R)) == (E_ARG, 0, j) and untouched(), j
    bad = off.copy()
    bad[-1] = n + 1
    d_bad = torch.from_numpy(bad).to("cuda")
    torch.cuda.synchronize()
    assert raw(*args(d_bad, R)) == (E_ARG, 0, len(lens)) and untouched()
    with pytest.raises(native.BadDocOffsets) as e:
        eng.rows_resident(d_ids.data_ptr(), n, d_bad.data_ptr(), len(lens), PACK, HAS_SEP, 8, 7, SEP, PAD, bufs[0][1], 8, R)
    assert e.value.index == len(lens) and untouched()
    two = off.copy()                                      # two bad entries: the first one is reported
    two[2], two[4] = 0, 1
    d_bad = torch.from_numpy(two).to("cuda")
    torch.cuda.synchronize()
    assert raw(*args(d_bad, R))[::2] == (E_ARG, 2) and untouched()
    # ... and the same buffers take the rows once everything is in order
    assert raw(*args(d_off, R)) == (0, R, NONE)
    assert np.array_equal(inside(bufs[0][0], R * 8).reshape(R, 8), want)


def test_argument_errors(torch, native, eng):
    ids = torch.arange(100, dtype=torch.int32, device="cuda")
    off = torch.tensor([0, 40, 100], dtype=torch.int64, device="cuda")
    rows, p_rows = guarded(torch, 200, torch.int64)
    comp, p_comp = guarded(torch, 200, torch.int32)
    torch.cuda.synchronize()
    base = dict(mode=PACK, flags=0, L=8, S=8, width=8, di=0, pos=0, ln=0)
    bad = [dict(L=0), dict(S=0), dict(S=9), dict(width=2), dict(width=16), dict(width=0), dict(mode=2), dict(mode=-1),
           dict(flags=8), dict(flags=1 << 31), dict(flags=TRUNC_LEFT), dict(flags=PAD_LEFT),
           dict(mode=PER_DOC, di=p_comp), dict(mode=PER_DOC, pos=p_comp), dict(ln=p_comp)]
    for change in bad:
        a = {**base, **change}
        rc, R, badj = raw(native, eng, ids.data_ptr(), 100, off.data_ptr(), 2, a["mode"], a["flags"], a["L"], a["S"], SEP,
                          PAD, p_rows, a["width"], 25, a["di"], a["pos"], a["ln"])
        assert (rc, badj) == (E_ARG, NONE), change
        with pytest.raises(ValueError):
            eng.rows_resident(ids.data_ptr(), 100, off.data_ptr(), 2, a["mode"], a["flags"], a["L"], a["S"], SEP, PAD,
                              p_rows, a["width"], 25, a["di"], a["pos"], a["ln"])
    # NULL ids with n > 0, NULL offsets
    assert raw(native, eng, 0, 100, off.data_ptr(), 2, PACK, 0, 8, 8, SEP, PAD, p_rows, 8, 25)[0] == E_ARG
    assert raw(native, eng, ids.data_ptr(), 100, 0, 2, PACK, 0, 8, 8, SEP, PAD, p_rows, 8, 25)[0] == E_ARG
    # limits, from the arguments alone: nothing of that size is touched
    assert raw(native, eng, ids.data_ptr(), 1 << 32, off.data_ptr(), 2, PACK, 0, 8, 8, SEP, PAD, 0, 8, 0)[0] == E_LIMIT
    assert raw(native, eng, ids.data_ptr(), (1 << 31) - 2, off.data_ptr(), 2, PACK, 0, 8, 8, SEP, PAD, p_rows, 8, 25, p_comp,
               0)[0] == E_LIMIT
    assert bool((rows == SENTINEL).all()) and bool((comp == SENTINEL).all())
    # stride is ignored in per-document mode
    assert raw(native, eng, ids.data_ptr(), 100, off.data_ptr(), 2, PER_DOC, 0, 8, 0, SEP, PAD, 0, 8, 0) == (0, 2, NONE)
    for name, v in (("rows_tile", 63), ("rows_tile", 66), ("rows_tile", 65540), ("rows_stage", -1), ("rows_stage", 4097)):
        with pytest.raises(ValueError):
            eng.set_option(name, v)


@pytest.mark.parametrize("form", list(FORMS))
def test_value_extremes(torch, native, eng, form):
    set_form(eng, form)
    off = offsets_of([3, 0, 70, 5])
    ids = 1000 + np.arange(off[-1])
    ids[[1, 50]] = [-(2**31), 2**31 - 1]
    for width in (8, 4):
        rows = check_pack(torch, native, eng, ids, off, 16, 15, 2**31 - 1, pad=-100, width=width)
        assert (rows == 2**31 - 1).sum() >= 5 and (rows == -100).any() and (rows == -(2**31)).any()
        check_pack(torch, native, eng, ids, off, 16, 16, -(2**31), pad=2**31 - 1, width=width)


@pytest.mark.parametrize("L", [1, 8, 100])
def test_per_document(torch, native, eng, L):
    lens = [max(x, 0) for x in (0, 1, L - 2, L - 1, L, L + 1, 3 * L)] + [0, 2]
    off = offsets_of(lens, start=11)
    n_docs = len(lens)
    ids = 1000 + np.arange(off[-1] + 5)
    d_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda")
    d_off = torch.from_numpy(off).to("cuda")
    for sep in (None, SEP):
        for trunc in ("right", "left"):
            for side in ("right", "left"):
                for width in (4, 8):
                    want, want_len = rows_model.per_doc(ids, off, L, sep, -100, trunc, side)
                    flags = (HAS_SEP if sep is not None else 0) | (TRUNC_LEFT if trunc == "left" else 0) | \
                        (PAD_LEFT if side == "left" else 0)
                    rows, p_rows = guarded(torch, n_docs * L, torch.int32 if width == 4 else torch.int64)
                    lengths, p_len = guarded(torch, n_docs, torch.int32)
                    torch.cuda.synchronize()
                    res = raw(native, eng, d_ids.data_ptr(), len(ids), d_off.data_ptr(), n_docs, PER_DOC, flags, L, L,
                              0 if sep is None else sep, -100, p_rows, width, n_docs, 0, 0, p_len)
                    what = f"L={L} sep={sep} truncate={trunc} pad_side={side} width={width}"
                    assert res == (0, n_docs, NONE), what
                    assert np.array_equal(inside(rows, n_docs * L).reshape(n_docs, L), want), what
                    assert np.array_equal(inside(lengths, n_docs), want_len), what
    # rows without lengths; one row short
    rows, p_rows = guarded(torch, n_docs * L, torch.int64)
    torch.cuda.synchronize()
    assert raw(native, eng, d_ids.data_ptr(), len(ids), d_off.data_ptr(), n_docs, PER_DOC, 0, L, L, 0, -100, p_rows, 8,
               n_docs - 1) == (E_CAP, n_docs, NONE)
    assert bool((rows == SENTINEL).all())
    assert raw(native, eng, d_ids.data_ptr(), len(ids), d_off.data_ptr(), n_docs, PER_DOC, 0, L, L, 0, -100, p_rows, 8,
               n_docs) == (0, n_docs, NONE)
    assert np.array_equal(inside(rows, n_docs * L).reshape(n_docs, L), rows_model.per_doc(ids, off, L, None, -100)[0])


# ---------------------------------------------------------------------------
# the classes

EOT = "<|endoftext|>"


@pytest.fixture(scope="module")
def trained(native):
    from minbpe_amd import RegexTokenizer
    tok = RegexTokenizer()
    tok.train(native.synth_text(30_000, 61).decode(), 256 + 40)
    tok.register_special_tokens({EOT: 100257})
    src = native.synth_text(200_000, 62).decode()
    rng = np.random.default_rng(5)
    texts, p = [], 0
    for i in range(200):
        k = 0 if i % 17 == 3 else int(rng.integers(1, 400))
        texts.append(src[p:p + k])
        p += k
    texts[0] = ""
    texts[77] = src[p:p + 50_000]          # one long text (50 kB of it ASCII or more)
    texts[-1] = ""
    texts.append(" don't  stop 12345 ünïcödé 😉")
    return tok, texts


def check_classes(torch, tok, texts):
    want_ids, want_off = tok.encode_ordinary_batch(texts)
    ids, doff = tok.encode_ordinary_batch_resident(texts)
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()
    assert doff.is_cuda and doff.dtype == torch.int64 and doff.device == ids.device
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert doff.cpu().tolist() == want_off.tolist() and len(doff) == len(texts) + 1
    docs = [tok.encode_ordinary(t) for t in texts]
    flat = np.array([i for d in docs for i in d], dtype=np.int64)
    assert np.array_equal(flat, want_ids)
    off = offsets_of([len(d) for d in docs])
    sep = tok.special_tokens[EOT]
    want = rows_model.pack(flat, off, 128, 127, sep, 0)
    rows, di, pos = tok.encode_batch_rows(texts, 128, stride=127, sep=EOT, return_doc_index=True, return_positions=True)
    assert rows.is_cuda and rows.dtype == torch.int64 and di.dtype == torch.int32 and pos.dtype == torch.int32
    for got, w in zip((rows, di, pos), want):
        assert got.shape == w.shape and np.array_equal(got.cpu().numpy(), w)
    assert np.array_equal(tok.encode_batch_rows(texts, 128, stride=127, sep=EOT).cpu().numpy(), want[0])
    return flat, off, sep


def test_regex_tokenizer(torch, trained):
    from minbpe_amd.tokenizer import rows_count
    tok, texts = trained
    flat, off, sep = check_classes(torch, tok, texts)
    T = len(flat) + len(texts)
    # rows at S = L back to bytes where they lie: the texts, each followed by the separator's text
    rows = tok.encode_batch_rows(texts, 128, sep=EOT, pad=sep)
    assert rows.shape == (rows_count(T, 128, 128), 128)
    back = tok.decode_batch_resident(rows.reshape(-1)[:T])
    assert back.cpu().numpy().tobytes() == b"".join(t.encode("utf-8") + EOT.encode() for t in texts)
    # rows_resident on the resident encode, int32 rows, an id for a separator, offsets from the host
    ids, doff = tok.encode_ordinary_batch_resident(texts)
    want = rows_model.pack(flat, off, 100, 50, 9, -100)[0]
    for d in (doff, doff.cpu().numpy(), doff.cpu().tolist(), doff.to(torch.int32)):
        got = tok.rows_resident(ids, d, 100, stride=50, sep=9, pad=-100, dtype=torch.int32)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    # per-document rows
    want, want_len = rows_model.per_doc(flat, off, 32, sep, 0, "left", "left")
    got, lengths = tok.rows_resident(ids, doff, 32, sep=EOT, mode="per_doc", truncate="left", pad_side="left")
    assert np.array_equal(got.cpu().numpy(), want) and lengths.dtype == torch.int32
    assert np.array_equal(lengths.cpu().numpy(), want_len)
    # pre-sized out: the view comes back; too small an out raises
    want = rows_model.pack(flat, off, 128, 127, sep, 0)[0]
    R = want.shape[0]
    out = torch.full((R + 3, 128), SENTINEL, dtype=torch.int64, device="cuda")
    view = tok.rows_resident(ids, doff, 128, stride=127, sep=EOT, out=out)
    assert view.data_ptr() == out.data_ptr() and view.shape == (R, 128)
    assert np.array_equal(view.cpu().numpy(), want) and bool((out[R:] == SENTINEL).all())
    flat_out = torch.full((R * 128 + 5,), SENTINEL, dtype=torch.int64, device="cuda")
    view = tok.encode_batch_rows(texts, 128, stride=127, sep=EOT, out=flat_out[1:])
    assert view.data_ptr() == flat_out.data_ptr() + 8 and np.array_equal(view.cpu().numpy(), want)
    assert int(flat_out[0]) == SENTINEL and bool((flat_out[1 + R * 128:] == SENTINEL).all())
    for small in (out[:R - 1], out[:0]):
        out.fill_(SENTINEL)
        with pytest.raises(ValueError):
            tok.rows_resident(ids, doff, 128, stride=127, sep=EOT, out=small)
        with pytest.raises(ValueError):
            tok.encode_batch_rows(texts, 128, stride=127, sep=EOT, out=small)
        assert bool((out == SENTINEL).all())
    # drop_last: the last row goes if it is partial, and only then
    assert (want[-1] == 0).any()
    for via in (lambda **kw: tok.rows_resident(ids, doff, 128, **kw), lambda **kw: tok.encode_batch_rows(texts, 128, **kw)):
        got, di = via(stride=127, sep=EOT, drop_last=True, return_doc_index=True)
        assert got.shape == (R - 1, 128) == di.shape and np.array_equal(got.cpu().numpy(), want[:-1])
        full = rows_model.pack(flat[:512], [0, 512], 128, 128, None, 0)[0]
        got = tok.rows_resident(ids[:512], [0, 512], 128, drop_last=True)
        assert got.shape == (4, 128) and np.array_equal(got.cpu().numpy(), full)
    # offsets that descend; a CPU tensor; an unknown separator
    with pytest.raises(ValueError):
        tok.rows_resident(ids, [0, 10, 5], 16)
    with pytest.raises(TypeError):
        tok.rows_resident(ids.cpu(), doff.cpu(), 16)
    with pytest.raises(KeyError):
        tok.encode_batch_rows(texts, 16, sep="<|nope|>")
    # nothing to encode: no engine call, empty results
    for none in ([], ["", ""]):
        ids0, doff0 = tok.encode_ordinary_batch_resident(none)
        assert ids0.numel() == 0 and ids0.dtype == torch.int32 and doff0.tolist() == [0] * (len(none) + 1)
        assert tok.encode_batch_rows(none, 16).shape == (0, 16)
    assert tok.encode_batch_rows(["", ""], 16, sep=EOT).cpu().tolist() == [[sep, sep] + [0] * 14]


def test_other_split_pattern(torch, trained):
    """a pattern the native scanner does not know goes through the regex module, one text at a time"""
    from minbpe_amd import RegexTokenizer
    base, texts = trained
    tok = RegexTokenizer(r"\s+|\S+")
    tok.merges, tok.vocab = dict(base.merges), dict(base.vocab)
    tok.register_special_tokens({EOT: 100257})
    check_classes(torch, tok, texts[:60] + [""])


def test_gpt4_tokenizer(torch, trained):
    from minbpe_amd import GPT4Tokenizer
    base, texts = trained
    _, ranks = toy_rank_table(base, 5)
    g = GPT4Tokenizer(ranks)
    check_classes(torch, g, texts)
