"""GPU: bpe_token_spans_resident -- token ids in HBM (int32 or int64) to the byte span and the character span of every
token inside its document -- and the Tokenizer methods on top of it.  Every case is compared element for element with
spans_model (the definition in NumPy); nothing is sampled.  One table serves the engine-level cases: entries of 0, 1, 3,
4, 15, 16, 17, 64, 200 and 40,000 random bytes (invalid UTF-8, many of them starting with a continuation byte) and
hand-made ones: a lone 0x80, a lone 0xC3, a two-byte character, a four-byte character whole and as its four bytes."""
import ctypes as C

import numpy as np
import pytest

import spans_model
from helpers import toy_rank_table

pytestmark = pytest.mark.gpu

DENSE_LENS = [0, 1, 3, 4, 15, 16, 17, 64, 200, 40_000, 2, 5, 7, 1, 0, 33]
BIG = DENSE_LENS.index(40_000)
WINK = "\U0001f609".encode("utf-8")
HAND = [b"\x80", b"\xc3", "\u00e9".encode("utf-8"), WINK, WINK[0:1], WINK[1:2], WINK[2:3], WINK[3:4], b"\x80\x80\x80"]
CONT_ONLY = len(DENSE_LENS)               # the lone 0x80: a continuation byte and nothing else
SPARSE_IDS = [300, 100257, 100276, 2**31 - 1]
SPARSE_LENS = [9, 0, 13, 6]
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_STATE = -2, -4
SEAM_N = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 12293]
STAGES = {"default": 1024, "small": 4, "global": 0}


def _table(seed):
    rng = np.random.default_rng(seed)
    dense = [rng.integers(0, 256, size=L, dtype=np.uint8).tobytes() for L in DENSE_LENS] + HAND
    sparse = [rng.integers(0, 256, size=L, dtype=np.uint8).tobytes() for L in SPARSE_LENS]
    return dense + sparse, len(dense)


TABLE, V_DENSE = _table(20240)
INDEX_OF = {**{i: i for i in range(V_DENSE)}, **{s: V_DENSE + j for j, s in enumerate(SPARSE_IDS)}}


def tidx_of(ids):
    return [INDEX_OF[int(i)] for i in ids]


def random_ids(n, seed, big=0.002):
    """ids over the dense and the sparse part; the 40,000-byte entry is rare"""
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in range(V_DENSE) if i != BIG] + SPARSE_IDS, dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), size=n)]
    ids[rng.random(n) < big] = BIG
    return ids


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _set_table(engine, table=TABLE, v_dense=V_DENSE, sparse=SPARSE_IDS):
    offs = np.zeros(len(table) + 1, np.uint64)
    np.cumsum([len(t) for t in table], out=offs[1:])
    engine.decode_set_vocab(b"".join(table), offs)
    engine.decode_set_sparse(np.array(sparse, np.int32), v_dense)


@pytest.fixture()
def eng(engine):
    _set_table(engine)
    yield engine
    engine.set_option("spans_stage", 1024)


def raw(native, engine, d_ids, width, n, d_doc=0, n_docs=0, d_bs=0, d_cs=0):
    """the C call itself: (rc, n_bytes, n_chars, bad_index, bad_doc)"""
    nb, nc, bad, bad_doc = C.c_uint64(12345), C.c_uint64(12345), C.c_uint64(12345), C.c_uint64(12345)
    rc = native._lib.bpe_token_spans_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_doc), n_docs,
                                              C.c_void_p(d_bs), C.c_void_p(d_cs), C.byref(nb), C.byref(nc),
                                              C.byref(bad), C.byref(bad_doc))
    return rc, nb.value, nc.value, bad.value, bad_doc.value


def dev_ids(torch, ids, dtype):
    """the ids one element into a device tensor: aligned to the element, not to 16 bytes"""
    buf = torch.empty(len(ids) + 1, dtype=dtype, device="cuda")
    buf[1:] = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to("cuda").to(dtype)
    t = buf[1:]
    assert t.data_ptr() % 16 != 0 or len(ids) == 0
    return t


def framed(torch, n, shift):
    """room for [n, 2] int64 inside a 0xA5-filled buffer, `shift` elements in (odd: 8-byte, not 16-byte aligned)"""
    buf = torch.full(((shift + 2 * n + 16) * 8,), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int64)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 8 * shift


def unframe(buf, n, shift):
    """the [n, 2] array, after checking that nothing around it was written"""
    host = buf.cpu().numpy()
    fill = np.frombuffer(b"\xa5" * 8, dtype=np.int64)[0]
    assert np.all(host[:shift] == fill) and np.all(host[shift + 2 * n:] == fill), "elements outside [0, 2 n) were written"
    return host[shift:shift + 2 * n].reshape(n, 2)


_MODEL = {}


def model(ids, doc, table, index_of):
    """spans_model's answer, computed once per case (the id widths and the staging forms share it) and left unchanged"""
    key = (np.asarray(ids, dtype=np.int64).tobytes(), None if doc is None else tuple(doc), tuple(table))
    if key not in _MODEL:
        tidx = [index_of[int(i)] for i in ids]
        want_b, want_c = spans_model.spans(table, tidx, doc)
        want_b.setflags(write=False)
        want_c.setflags(write=False)
        _MODEL[key] = (want_b, want_c, spans_model.totals(table, tidx))
    return _MODEL[key]


def spans(torch, native, engine, ids, dtype, doc=None, shift=1, want=("b", "c"), table=TABLE, index_of=None):
    """run `ids` (with document offsets `doc`) and compare everything with the model"""
    t = dev_ids(torch, ids, dtype)
    keep = t.clone()
    n = len(ids)
    d_doc = None if doc is None else torch.from_numpy(np.asarray(doc, dtype=np.int64)).to("cuda")
    fb, pb = framed(torch, n, shift) if "b" in want else (None, 0)
    fc, pc = framed(torch, n, shift) if "c" in want else (None, 0)
    torch.cuda.synchronize()
    rc, nb, nc, bad, bad_doc = raw(native, engine, t.data_ptr() if n else 0, t.element_size(), n,
                                   0 if doc is None else d_doc.data_ptr(), 0 if doc is None else len(doc) - 1, pb, pc)
    assert (rc, bad, bad_doc) == (0, NONE, NONE), native._lib.bpe_last_error(engine._h)
    want_b, want_c, want_totals = model(ids, doc, table, index_of or INDEX_OF)
    assert (nb, nc) == want_totals
    if fb is not None:
        assert np.array_equal(unframe(fb, n, shift), want_b), "byte spans"
    if fc is not None:
        assert np.array_equal(unframe(fc, n, shift), want_c), "char spans"
    assert torch.equal(t, keep), "the ids were written"
    return want_b, want_c


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_seams(torch, native, eng, dtype):
    """every n around a wave, a workgroup, an emit tile and a scan tile, without documents and as one document; outputs
    8-byte but not 16-byte aligned, and 16-byte aligned"""
    dt = getattr(torch, dtype)
    for n in SEAM_N:
        ids = random_ids(n, 1000 + n)
        spans(torch, native, eng, ids, dt)
        spans(torch, native, eng, ids, dt, doc=[0, n], shift=2)


def doc_layouts(n):
    rng = np.random.default_rng(n)
    cuts = sorted(rng.integers(0, n + 1, 40).tolist())
    return {
        "one": [0, n],
        "wave_seams": [0, 63, 64, 65, 255, 256, 257, n],
        "tile_seams": [0, 1023, 1024, 1025, 4095, 4096, 4097, n],
        "three_scan_tiles": [0, 100, 100 + 3 * 4096 + 17, n],
        "per_token": list(range(n + 1)),
        "empties_3000": [0, 500] + [1500] * 3000 + [1501, 5000, 5000, n],
        "inner": [5, 700, 700, 4096, n - 7],
        "random": [0] + cuts + [n],
        "no_docs_one_entry": [17],
        "nothing_inside": [n, n, n],
    }


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_documents(torch, native, eng, dtype, stage):
    eng.set_option("spans_stage", STAGES[stage])
    dt = getattr(torch, dtype)
    n = 12293 + 4096
    ids = random_ids(n, 77)
    for name, doc in doc_layouts(n).items():
        want_b, _ = spans(torch, native, eng, ids, dt, doc=doc)
        if name == "inner":
            assert (want_b[:5] == -1).all() and (want_b[n - 7:] == -1).all() and (want_b[5:n - 7] >= 0).all()
        if name in ("no_docs_one_entry", "nothing_inside"):
            assert (want_b == -1).all()
    # a first token that is nothing but a continuation byte: the clamp at 0, in the batch and in a later document
    ids = np.array([CONT_ONLY, 1, CONT_ONLY, CONT_ONLY, 2, CONT_ONLY + 1, CONT_ONLY], dtype=np.int64)
    _, want_c = spans(torch, native, eng, ids, dt)
    assert want_c[0].tolist() == [0, 0]
    _, want_c = spans(torch, native, eng, ids, dt, doc=[0, 2, 7])
    assert want_c[2].tolist() == [0, 0] and want_c[3].tolist() == [0, 0]


def test_empty_documents_take_the_global_search(torch, native, eng):
    """3,000 empty documents in a row are more starts than a tile stages (1024 at most 4096): the same answer"""
    n = 6000
    ids = random_ids(n, 5)
    for stage in (1024, 4096):
        eng.set_option("spans_stage", stage)
        spans(torch, native, eng, ids, torch.int32, doc=[0, 10] + [2500] * 5000 + [2600, n])


def test_bounds_and_optional_outputs(torch, native, eng):
    ids = random_ids(4097, 9)
    doc = [3, 1000, 1000, 4090]
    for shift in (0, 1, 2, 3):
        for want in (("b", "c"), ("b",), ("c",), ()):
            spans(torch, native, eng, ids, torch.int32, doc=doc, shift=shift, want=want)
            spans(torch, native, eng, ids, torch.int64, shift=shift, want=want)
    # n = 0: totals 0, nothing indexed, with and without offsets
    fb, pb = framed(torch, 0, 1)
    zero = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert raw(native, eng, 0, 4, 0, 0, 0, pb, pb) == (0, 0, 0, NONE, NONE)
    assert raw(native, eng, 0, 8, 0, zero.data_ptr(), 2, pb, pb) == (0, 0, 0, NONE, NONE)
    unframe(fb, 0, 1)
    # a span array that is not 8-byte aligned is refused
    t = dev_ids(torch, ids, torch.int32)
    torch.cuda.synchronize()
    assert raw(native, eng, t.data_ptr(), 4, len(ids), d_bs=pb + 4)[0] == E_ARG


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_errors(torch, native, eng, dtype):
    dt = getattr(torch, dtype)
    width = 4 if dtype == "int32" else 8
    n = 5000
    good = random_ids(n, 11)
    t = dev_ids(torch, good, dt)
    fb, pb = framed(torch, n, 1)
    fc, pc = framed(torch, n, 1)
    doc = torch.tensor([0, 100, 100, 4097, n], dtype=torch.int64, device="cuda")

    def call(changes, d=None):
        """(rc, bad_index, bad_doc) with `changes` applied to the ids; a call that fails has written nothing"""
        ids = t.clone()
        for p, v in changes.items():
            ids[p] = v
        torch.cuda.synchronize()
        rc, _, _, bad, bad_doc = raw(native, eng, ids.data_ptr(), width, n, 0 if d is None else d.data_ptr(),
                                     0 if d is None else d.numel() - 1, pb, pc)
        if rc != 0:
            unframe(fb, 0, 1 + 2 * n)   # (the whole buffer is still the fill)
            unframe(fc, 0, 1 + 2 * n)
        return rc, bad, bad_doc

    bad_ids = [-1, V_DENSE, 299, 301, 100258, -(2**31)] + ([2**32 + 65, -(2**32) + 65, 2**63 - 1, 2**31] if width == 8 else [])
    for v in bad_ids:
        for pos in (0, 2500, n - 1):
            assert call({pos: v}) == (E_ARG, pos, NONE), (v, pos)
            assert call({pos: v}, doc) == (E_ARG, pos, NONE), (v, pos)
    assert call({4500: -1, 700: V_DENSE, 4999: -1}) == (E_ARG, 700, NONE)   # the minimum position
    with pytest.raises(native.InvalidToken) as e:
        ids = t.clone()
        ids[4999] = -1
        torch.cuda.synchronize()
        eng.token_spans_resident(ids.data_ptr(), width, n)
    assert e.value.args[0] == 4999
    # offsets: descending, past n
    for entries, bad_at in (([0, 200, 100, n], 2), ([0, 100, n + 1], 2), ([n + 1, n + 1], 0), ([7, 3], 1)):
        d = torch.tensor(entries, dtype=torch.int64, device="cuda")
        assert call({}, d) == (E_ARG, NONE, bad_at), entries
        with pytest.raises(native.BadDocOffsets) as e:
            eng.token_spans_resident(t.data_ptr(), width, n, d.data_ptr(), d.numel() - 1)
        assert e.value.index == bad_at
    assert call({}, doc) == (0, NONE, NONE)
    # id_width is 4 or 8; offsets are needed for n_docs > 0
    assert raw(native, eng, t.data_ptr(), 2, n)[0] == E_ARG
    assert raw(native, eng, t.data_ptr(), width, n, 0, 3)[0] == E_ARG


def test_no_vocab_is_a_state_error(torch, native):
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with native.Engine(0) as fresh:
        assert raw(native, fresh, t.data_ptr(), 4, 4)[0] == E_STATE


def test_meta_follows_the_table(torch, native, eng):
    """a second table through bpe_decode_set_vocab (+ set_sparse): the spans are those of the new table, and a table
    without sparse ids refuses what was a sparse id"""
    ids = random_ids(3000, 21)
    spans(torch, native, eng, ids, torch.int64, doc=[0, 1500, 3000])
    table2, v2 = _table(999)
    table2 = [e[::-1] + b"\xc3\xa9" for e in table2]          # other lengths, other leads
    sparse2 = [400, 100257, 100276, 2**31 - 1]
    index2 = {**{i: i for i in range(v2)}, **{s: v2 + j for j, s in enumerate(sparse2)}}
    _set_table(eng, table2, v2, sparse2)
    ids2 = np.where(ids == 300, 400, ids)
    spans(torch, native, eng, ids2, torch.int64, doc=[0, 1500, 3000], table=table2, index_of=index2)
    t = dev_ids(torch, ids, torch.int64)                       # 300 is no id any more
    torch.cuda.synchronize()
    rc, _, _, bad, _ = raw(native, eng, t.data_ptr(), 8, len(ids))
    assert (rc, bad) == (E_ARG, int(np.flatnonzero(ids == 300)[0]))
    _set_table(eng)
    spans(torch, native, eng, ids, torch.int64, doc=[0, 1500, 3000])


def test_decode_shares_the_scratch(torch, native, eng):
    """bpe_decode_batch_resident on the same engine gives its answer before and after a spans call"""
    ids = random_ids(5000, 31)
    want = b"".join(TABLE[i] for i in tidx_of(ids))
    t = dev_ids(torch, ids, torch.int32)

    def decode():
        out = torch.empty(len(want), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert eng.decode_batch_resident(t.data_ptr(), 4, len(ids), 0, 0, out.data_ptr(), out.numel(), 0) == len(want)
        return out.cpu().numpy().tobytes()

    assert decode() == want
    spans(torch, native, eng, random_ids(9000, 32), torch.int64, doc=[0, 4000, 9000])
    assert decode() == want
    spans(torch, native, eng, ids, torch.int32)
    assert decode() == want


# ---------------------------------------------------------------------------
# the classes

TAIL = " \u00fcn\u00efc\u00f6d\u00e9 \U0001f609 \u65e5\u672c\u8a9e e\u0301"


@pytest.fixture(scope="module")
def trained(native):
    from minbpe_amd import RegexTokenizer
    text = native.synth_text(200_000, 41).decode()
    tok = RegexTokenizer()
    tok.train(text, 256 + 300)
    tok.register_special_tokens({"<|endoftext|>": 100257, "<|fim_prefix|>": 100258, "<|gap|>": 600,
                                 "<|endofprompt|>": 100276})
    return tok, text


def check_text(text, pieces, bs, cs):
    """the two properties of the definition for the tokens `pieces` (bytes each) of `text`"""
    spans_model.check_against_str(text, pieces, np.asarray(bs), np.asarray(cs))


def test_regex_tokenizer(torch, trained):
    tok, text = trained
    probe = text[:20_000] + TAIL
    ids, (bs, cs) = tok.encode_ordinary_with_offsets(probe, unit="both")
    assert ids == tok.encode_ordinary(probe) and isinstance(bs, list) and isinstance(bs[0], tuple)
    assert any(len(tok.vocab[i]) == 1 and tok.vocab[i][0] >= 0x80 for i in ids)   # characters split into byte tokens
    check_text(probe, [tok.vocab[i] for i in ids], bs, cs)
    assert tok.encode_ordinary_with_offsets(probe) == (ids, cs)
    assert tok.encode_ordinary_with_offsets(probe, unit="byte") == (ids, bs)
    # special tokens: the ids of encode(..., allowed_special="all") through token_spans
    sp = "<|endoftext|>" + text[:3000] + "<|gap|><|fim_prefix|>" + text[3000:9000] + TAIL + "<|endofprompt|>"
    sids = tok.encode(sp, allowed_special="all")
    assert 100257 in sids and 600 in sids and 100276 in sids
    pieces = [tok.vocab[i] if i in tok.vocab else tok.inverse_special_tokens[i].encode() for i in sids]
    for arr in (sids, np.array(sids), np.array(sids, dtype=np.int32)):
        b2, c2 = tok.token_spans(arr, unit="both")
        assert isinstance(b2, np.ndarray) and b2.dtype == np.int64 and b2.shape == (len(sids), 2)
        check_text(sp, pieces, b2, c2)
    assert np.array_equal(tok.token_spans(sids), c2) and np.array_equal(tok.token_spans(sids, unit="byte"), b2)
    # a batch of texts, an empty one among them: every document counts from its own start
    texts = [text[:5000] + TAIL, "", TAIL, text[5000:6000], ""]
    d_ids, doff = tok.encode_ordinary_batch_resident(texts)
    off = doff.cpu().tolist()
    for dt in (torch.int32, torch.int64):
        b3, c3 = tok.token_spans_resident(d_ids.to(dt), doff, unit="both")
        assert b3.is_cuda and b3.dtype == torch.int64 and tuple(b3.shape) == (d_ids.numel(), 2)
        b3, c3, host = b3.cpu().numpy(), c3.cpu().numpy(), d_ids.cpu().tolist()
        for d, s in enumerate(texts):
            a, z = off[d], off[d + 1]
            check_text(s, [tok.vocab[i] for i in host[a:z]], b3[a:z], c3[a:z])
        c4 = tok.token_spans_resident(d_ids.to(dt), off)                     # offsets from the host
        assert torch.equal(c4.cpu(), torch.from_numpy(c3))
        assert torch.equal(tok.token_spans_resident(d_ids.to(dt), doff, unit="byte").cpu(), torch.from_numpy(b3))
        with pytest.raises(ValueError, match="invalid token id: 999999"):
            bad = d_ids.to(dt).clone()
            bad[d_ids.numel() // 3] = 999999
            tok.token_spans_resident(bad, doff)
        with pytest.raises(ValueError):
            tok.token_spans_resident(d_ids.to(dt), [0, 10, 5, d_ids.numel()])
        with pytest.raises(ValueError):
            tok.token_spans_resident(d_ids.to(dt), [0, d_ids.numel() + 1])
    with pytest.raises(ValueError, match=r"invalid token id: %d$" % (2**32 + 65)):
        tok.token_spans([65, 2**32 + 65])
    assert tok.token_spans([]).shape == (0, 2)
    assert tuple(tok.token_spans_resident(torch.empty(0, dtype=torch.int64, device="cuda")).shape) == (0, 2)


def test_basic_and_gpt4_tokenizers(torch, native, trained):
    from minbpe_amd import BasicTokenizer, GPT4Tokenizer
    b = BasicTokenizer()
    s = "aaabdaaabac \u00e9\u00e9 \U0001f609"
    b.train(s, 259)
    ids, (bs, cs) = b.encode_with_offsets(s, unit="both")
    assert ids == b.encode(s)
    check_text(s, [b.vocab[i] for i in ids], bs, cs)
    assert b.encode_with_offsets(s) == (ids, cs)
    with pytest.raises(KeyError):
        b.token_spans([1, 4000])
    with pytest.raises(KeyError):
        b.token_spans_resident(torch.tensor([1, 4000], device="cuda"))
    base, text = trained
    perm, ranks = toy_rank_table(base, 5)
    g = GPT4Tokenizer(ranks)
    probe = text[:5000] + " don't  stop 12345" + TAIL
    ids = g.encode_ordinary(probe)
    # the pieces as the text holds them: the vocab's bytes un-shuffled
    pieces = [g.vocab[i].translate(g._unshuffle_lut) for i in ids]
    assert b"".join(pieces) == probe.encode("utf-8")
    for dt in (np.int64, np.int32):
        bs, cs = g.token_spans(np.array(ids, dtype=dt), unit="both")
        check_text(probe, pieces, bs, cs)
    ids2, cs2 = g.encode_ordinary_with_offsets(probe)
    assert ids2 == ids and cs2 == list(map(tuple, cs.tolist()))
    with pytest.raises(KeyError):                     # gpt4.py:89: specials do not decode
        g.token_spans([65, 100257])
