"""GPU: bpe_decode_batch_resident -- token ids in HBM (int32 or int64) to bytes in HBM, special tokens resolved on the
device -- and Tokenizer.decode_batch_resident on top of it.  Every case is compared byte for byte with
b"".join(table[i] for i in ids) computed on the host; nothing is sampled.  One vocab table serves the engine-level cases:
entries of 0, 1, 3, 4, 15, 16, 17, 64 and 200 bytes and one of 40,000, longer than any staging window of the copy pass."""
import ctypes as C

import numpy as np
import pytest

from helpers import toy_rank_table

pytestmark = pytest.mark.gpu

DENSE_LENS = [0, 1, 3, 4, 15, 16, 17, 64, 200, 40_000, 2, 5, 7, 1, 0, 33]
BIG = DENSE_LENS.index(40_000)
SPARSE_IDS = [300, 100257, 100276, 2**31 - 1]   # 300: a gap above V_dense
SPARSE_LENS = [9, 0, 13, 6]
V_DENSE = len(DENSE_LENS)
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_CAP = -2, -5

# the copy pass as shipped, with a window and a tile so small that every case spans many of both, and the
# one-token-per-lane kernel kept for comparison
COPY_FORMS = {"default": {}, "small": {"dec_window": 1024, "dec_tile": 256}, "per_lane": {"dec_copy": 0}}
COPY_DEFAULTS = {"dec_copy": 1, "dec_window": 8192, "dec_tile": 1024}


def _table():
    rng = np.random.default_rng(20240)
    return [rng.integers(0, 256, size=L, dtype=np.uint8).tobytes() for L in DENSE_LENS + SPARSE_LENS]


TABLE = _table()
INDEX_OF = {**{i: i for i in range(V_DENSE)}, **{s: V_DENSE + j for j, s in enumerate(SPARSE_IDS)}}


def expected(ids):
    return b"".join(TABLE[INDEX_OF[int(i)]] for i in ids)


def random_ids(n, seed, big=0.002):
    """ids over the dense and the sparse part; the 40,000-byte entry is rare so that the batches stay small"""
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in range(V_DENSE) if i != BIG] + SPARSE_IDS, dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), size=n)]
    ids[rng.random(n) < big] = BIG
    return ids


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _set_table(engine):
    offs = np.zeros(len(TABLE) + 1, np.uint64)
    np.cumsum([len(t) for t in TABLE], out=offs[1:])
    engine.decode_set_vocab(b"".join(TABLE), offs)
    engine.decode_set_sparse(np.array(SPARSE_IDS, np.int32), V_DENSE)


@pytest.fixture()
def eng(engine):
    _set_table(engine)
    yield engine
    for k, v in COPY_DEFAULTS.items():
        engine.set_option(k, v)


def raw(native, engine, d_ids, width, n, d_doc=0, k=0, d_out=0, cap=0, d_boff=0):
    """the C call itself: (rc, n_bytes, bad_index)"""
    nb, bad = C.c_uint64(12345), C.c_uint64(12345)
    rc = native._lib.bpe_decode_batch_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_doc), k,
                                               C.c_void_p(d_out), cap, C.c_void_p(d_boff), C.byref(nb), C.byref(bad))
    return rc, nb.value, bad.value


def dev_ids(torch, ids, dtype):
    """the ids one element into a device tensor: aligned to the element, not to 16 bytes"""
    buf = torch.empty(len(ids) + 1, dtype=dtype, device="cuda")
    buf[1:] = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to("cuda").to(dtype)
    t = buf[1:]
    assert t.data_ptr() % 16 != 0 or len(ids) == 0
    return t


def decode(torch, native, engine, ids, dtype, shift=0, doc=None):
    """decode `ids` into a 0xA5-filled buffer at byte `shift` with out_cap == total exactly; returns the bytes (and the
    byte offsets of `doc`) after checking that nothing around them was written and the ids are unchanged"""
    t = dev_ids(torch, ids, dtype)
    keep = t.clone()
    width, n = t.element_size(), len(ids)
    d_doc = d_boff = None
    if doc is not None:
        d_doc = torch.from_numpy(np.asarray(doc, dtype=np.int64)).to("cuda")
        d_boff = torch.full((len(doc),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, total, bad = raw(native, engine, t.data_ptr(), width, n)   # d_out = NULL: only count
    assert (rc, bad) == (0, NONE), native._lib.bpe_last_error(engine._h)
    base = torch.full((shift + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, total2, bad = raw(native, engine, t.data_ptr(), width, n, 0 if doc is None else d_doc.data_ptr(),
                          0 if doc is None else len(doc), base.data_ptr() + shift, total,
                          0 if doc is None else d_boff.data_ptr())
    assert (rc, total2, bad) == (0, total, NONE), native._lib.bpe_last_error(engine._h)
    host = base.cpu().numpy()
    assert np.all(host[:shift] == 0xA5) and np.all(host[shift + total:] == 0xA5), "bytes outside [0, total) were written"
    assert torch.equal(t, keep), "the ids were written"
    got = host[shift:shift + total].tobytes()
    return got if doc is None else (got, d_boff.cpu().numpy())


def layouts():
    """the two layouts beside the random ones: runs of several thousand empty tokens that straddle the 1024-token tiles
    of the copy pass (and the 4096-value tiles of the scan), and three 40,000-byte tokens among short ones"""
    rng = np.random.default_rng(7)
    short = np.array([1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 15, 300, 100276], dtype=np.int64)
    empties = np.concatenate([short[rng.integers(0, len(short), 1500)], np.full(3000, 0), np.array([3]),
                              np.full(2500, 14), np.full(2100, 100257), short[rng.integers(0, len(short), 700)],
                              np.full(2048, 0)])
    big = short[rng.integers(0, len(short), 5000)]
    big[[0, 2047, 2048]] = BIG          # first of the batch, last of a copy tile and first of the next
    return {"empties": empties, "big": big, "all_empty": np.full(4100, 14, dtype=np.int64)}


SEAM_N = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 12293]


@pytest.mark.parametrize("form", list(COPY_FORMS))
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_seams(torch, native, eng, dtype, form):
    """every n around a wave, a workgroup, a copy tile and a scan tile, the runs of empty tokens and the entry longer
    than the window; total 0 (n = 0, or nothing but empty tokens) is a valid result"""
    for k, v in COPY_FORMS[form].items():
        eng.set_option(k, v)
    dt = getattr(torch, dtype)
    for n in SEAM_N:
        ids = random_ids(n, 1000 + n)
        assert decode(torch, native, eng, ids, dt) == expected(ids), f"n = {n}"
    for name, ids in layouts().items():
        want = expected(ids)
        assert (len(want) == 0) == (name == "all_empty")
        assert decode(torch, native, eng, ids, dt) == want, name


@pytest.mark.parametrize("form", list(COPY_FORMS))
def test_alignment_and_bounds(torch, native, eng, form):
    for k, v in COPY_FORMS[form].items():
        eng.set_option(k, v)
    ids = random_ids(4097, 5)
    want = expected(ids)
    for shift in (0, 1, 2, 3, 5, 15):
        assert decode(torch, native, eng, ids, torch.int32, shift=shift) == want, f"shift {shift}"
    # one byte short: BPE_E_CAP, the total is still reported, nothing is written
    t = dev_ids(torch, ids, torch.int32)
    base = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, total, bad = raw(native, eng, t.data_ptr(), 4, len(ids), d_out=base.data_ptr() + 3, cap=len(want) - 1)
    assert (rc, total, bad) == (E_CAP, len(want), NONE)
    assert bool((base == 0xA5).all())
    with pytest.raises(native.OutputTooSmall) as e:
        eng.decode_batch_resident(t.data_ptr(), 4, len(ids), 0, 0, base.data_ptr(), len(want) - 1, 0)
    assert e.value.needed == len(want) and bool((base == 0xA5).all())
    # d_out = NULL counts, whatever out_cap says
    assert raw(native, eng, t.data_ptr(), 4, len(ids), d_out=0, cap=1 << 40) == (0, len(want), NONE)
    assert eng.decode_batch_resident(t.data_ptr(), 4, len(ids), 0, 0, 0, 0, 0) == len(want)
    assert torch.equal(t.cpu(), torch.from_numpy(ids).to(torch.int32))


BAD_BOTH = [-1, 17, 299, 301, V_DENSE + len(SPARSE_IDS) - 1, V_DENSE + len(SPARSE_IDS), 100258, -(2**31)]
BAD_64 = [2**32 + 65, -(2**32) + 65, 2**63 - 1, -(2**63), 2**32 + 100257, 2**31]


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_id_validity(torch, native, eng, dtype):
    dt = getattr(torch, dtype)
    width = 4 if dtype == "int32" else 8
    good = random_ids(5000, 11)
    good[[10, 2500, 4999]] = [2**31 - 1, 100257, 300]
    assert decode(torch, native, eng, good, dt) == expected(good)   # valid sparse ids decode to their entries
    t = dev_ids(torch, good, dt)

    room = torch.full((len(expected(good)) + 40_000,), 0xA5, dtype=torch.uint8, device="cuda")

    def first_bad(changes):
        """(rc, bad_index) with `changes` applied; a call that fails has written nothing"""
        ids = t.clone()
        for p, v in changes.items():
            ids[p] = v
        room.fill_(0xA5)
        torch.cuda.synchronize()
        rc, total, bad = raw(native, eng, ids.data_ptr(), width, len(good), d_out=room.data_ptr(), cap=room.numel())
        assert rc == 0 or bool((room == 0xA5).all())
        return rc, bad

    for v in BAD_BOTH + (BAD_64 if width == 8 else []):
        assert first_bad({2500: v}) == (E_ARG, 2500), v
        with pytest.raises(native.InvalidToken) as e:
            ids = t.clone()
            ids[4999] = v
            torch.cuda.synchronize()
            eng.decode_batch_resident(ids.data_ptr(), width, len(good), 0, 0, 0, 0, 0)
        assert e.value.args[0] == 4999
    # two bad ids in different tiles: the earlier position
    assert first_bad({4500: -1, 700: 17}) == (E_ARG, 700)
    assert first_bad({0: 299, 4999: -1}) == (E_ARG, 0)
    # id_width is 4 or 8
    assert raw(native, eng, t.data_ptr(), 2, len(good))[0] == E_ARG
    # what bpe_decode_set_sparse refuses leaves the list as it was
    lib, h = native._lib, eng._h
    for lst, vd in [([300, 100276, 100257, 2**31 - 1], V_DENSE), ([300, 300, 100276, 2**31 - 1], V_DENSE),
                    ([5, 300, 100257, 100276], V_DENSE), ([300, 100257, 100276], V_DENSE),
                    (SPARSE_IDS, V_DENSE - 1), (SPARSE_IDS, V_DENSE + 1)]:
        arr = np.array(lst, np.int32)
        assert lib.bpe_decode_set_sparse(h, arr.ctypes.data_as(C.c_void_p), len(arr), vd) == E_ARG, (lst, vd)
    with pytest.raises(ValueError):
        eng.decode_set_sparse([100257, 300, 100276, 2**31 - 1], V_DENSE)
    assert decode(torch, native, eng, good, dt) == expected(good)
    # a negative sparse id is an id like any other
    eng.decode_set_sparse([-7, 300, 100257, 100276], V_DENSE)
    neg = np.array([1, -7, 4, 300], dtype=np.int64)
    assert decode(torch, native, eng, neg, dt) == TABLE[1] + TABLE[V_DENSE] + TABLE[4] + TABLE[V_DENSE + 1]
    assert first_bad({}) == (E_ARG, int(np.flatnonzero(good == 2**31 - 1)[0]))
    no_max = {int(p): 5 for p in np.flatnonzero(good == 2**31 - 1)}
    assert first_bad({**no_max, 2500: 100257, 2501: -7}) == (0, NONE)
    # bpe_decode_set_vocab clears the list: the table's sparse entries are no ids any more
    offs = np.zeros(len(TABLE) + 1, np.uint64)
    np.cumsum([len(x) for x in TABLE], out=offs[1:])
    eng.decode_set_vocab(b"".join(TABLE), offs)
    assert first_bad({}) == (E_ARG, int(np.flatnonzero(good >= len(TABLE))[0]))
    only_dense = np.arange(len(TABLE), dtype=np.int64)   # ... and every entry is a dense id
    got = decode(torch, native, eng, only_dense, dt)
    assert got == b"".join(TABLE)


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_document_offsets(torch, native, eng, dtype):
    dt = getattr(torch, dtype)
    ids = layouts()["empties"]
    n = len(ids)
    lens = np.array([len(TABLE[INDEX_OF[int(i)]]) for i in ids], dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(lens)])
    doc = [0, n, 17, 17, 1500, 2047, 2048, 3000, 4499, 4500, 4501, 6000, n - 1, n, 0]   # 1500..4499 and 4501..: runs of empty tokens
    got, boff = decode(torch, native, eng, ids, dt, shift=5, doc=doc)
    assert got == expected(ids) and boff.tolist() == cum[doc].tolist()
    # count-only with positions: the offsets are there already
    t = dev_ids(torch, ids, dt)
    d_doc = torch.tensor(doc, dtype=torch.int64, device="cuda")
    d_boff = torch.full((len(doc),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert raw(native, eng, t.data_ptr(), t.element_size(), n, d_doc.data_ptr(), len(doc), 0, 0, d_boff.data_ptr()) == \
        (0, int(cum[-1]), NONE)
    assert d_boff.cpu().tolist() == cum[doc].tolist()
    # a position past n
    d_doc[3] = n + 1
    out = torch.full((int(cum[-1]),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, total, bad = raw(native, eng, t.data_ptr(), t.element_size(), n, d_doc.data_ptr(), len(doc), out.data_ptr(),
                         out.numel(), d_boff.data_ptr())
    assert (rc, bad) == (E_ARG, NONE) and bool((out == 0xA5).all())
    assert b"doc_token_offsets[3]" in native._lib.bpe_last_error(eng._h)
    # k > 0 needs both arrays
    assert raw(native, eng, t.data_ptr(), t.element_size(), n, d_doc.data_ptr(), 2, 0, 0, 0)[0] == E_ARG
    # n = 0 with k > 0: all zeros
    zeros = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_boff = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert raw(native, eng, 0, t.element_size(), 0, zeros.data_ptr(), 3, 0, 0, d_boff.data_ptr()) == (0, 0, NONE)
    assert d_boff.cpu().tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------
# the classes

@pytest.fixture(scope="module")
def trained(native):
    from minbpe_amd import RegexTokenizer
    text = native.synth_text(200_000, 41).decode()
    tok = RegexTokenizer()
    tok.train(text, 256 + 300)
    tok.register_special_tokens({"<|endoftext|>": 100257, "<|fim_prefix|>": 100258, "<|gap|>": 600,
                                 "<|endofprompt|>": 100276})
    return tok, text


def test_regex_tokenizer(torch, trained):
    tok, text = trained
    probe = "<|endoftext|>" + text[:3000] + "<|gap|><|fim_prefix|>" + text[3000:9000] + " ünïcödé 😉<|endofprompt|>"
    ids = tok.encode(probe, allowed_special="all")
    assert 100257 in ids and 600 in ids and 100276 in ids
    want = tok.decode_batch(ids)
    assert want == probe.encode("utf-8")
    doc = [0, 1, 1, len(ids) // 2, len(ids)]
    want_off = tok.decode_batch(ids, doc)[1]
    for dt in (torch.int64, torch.int32):
        t = torch.tensor(ids, dtype=dt, device="cuda")
        got = tok.decode_batch_resident(t)
        assert got.is_cuda and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want
        for d in (doc, torch.tensor(doc, device="cuda")):
            got, boff = tok.decode_batch_resident(t, d)
            assert got.cpu().numpy().tobytes() == want
            assert boff.is_cuda and boff.dtype == torch.int64 and boff.cpu().tolist() == want_off.tolist()
        # out=: decoded in place, the view of exactly the bytes comes back
        out = torch.full((len(want) + 100,), 0xA5, dtype=torch.uint8, device="cuda")
        view = tok.decode_batch_resident(t, out=out[7:])
        assert view.data_ptr() == out.data_ptr() + 7 and view.numel() == len(want)
        assert view.cpu().numpy().tobytes() == want and bool((out[7 + len(want):] == 0xA5).all()) and bool((out[:7] == 0xA5).all())
        with pytest.raises(ValueError):
            tok.decode_batch_resident(t, out=out[:len(want) - 1])
        with pytest.raises(ValueError):
            tok.decode_batch_resident(t, out=out[:0])
        with pytest.raises(ValueError, match="invalid token id: 999999"):
            bad = t.clone()
            bad[len(ids) // 3] = 999999
            tok.decode_batch_resident(bad)
        assert torch.equal(t.cpu(), torch.tensor(ids, dtype=dt))
    with pytest.raises(ValueError, match=r"invalid token id: %d$" % (2**32 + 65)):
        tok.decode_batch_resident(torch.tensor([65, 2**32 + 65], dtype=torch.int64, device="cuda"))
    assert tok.decode_batch_resident(torch.empty(0, dtype=torch.int64, device="cuda")).numel() == 0
    for wrong in (ids, np.array(ids), torch.tensor(ids, dtype=torch.float32, device="cuda"), torch.tensor(ids),
                  torch.tensor(ids, device="cuda").reshape(1, -1), torch.tensor(ids + ids, device="cuda")[::2]):
        with pytest.raises(TypeError):
            tok.decode_batch_resident(wrong)


def test_basic_and_gpt4_tokenizers(torch, native, trained):
    from minbpe_amd import BasicTokenizer, GPT4Tokenizer
    b = BasicTokenizer()
    b.train("aaabdaaabac", 259)
    t = torch.tensor(b.encode("aaabdaaabac"), device="cuda")
    assert b.decode_batch_resident(t).cpu().numpy().tobytes() == b"aaabdaaabac"
    with pytest.raises(KeyError):
        b.decode_batch_resident(torch.tensor([1, 4000], device="cuda"))
    base, text = trained
    perm, ranks = toy_rank_table(base, 5)
    g = GPT4Tokenizer(ranks)
    probe = text[:5000] + " don't  stop 12345 ünïcödé 😉"
    ids = g.encode_ordinary(probe)
    want = g.decode_batch(ids)
    assert want == probe.encode("utf-8")
    for dt in (torch.int64, torch.int32):
        got = g.decode_batch_resident(torch.tensor(ids, dtype=dt, device="cuda"))
        assert got.cpu().numpy().tobytes() == want        # the table went up already translated
        with pytest.raises(KeyError):                     # gpt4.py:89: specials do not decode
            g.decode_batch_resident(torch.tensor([65, 100257], dtype=dt, device="cuda"))
        # the host form after the resident form on the same engine: its own (untranslated) table is back
        assert g.decode_batch(ids) == want


def test_round_trip_in_hbm(torch, native, trained):
    """text -> engine.encode_batch_resident -> decode_batch_resident on the int32 ids where they lie -> the text"""
    from minbpe_amd.tokenizer import engine as the_engine
    tok, _ = trained
    data = native.synth_text(1_000_000, 43)
    offs = native.split_offsets(data, 4)
    pairs, mids = tok._merge_table()
    d_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    d_offs = torch.from_numpy(offs.astype(np.int64)).to("cuda")
    d_ids = torch.full((len(data),), -1, dtype=torch.int32, device="cuda")
    d_ooff = torch.empty(len(offs) + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = the_engine().encode_batch_resident(pairs, mids, d_bytes.data_ptr(), len(data), d_offs.data_ptr(), len(offs),
                                               d_ids.data_ptr(), d_ooff.data_ptr())
    assert 0 < total < len(data) // 2
    back = tok.decode_batch_resident(d_ids[:total])
    assert torch.equal(back, d_bytes)
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda")   # the caller's bound: the bytes it encoded
    assert torch.equal(tok.decode_batch_resident(d_ids[:total], out=out), d_bytes)
