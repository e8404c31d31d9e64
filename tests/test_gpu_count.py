"""GPU: bpe_count_resident -- how often each id occurs in token ids that live in HBM (int32 or int64) -- and the Tokenizer
methods on top of it.  Every case is compared element for element with count_model (the definition in NumPy); nothing is
sampled.  The hand-made merge list is test_gpu_project.py's (top id 277, restated in test_count_host.py): with
count_lds_bins = 256 its ids 256..277 take the 64-bit adds to memory, at the default and at 32768 all of them are LDS
counters.  The wide list has 40,000 merges, so that dense ids take the memory path at every setting."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import count_model
import project_model
from test_count_host import MERGES, M, TOP, PASS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_STATE = -2, -4
CANARY = -0x5A5A5A5B5A5A5A5B
B = TOP + len(PASS)
SEAM_N = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 12293]
WIDE_M = 40_000
WIDE = [(r % 256, r // 256) for r in range(WIDE_M)]      # byte pairs, all distinct
# the defaults are the fields' initialisers (api_ctx.hip): the fixtures put them back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
LDS_DEFAULT = int(re.search(r"int count_lds_bins = (\d+);", _CTX).group(1))
COMBINE_DEFAULT = int(re.search(r"int count_combine = (\d+);", _CTX).group(1))
LDS_SETTINGS = sorted({256, LDS_DEFAULT, 16384, 32768})     # 16384: two workgroups per CU, 32768: one
FLUSH_DEFAULT = 2**31


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def restore(engine):
    engine.set_option("count_lds_bins", LDS_DEFAULT)
    engine.set_option("count_flush", FLUSH_DEFAULT)
    engine.set_option("count_combine", COMBINE_DEFAULT)


@pytest.fixture()
def eng(engine):
    engine.project_set_merges(np.array(MERGES, np.int32), np.array(PASS, np.int32))
    yield engine
    restore(engine)


@pytest.fixture()
def wide(engine):
    engine.project_set_merges(np.array(WIDE, np.int32), np.array(PASS, np.int32))
    yield engine
    restore(engine)


def raw(native, engine, d_ids, width, n, d_counts, n_bins, accumulate=0):
    """the C call itself: (rc, bad_index)"""
    bad = C.c_uint64(12345)
    rc = native._lib.bpe_count_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_counts), n_bins, accumulate,
                                        C.byref(bad))
    return rc, bad.value


def dev_ids(torch, ids, dtype, shift=0):
    """the ids on the device, `shift` elements past a 16-byte aligned address"""
    per16 = 16 // (4 if dtype == torch.int32 else 8)
    buf = torch.empty(len(ids) + per16 + shift, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[per16 + shift:per16 + shift + len(ids)]
    view[:] = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to("cuda").to(dtype)
    if len(ids):
        assert view.data_ptr() % 16 == (shift * buf.element_size()) % 16
    return view


def framed(torch, n_bins, prefill=None):
    """n_bins words (prefilled, or a pattern no count equals) and a canary in one more"""
    buf = torch.empty(n_bins + 1, dtype=torch.int64, device="cuda")
    start = np.arange(n_bins, dtype=np.int64) * 1_000_003 + 17 if prefill is None else np.asarray(prefill, dtype=np.int64)
    buf[:n_bins] = torch.from_numpy(start).to("cuda")
    buf[n_bins] = CANARY
    return buf, start


def unframe(buf, n_bins):
    host = buf.cpu().numpy()
    assert host[n_bins] == CANARY, "the word past the bins was written"
    return host[:n_bins]


_MODEL = {}


def model(ids, m, pas=PASS):
    """count_model's answer, computed once per case (widths, alignments and settings share it) and left unchanged"""
    key = (np.asarray(ids, dtype=np.int64).tobytes(), m)
    if key not in _MODEL:
        arr = count_model.count(ids, m, pas)
        arr.setflags(write=False)
        _MODEL[key] = arr
    return _MODEL[key]


def count_checked(native, torch, engine, ids, dtype, m=M, shift=0):
    """one count through the C call into a framed array of exactly the bins, against the model"""
    width = 4 if dtype == torch.int32 else 8
    n_bins = 256 + m + len(PASS)
    want = model(ids, m)
    d = dev_ids(torch, ids, dtype, shift)
    buf, _ = framed(torch, n_bins)
    assert raw(native, engine, d.data_ptr() if len(ids) else 0, width, len(ids), buf.data_ptr(), n_bins) == (0, NONE)
    got = unframe(buf, n_bins)
    assert np.array_equal(got, want), f"first difference at bin {int(np.flatnonzero(got != want)[0])}"
    assert np.array_equal(d.cpu().numpy().astype(np.int64), np.asarray(ids, dtype=np.int64)), "the input was written"


def hand_ids(n, seed):
    """ids over every bin of the hand list, with many plain bytes and runs of one id"""
    rng = np.random.default_rng(seed)
    pool = np.array(list(range(TOP)) + PASS, dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), size=n)]
    ids[rng.integers(0, 256, size=n) < 96] = 65
    runs = rng.random(n) < 0.25
    ids[runs] = (259, 276, 32, PASS[1])[seed % 4]
    return ids


def wide_ids(n, seed):
    """ids over the whole range of the wide list plus a Zipf head (rank r with weight 1 / (r + 1)) and the pass ids"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 256 + WIDE_M, size=n)
    head = rng.random(n) < 0.6
    ids[head] = np.minimum(rng.zipf(1.3, size=int(head.sum())) - 1, 256 + WIDE_M - 1)
    sp = rng.random(n) < 0.01
    ids[sp] = np.array(PASS)[rng.integers(0, len(PASS), size=int(sp.sum()))]
    ids[[0, n - 1]] = 256 + WIDE_M - 1
    return ids.astype(np.int64)


@pytest.mark.parametrize("combine", [1, 0])
@pytest.mark.parametrize("lds", LDS_SETTINGS)
@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_seams(native, torch, eng, dtype_name, lds, combine):
    eng.set_option("count_lds_bins", lds)
    eng.set_option("count_combine", combine)
    for n in SEAM_N:
        ids = hand_ids(n, 1000 + n)
        for shift in (0, 1):
            count_checked(native, torch, eng, ids, getattr(torch, dtype_name), shift=shift)


@pytest.mark.parametrize("lds", LDS_SETTINGS)
@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_wide_list(native, torch, wide, dtype_name, lds):
    wide.set_option("count_lds_bins", lds)
    ids = wide_ids(200_000, 77)
    assert (ids >= 32768).sum() > 10_000 and (ids < 256).sum() > 50_000
    for shift in (0, 1):
        count_checked(native, torch, wide, ids, getattr(torch, dtype_name), m=WIDE_M, shift=shift)
    wide.set_option("count_combine", 0)
    count_checked(native, torch, wide, ids, getattr(torch, dtype_name), m=WIDE_M, shift=1)


@pytest.mark.parametrize("combine", [1, 0])
@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_many_flushes(native, torch, eng, dtype_name, combine):
    eng.set_option("count_combine", combine)
    ids = hand_ids(12293, 3)
    for flush, lds in ((64, 256), (64, LDS_DEFAULT), (68, 256), (4096, 256), (FLUSH_DEFAULT, 256)):
        eng.set_option("count_flush", flush)
        eng.set_option("count_lds_bins", lds)
        for shift in (0, 1):
            count_checked(native, torch, eng, ids, getattr(torch, dtype_name), shift=shift)


def contention_cases():
    n = 200_000
    rng = np.random.default_rng(12)
    pool = np.array(list(range(TOP)) + PASS, dtype=np.int64)
    lengths = rng.permutation(np.arange(1, 301))
    runs = np.repeat(pool[rng.integers(0, len(pool), size=300)], lengths)
    return {"one_low": np.full(n, 65, np.int64), "one_high": np.full(n, 270, np.int64),
            "one_pass": np.full(n, PASS[1], np.int64), "two_low": np.tile(np.array([65, 66], np.int64), n // 2),
            "low_high": np.tile(np.array([65, 270], np.int64), n // 2), "runs": runs}


@pytest.mark.parametrize("combine", [1, 0])
@pytest.mark.parametrize("case", ["one_low", "one_high", "one_pass", "two_low", "low_high", "runs"])
def test_contention(native, torch, eng, case, combine):
    """every lane of every wave adding to one address: LDS counter, memory word, pass bin (ids 256..277 are above L = 256)"""
    eng.set_option("count_lds_bins", 256)
    eng.set_option("count_combine", combine)
    ids = contention_cases()[case]
    for dtype, shift in ((torch.int32, 0), (torch.int32, 1), (torch.int64, 1)):
        count_checked(native, torch, eng, ids, dtype, shift=shift)


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_accumulate(native, torch, eng, dtype_name):
    dtype = getattr(torch, dtype_name)
    width = 4 if dtype == torch.int32 else 8
    ids = hand_ids(12293, 8)
    whole = model(ids, M)
    halves = [dev_ids(torch, ids[:5000], dtype, 1), dev_ids(torch, ids[5000:], dtype, 0)]
    # two halves accumulated onto zeros equal the whole
    buf, _ = framed(torch, B, np.zeros(B, np.int64))
    for h in halves:
        assert raw(native, eng, h.data_ptr(), width, h.numel(), buf.data_ptr(), B, 1) == (0, NONE)
    assert np.array_equal(unframe(buf, B), whole)
    # ... the first half overwriting, the second accumulating, too
    buf, _ = framed(torch, B)
    assert raw(native, eng, halves[0].data_ptr(), width, halves[0].numel(), buf.data_ptr(), B, 0) == (0, NONE)
    assert raw(native, eng, halves[1].data_ptr(), width, halves[1].numel(), buf.data_ptr(), B, 7) == (0, NONE)
    assert np.array_equal(unframe(buf, B), whole)
    # onto a prefilled array: added; without accumulate: overwritten
    buf, start = framed(torch, B)
    d = dev_ids(torch, ids, dtype)
    assert raw(native, eng, d.data_ptr(), width, len(ids), buf.data_ptr(), B, 1) == (0, NONE)
    assert np.array_equal(unframe(buf, B), start + whole)
    assert raw(native, eng, d.data_ptr(), width, len(ids), buf.data_ptr(), B, 0) == (0, NONE)
    assert np.array_equal(unframe(buf, B), whole)
    # n = 0: zeros, or the array as it is
    buf, start = framed(torch, B)
    assert raw(native, eng, 0, width, 0, buf.data_ptr(), B, 1) == (0, NONE)
    assert np.array_equal(unframe(buf, B), start)
    assert raw(native, eng, d.data_ptr(), width, 0, buf.data_ptr(), B, 0) == (0, NONE)
    assert not unframe(buf, B).any()


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_bad_ids(native, torch, eng, dtype_name):
    dtype = getattr(torch, dtype_name)
    width = 4 if dtype == torch.int32 else 8
    n = 4097
    good = hand_ids(n, 21)
    bads = [TOP, -1, -8, 299999, 2**31 - 2, -2**31]
    if width == 8:
        bads += [2**32 + 5, -2**32 + 65, 2**31, 2**63 - 1]      # (low words 5 and 65 are legal ids)
    cases = [([p], b) for b in bads[:2] + bads[6:7] for p in (0, 2048, n - 1)]          # 278, -1, 2^32 + 5: first, middle, last
    cases += [([1024, 1023], bads[0]), ([n - 1, 5], bads[1]), ([3000, 64, 65], bads[2])]   # several: the lowest position wins
    cases += [([p], b) for p, b in zip((1, 63, 64, 1025, 4095, 4000, 7), bads[3:])]
    for lds in (256, LDS_DEFAULT):
        eng.set_option("count_lds_bins", lds)
        for positions, bad_id in cases:
            ids = good.copy()
            ids[positions] = bad_id
            for shift in (0, 1):
                d = dev_ids(torch, ids, dtype, shift)
                buf, start = framed(torch, B)
                for acc in (0, 1):
                    assert raw(native, eng, d.data_ptr(), width, n, buf.data_ptr(), B, acc) == (E_ARG, min(positions)), \
                        (positions, bad_id, lds, shift, acc)
                    assert np.array_equal(unframe(buf, B), start), "d_counts was written"
        d = dev_ids(torch, [5, 6, TOP], dtype)
        with pytest.raises(native.InvalidToken) as e:
            eng.count_resident(d.data_ptr(), width, 3, framed(torch, B)[0].data_ptr(), B)
        assert e.value.args[0] == 2
    # the call after a refused one is clean
    count_checked(native, torch, eng, good, dtype)


def test_contracts(native, torch, eng):
    d = dev_ids(torch, [65, 66, 277], torch.int64)
    buf, start = framed(torch, B)
    with native.Engine(0) as fresh:
        assert raw(native, fresh, d.data_ptr(), 8, 3, buf.data_ptr(), B)[0] == E_STATE
        assert raw(native, fresh, d.data_ptr(), 8, 3, buf.data_ptr(), 256)[0] == E_STATE
        fresh.project_set_merges(np.empty((0, 2), np.int32))          # no merges, no pass ids: 256 bins
        small, _ = framed(torch, 256)
        assert raw(native, fresh, d.data_ptr(), 8, 2, small.data_ptr(), 256) == (0, NONE)
        assert unframe(small, 256).nonzero()[0].tolist() == [65, 66]
        assert raw(native, fresh, d.data_ptr(), 8, 3, small.data_ptr(), 256) == (E_ARG, 2)
    assert raw(native, eng, d.data_ptr(), 2, 3, buf.data_ptr(), B)[0] == E_ARG
    assert raw(native, eng, d.data_ptr(), 8, 3, buf.data_ptr(), B - 1)[0] == E_ARG
    assert raw(native, eng, d.data_ptr(), 8, 3, buf.data_ptr(), B + 1)[0] == E_ARG
    assert raw(native, eng, d.data_ptr(), 8, 3, 0, B)[0] == E_ARG
    assert raw(native, eng, 0, 8, 3, buf.data_ptr(), B)[0] == E_ARG
    assert raw(native, eng, d.data_ptr() + 4, 8, 1, buf.data_ptr(), B)[0] == E_ARG      # not aligned to its width
    assert raw(native, eng, d.data_ptr(), 8, 3, buf.data_ptr() + 4, B)[0] == E_ARG
    assert np.array_equal(unframe(buf, B), start)
    assert raw(native, eng, d.data_ptr(), 8, 3, buf.data_ptr(), B) == (0, NONE)
    assert unframe(buf, B).nonzero()[0].tolist() == [65, 66, 277]
    for name, wrong in (("count_lds_bins", 0), ("count_lds_bins", 128), ("count_lds_bins", 300), ("count_lds_bins", 33024),
                        ("count_flush", 63), ("count_flush", 2**31 + 1), ("count_flush", 0)):
        with pytest.raises(ValueError):
            eng.set_option(name, wrong)
    for name, right in (("count_lds_bins", 256), ("count_lds_bins", 32768), ("count_flush", 64), ("count_flush", 2**31)):
        eng.set_option(name, right)


def test_neighbours(native, torch):
    """a pending bpe_decode_batch result, the decode table and the projection table outlive a count; the time is booked
    under decode, as the projection's is"""
    lib = native._lib
    table = [bytes([i]) for i in range(256)] + [b"ab", b"abc", "é".encode(), b"\x80"]
    offs = np.zeros(len(table) + 1, np.uint64)
    np.cumsum([len(t) for t in table], out=offs[1:])
    dec = np.random.default_rng(3).integers(0, len(table), size=3000).astype(np.int32)
    want_bytes = b"".join(table[i] for i in dec)
    ids = hand_ids(4097, 5)
    d = dev_ids(torch, ids, torch.int32, 1)
    with native.Engine(0) as e:
        e.decode_set_vocab(b"".join(table), offs)
        e.project_set_merges(np.array(MERGES, np.int32), np.array(PASS, np.int32))
        nb, bad = C.c_uint64(0), C.c_uint64(0)
        assert lib.bpe_decode_batch(e._h, dec.ctypes.data_as(C.c_void_p), len(dec), C.byref(nb), C.byref(bad)) == 0
        assert nb.value == len(want_bytes)
        count_checked(native, torch, e, ids, torch.int32, shift=1)          # ... with the result pending
        out = np.empty(nb.value, np.uint8)
        assert lib.bpe_decode_read(e._h, out.ctypes.data_as(C.c_void_p), len(out), None, 0, None) == 0
        assert out.tobytes() == want_bytes
        want = np.array(project_model.project(ids, MERGES, 266, PASS), dtype=np.int64)
        first = torch.empty(len(want), dtype=torch.int32, device="cuda")
        assert e.project_resident(d.data_ptr(), 4, len(ids), 266, d_out=first.data_ptr(), out_cap=len(want)) == len(want)
        count_checked(native, torch, e, ids, torch.int64)
        again = torch.full((len(want),), -1, dtype=torch.int32, device="cuda")
        assert e.project_resident(d.data_ptr(), 4, len(ids), 266, d_out=again.data_ptr(), out_cap=len(want)) == len(want)
        assert np.array_equal(first.cpu().numpy(), want) and np.array_equal(again.cpu().numpy(), want)
        assert e.decode_batch(dec) == want_bytes                                # the decode table is still there
        e.set_option("profile", 2)
        e.prof_reset()
        count_checked(native, torch, e, ids, torch.int32)
        prof = e.prof_read()
        e.set_option("profile", 0)
        assert prof["decode"]["launches"] == 2 and prof["decode"]["alg_bytes"] == 4 * len(ids) and prof["decode"]["ms"] > 0
        assert all(prof[k]["launches"] == 0 for k in prof if k != "decode")


# ---------------------------------------------------------------------------
# the Tokenizer methods

@pytest.fixture(scope="module")
def taylor():
    with open(os.path.join(ROOT, "tests", "golden", "taylorswift.txt"), encoding="utf-8") as f:
        return f.read()[:60_000]


def laid_out(tok, ids):
    """the occurrences of every id of count_bins(), in its order"""
    layout = tok.count_bins()
    top = 256 + len(tok.merges)
    assert layout[:top].tolist() == list(range(top))
    return count_model.count(ids, len(tok.merges), layout[top:].tolist())


@pytest.mark.parametrize("kind", ["regex", "basic"])
def test_tokenizer_end_to_end(native, torch, taylor, kind):
    from minbpe_amd import BasicTokenizer, RegexTokenizer
    tok = RegexTokenizer() if kind == "regex" else BasicTokenizer()
    tok.train(taylor, 256 + 400)
    if kind == "regex":
        tok.register_special_tokens({"<|endoftext|>": 100257})
    nb = 656 + (kind == "regex")
    assert tok.count_bins().tolist() == list(range(656)) + [100257] * (kind == "regex")
    host_ids = tok.encode(taylor)
    ids = torch.tensor(host_ids, dtype=torch.int32, device="cuda")
    want = np.bincount(host_ids, minlength=nb).astype(np.int64)
    assert np.array_equal(want, laid_out(tok, host_ids))
    counts = tok.token_counts_resident(ids)
    assert counts.dtype == torch.int64 and counts.device == ids.device and counts.shape == (nb,)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(tok.token_counts_resident(ids.to(torch.int64)).cpu().numpy(), want)
    got = tok.token_counts(host_ids)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(tok.token_counts(np.array(host_ids, dtype=np.uint16)), want)
    curve = tok.compression_curve(counts)
    for k in (0, 1, 44, 399, 400):
        assert curve[k] == tok.projected_count(ids, 256 + k), k
    for size in (256, 300, 655, 656):
        small = tok.project(host_ids, size)
        assert np.array_equal(tok.counts_at_vocab(counts, size), np.bincount(small, minlength=nb)), size
        assert np.array_equal(tok.counts_at_vocab(want, size), np.bincount(small, minlength=nb))
    # out= and accumulate
    room = torch.full((nb,), 3, dtype=torch.int64, device="cuda")
    back = tok.token_counts_resident(ids, out=room)
    assert back.data_ptr() == room.data_ptr() and np.array_equal(room.cpu().numpy(), want)
    tok.token_counts_resident(ids[:1000].contiguous(), out=room)
    tok.token_counts_resident(ids[1000:], out=room, accumulate=True)         # (a view one thousand elements in)
    assert np.array_equal(room.cpu().numpy(), want)
    for wrong in (room.to(torch.int32), room.cpu(), room[:nb - 1], torch.zeros(nb + 1, dtype=torch.int64, device="cuda"),
                  room.cpu().numpy(), torch.zeros((nb, 2), dtype=torch.int64, device="cuda")[:, 0]):
        with pytest.raises(TypeError):
            tok.token_counts_resident(ids, out=wrong)
    with pytest.raises(TypeError):
        tok.token_counts_resident(ids, accumulate=True)
    # special tokens have their bin; an unknown id raises what decode() raises, and out stays as it is
    if kind == "regex":
        mixed = torch.tensor([100257, 655, 100257, 65], dtype=torch.int64, device="cuda")
        assert tok.token_counts_resident(mixed).cpu().numpy().nonzero()[0].tolist() == [65, 655, 656]
        with pytest.raises(ValueError, match="invalid token id: 656"):
            tok.token_counts_resident(torch.tensor([65, 656], dtype=torch.int64, device="cuda"), out=room)
        with pytest.raises(ValueError, match="invalid token id: 657"):
            tok.token_counts([65, 66, 657])
        tok.register_special_tokens({})                       # a new state of the tokenizer uploads its list anew
        with pytest.raises(ValueError, match="invalid token id: 100257"):
            tok.token_counts_resident(mixed)
        assert tok.token_counts_resident(ids).shape == (656,)
    else:
        with pytest.raises(KeyError):
            tok.token_counts_resident(torch.tensor([65, 656], dtype=torch.int32, device="cuda"), out=room)
    assert np.array_equal(room.cpu().numpy(), want)
