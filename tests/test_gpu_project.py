"""GPU: bpe_project_resident -- token ids in HBM (int32 or int64) to the ids the tokenizer of a smaller vocab_size makes of
the same text -- and the Tokenizer methods on top of it.  Every case is compared element for element with project_model
(the definition in plain Python); nothing is sampled.  One hand-made merge list serves the engine-level cases: at
vocab_size 256 its ids expand to 1, 2, 3, 4, 5, 63, 64, 65 and (a doubling chain) 4,096 ids; 64 ids is the length from
which a lane hands its part to the whole workgroup."""
import ctypes as C
import os

import numpy as np
import pytest

import project_model
import spans_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_STATE, E_CAP, E_LIMIT = -2, -4, -5, -6
CANARY = -0x5A5A5A5B

# id: length at vocab_size 256
MERGES = [(97, 98),      # 256: 2
          (256, 99),     # 257: 3
          (256, 256),    # 258: 4
          (258, 100),    # 259: 5
          (101, 101)]    # 260: 2, then the doubling chain 261: 4 ... 265: 64 ... 271: 4096
MERGES += [(259 + j, 259 + j) for j in range(1, 12)]
MERGES += [(264, 263),   # 272: 48
           (272, 262),   # 273: 56
           (273, 261),   # 274: 60
           (274, 260),   # 275: 62
           (275, 102),   # 276: 63
           (265, 103)]   # 277: 65
M = len(MERGES)
TOP = 256 + M
BIG = 271
PASS = [-7, 300000, 2**31 - 1]
assert 300000 >= TOP
LEN_256 = {256: 2, 257: 3, 258: 4, 259: 5, 276: 63, 265: 64, 277: 65, BIG: 4096}
SIZES = [256, 266, TOP - 1, TOP]       # all, the middle, one merge undone, the identity
SEAM_N = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 12293]
# (proj_tile, proj_window): the minima; the defaults; several tokens per lane and many windows per tile
GEOMETRY = {"seams": (64, 64), "default": (256, 2048), "wide": (1024, 128)}


def test_the_list_is_what_the_docstring_says():
    for t, L in LEN_256.items():
        assert len(project_model.expand(t, MERGES, 256)) == L
        assert len(project_model.expansions(MERGES, 256)[t]) == L
    assert project_model.expand(5, MERGES, 256) == [5] and project_model.expand(-7, MERGES, 256, PASS) == [-7]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture()
def eng(engine):
    engine.project_set_merges(np.array(MERGES, np.int32), np.array(PASS, np.int32))
    yield engine
    engine.set_option("proj_tile", GEOMETRY["default"][0])
    engine.set_option("proj_window", GEOMETRY["default"][1])


def geometry(engine, name):
    engine.set_option("proj_tile", GEOMETRY[name][0])
    engine.set_option("proj_window", GEOMETRY[name][1])


def raw(native, engine, d_ids, width, n, size, d_doc=0, k=0, d_out=0, cap=0, d_ooff=0):
    """the C call itself: (rc, n_out, bad_index)"""
    no, bad = C.c_uint64(12345), C.c_uint64(12345)
    rc = native._lib.bpe_project_resident(engine._h, C.c_void_p(d_ids), width, n, size, C.c_void_p(d_doc), k,
                                          C.c_void_p(d_out), cap, C.c_void_p(d_ooff), C.byref(no), C.byref(bad))
    return rc, no.value, bad.value


def random_ids(n, seed, big=0.002):
    """ids over the whole legal set; the 4,096-id token is rare, and also first, last and at the seam of 64-token tiles"""
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in range(TOP) if i != BIG] + PASS, dtype=np.int64)
    ids = pool[rng.integers(0, len(pool), size=n)]
    ids[rng.integers(0, 256, size=n) < 96] = 65          # many plain bytes: runs of tokens that stand for themselves
    ids[rng.random(n) < 0.25] = (259, 276, 265, 277)[seed % 4]   # ... and of one merged id (5, 63, 64 or 65 ids)
    ids[rng.random(n) < big] = BIG
    for p in (0, n - 1, 63, 64):
        if 0 <= p < n and n > 1:
            ids[p] = BIG
    return ids


def dev_ids(torch, ids, dtype):
    """the ids one element into a device tensor: aligned to the element, not to 16 bytes"""
    buf = torch.empty(len(ids) + 1, dtype=dtype, device="cuda")
    buf[1:] = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to("cuda").to(dtype)
    return buf[1:]


def framed(torch, cap, shift, dtype):
    """room for cap ids inside a canary-filled buffer, `shift` elements in; the buffer itself is 16-byte aligned"""
    buf = torch.full((shift + cap + 16,), CANARY, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + shift * buf.element_size()


def unframe(buf, n_out, shift):
    """the n_out ids, after checking that nothing around them was written (the element at out_cap included)"""
    host = buf.cpu().numpy().astype(np.int64)
    assert np.all(host[:shift] == CANARY) and np.all(host[shift + n_out:] == CANARY), "elements outside [0, n_out) were written"
    return host[shift:shift + n_out]


_MODEL = {}


def model(ids, size):
    """project_model's answer, computed once per case (widths and geometries share it) and left unchanged"""
    key = (np.asarray(ids, dtype=np.int64).tobytes(), size)
    if key not in _MODEL:
        arr = np.array(project_model.project(ids, MERGES, size, PASS), dtype=np.int64)
        arr.setflags(write=False)
        _MODEL[key] = arr
    return _MODEL[key]


def project_checked(native, torch, engine, ids, dtype, size, shift=1):
    """one projection through the C call into a framed buffer of exactly the room needed, against the model"""
    width = 4 if dtype == torch.int32 else 8
    want = model(ids, size)
    d = dev_ids(torch, ids, dtype)
    rc, n_out, bad = raw(native, engine, d.data_ptr(), width, len(ids), size)      # count only
    assert (rc, n_out, bad) == (0, len(want), NONE)
    buf, ptr = framed(torch, len(want), shift, dtype)
    rc, n_out, bad = raw(native, engine, d.data_ptr(), width, len(ids), size, d_out=ptr, cap=len(want))
    assert (rc, n_out, bad) == (0, len(want), NONE)
    got = unframe(buf, len(want), shift)
    assert np.array_equal(got, want), f"first difference at {int(np.flatnonzero(got != want)[0])}"
    assert np.array_equal(d.cpu().numpy().astype(np.int64), np.asarray(ids, dtype=np.int64)), "the input was written"


@pytest.mark.parametrize("geom", sorted(GEOMETRY))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_sizes_and_shapes(native, torch, eng, dtype_name, size, geom):
    geometry(eng, geom)
    dtype = getattr(torch, dtype_name)
    for n in SEAM_N:
        ids = random_ids(n, 1000 + n)
        project_checked(native, torch, eng, ids, dtype, size)
        if size == TOP:
            assert np.array_equal(model(ids, size), ids)   # the identity: every tile goes straight through


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_only_one_tile_is_not_straight_through(native, torch, eng, dtype_name):
    geometry(eng, "seams")
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 256, size=2049).astype(np.int64)
    ids[rng.integers(0, 2049, size=40)] = np.array(PASS)[rng.integers(0, 3, size=40)]
    for where, tok in ((700, 259), (64, 276), (2048, BIG)):
        one = ids.copy()
        one[where] = tok
        project_checked(native, torch, eng, one, getattr(torch, dtype_name), 256)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_alignment_of_out(native, torch, eng, dtype_name, shift):
    for geom in sorted(GEOMETRY):
        geometry(eng, geom)
        for n, size in ((257, 256), (2049, 266), (300, TOP)):
            project_checked(native, torch, eng, random_ids(n, 50 + n), getattr(torch, dtype_name), size, shift=shift)


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_capacity(native, torch, eng, dtype_name):
    dtype = getattr(torch, dtype_name)
    width = 4 if dtype == torch.int32 else 8
    ids = random_ids(2049, 11)
    want = model(ids, 256)
    d = dev_ids(torch, ids, dtype)
    buf, ptr = framed(torch, len(want), 1, dtype)
    rc, n_out, bad = raw(native, eng, d.data_ptr(), width, len(ids), 256, d_out=ptr, cap=len(want) - 1)
    assert (rc, n_out, bad) == (E_CAP, len(want), NONE)
    unframe(buf, 0, 1)                                    # nothing was written
    assert raw(native, eng, d.data_ptr(), width, len(ids), 256) == (0, len(want), NONE)
    assert raw(native, eng, d.data_ptr(), width, len(ids), 256, d_out=ptr, cap=0) == (0, len(want), NONE)
    unframe(buf, 0, 1)
    with pytest.raises(native.OutputTooSmall) as e:
        eng.project_resident(d.data_ptr(), width, len(ids), 256, d_out=ptr, out_cap=5)
    assert e.value.needed == len(want)
    # more room than needed: only [0, n_out) is written
    rc, n_out, _ = raw(native, eng, d.data_ptr(), width, len(ids), 256, d_out=ptr, cap=len(want) + 7)
    assert rc == 0 and np.array_equal(unframe(buf, len(want), 1), want)


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_bad_ids(native, torch, eng, dtype_name):
    geometry(eng, "seams")
    dtype = getattr(torch, dtype_name)
    width = 4 if dtype == torch.int32 else 8
    n = 300
    good = random_ids(n, 21)
    bads = [TOP, -1, -8, 299999, 2**31 - 2, -2**31]
    if width == 8:
        bads += [2**32 + 5, -2**32 + 65, 2**31, 2**63 - 1]      # (low words 5 and 65 are legal ids)
    cases = [([0], bads[0]), ([n - 1], bads[1]), ([64], bads[2]), ([63, 64], bads[3]), ([200, 17], bads[4])]
    cases += [([p], b) for p, b in zip((0, 64, n - 1, 150, 99, 7), bads[5:])]
    for positions, bad_id in cases:
        ids = good.copy()
        ids[positions] = bad_id
        d = dev_ids(torch, ids, dtype)
        buf, ptr = framed(torch, 20000, 1, dtype)
        ooff = torch.full((2,), CANARY, dtype=torch.int64, device="cuda")
        doc = torch.tensor([0, n], dtype=torch.int64, device="cuda")
        for size in (256, TOP):
            rc, n_out, bad = raw(native, eng, d.data_ptr(), width, n, size, doc.data_ptr(), 2, ptr, 20000, ooff.data_ptr())
            assert (rc, n_out, bad) == (E_ARG, 0, min(positions)), (positions, bad_id, size)   # the lowest position wins
            unframe(buf, 0, 1)
            assert ooff.tolist() == [CANARY, CANARY]
        with pytest.raises(native.InvalidToken) as e:
            eng.project_resident(d.data_ptr(), width, n, 256)
        assert e.value.args[0] == min(positions)
    # at the identity size too: TOP - 1 stands for itself, TOP is no id of this list
    d = dev_ids(torch, [TOP - 1, TOP], dtype)
    assert raw(native, eng, d.data_ptr(), width, 2, TOP)[0::2] == (E_ARG, 1)


def test_document_offsets(native, torch, eng):
    geometry(eng, "seams")
    n = 2049
    ids = random_ids(n, 31)
    d = dev_ids(torch, ids, torch.int32)
    want = model(ids, 256)
    for pos in ([0, 0, 5, 5, 5, 64, 700, n, n], [n], [0], [17, 3, n, 0]):    # empty documents, n itself, any order
        doc = torch.tensor(pos, dtype=torch.int64, device="cuda")
        ooff = torch.full((len(pos) + 1,), CANARY, dtype=torch.int64, device="cuda")
        exp = project_model.doc_offsets(ids, MERGES, 256, pos, PASS).tolist()
        # count only: the offsets are written all the same
        assert raw(native, eng, d.data_ptr(), 4, n, 256, doc.data_ptr(), len(pos), 0, 0, ooff.data_ptr()) == (0, len(want), NONE)
        assert ooff.tolist() == exp + [CANARY]
        ooff.fill_(CANARY)
        buf, ptr = framed(torch, len(want), 3, torch.int32)
        assert raw(native, eng, d.data_ptr(), 4, n, 256, doc.data_ptr(), len(pos), ptr, len(want), ooff.data_ptr())[0] == 0
        assert ooff.tolist() == exp + [CANARY] and np.array_equal(unframe(buf, len(want), 3), want)
    # a position > n
    doc = torch.tensor([0, n + 1, n], dtype=torch.int64, device="cuda")
    ooff = torch.empty(3, dtype=torch.int64, device="cuda")
    buf, ptr = framed(torch, len(want), 1, torch.int32)
    rc, n_out, bad = raw(native, eng, d.data_ptr(), 4, n, 256, doc.data_ptr(), 3, ptr, len(want), ooff.data_ptr())
    assert (rc, n_out, bad) == (E_ARG, len(want), NONE)
    unframe(buf, 0, 1)
    # k = 0 with and without arrays; k > 0 without arrays
    assert raw(native, eng, d.data_ptr(), 4, n, 256, doc.data_ptr(), 0, 0, 0, ooff.data_ptr())[0] == 0
    assert raw(native, eng, d.data_ptr(), 4, n, 256, 0, 1)[0] == E_ARG
    # n = 0: every position maps to 0
    doc = torch.tensor([0, 0], dtype=torch.int64, device="cuda")
    assert raw(native, eng, 0, 4, 0, 256, doc.data_ptr(), 2, 0, 0, ooff.data_ptr()) == (0, 0, NONE)
    assert ooff[:2].tolist() == [0, 0]


def test_arguments(native, torch, eng):
    d = dev_ids(torch, [65, 66], torch.int64)
    for size in (255, TOP + 1, 0, -1):
        assert raw(native, eng, d.data_ptr(), 8, 2, size)[0] == E_ARG
    assert raw(native, eng, d.data_ptr(), 2, 2, 256)[0] == E_ARG
    assert raw(native, eng, d.data_ptr() + 4, 8, 1, 256)[0] == E_ARG      # not aligned to its width
    assert raw(native, eng, 0, 8, 2, 256)[0] == E_ARG
    lib = native._lib

    def set_merges(pairs, pas=()):
        pairs, pas = np.array(pairs, np.int32).reshape(-1, 2), np.array(pas, np.int32)
        return lib.bpe_project_set_merges(eng._h, pairs.ctypes.data_as(C.c_void_p), len(pairs),
                                          pas.ctypes.data_as(C.c_void_p), len(pas))

    for pairs in ([(97, 256)], [(97, 98), (257, 99)], [(97, 98), (97, 98)], [(-1, 5)]):
        assert set_merges(pairs) == E_ARG
    for pas in ([5], [256], [-7, -7], [300, -7], [257]):
        assert set_merges([(97, 98), (256, 99)], pas) == E_ARG
    assert set_merges([(97, 98), (256, 99)], [-7, 258]) == 0
    assert raw(native, eng, d.data_ptr(), 8, 2, 259)[0] == E_ARG          # the list was replaced: 256 + M is 258 now
    assert raw(native, eng, d.data_ptr(), 8, 2, 258) == (0, 2, NONE)
    assert set_merges([]) == 0                                              # no merges: only vocab_size 256
    assert raw(native, eng, d.data_ptr(), 8, 2, 256) == (0, 2, NONE)
    for name, wrong in (("proj_tile", 0), ("proj_tile", 32), ("proj_tile", 100), ("proj_tile", 16448),
                        ("proj_window", 60), ("proj_window", 66), ("proj_window", 8196)):
        with pytest.raises(ValueError):
            eng.set_option(name, wrong)


def test_limits_from_the_merge_list(native, torch, eng):
    """a 40-merge doubling chain: at vocab_size 256 the expansions pass the table's cap of 2^28 ids (the last one alone
    would hold 2^40) -- BPE_E_LIMIT, decided on the host from the merge list; 256 + 30 is within it, expansions of at
    most 2^10 ids"""
    chain = [(97, 97)] + [(255 + r, 255 + r) for r in range(1, 40)]
    eng.project_set_merges(np.array(chain, np.int32))
    ids = [295, 97, 290]
    d = dev_ids(torch, ids, torch.int32)
    rc, n_out, bad = raw(native, eng, d.data_ptr(), 4, 3, 256)
    assert (rc, n_out, bad) == (E_LIMIT, 0, NONE)
    assert "2^28" in native._lib.bpe_last_error(eng._h).decode()
    with pytest.raises(RuntimeError, match="2\\^28"):
        eng.project_resident(d.data_ptr(), 4, 3, 256)
    want = project_model.project(ids, chain, 286)
    assert len(want) == 2**10 + 1 + 2**5
    buf, ptr = framed(torch, len(want), 1, torch.int32)
    assert raw(native, eng, d.data_ptr(), 4, 3, 286, d_out=ptr, cap=len(want)) == (0, len(want), NONE)
    assert np.array_equal(unframe(buf, len(want), 1), want)
    assert raw(native, eng, d.data_ptr(), 4, 3, 256)[0] == E_LIMIT        # (the table of 286 is still the one kept)
    assert raw(native, eng, d.data_ptr(), 4, 3, 286) == (0, len(want), NONE)


def test_state_and_neighbours(native, torch):
    """BPE_E_STATE before the merges are set; decode and spans on the same ctx are not disturbed by projections"""
    table = [bytes([i]) for i in range(256)] + [b"ab", b"abc", "é".encode(), b"\x80"]
    offs = np.zeros(len(table) + 1, np.uint64)
    np.cumsum([len(t) for t in table], out=offs[1:])
    ids = np.random.default_rng(3).integers(0, len(table), size=3000)
    d = dev_ids(torch, ids, torch.int32)
    with native.Engine(0) as e:
        assert raw(native, e, d.data_ptr(), 4, len(ids), 256)[0] == E_STATE
        e.decode_set_vocab(b"".join(table), offs)
        e.decode_set_sparse(np.empty(0, np.int32), len(table))
        e.project_set_merges(np.array(MERGES, np.int32), np.array(PASS, np.int32))
        pids = random_ids(2049, 5)
        for size in (256, TOP, 266):
            project_checked(native, torch, e, pids, torch.int64, size)
        want = b"".join(table[i] for i in ids)
        out = torch.empty(len(want), dtype=torch.uint8, device="cuda")
        assert e.decode_batch_resident(d.data_ptr(), 4, len(ids), 0, 0, out.data_ptr(), len(want), 0) == len(want)
        assert out.cpu().numpy().tobytes() == want
        project_checked(native, torch, e, pids, torch.int32, 256)
        bs = torch.empty((len(ids), 2), dtype=torch.int64, device="cuda")
        cs = torch.empty((len(ids), 2), dtype=torch.int64, device="cuda")
        e.token_spans_resident(d.data_ptr(), 4, len(ids), 0, 0, bs.data_ptr(), cs.data_ptr())
        mb, mc = spans_model.spans(table, ids.tolist())
        assert np.array_equal(bs.cpu().numpy(), mb) and np.array_equal(cs.cpu().numpy(), mc)
        prof = e.prof_read()
        assert set(prof) == set(native.PROF_KINDS) and len(native.PROF_KINDS) == 7


@pytest.mark.parametrize("order", [(256, 256, 266), (266, 256, 256), (256, 266, 256), (TOP, 256, TOP)])
def test_caching(native, torch, eng, order):
    ids = random_ids(2049, 41)
    for size in order:
        project_checked(native, torch, eng, ids, torch.int32, size)


def test_tokenizer_end_to_end(native, torch):
    from minbpe_amd import RegexTokenizer
    with open(os.path.join(ROOT, "tests", "golden", "taylorswift.txt"), encoding="utf-8") as f:
        text = f.read()[:60_000]
    tok = RegexTokenizer()
    tok.train(text, 256 + 400)
    tok.register_special_tokens({"<|endoftext|>": 100257})
    rng = np.random.default_rng(9)
    docs = []
    for j in range(200):
        b = int(rng.integers(0, len(text) - 400))
        docs.append("" if j % 17 == 3 else text[b:b + int(rng.integers(1, 400))])
    ids, offs = tok.encode_ordinary_batch_resident(docs)
    assert ids.dtype == torch.int32 and offs.numel() == 201
    for size in (256, 300, 655):
        small = tok.at_vocab(size)
        want_ids, want_offs = small.encode_ordinary_batch_resident(docs)
        got_ids, got_offs = tok.project_resident(ids, size, offs)
        assert got_ids.dtype == torch.int32 and got_offs.dtype == torch.int64
        assert torch.equal(got_ids, want_ids) and torch.equal(got_offs, want_offs)
        assert tok.projected_count(ids, size) == want_ids.numel()
        assert tok.projected_count(ids.cpu().tolist(), size) == want_ids.numel()
        assert torch.equal(small.decode_batch_resident(got_ids), tok.decode_batch_resident(ids))
        wide, none = tok.project_resident(ids.to(torch.int64), size)
        assert none is None and wide.dtype == torch.int64 and torch.equal(wide, want_ids.to(torch.int64))
    assert tok.project(ids[:500].cpu().tolist(), 300) == tok.project_resident(ids[:500].contiguous(), 300)[0].cpu().tolist()
    # out=: the view of what was written; too small raises
    room = torch.empty(ids.numel() * 8, dtype=torch.int32, device="cuda")
    got, _ = tok.project_resident(ids, 256, out=room)
    assert got.data_ptr() == room.data_ptr() and torch.equal(got, tok.at_vocab(256).encode_ordinary_batch_resident(docs)[0])
    with pytest.raises(ValueError, match="projects to"):
        tok.project_resident(ids, 256, out=room[:10])
    # special tokens pass through; an id that does not project raises what decode() raises
    mixed = torch.tensor([100257, 655, 100257, 65], dtype=torch.int64, device="cuda")
    got, _ = tok.project_resident(mixed, 256)
    assert got.tolist() == [100257] + project_model.project([655], [p for p, _ in sorted(tok.merges.items(), key=lambda kv: kv[1])],
                                                            256) + [100257, 65]
    with pytest.raises(ValueError, match="invalid token id: 656"):
        tok.project_resident(torch.tensor([65, 656], dtype=torch.int64, device="cuda"), 300)
    # a new state of the tokenizer uploads its list anew
    tok.register_special_tokens({})
    with pytest.raises(ValueError, match="invalid token id: 100257"):
        tok.project_resident(mixed, 256)
