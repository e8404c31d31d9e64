"""GPU: bpe_dup_docs_resident -- for every document of an id stream that lives in HBM the number of its first copy, exact
-- and the Tokenizer methods on top of it.  Every case is compared element for element with dupdocs_model (a dict from
the bytes of a document to its first index); nothing is sampled.  first and counts are framed with canaries and
prefilled; the inputs are read back and must be as they were.  The shapes are the smallest at which each pass can go
wrong: the hash pass's tile is 64 positions in most cases, so that a few hundred ids are many tiles; dup_hash_bits = 0
drives every document through a chain of full comparisons; dup_wave_len puts the lattice on either side of the length
at which the comparison changes from a lane to a wave."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dupdocs_model
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
E_ARG, E_LIMIT = -2, -6
TAIL = 1
CANARY, PREFILL = -0x5A5A5A5B5A5A5A5B, 0x3C3C3C3D3C3C3C3D
# the defaults are the fields' initialisers (api_ctx.hip): the fixture puts them back, and "the default" is a case
with open(os.path.join(ROOT, "minbpe_amd", "csrc", "api", "api_ctx.hip")) as _f:
    _CTX = _f.read()
DEFAULTS = {name: int(re.search(rf"int {name} = (\d+);", _CTX).group(1))
            for name in ("dup_tile", "dup_wave_len", "dup_hash_bits")}
TILES = (64, DEFAULTS["dup_tile"], 65536)
WAVE_LEN_MAX = 1024
MIX = [0, 1, 3, 4, 5, 63, 64, 65, 257, 0, 0, 1023]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture()
def eng(engine):
    yield engine
    for name, value in DEFAULTS.items():
        engine.set_option(name, value)


def make_ids(n, width, seed):
    """n ids that use the whole width: a 64-bit id differs from its neighbours above bit 32 too"""
    rng = np.random.default_rng(seed)
    if width == 4:
        return rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    return rng.integers(-2**63, 2**63, size=n, dtype=np.int64)


def stream_of(docs, width, lead=0, trail=0, seed=0):
    """(ids, off) of the documents laid back to back, `lead` stray ids in front (doc_offsets[0] > 0) and `trail` behind"""
    dt = np.int32 if width == 4 else np.int64
    parts = [make_ids(lead, width, seed + 1)] + [np.asarray(d, dtype=dt) for d in docs] + [make_ids(trail, width, seed + 2)]
    off = lead + np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return np.concatenate(parts).astype(dt), off


def lattice(width, seed, extra=()):
    """documents of the lengths MIX, each present 1 - 3 times, in shuffled order (+ extra documents)"""
    rng = np.random.default_rng(seed)
    docs = []
    for i, l in enumerate(MIX):
        doc = make_ids(l, width, 1000 * seed + i)
        docs += [doc] * int(rng.integers(1, 4))
    docs += list(extra)
    return [docs[i] for i in rng.permutation(len(docs))]


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
    """room for n_docs words of first and of counts, prefilled, a canary before and after each"""

    def __init__(self, torch, n_docs):
        self.n = n_docs
        self.bufs = [torch.full((n_docs + 2,), PREFILL, dtype=torch.int64, device="cuda") for _ in range(2)]
        for b in self.bufs:
            b[0] = CANARY
            b[n_docs + 1] = CANARY
        self.d_first, self.d_counts = (b.data_ptr() + 8 for b in self.bufs)

    def read(self):
        """(first, counts) on the host, the canaries checked"""
        out = []
        for b, name in zip(self.bufs, ("d_first", "d_counts")):
            host = b.cpu().numpy()
            assert host[0] == CANARY and host[self.n + 1] == CANARY, f"a word outside {name} was written"
            out.append(host[1:self.n + 1])
        return out

    def untouched(self, first=True, counts=True):
        got = self.read()
        assert not first or (got[0] == PREFILL).all(), "d_first was written"
        assert not counts or (got[1] == PREFILL).all(), "d_counts was written"


def raw(native, engine, d_ids, width, n, d_off, n_docs, max_len, flags, d_first, d_counts):
    """the C call itself: (rc, n_distinct, bad_doc)"""
    nd, bd = C.c_uint64(12345), C.c_uint64(12345)
    rc = native._lib.bpe_dup_docs_resident(engine._h, C.c_void_p(d_ids), width, n, C.c_void_p(d_off), n_docs, max_len, flags,
                                           C.c_void_p(d_first), C.c_void_p(d_counts), C.byref(nd), C.byref(bd))
    return rc, nd.value, bd.value


def dup_checked(torch, native, engine, ids, off, max_len=None, tail=False, shift=0, counts=True):
    """one call through the C ABI into framed outputs, against the model; returns (first, counts, n_distinct)"""
    ids = np.asarray(ids)
    width = ids.dtype.itemsize
    off = np.asarray(off, dtype=np.int64)
    n_docs = len(off) - 1
    want = dupdocs_model.duplicates(ids, off, max_len, tail)
    d_ids, d_off = dev_array(torch, ids, shift), dev_array(torch, off)
    assert d_ids.data_ptr() % 16 == (shift * width) % 16
    fr = Frame(torch, n_docs)
    got = raw(native, engine, d_ids.data_ptr() if len(ids) else 0, width, len(ids), d_off.data_ptr(), n_docs,
              0 if max_len is None else max_len, TAIL if tail else 0, fr.d_first if n_docs else 0, fr.d_counts if counts else 0)
    assert got == (0, want[2], NONE)
    first, cnt = fr.read()
    assert np.array_equal(first, want[0]), f"first differs at document {int(np.flatnonzero(first != want[0])[0])}"
    if counts:
        assert np.array_equal(cnt, want[1]), f"counts differ at document {int(np.flatnonzero(cnt != want[1])[0])}"
    else:
        fr.untouched(first=False)
    assert np.array_equal(d_ids.cpu().numpy(), ids), "the ids were written"
    assert np.array_equal(d_off.cpu().numpy(), off), "the offsets were written"
    return want


# ---------------------------------------------------------------------------
# the length lattice: both widths x the tile sizes x where the stream sits on its 16 bytes

@pytest.mark.parametrize("shift", range(4))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (4, 8))
def test_lattice(torch, native, eng, width, tile, shift):
    eng.set_option("dup_tile", tile)
    docs = lattice(width, 10 * shift + width)
    ids, off = stream_of(docs, width, lead=1 + shift, trail=shift, seed=shift)
    assert off[0] > 0
    first, counts, n_distinct = dup_checked(torch, native, eng, ids, off, shift=shift)
    assert n_distinct == len(MIX) - 2 and counts.max() >= 3        # (the three empty lengths are one document)
    dup_checked(torch, native, eng, ids, off, shift=shift, counts=False)


@pytest.mark.parametrize("wave_len", (4, WAVE_LEN_MAX))
@pytest.mark.parametrize("width", (4, 8))
def test_wave_len(torch, native, eng, width, wave_len):
    """the lattice with every key of 5 ids or more compared by a wave, and with every key compared by its lane; copies
    that sit alike on their 16 bytes and copies that do not (the documents' lengths are odd and even)"""
    eng.set_option("dup_wave_len", wave_len)
    eng.set_option("dup_tile", 64)
    for bits in (64, 0):
        eng.set_option("dup_hash_bits", bits)
        docs = lattice(width, 77 + width)
        ids, off = stream_of(docs, width, lead=3, seed=5)
        dup_checked(torch, native, eng, ids, off, shift=1)


# ---------------------------------------------------------------------------
# near-duplicates that must stay apart

def near_duplicates(width, seed):
    """(documents, groups): the expected number of distinct documents among them is `groups`"""
    base = make_ids(150, width, seed)
    docs = [base]
    for pos in (149, 0, 75):                                   # the last id, the first, one in the middle
        other = base.copy()
        other[pos] ^= 1
        docs.append(other)
    docs += [base[:10], base[:20], base[:149]]                 # proper prefixes
    docs += [base.copy(), base[:10].copy()]                    # ... and two true copies among them
    return docs, 7


@pytest.mark.parametrize("bits", (64, 0))
@pytest.mark.parametrize("width", (4, 8))
def test_near_duplicates(torch, native, eng, width, bits):
    eng.set_option("dup_tile", 64)
    eng.set_option("dup_hash_bits", bits)
    docs, groups = near_duplicates(width, 31)
    for order in (np.arange(len(docs)), np.arange(len(docs))[::-1]):
        ids, off = stream_of([docs[i] for i in order], width, lead=2)
        assert dup_checked(torch, native, eng, ids, off)[2] == groups


@pytest.mark.parametrize("width", (4, 8))
def test_difference_on_a_tile_seam(torch, native, eng, width):
    """two documents of one length that differ in one id only, that id being the last position of a tile of the hash
    pass, then the first of the next"""
    eng.set_option("dup_tile", 64)
    base = make_ids(200, width, 32)
    for shift in (0, 3):
        for seam_side in (63, 64):
            # the kernel counts its tiles from the 16-byte boundary below the ids: a = the ELEMENTS by which they are past
            # it (dup_checked asserts the address), shift % 4 for int32 and shift % 2 for int64.  Document 1 starts at
            # stream position lead + 200; its id k sits at g = a + lead + 200 + k
            lead = 5
            a = shift % (16 // width)
            k = (seam_side - (a + lead + 200)) % 64 + 64
            other = base.copy()
            other[k] += 1
            ids, off = stream_of([base, other, base], width, lead=lead)
            assert (a + off[1] + k) % 64 == seam_side % 64
            first, _, n_distinct = dup_checked(torch, native, eng, ids, off, shift=shift)
            assert first.tolist() == [0, 1, 0] and n_distinct == 2


def test_ids_are_compared_at_their_full_width(torch, native, eng):
    """int64 ids equal in their low 32 bits and different above are different ids; the same ids as int32, negative values
    among them, are equal"""
    eng.set_option("dup_tile", 64)
    low = make_ids(40, 4, 33).astype(np.int64) & 0xFFFFFFFF
    assert (low >= 2**31).any()                                 # (negative as int32)
    a, b, c = low.copy(), low.copy(), low.copy()
    b[17] += 1 << 32
    c[39] += np.int64(-2**63)                                   # (the sign bit alone)
    for bits in (64, 0):
        eng.set_option("dup_hash_bits", bits)
        ids, off = stream_of([a, b, c, a], 8)
        assert dup_checked(torch, native, eng, ids, off)[0].tolist() == [0, 1, 2, 0]
        ids32 = ids.astype(np.int32)
        assert (ids32 < 0).any()
        assert dup_checked(torch, native, eng, ids32, off)[0].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------
# forced collisions: the same outputs under every number of hash bits

@pytest.mark.parametrize("width", (4, 8))
def test_forced_collisions(torch, native, eng, width):
    eng.set_option("dup_tile", 64)
    rng = np.random.default_rng(34)
    short = [make_ids(int(rng.integers(1, 9)), width, 2000 + i) for i in range(300)]
    docs = lattice(width, 35, extra=short)
    ids, off = stream_of(docs, width, lead=1)
    results = []
    for bits in (0, 1, 4, 64):
        eng.set_option("dup_hash_bits", bits)
        results.append(dup_checked(torch, native, eng, ids, off, shift=2))
    assert results[0][2] == len(MIX) - 2 + 300
    for r in results[1:]:
        assert np.array_equal(r[0], results[0][0]) and np.array_equal(r[1], results[0][1]) and r[2] == results[0][2]


# ---------------------------------------------------------------------------
# contention: every fold on one address, every document on one slot

@pytest.mark.parametrize("width", (4, 8))
def test_contention(torch, native, eng, width):
    hot = make_ids(7, width, 36)
    distinct = [make_ids(7, width, 3000 + i) for i in range(50)]
    docs = []
    for i in range(5000):
        docs.append(hot)
        if i % 100 == 50:
            docs.append(distinct[i // 100])
    ids, off = stream_of(docs, width)
    first, counts, n_distinct = dup_checked(torch, native, eng, ids, off)
    assert counts[0] == 5000 and n_distinct == 51 and (first[[i for i, d in enumerate(docs) if d is hot]] == 0).all()
    # all empty: one group, with and without ids around the documents
    for n_ids in (0, 5):
        first, counts, n_distinct = dup_checked(torch, native, eng, make_ids(n_ids, width, 37), np.full(3001, n_ids // 2))
        assert (first == 0).all() and counts[0] == 3000 and n_distinct == 1
    # all distinct
    ids, off = stream_of([make_ids(5, width, 4000 + i) for i in range(3000)], width)
    first, counts, n_distinct = dup_checked(torch, native, eng, ids, off)
    assert np.array_equal(first, np.arange(3000)) and (counts == 1).all() and n_distinct == 3000


# ---------------------------------------------------------------------------
# more documents in a tile than the hash pass stages in LDS (1,024): its search in global memory, its adds straight
# into the column -- in one stream with tiles that are staged

STAGE = 1024                                                     # DUP_STAGE of k_dupdocs.hip


def crowded_stream(width, seed):
    """documents: ordinary ones, thousands of 0 - 2 ids, a long one that crosses into a run of empty ones, copies of all"""
    rng = np.random.default_rng(seed)
    dt = np.int32 if width == 4 else np.int64
    ordinary = [make_ids(int(rng.integers(5, 40)), width, 7000 + i) for i in range(120)]
    tiny_few = [rng.integers(0, 3, size=int(rng.integers(0, 3))).astype(dt) for _ in range(3000)]   # 13 distinct keys
    long_doc = make_ids(5000, width, seed + 1)
    near = long_doc.copy()
    near[4999] ^= 1
    empties = [np.zeros(0, dt)] * 1500
    tiny_wide = [make_ids(int(rng.integers(0, 3)), width, 8000 + i) for i in range(1000)]
    tiny_wide = tiny_wide + [tiny_wide[i] for i in rng.integers(0, 1000, size=1000)]                # ... and copies
    return (ordinary + tiny_few + [long_doc] + empties + [tiny_wide[0]] + empties[:1100] + tiny_wide + [near] + ordinary[:40]
            + [long_doc] + tiny_few[:500])


def docs_per_tile(off, tile, a):
    """how many documents' offsets each tile of the hash pass would have to stage: off[j_lo .. j_hi + 1]"""
    g = np.asarray(off) + a
    out = []
    for t in range(int(g[0]) // tile, -(-int(g[-1]) // tile)):
        p_lo, p_hi = max(t * tile, int(g[0])), min((t + 1) * tile, int(g[-1]))
        j_lo = int(np.searchsorted(g, p_lo, side="right")) - 1
        j_hi = int(np.searchsorted(g, p_hi - 1, side="right")) - 1
        out.append(j_hi - j_lo + 2)
    return out


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", (4, 8))
def test_more_documents_in_a_tile_than_are_staged(torch, native, eng, width, tile):
    eng.set_option("dup_tile", tile)
    docs = crowded_stream(width, 50 + width)
    ids, off = stream_of(docs, width, lead=3, trail=2)
    for a in range(4):                                           # wherever the stream sits on its 16 bytes
        per_tile = docs_per_tile(off, tile, a)
        assert max(per_tile) > STAGE + 1, "no tile overflows the staging area"
        if tile < 65536:
            assert min(per_tile) <= STAGE + 1, "no tile is staged"
    for shift in (0, 1):
        first, counts, n_distinct = dup_checked(torch, native, eng, ids, off, shift=shift)
    long_at = [i for i, d in enumerate(docs) if len(d) == 5000]
    assert first[long_at].tolist() == [long_at[0], long_at[1], long_at[0]]       # the near copy stays apart
    empty_at = [i for i, d in enumerate(docs) if len(d) == 0]
    assert len(empty_at) > 3000 and (first[empty_at] == empty_at[0]).all() and counts[empty_at[0]] == len(empty_at)
    dup_checked(torch, native, eng, ids, off, max_len=1, tail=True, shift=2)
    dup_checked(torch, native, eng, ids, off, max_len=3000, shift=3)


# ---------------------------------------------------------------------------
# max_len / keep: documents are compared by the slices selection emits

@pytest.mark.parametrize("width", (4, 8))
def test_max_len(torch, native, eng, width):
    eng.set_option("dup_tile", 64)
    eng.set_option("dup_wave_len", 8)
    head, tail = make_ids(12, width, 38), make_ids(12, width, 39)
    docs = [np.concatenate([head, make_ids(l, width, 5000 + l)]) for l in (0, 3, 70, 200)]           # differ beyond 12 ids
    docs += [np.concatenate([make_ids(l, width, 6000 + l), tail]) for l in (0, 3, 70, 200)]          # differ before the last 12
    docs += [head[:5], make_ids(0, width, 0)]
    ids, off = stream_of(docs, width, lead=3, trail=2)
    whole = dup_checked(torch, native, eng, ids, off)
    assert whole[2] == len(docs)
    first, counts, n_distinct = dup_checked(torch, native, eng, ids, off, max_len=12)
    assert first[:4].tolist() == [0, 0, 0, 0] and counts[0] == 4 and n_distinct == len(docs) - 3
    first, counts, n_distinct = dup_checked(torch, native, eng, ids, off, max_len=12, tail=True)
    assert first[4:8].tolist() == [4, 4, 4, 4] and counts[4] == 4 and n_distinct == len(docs) - 3
    for max_len in (1, 5, 13, 64, 65):
        for tl in (False, True):
            dup_checked(torch, native, eng, ids, off, max_len=max_len, tail=tl, shift=1)
    # max_len larger than every document changes nothing
    for max_len in (212, 2**40, 2**64 - 1):
        for tl in (False, True):
            got = dup_checked(torch, native, eng, ids, off, max_len=max_len, tail=tl)
            assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


# ---------------------------------------------------------------------------
# degenerate sizes, and the scratch growing and not shrinking

def test_degenerate_sizes_and_growth(torch, native, eng):
    eng.set_option("dup_tile", 64)
    ids = make_ids(10, 4, 40)
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, np.array([4], np.int64))
    fr = Frame(torch, 1)
    assert raw(native, eng, d_ids.data_ptr(), 4, 10, d_off.data_ptr(), 0, 0, 0, fr.d_first, fr.d_counts) == (0, 0, NONE)
    fr.untouched()
    assert raw(native, eng, d_ids.data_ptr(), 4, 10, d_off.data_ptr(), 0, 0, 0, 0, 0) == (0, 0, NONE)
    for off in ([0, 10], [3, 3], [10, 10], [2, 9]):                          # one document
        assert dup_checked(torch, native, eng, ids, off)[0].tolist() == [0]
    assert dup_checked(torch, native, eng, np.zeros(0, np.int64), [0, 0, 0, 0])[0].tolist() == [0, 0, 0]   # n == 0
    # more documents than the call before, then fewer, on the same engine
    rng = np.random.default_rng(41)
    for n_docs in (100, 20000, 50, 20001):
        docs = [np.full(int(rng.integers(0, 4)), int(rng.integers(0, 3)), np.int32) for _ in range(n_docs)]
        ids, off = stream_of(docs, 4)
        assert dup_checked(torch, native, eng, ids, off)[2] <= 10


# ---------------------------------------------------------------------------
# errors

def test_bad_offsets(torch, native, eng):
    docs = lattice(4, 42)
    ids, off = stream_of(docs, 4, lead=2)
    n, n_docs = len(ids), len(off) - 1
    d_ids = dev_array(torch, ids)
    descends = off.copy()
    descends[3] = descends[2] - 1
    beyond = off.copy()
    beyond[4:] += n
    both = descends.copy()
    both[n_docs] = n + 1
    for bad_off, where in ((descends, 3), (beyond, 4), (both, 3)):
        assert select_model.check_offsets(bad_off, n) == where
        with pytest.raises(select_model.BadOffsets):
            dupdocs_model.duplicates(ids, bad_off)
        fr = Frame(torch, n_docs)
        d_off = dev_array(torch, bad_off)
        assert raw(native, eng, d_ids.data_ptr(), 4, n, d_off.data_ptr(), n_docs, 0, 0, fr.d_first, fr.d_counts) == (E_ARG, 0, where)
        fr.untouched()
        assert f"doc_offsets[{where}]" in (native._lib.bpe_last_error(eng._h) or b"").decode()
        dup_checked(torch, native, eng, ids, off)                            # a good call follows


def test_argument_errors(torch, native, eng):
    docs = lattice(4, 43)
    ids, off = stream_of(docs, 4)
    n, n_docs = len(ids), len(off) - 1
    d_ids, d_off = dev_array(torch, ids), dev_array(torch, off)
    good = dict(d_ids=d_ids.data_ptr(), width=4, n=n, d_off=d_off.data_ptr(), n_docs=n_docs, max_len=0, flags=0)
    refused = [
        (E_ARG, dict(width=2)), (E_ARG, dict(width=0)), (E_ARG, dict(width=16)),
        (E_ARG, dict(flags=2)), (E_ARG, dict(flags=0x80000001)), (E_ARG, dict(flags=TAIL, max_len=0)),
        (E_ARG, dict(d_ids=0)), (E_ARG, dict(d_off=0)), (E_ARG, dict(d_first=0)),
        (E_ARG, dict(d_ids=d_ids.data_ptr() + 2)), (E_ARG, dict(d_off=d_off.data_ptr() + 4)),
        (E_ARG, dict(d_first=4)), (E_ARG, dict(d_counts=4)),
        # the limits, on these tiny buffers: refused before anything is launched or allocated
        (E_LIMIT, dict(n=2**32)), (E_LIMIT, dict(n_docs=2**32 - 1)), (E_LIMIT, dict(n_docs=2**40)),
    ]
    for code, kw in refused:
        fr = Frame(torch, n_docs)
        args = dict(good, d_first=fr.d_first, d_counts=fr.d_counts)
        if kw.get("d_first") == 4 or kw.get("d_counts") == 4:                  # misaligned by 4 bytes
            kw = {k: args[k] + 4 for k in kw}
        args.update(kw)
        assert raw(native, eng, **args) == (code, 0, NONE), kw
        fr.untouched()
    dup_checked(torch, native, eng, ids, off)
    # options: the rows of the table
    for name, bad in (("dup_tile", 32), ("dup_tile", 66), ("dup_tile", 65540), ("dup_wave_len", 3),
                      ("dup_wave_len", WAVE_LEN_MAX + 1), ("dup_hash_bits", -1), ("dup_hash_bits", 65)):
        with pytest.raises(Exception):
            eng.set_option(name, bad)
    dup_checked(torch, native, eng, ids, off)


# ---------------------------------------------------------------------------
# the Tokenizer methods, and the calls next to this one

def test_tokenizer_methods(torch, native):
    from minbpe_amd import BasicTokenizer
    tok = BasicTokenizer()
    for width, dt in ((4, torch.int32), (8, torch.int64)):
        docs = lattice(width, 44)
        h_ids, off = stream_of(docs, width, lead=4, trail=6)
        ids = torch.from_numpy(h_ids).to("cuda")
        want = dupdocs_model.duplicates(h_ids, off)
        for form in (off, off.tolist(), torch.from_numpy(off).to("cuda"), torch.from_numpy(off.astype(np.int32)).to("cuda")):
            first = tok.duplicate_docs_resident(ids, form)
            assert first.dtype == torch.int64 and first.device == ids.device and np.array_equal(first.cpu().numpy(), want[0])
            assert tok.n_distinct_docs == want[2]
        first, counts = tok.duplicate_docs_resident(ids, off, return_counts=True)
        assert counts.dtype == torch.int64 and counts.device == ids.device
        assert np.array_equal(first.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])
        for max_len, keep in ((3, "head"), (3, "tail"), (2**40, "tail"), (np.int64(64), "head")):
            first, counts = tok.duplicate_docs_resident(ids, off, max_len=max_len, keep=keep, return_counts=True)
            w = dupdocs_model.duplicates(h_ids, off, int(max_len), keep == "tail")
            assert np.array_equal(first.cpu().numpy(), w[0]) and np.array_equal(counts.cpu().numpy(), w[1])
            assert tok.n_distinct_docs == w[2]
            # unique: the selection over first == arange, cut as it was compared
            u_ids, u_off, index, u_counts = tok.unique_docs_resident(ids, off, max_len=max_len, keep=keep)
            kept = np.flatnonzero(w[0] == np.arange(len(w[0])))
            s_ids, s_off = tok.select_docs_resident(ids, off, torch.from_numpy(w[0] == np.arange(len(w[0]))).to("cuda"),
                                                    max_len=max_len, keep=keep)
            m_ids, m_off = select_model.select(h_ids, off, kept, int(max_len), keep == "tail")
            assert torch.equal(u_ids, s_ids) and torch.equal(u_off, s_off) and u_ids.dtype == dt
            assert np.array_equal(u_ids.cpu().numpy(), m_ids) and np.array_equal(u_off.cpu().numpy(), m_off)
            assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), kept)
            assert u_counts.dtype == torch.int64 and np.array_equal(u_counts.cpu().numpy(), w[1][kept])
        u_ids, u_off, index, u_counts = tok.unique_docs_resident(ids, off)
        kept = np.flatnonzero(want[0] == np.arange(len(want[0])))
        m_ids, m_off = select_model.select(h_ids, off, kept)
        assert np.array_equal(u_ids.cpu().numpy(), m_ids) and np.array_equal(u_off.cpu().numpy(), m_off)
        assert int(u_counts.sum()) == len(docs) and tok.n_distinct_docs == len(kept)
        # ids on the host: numpy in, numpy out
        first = tok.duplicate_docs(h_ids, off)
        assert isinstance(first, np.ndarray) and first.dtype == np.int64 and np.array_equal(first, want[0])
        first, counts = tok.duplicate_docs(h_ids.tolist(), off.tolist(), return_counts=True, max_len=5, keep="tail")
        w = dupdocs_model.duplicates(h_ids, off, 5, True)
        assert np.array_equal(first, w[0]) and np.array_equal(counts, w[1])
        got = tok.unique_docs(h_ids, off.tolist())
        assert all(isinstance(x, np.ndarray) for x in got) and got[0].dtype == h_ids.dtype
        assert np.array_equal(got[0], m_ids) and np.array_equal(got[1], m_off) and np.array_equal(got[2], kept)
        assert np.array_equal(got[3], want[1][kept])
        assert tok.unique_docs(h_ids.tolist(), off)[0].dtype == np.int64
        # the exceptions' types and positions; no documents at all
        bad_off = off.copy()
        bad_off[5] = bad_off[4] - 1
        for call in (lambda: tok.duplicate_docs_resident(ids, bad_off), lambda: tok.unique_docs_resident(ids, bad_off),
                     lambda: tok.duplicate_docs(h_ids, bad_off), lambda: tok.unique_docs(h_ids, bad_off)):
            with pytest.raises(ValueError) as e:
                call()
            assert isinstance(e.value, native.BadDocOffsets) and e.value.index == 5 and "doc_offsets[5]" in str(e.value)
        first, counts = tok.duplicate_docs_resident(ids, [3], return_counts=True)
        assert first.numel() == 0 and counts.numel() == 0 and tok.n_distinct_docs == 0
        assert [x.numel() for x in tok.unique_docs_resident(ids, [3])] == [0, 1, 0, 0]


@pytest.fixture(scope="module")
def trained(native):
    from minbpe_amd import RegexTokenizer
    tok = RegexTokenizer()
    tok.train(native.synth_text(30_000, 61).decode(), 256 + 40)
    src = native.synth_text(20_000, 63).decode()
    rng = np.random.default_rng(6)
    pool, p = [], 0
    for i in range(25):
        k = 0 if i % 11 == 3 else int(rng.integers(1, 300))
        pool.append(src[p:p + k])
        p += k
    pool.append(" don't  stop 12345 ünïcödé 😉")
    texts = [pool[i] for i in rng.integers(0, len(pool), size=80)]           # a batch with repeats
    return tok, texts


def test_round_trip_and_neighbours(torch, native, trained):
    """texts -> ids in HBM -> one copy of each -> bytes: the distinct texts in first-seen order; and what the calls next
    to this one hold is as it was: a decode result not yet read, the decode table"""
    import minbpe_amd.tokenizer as T
    tok, texts = trained
    ids, doff = tok.encode_ordinary_batch_resident(texts)
    before = tok.decode_batch_resident(ids, doff)
    # a bpe_decode_batch result is pending on the same ctx while the documents are de-duplicated
    proc = T.engine(ids.device.index)
    h_ids = ids.cpu().numpy().astype(np.int32)
    nb, bad = C.c_uint64(0), C.c_uint64(0)
    assert native._lib.bpe_decode_batch(proc._h, h_ids.ctypes.data_as(C.c_void_p), len(h_ids), C.byref(nb), C.byref(bad)) == 0
    first = tok.duplicate_docs_resident(ids, doff)
    out = np.empty(max(nb.value, 1), np.uint8)
    assert native._lib.bpe_decode_read(proc._h, out.ctypes.data_as(C.c_void_p), len(out), None, 0, None) == 0
    assert out[:nb.value].tobytes() == "".join(texts).encode("utf-8")
    assert first.cpu().tolist() == [texts.index(t) for t in texts]
    u_ids, u_off, index, counts = tok.unique_docs_resident(ids, doff)
    seen = list(dict.fromkeys(texts))                                        # the distinct texts, first seen first
    assert tok.n_distinct_docs == len(seen) == index.numel()
    assert index.cpu().tolist() == [texts.index(t) for t in seen]
    assert counts.cpu().tolist() == [texts.count(t) for t in seen]
    back, boff = tok.decode_batch_resident(u_ids, u_off)
    assert back.cpu().numpy().tobytes() == "".join(seen).encode("utf-8")
    assert boff.cpu().tolist() == np.concatenate([[0], np.cumsum([len(t.encode("utf-8")) for t in seen])]).tolist()
    after = tok.decode_batch_resident(ids, doff)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
