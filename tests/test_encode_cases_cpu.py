"""CPU: oracle.encode on the cases of encode_cases.py against the reference's own loop, and each case's precondition.

The goldens never held inputs like these (runs of 9,216 bytes, NULs, 133,123 chunks), so the oracle is pinned on them
here, one step from the reference: _encode_chunk (regex.py:92-109) restated with pyref.get_stats / pyref.merge, applied
to every DISTINCT chunk of a batch (_encode_chunk is a function of the chunk's bytes and the merges alone, so each
distinct chunk goes through the loop once and the whole batch is compared).  The preconditions are read off the
reference output, so that no case silently stops landing on the seam it was built for."""
import numpy as np
import pytest

import encode_cases as ec
import oracle
from encode_cases import SEAMS
from oracle import pyref


def _merges_dict(pairs, mids):
    """the reference's self.merges: pair -> id"""
    return {(int(a), int(b)): (256 + r if mids is None else int(mids[r])) for r, (a, b) in enumerate(pairs)}


def ref_encode_chunk(chunk, merges):
    ids = list(chunk)
    while len(ids) >= 2:
        stats = pyref.get_stats(ids)
        pair = min(stats, key=lambda p: merges.get(p, float("inf")))
        if pair not in merges:
            break
        ids = pyref.merge(ids, pair, merges[pair])
    return ids


_MEMO = {}


def pinned(case):
    """oracle.encode of the case, after comparing it chunk for chunk with the reference's loop; returns
    (token lists per chunk, chunks)"""
    pairs, mids, data, offs = case
    exp_ids, exp_off = oracle.encode(pairs, data, ec.oracle_offsets(data, offs), merge_ids=mids)
    assert len(exp_off) == len(offs) + 1 and exp_off[0] == 0 and exp_off[-1] == len(exp_ids)
    merges = _merges_dict(pairs, mids)
    memo = _MEMO.setdefault((len(pairs), hash(np.asarray(pairs).tobytes()), None if mids is None else hash(np.asarray(mids).tobytes())), {})
    chunks = ec.chunks_of(data, offs)
    assert len(chunks) == len(offs) and sum(map(len, chunks)) == len(data)
    toks = []
    exp_list = exp_ids.tolist()
    bounds = exp_off.astype(np.int64).tolist()
    for i, ch in enumerate(chunks):
        want = memo.get(ch)
        if want is None:
            want = memo[ch] = ref_encode_chunk(ch, merges)
        got = exp_list[bounds[i]:bounds[i + 1]]
        assert got == want, f"chunk {i} ({len(ch)} bytes): the oracle differs from the reference's loop"
        toks.append(want)
    return toks, chunks


# ---------------------------------------------------------------------------

def test_seam_table_matches_the_sources():
    """every entry of SEAMS against the constant it mirrors, read from the sources"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ""
    for f in ("bpe_device.h", "kernels/k_encode.hip", "api/api_encode.hip"):
        with open(os.path.join(root, "minbpe_amd", "csrc", f), encoding="utf-8") as fh:
            src += fh.read()
    for name in ("ENC_LMAX", "SCAN_TILE", "ENC_LONG_MID", "ENC_LONG_MAX", "ENC_LONG_TOP", "ENC_PROBES", "ENC_KEYBYTES",
                 "ENC_PLACE_TILE", "ENC_PLACE_BIG", "ENC_PLACE_NBIG"):
        m = re.search(r"\b%s = (\d+)" % name, src)
        assert m and int(m.group(1)) == SEAMS[name], name
    assert "tslots = 1ull << 12" in src and SEAMS["ENC_TAB_MIN"] == 1 << 12
    assert "idx -= 64" in src and SEAMS["LOOKBACK"] == 64


def test_tables_are_what_they_claim():
    runs = ec.t_runs()
    assert len(runs) == 28 and runs[0] == (97, 97) and runs[1] == (98, 98) and runs[2] == (256, 256) and runs[3] == (257, 257)
    alt = ec.t_alt()
    assert alt[:5] == ((98, 97), (97, 98), (97, 256), (256, 256), (256, 98))
    text = ec.t_text()
    assert len(text) == 300 and len(set(text)) == 300
    for t in (runs, alt, text, ec.t_text_sparse()[0]):
        assert ec.table_is_inert(t)
        assert len(set(t)) == len(t)  # no pair twice
    pairs, ids = ec.t_text_sparse()
    assert ids[0] == 1000 and ids[-1] == 1000 + 3 * 299 and max(max(p) for p in pairs) <= ids[-1]
    assert len(ec.short_words()) == 50 and all(1 <= len(w) <= 5 for w in ec.short_words())


@pytest.mark.parametrize("order", ["mixed", "packed"])
@pytest.mark.parametrize("table", ["T_runs", "T_alt", "T_text"])
def test_tier_lattice(table, order):
    case = ec.tier_lattice(table, order)
    toks, chunks = pinned(case)
    lens = np.array([len(c) for c in chunks])
    lmax, mid, mx, top = (SEAMS[k] for k in ("ENC_LMAX", "ENC_LONG_MID", "ENC_LONG_MAX", "ENC_LONG_TOP"))
    assert sorted(set(lens[lens >= lmax - 1].tolist())) == [31, 32, 33, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 9215,
                                                           9216, 9217, 9300] == sorted(ec.lattice_lengths())
    # every tier has work in the one launch, and every seam length comes in every content
    tiers = [(lens <= SEAMS["ENC_KEYBYTES"]).sum(), ((lens > lmax) & (lens <= mid)).sum(), ((lens > mid) & (lens <= mx)).sum(),
             ((lens > mx) & (lens <= top)).sum(), (lens > top).sum()]
    assert tiers[0] >= 300 and min(tiers[1:4]) >= 30 and tiers[4] >= 20, tiers
    for L in ec.lattice_lengths():
        assert (lens == L).sum() >= 8, L
    by_bytes = dict(zip(chunks, toks))
    g = SEAMS["GROUP"]
    for L in ec.lattice_lengths():
        assert len(by_bytes[ec.inert(L, L)]) == L  # a token per inert byte
        ab = ec.abab(L, ec.A)
        assert all(ab[i] == ec.B and ab[i + 1] == ec.A for i in range(1, L - 1, 2))  # the rank-0 pair at every odd position
        if L > g:
            assert ab[g - 1:g + 1] == b"ba" and ec.run(L)[g - 1:g + 1] == b"aa"  # a site across positions 63 | 64
            assert ec.with_foreign(ec.run(L), g - 1) in by_bytes and ec.with_foreign(ec.run(L), g) in by_bytes
        assert ec.with_foreign(ec.run(L), L - 2) in by_bytes
    n_long = int((lens >= lmax - 1).sum())
    if order == "packed":  # the long chunks adjacent, tier by tier
        assert (lens[:n_long] >= lmax - 1).all() and (np.diff(lens[:n_long]) >= 0).all()
    else:  # a long chunk, three short ones, the next long chunk from another tier
        assert (lens[0::4] >= lmax - 1).all() and n_long == len(lens[0::4])
    if table == "T_runs":
        def binary(n, letter):
            return [254 + 2 * k + letter if k else 97 + letter for k in range(14, -1, -1) if n >> k & 1]
        # a run is its length in binary: highest power first, one token per set bit
        for L in ec.lattice_lengths():
            assert by_bytes[ec.run(L)] == binary(L, 0), L
            k = g - 1 if L > g else L // 2
            assert by_bytes[ec.run(k) + ec.run(L - k, ec.B)] == binary(k, 0) + binary(L - k, 1), L  # two runs abut
        three = [by_bytes[ec.run(L)] for L in (top - 1, top, top + 1)]
        assert three[0] != three[1] != three[2] != three[0]
        assert len(three[1]) == 2 and len(three[0]) == 11  # 9216 tokens down to a handful within one call
    if table == "T_alt":
        for L in (mid, mx, top):
            assert len(by_bytes[ec.abab(L, ec.A)]) <= 16 and len(by_bytes[ec.abab(L, ec.B)]) <= 16
        fired = set(t for tk in toks for t in tk)
        assert {257, 260, 261, 264} <= fired  # (a, b) survives somewhere; 261 and 264 are made of every other hand-written rule
    if table == "T_text":
        assert len(set(t for tk in toks for t in tk if t >= 256)) >= 250  # nearly every trained merge is in the output


@pytest.mark.parametrize("table", ["T_runs", "T_alt"])
def test_lds_reuse(table):
    toks, chunks = pinned(ec.lds_reuse(table))
    lens = np.array([len(c) for c in chunks])
    mid, mx, top = (SEAMS[k] for k in ("ENC_LONG_MID", "ENC_LONG_MAX", "ENC_LONG_TOP"))
    assert ((lens > mid) & (lens <= mx)).sum() > SEAMS["LONG_GRID_MAX"]  # more chunks than workgroups: one takes two
    assert ((lens > mx) & (lens <= top)).sum() > SEAMS["LONG_GRID_TOP"]
    assert all(chunks[i] != chunks[i + 1] for i in range(len(chunks) - 1))
    assert min(len(t) for t in toks) <= 3 and max(len(t) for t in toks) > mx  # collapsing and inert chunks side by side


def test_tier_lattice_sparse_ids_equal_the_plain_ids():
    """the T_text lattice with merge ids 1000 + 3 rank: the tokens of the plain table (pinned above), renamed -- the
    reference's loop picks the pair with the lowest id, and the renaming keeps the order of the ids"""
    pairs, mids = ec.t_text_sparse()
    _, _, data, offs = ec.tier_lattice("T_text", "mixed")
    plain, chunks = pinned(ec.tier_lattice("T_text", "mixed"))
    rename = list(range(256)) + list(mids)
    ids, oo = oracle.encode(pairs, data, ec.oracle_offsets(data, offs), merge_ids=mids)
    assert ids.tolist() == [rename[t] for tk in plain for t in tk]
    assert oo.tolist() == np.concatenate([[0], np.cumsum([len(tk) for tk in plain])]).tolist()
    merges = _merges_dict(pairs, mids)
    for ch, tk in zip(chunks, plain):  # ... and the loop itself with the sparse ids, on the chunks of one wave or less
        if len(ch) <= SEAMS["GROUP"] + 1:
            assert ref_encode_chunk(ch, merges) == [rename[t] for t in tk]


@pytest.mark.parametrize("kind", ["key", "hashed", "mixed"])
def test_cache_overflow(kind):
    case = ec.cache_overflow(kind)
    toks, chunks = pinned(case)
    distinct = len(set(chunks))
    slots = ec.cache_slots(len(chunks))
    want_distinct = 24_000 if kind == "mixed" else 12_000
    assert distinct == want_distinct and len(chunks) == want_distinct + (4000 if kind == "mixed" else 2000)
    assert slots == (8192 if kind == "mixed" else SEAMS["ENC_TAB_MIN"])
    assert distinct - slots >= (7904 if kind != "mixed" else 15_000)  # chunks the table has no slot for
    lens = {len(c) for c in chunks}
    assert lens == {"key": {3}, "hashed": {10}, "mixed": {3, 10}}[kind]
    assert 3 <= SEAMS["ENC_KEYBYTES"] < 10 <= SEAMS["ENC_LMAX"]  # their own key | hashed, four words compared
    assert chunks[-1] in chunks[:2000 * (2 if kind == "mixed" else 1)]  # the repeats are of early chunks
    assert len({tuple(t) for t in toks}) > slots  # and the encodings differ as the chunks do


@pytest.mark.parametrize("n_chunks", ec.placement_counts())
def test_placement_tiles(n_chunks):
    case = ec.placement_tiles(n_chunks)
    toks, chunks = pinned(case)
    assert len(chunks) == n_chunks
    ntok = np.array([len(t) for t in toks])
    tile, big, nbig = SEAMS["ENC_PLACE_TILE"], SEAMS["ENC_PLACE_BIG"], SEAMS["ENC_PLACE_NBIG"]
    at = ec.placement_big_at(n_chunks)
    if at is None:
        assert ntok.max() <= 5
        return
    t = at // tile
    in_tile = ntok[t * tile:(t + 1) * tile]
    assert t >= 1 and (in_tile > big).sum() >= nbig + 1  # more big chunks than the tile hands to the workgroup
    assert (in_tile == big).sum() == 1 and (in_tile == big + 1).sum() == 1 and (in_tile == 5000).sum() == 1
    assert (ntok > 5).sum() == nbig + 8 + 3 and (ntok[:t * tile] <= 5).all()
    assert at // SEAMS["SCAN_TILE"] == (at + 2 * (nbig + 8 + 3)) // SEAMS["SCAN_TILE"]  # one tile of the three-launch form too


def test_placement_counts():
    tile, scan = SEAMS["ENC_PLACE_TILE"], SEAMS["SCAN_TILE"]
    counts = ec.placement_counts()
    assert counts == [2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193, 2048 * 65 + 3]
    assert counts[-1] > tile * SEAMS["LOOKBACK"] + tile and counts[-1] % tile == 3  # past one look-back group, short last tile
    assert {tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, scan - 1, scan, scan + 1, 2 * scan + 1} <= set(counts)


def test_empties():
    cases = ec.empties()
    top = SEAMS["ENC_LONG_TOP"]
    for label, case in cases.items():
        toks, chunks = pinned(case)
        assert [len(t) for t, c in zip(toks, chunks) if not c] == [0] * sum(1 for c in chunks if not c), label
    ch = {label: ec.chunks_of(c[2], c[3]) for label, c in cases.items()}
    assert ch["first"][0] == b"" and ch["first"][1] and ch["last"][-1] == b"" and ch["last"][-2]
    assert int(cases["last"][3][-1]) == len(cases["last"][2])  # the last offset is the batch's length
    assert b"".join(b"x" if c else b"." for c in ch["five_in_a_row"]).count(b".....") == 1
    for label, size in (("around_600", 600), ("around_9300", top + 84)):
        i = [len(c) for c in ch[label]].index(size)
        assert ch[label][i - 1] == b"" == ch[label][i + 1]
    assert [len(c) for c in ch["one_byte_only"]] == [0, 0, 1, 0, 0]
    assert SEAMS["ENC_LMAX"] < 600 <= SEAMS["ENC_LONG_MAX"] and top + 84 > top


def test_nul_and_ff():
    case = ec.nul_and_ff()
    toks, chunks = pinned(case)
    by_bytes = dict(zip(chunks, toks))
    assert min(chunks.count(c) for c in set(chunks)) >= 3  # the cache serves every one of them
    w = SEAMS["WORD"]
    for pad in (b"\x00", b"\xff"):
        for L in range(1, 41):
            assert pad * L in by_bytes
        for plen in (1, w, 2 * w, 3 * w):
            fam = sorted((c for c in by_bytes if len(c) >= plen and c[plen - 1:plen] == b"a" and c[plen:] == pad * (len(c) - plen)
                          and (plen == 1 or c[:1] == b"b")), key=len)
            assert len(fam) >= w + 2 and len(fam[0]) == plen and [len(c) for c in fam] == list(range(plen, plen + len(fam)))
            assert len(fam[-1]) > plen + w  # the padding crosses the next word of chunk_words
            # chunks that differ only by trailing NULs (0xFFs) encode differently
            assert all(by_bytes[a] != by_bytes[b] for a, b in zip(fam, fam[1:]))
    assert max(len(c) for c in chunks) > SEAMS["ENC_LMAX"]


def test_tail_alignment():
    cases = ec.tail_alignment()
    assert len(cases) == 40
    seen = set()
    for (r, last), case in cases.items():
        toks, chunks = pinned(case)
        assert len(case[2]) % SEAMS["WORD"] == r and len(chunks[-1]) == last and chunks[-1][-1:] == b"a"
        assert chunks[-1] in chunks[:-1]
        assert toks[-1][-1] == 97  # nothing behind the last byte: the letter stays (a stale 0xFF would merge with it)
        seen.add((len(case[2]) % SEAMS["WORD"], last))
    assert seen == {(r, last) for r in range(8) for last in (1, 7, 8, 9, 32)}
    pre = ec.tail_prefill()
    assert len(pre[2]) == 65536 and set(pre[2]) == {255} and (255, 255) in pre[0]
    assert max(len(c[2]) for c in cases.values()) + 16 < len(pre[2])


@pytest.mark.parametrize("label", list(ec.WIDTH_CASES))
def test_width_seam(native, label):
    M, with_ids, last_id, narrow, highest = ec.WIDTH_CASES[label]
    pairs, mids, data, offs = ec.width_seam(label)
    assert len(pairs) == M and (mids is not None) == with_ids and 19_000 <= len(data) <= 21_000
    toks, _ = pinned((pairs, mids, data, offs))
    top_id = max(t for tk in toks for t in tk)
    assert top_id == highest == (256 + M - 1 if mids is None else int(mids[-1]))  # the last rank fires
    assert native._lib.bpe_encode_uses_16bit(None if mids is None else mids.ctypes.data, M) == narrow
