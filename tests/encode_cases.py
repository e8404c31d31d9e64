"""Deterministic inputs for the seams of batch encode (minbpe_amd/csrc/kernels/k_encode.hip, api/api_encode.hip).

Pure numpy: no GPU, no synth_text.  Every case is (pairs, merge_ids or None, data, offs) -- a merge table in rank
order, the id each merge writes (None: 256 + rank), the batch's bytes and its chunk start offsets (uint64) -- or a
dict {label: such a tuple} where a family is several batches.  tests/test_encode_cases_cpu.py pins oracle.encode on
them to the reference's loop; tests/test_gpu_encode_edges.py runs them through every form of the encoder.

The lengths and counts the cases sit on come from SEAMS alone: one entry per constant of the source, so a change
of the encoder's geometry is a one-line edit here."""
import functools
import os

import numpy as np

import oracle

SEAMS = dict(
    ENC_LMAX=32,           # bpe_device.h ENC_LMAX: longer chunks leave the one-chunk-per-lane kernels
    GROUP=64,              # k_enc_long: one ballot (and one wave of encode_wave) per 64 positions
    ENC_LONG_MID=512,      # k_encode.hip ENC_LONG_MID: k_enc_long<512, 64>, one wave
    ENC_LONG_MAX=4096,     # k_encode.hip ENC_LONG_MAX: k_enc_long<4096, 256>, four waves
    ENC_LONG_TOP=9216,     # k_encode.hip ENC_LONG_TOP: k_enc_long<9216, 1024>, sixteen waves; beyond: huge_list
    LONG_GRID_MAX=512,     # api_encode.hip: k_enc_long<4096, 256> runs on at most 2 * num_cus workgroups (MI355X: 256 CUs)
    LONG_GRID_TOP=256,     # api_encode.hip: k_enc_long<9216, 1024> runs on at most num_cus workgroups
    ENC_KEYBYTES=7,        # k_encode.hip ENC_KEYBYTES: chunks up to here are their own cache key
    ENC_TAB_MIN=4096,      # api_encode.hip tslots: at least 2^12 slots, else the power of two >= n_chunks / 4
    ENC_PROBES=64,         # k_encode.hip ENC_PROBES: slots tried before a chunk goes uncached
    ENC_PLACE_TILE=2048,   # k_encode.hip ENC_PLACE_TILE: chunks per tile of k_enc_place_chained
    ENC_PLACE_BIG=256,     # k_enc_place_chained: more tokens than this -> copied by the whole workgroup
    ENC_PLACE_NBIG=32,     # k_enc_place_chained: ... for at most this many chunks of a tile
    LOOKBACK=64,           # k_enc_place_chained: the look-back reads 64 tile descriptors at a time
    SCAN_TILE=4096,        # bpe_device.h SCAN_TILE: chunks per tile of k_enc_lens / k_enc_place / k_scan_*
    WORD=8,                # chunk_word0 / chunk_words: aligned 64-bit loads
)

A, B, FOREIGN = 97, 98, 99
INERT = tuple(range(0x01, 0x20))  # bytes no table below has in a pair: k of them encode to k tokens
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pack(chunks):
    """(data, start offsets) of a list of chunks"""
    lens = np.fromiter((len(c) for c in chunks), dtype=np.uint64, count=len(chunks))
    offs = np.zeros(len(chunks), dtype=np.uint64)
    if len(chunks) > 1:
        np.cumsum(lens[:-1], out=offs[1:])
    return b"".join(chunks), offs


def chunks_of(data, offs):
    ends = np.append(offs[1:], np.uint64(len(data))).astype(np.int64)
    return [data[int(a):int(b)] for a, b in zip(offs.astype(np.int64), ends)]


def oracle_offsets(data, offs):
    """oracle._offsets takes a final offset equal to len(data) for the terminator: always hand it one, so that a
    trailing empty chunk is not dropped"""
    return np.append(np.asarray(offs, dtype=np.uint64), np.uint64(len(data)))


def cache_slots(n_chunks):
    """slots of the chunk cache for a batch of n_chunks (api_encode.hip: tslots)"""
    t = SEAMS["ENC_TAB_MIN"]
    while t < n_chunks // 4 and t < (1 << 22):
        t <<= 1
    return t


# ---------------------------------------------------------------------------
# merge tables

def _ladder(pairs, tok, levels):
    """(tok, tok) -> X, (X, X) -> Y, ...: appended to pairs, ids 256 + rank; returns the last id"""
    for _ in range(levels):
        pairs.append((tok, tok))
        tok = 255 + len(pairs)
    return tok


@functools.lru_cache(maxsize=None)
def t_runs():
    """a run of one letter collapses to its length's binary digits: 14 levels, the ladders of `a` and `b` rank by
    rank in turn ((97,97) -> 256, (98,98) -> 257, (256,256) -> 258, ...)"""
    pairs, ta, tb = [], A, B
    for _ in range(14):
        ta = _ladder(pairs, ta, 1)
        tb = _ladder(pairs, tb, 1)
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def t_alt():
    """over "abab...": X = (b, a) at rank 0 sits at every odd position and takes the a of every rank-1 (a, b) with it;
    then (a, X), the run of X (an a == a walk over merged tokens), (X, b), and a ladder over X X down to a handful"""
    pairs = [(B, A), (A, B)]            # 256 = X, 257
    pairs += [(A, 256), (256, 256), (256, B)]   # 258 = aX, 259 = XX, 260 = Xb
    pairs.append((258, 259))            # 261 = aX XX (ahead of the ladder, which would pair that XX off to the right)
    pairs.append((259, 259))            # 262: eight bytes
    pairs.append((262, 262))            # 263: sixteen bytes
    pairs.append((259, 260))            # 264 = XX Xb
    _ladder(pairs, 263, 10)             # ... up to 2^14 bytes
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def text_source():
    """the ASCII words of tests/golden/taylorswift.txt, one space apart: 30,000 bytes, none below 0x20"""
    with open(os.path.join(_GOLDEN, "taylorswift.txt"), encoding="utf-8") as f:
        words = [w for w in f.read().split() if w.isascii()]
    text = " ".join(words).encode("ascii")[:30_000]
    assert len(text) == 30_000 and min(text) >= 0x20
    return text


@functools.lru_cache(maxsize=None)
def t_text():
    """300 merges trained on text_source(): realistic, interleaved ranks"""
    return tuple(oracle.train(text_source(), 300, None)[0])


@functools.lru_cache(maxsize=None)
def t_text_sparse():
    """t_text() with merge r writing id 1000 + 3 r: (pairs, merge_ids)"""
    ids = [1000 + 3 * r for r in range(len(t_text()))]
    new = list(range(256)) + ids
    return tuple((new[a], new[b]) for a, b in t_text()), tuple(ids)


@functools.lru_cache(maxsize=None)
def t_nul_ff():
    """merges over 0x00 and 0xFF, and of a letter with each"""
    return ((0, 0), (255, 255), (A, 0), (A, 255), (256, 256), (257, 257), (258, 256), (259, 257), (0, 255))


TABLES = {"T_runs": t_runs, "T_alt": t_alt, "T_text": t_text, "T_nul_ff": t_nul_ff}


def table_is_inert(pairs):
    """no INERT byte occurs in any pair"""
    return not any(a in INERT or b in INERT for a, b in pairs)


# ---------------------------------------------------------------------------
# chunk contents

def run(L, letter=A):
    return bytes([letter]) * L


def abab(L, first=A):
    other = A + B - first
    return (bytes([first, other]) * (L // 2 + 1))[:L]


def inert(L, phase=0):
    return bytes(INERT[(phase + 7 * i) % len(INERT)] for i in range(L))


def text_cut(L, start=0):
    return text_source()[start:start + L]


def with_foreign(chunk, p):
    """one byte that no hand-written table merges, at position p (None if the chunk has no such position)"""
    if not 0 <= p < len(chunk):
        return None
    return chunk[:p] + bytes([FOREIGN]) + chunk[p + 1:]


@functools.lru_cache(maxsize=None)
def short_words():
    """50 distinct words of 1..5 bytes out of text_source()"""
    seen = []
    for w in text_source().split(b" "):
        if 1 <= len(w) <= 5 and w not in seen:
            seen.append(w)
        if len(seen) == 50:
            break
    assert len(seen) == 50
    return tuple(seen)


def word_stream(n, seed):
    """n words of short_words(), drawn with a fixed seed"""
    words = short_words()
    return [words[i] for i in np.random.default_rng(seed).integers(0, len(words), size=n)]


# ---------------------------------------------------------------------------
# tier_lattice: every length at a seam of the long-chunk tiers x every content

def lattice_lengths():
    """one below, at and one above: ENC_LMAX, a ballot group, the three caps of k_enc_long; and one well beyond"""
    out = []
    for name in ("ENC_LMAX", "GROUP", "ENC_LONG_MID", "ENC_LONG_MAX", "ENC_LONG_TOP"):
        out += [SEAMS[name] - 1, SEAMS[name], SEAMS[name] + 1]
    return out + [SEAMS["ENC_LONG_TOP"] + 84]


def lattice_contents(L):
    """{kind: chunk of L bytes}: the contents of the lattice at one length (a foreign byte the chunk has no
    position for is left out)"""
    g = SEAMS["GROUP"]
    out = {
        "run": run(L), "abab_a": abab(L, A), "abab_b": abab(L, B), "inert": inert(L, L), "text": text_cut(L, L % 13),
        "ab_runs": run(g - 1 if L > g else L // 2) + run(L - (g - 1 if L > g else L // 2), B),  # two runs abut
        "run_f63": with_foreign(run(L), g - 1), "run_f64": with_foreign(run(L), g), "run_fL2": with_foreign(run(L), L - 2),
        "abab_a_fL3": with_foreign(abab(L, A), L - 3), "abab_b_f64": with_foreign(abab(L, B), g),
    }
    return {k: v for k, v in out.items() if v is not None}


@functools.lru_cache(maxsize=None)
def tier_lattice(table, order="mixed"):
    """table: a key of TABLES.  order "mixed": tiers alternate from one long chunk to the next and three 1..7-byte
    chunks follow each, so that the three instantiations of k_enc_long and the huge list all have work in one launch;
    "packed": the long chunks adjacent, sorted by length, the short ones after them."""
    lengths = lattice_lengths()
    per_len = {L: lattice_contents(L) for L in lengths}
    kinds = list(per_len[lengths[-1]])
    long_chunks = [per_len[L][k] for k in kinds for L in lengths if k in per_len[L]]
    shorts = [w + bytes([A, B][i % 3:]) for i, w in enumerate(word_stream(3 * len(long_chunks), 11))]  # 1..7 bytes
    if order == "mixed":
        chunks = []
        for i, c in enumerate(long_chunks):
            chunks += [c] + shorts[3 * i:3 * i + 3]
    else:
        chunks = sorted(long_chunks, key=len) + shorts
    data, offs = pack(chunks)
    return TABLES[table](), None, data, offs


@functools.lru_cache(maxsize=None)
def lds_reuse(table):
    """One more chunk of the four-wave tier than k_enc_long<4096, 256> has workgroups, and one more of the sixteen-wave
    tier than k_enc_long<9216, 1024> has: wherever the chunks land on the list, some workgroup of each takes two, the
    second in the LDS buffers the first left behind.  (The one-wave form has more workgroups than the batch can have
    long chunks: n / 33 + 1.)  Contents and lengths differ from one chunk to the next."""
    makers = [lambda L: run(L), lambda L: inert(L, L), lambda L: abab(L, A), lambda L: run(L, B), lambda L: abab(L, B),
              lambda L: with_foreign(run(L), SEAMS["GROUP"])]
    chunks = []
    for i in range(SEAMS["LONG_GRID_TOP"] + 1):
        chunks.append(makers[i % len(makers)](SEAMS["ENC_LONG_MAX"] + 1 + i % 5))
    for i in range(SEAMS["LONG_GRID_MAX"] + 1):
        chunks.append(makers[(i + 2) % len(makers)](SEAMS["ENC_LONG_MID"] + 1 + i % 7))
    data, offs = pack(chunks)
    return TABLES[table](), None, data, offs


# ---------------------------------------------------------------------------
# cache_overflow: more distinct chunks than the cache has slots

def _letters3(i):
    i = (i * 7919) % 17576  # (7919 is coprime to 26^3: distinct i < 17576 give distinct triples, scattered)
    return bytes([A + i // 676, A + i // 26 % 26, A + i % 26])


@functools.lru_cache(maxsize=None)
def cache_overflow(kind):
    """kind "key": 12,000 distinct 3-byte chunks (their own key: enc_probe must give up, ENC_NOSLOT in pass 1), then
    2,000 repeats of the first ones; "hashed": the same with 10-byte chunks (hashed at the full width, the distinct
    part in the first or the second 64-bit word); "mixed": both in one batch, interleaved."""
    n, rep = 12_000, 2_000
    src = text_source()
    key = [_letters3(i) for i in range(n)]
    hashed = [(_letters3(i) + src[i:i + 7]) if i % 2 else (src[i:i + 7] + _letters3(i)) for i in range(n)]
    if kind == "key":
        chunks = key + key[:rep]
    elif kind == "hashed":
        chunks = hashed + hashed[:rep]
    else:
        chunks = [c for pair in zip(key, hashed) for c in pair] + key[:rep] + hashed[:rep]
    data, offs = pack(chunks)
    return t_text(), None, data, offs


# ---------------------------------------------------------------------------
# placement_tiles: chunk counts at the tile seams of the offset scans, big chunks inside a tile

def placement_counts():
    """n_chunks at a tile, a tile +- 1, two tiles (+ 1) of the chained pass and of the three-launch form; and more
    tiles than one look-back group, with a short last one"""
    out = set()
    for t in (SEAMS["ENC_PLACE_TILE"], SEAMS["SCAN_TILE"]):
        out |= {t - 1, t, t + 1, 2 * t, 2 * t + 1}
    out.add(SEAMS["ENC_PLACE_TILE"] * (SEAMS["LOOKBACK"] + 1) + 3)
    return sorted(out)


def placement_big_at(n_chunks):
    """where the group of big chunks starts (None: the batch has none): in the second tile of either form when the
    batch has a second tile's worth of chunks, in the first tile of the second look-back group of the largest"""
    tile, scan = SEAMS["ENC_PLACE_TILE"], SEAMS["SCAN_TILE"]
    if n_chunks > tile * SEAMS["LOOKBACK"]:
        return tile * SEAMS["LOOKBACK"] + 5
    if n_chunks == 2 * scan + 1:
        return scan + 100
    if n_chunks == 2 * tile + 1:
        return tile + 100
    return None


def placement_big_chunks():
    """more chunks of over ENC_PLACE_BIG tokens than a tile hands to the workgroup (inert: a token per byte), one of
    exactly ENC_PLACE_BIG and one of ENC_PLACE_BIG + 1 tokens, one of 5,000"""
    big, nbig = SEAMS["ENC_PLACE_BIG"], SEAMS["ENC_PLACE_NBIG"]
    out = [inert(big + 44, i) for i in range(nbig + 8)]
    return out[:20] + [inert(big, 3)] + out[20:] + [inert(big + 1, 5), inert(5000, 9)]


@functools.lru_cache(maxsize=None)
def placement_tiles(n_chunks):
    chunks = word_stream(n_chunks, n_chunks)
    at = placement_big_at(n_chunks)
    if at is not None:
        for i, c in enumerate(placement_big_chunks()):
            chunks[at + 2 * i] = c  # (every other chunk: ordinary words in between)
    data, offs = pack(chunks)
    return t_text(), None, data, offs


# ---------------------------------------------------------------------------
# empties

@functools.lru_cache(maxsize=None)
def empties():
    w = list(short_words()[:6])
    mid, huge = text_cut(600, 3), text_cut(SEAMS["ENC_LONG_TOP"] + 84, 5)
    batches = {
        "first": [b""] + w,
        "last": w + [b""],
        "five_in_a_row": w[:3] + [b""] * 5 + w[3:],
        "around_600": w[:2] + [b"", mid, b""] + w[2:],
        "around_9300": w[:2] + [b"", huge, b""] + w[2:],
        "one_byte_only": [b"", b"", b"a", b"", b""],
        "everything": [b""] + w[:2] + [b""] * 5 + [mid, b"", b"", huge, b""] + w[2:] + [b"", b""],
    }
    out = {}
    for label, chunks in batches.items():
        data, offs = pack(chunks)
        out[label] = (t_text(), None, data, offs)
    return out


# ---------------------------------------------------------------------------
# nul_and_ff: chunks that differ only by trailing 0x00 (the zero padding of chunk_words) or 0xFF

@functools.lru_cache(maxsize=None)
def nul_and_ff():
    w = SEAMS["WORD"]
    chunks = []
    for pad in (0, 255):
        for plen in (1, w, 2 * w, 3 * w):  # the prefix ends with `a`: (a, 0) and (a, 255) are in the table
            prefix = (b"bcdefghi" * 3)[:plen - 1] + bytes([A])
            top = SEAMS["ENC_LMAX"] + 1 - plen if plen == 1 else w + 1
            chunks += [prefix + bytes([pad]) * j for j in range(top + 1)]
        chunks += [bytes([pad]) * L for L in range(1, 41)]
    chunks = chunks * 3
    order = np.random.default_rng(17).permutation(len(chunks))
    data, offs = pack([chunks[i] for i in order])
    return t_nul_ff(), None, data, offs


# ---------------------------------------------------------------------------
# tail_alignment: the aligned loads of the last chunk read up to 7 bytes past the batch

@functools.lru_cache(maxsize=None)
def tail_prefill():
    """64 KiB of 0xFF: what the device buffer holds before the small batches (the table merges (255, 255))"""
    data = b"\xff" * 65536
    return t_nul_ff(), None, data, np.arange(0, len(data), 16, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def tail_alignment():
    """{(r, last): batch}: total length = r (mod 8), a last chunk of `last` bytes that ends with `a` -- a stale 0xFF
    behind it would merge --, the same chunk earlier in the batch (so that the cache has a slot for it), fillers"""
    w = SEAMS["WORD"]
    out = {}
    for r in range(w):
        for last in (1, SEAMS["ENC_KEYBYTES"], w, w + 1, SEAMS["ENC_LMAX"]):
            tail = (b"\xffa" * last)[-last:]
            filler = b"\xff" * ((r - 2 * last - 3) % w + w)
            chunks = [b"a\xff\xff", tail, filler, tail]
            data, offs = pack(chunks)
            assert len(data) % w == r
            out[(r, last)] = (t_nul_ff(), None, data, offs)
    return out


# ---------------------------------------------------------------------------
# the switch between 16-bit and 32-bit token / rank columns (bpe_encode_uses_16bit, k_encode_short)

WIDTH_CASES = {  # label: (M, merge ids?, id of the last merge or None for 256 + rank, bpe_encode_uses_16bit, highest id)
    "M65280": (65280, False, None, 1, 65535),
    "M65281": (65281, False, None, 0, 65536),
    "M65534_ids": (65534, True, 65535, 1, 65535),
    "M65535_ids": (65535, True, 65535, 0, 65535),
    "M65534_one_id_65536": (65534, True, 65536, 0, 65536),
}


@functools.lru_cache(maxsize=None)
def width_probe():
    """about 20 KB of text_source(), one chunk per word (the space leads)"""
    words = text_source()[8000:28000].split(b" ")
    return pack([words[0]] + [b" " + x for x in words[1:]])


@functools.lru_cache(maxsize=None)
def _width_base():
    """65,000 merges around t_text() (helpers.cl100k_shaped_table, ids 256 + rank), and the pairs that take part"""
    from helpers import cl100k_shaped_table
    pairs, _ = cl100k_shaped_table(list(t_text()), 65_000, 7)
    return pairs


@functools.lru_cache(maxsize=None)
def width_seam(label):
    """A table of exactly M merges whose LAST rank fires on width_probe().  Ranks 0 .. 64,999: the cl100k-shaped table;
    from there to M - 2: pairs of INERT bytes, which the probe does not contain (never merged, they only count); rank
    M - 1: the most frequent pair of adjacent tokens the probe encodes to under the M - 1 merges before it.
    With ids, merge r writes 256 + r as long as that stays below 65535 -- no table of 65,534 merges can have distinct
    ids below 65536 next to the 256 bytes, so the inert merges beyond share 65534, an id that is never written -- and
    the last merge writes the id the case names."""
    M, with_ids, last_id, _, _ = WIDTH_CASES[label]
    base = _width_base()
    have = {(int(a), int(b)) for a, b in base}
    fill = [(a, b) for a in INERT for b in INERT if (a, b) not in have][:M - 1 - len(base)]
    assert len(fill) == M - 1 - len(base)
    pairs = np.concatenate([base, np.array(fill, dtype=np.int32)])
    mids = np.minimum(256 + np.arange(M, dtype=np.int64), 65534).astype(np.int32) if with_ids else None
    data, offs = width_probe()
    ids, oo = oracle.encode(pairs, data, oracle_offsets(data, offs), merge_ids=None if mids is None else mids[:M - 1])
    inner = np.ones(len(ids), dtype=bool)  # positions whose right neighbour is in the same chunk
    inner[oo[1:].astype(np.int64) - 1] = False
    cand = {}
    for p in np.flatnonzero(inner):
        k = (int(ids[p]), int(ids[p + 1]))
        cand[k] = cand.get(k, 0) + 1
    last = max(cand, key=lambda k: (cand[k], k))
    assert last not in have and last not in set(fill)  # (else an earlier rank would have merged it)
    pairs = np.concatenate([pairs, np.array([last], dtype=np.int32)])
    if with_ids:
        mids[M - 1] = last_id
    assert len(pairs) == M
    return pairs, mids, data, offs
