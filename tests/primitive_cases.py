"""Id streams beyond the byte range for the single-step API (bpe_load_ids, bpe_get_stats, bpe_argmax, bpe_merge).

Every case is a small deterministic function that returns (ids int32, chunk start offsets uint64 or None) and is
named for the branch of the engine it is meant to reach: a table width, a regime of k_select's contiguous form, a
place of the first occurrence that decides a tie, a merge whose new id grows the table.  classify() says, from
oracle.get_stats alone, what select_core would see in a stream; tests/test_primitive_cases_cpu.py pins that every
case has the property it is named for, tests/test_gpu_primitives_wide.py runs them on the device.

No GPU, no torch: numpy and the CPU oracle.

How the streams are made.  A chunk of two ids [a, b] adds exactly one to the count of (a, b) and nothing else (no
pair forms across a chunk start), so a block of such chunks sets counts and first occurrences exactly.  _filler()
is a long chunk-free stretch in which every pair occurs exactly once: block j = 1, 2, ... of it is the arithmetic
progression 0, j, 2j, ... modulo the prime FILL_A, which holds every pair of difference j once, the last of them
astride the junction with the next block.  Fillers use ids FILL_BASE .. FILL_BASE + FILL_A - 1, tied pairs ids from
TIED_BASE up, so the two never share a pair.
"""
import collections
import functools

import numpy as np

import oracle

# what the engine's code says (pinned against the sources in test_primitive_cases_cpu.py)
TILE = 4096           # ids per tile of the contiguous view (view_tile(SlotRef))
TIE_CAP = 96          # tied pairs listed explicitly
ARGMAX_ROWS = 2048    # multi-column rows scanned
TIE_BLOCKS = 256      # workgroups of the tie sweep
SEL_ROWS = 20 * 1024  # row maxima kept in registers (SEL_RPT x 1024)
TIE_WIN = 8           # tiles option "tie_window" covers

FILL_A = 1031
FILL_BASE = 2
FILL_MAX = FILL_A * (FILL_A - 1) + 1
TIED_BASE = 1100

Regime = collections.namedtuple("Regime", "M single_rows multi_rows tied pos pair")


def classify(ids, offsets=None):
    """What select_core sees: the maximum M, the rows at M whose maximum one column / several columns attain, the number
    of tied pairs, and the position and pair of the first occurrence among them (the reference's answer)."""
    st = oracle.get_stats(ids, offsets)
    if not st:
        return Regime(0, 0, 0, 0, None, None)
    M = max(c for _, c, _ in st)
    cols = {}
    pos, pair = None, None
    for p, c, f in st:
        if c != M:
            continue
        cols[p[0]] = cols.get(p[0], 0) + 1
        if pos is None or f < pos:
            pos, pair = f, p
    return Regime(M, sum(1 for v in cols.values() if v == 1), sum(1 for v in cols.values() if v > 1),
                  sum(cols.values()), pos, pair)


def _filler(n, start=0):
    """n ids, no chunk start, every pair exactly once (start: skip that many ids of the sequence)."""
    assert start + n <= FILL_MAX
    i = np.arange(start, start + n, dtype=np.int64)
    return (FILL_BASE + (i % FILL_A) * (i // FILL_A + 1) % FILL_A).astype(np.int32)


class _Stream:
    """Chunks laid end to end."""

    def __init__(self):
        self.parts, self.starts, self.n = [], [], 0

    def chunk(self, ids):
        ids = np.asarray(ids, dtype=np.int32).reshape(-1)
        assert len(ids)
        self.starts.append(np.array([self.n], np.uint64))
        self.parts.append(ids)
        self.n += len(ids)
        return self.n - len(ids)

    def pairs(self, pairs):
        """one two-id chunk per pair, in the order given; returns the position of the first"""
        p = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        at = self.n
        self.starts.append(at + 2 * np.arange(len(p), dtype=np.uint64))
        self.parts.append(p.reshape(-1))
        self.n += 2 * len(p)
        return at

    def done(self):
        return np.concatenate(self.parts).astype(np.int32), np.concatenate(self.starts).astype(np.uint64)


def _rounds(s, tied, M, first):
    """M rounds of the tied pairs as two-id chunks; the first round begins with tied[first].  Returns its position."""
    tied = np.asarray(tied, np.int32).reshape(-1, 2)
    at = s.pairs(np.roll(tied, -first, axis=0))
    for _ in range(M - 1):
        s.pairs(tied)
    return at


def _single_rows(T, base=TIED_BASE):
    """T pairs in T distinct rows (and columns)"""
    r = base + 2 * np.arange(T)
    return np.stack([r, r + 1], axis=1)


# ---------------------------------------------------------------------------
# table width

WIDTHS = (257, 300, 1024, 1919, 1920, 1921, 2048, 2049, 20479, 20480, 20481)
WIDTH_VARIANTS = ("row", "col", "run")


@functools.lru_cache(maxsize=None)
def width_case(V, variant):
    """About 5000 ids over {0, 1, 255, 256, V - 2, V - 1}, chunk starts in the body (two of them neighbours, one inside
    the run), and a unique maximum in row V - 1 ("row": pair (V - 1, 0)), in column V - 1 ("col": (0, V - 1)) or at
    (V - 1, V - 1) ("run": a run of 301 ids behind a chunk that ends in 150 more).  max id + 1 == V."""
    alphabet = np.array(sorted({0, 1, 255, 256, V - 2, V - 1}), np.int32)
    rng = np.random.default_rng(1000 * V + WIDTH_VARIANTS.index(variant))
    body = alphabet[rng.integers(0, len(alphabet), size=4403)]
    s = _Stream()
    s.chunk(body[:1237])
    s.chunk(body[1237:1238])
    s.chunk(body[1238:2601])
    if variant == "run":
        s.chunk(np.concatenate([body[2601:2700], np.full(150, V - 1, np.int32)]))
        s.chunk(np.concatenate([np.full(301, V - 1, np.int32), body[2700:]]))
    else:
        s.chunk(body[2601:2700])
        s.pairs([(V - 1, 0) if variant == "row" else (0, V - 1)] * 300)
        s.chunk(body[2700:])
    return s.done()


WIDTH_PAIR = {"row": lambda V: (V - 1, 0), "col": lambda V: (0, V - 1), "run": lambda V: (V - 1, V - 1)}


# ---------------------------------------------------------------------------
# selection regimes

def sel_unique():
    """a unique maximum: (1500, 1400) three times among pairs that occur once or twice"""
    s = _Stream()
    s.chunk(_filler(3001))
    _rounds(s, [(1400, 1500), (1500, 1400), (1500, 1501)], 2, 1)
    s.pairs([(1500, 1400)])
    s.chunk(_filler(2000, 3001))
    return s.done()


def sel_tied(T, lead=4099, M=3):
    """T tied pairs (count M) in T distinct rows behind `lead` filler ids; the first to occur is pair T // 2: neither the
    smallest ids nor the first row."""
    s = _Stream()
    s.chunk(_filler(lead))
    _rounds(s, _single_rows(T), M, T // 2)
    s.chunk(_filler(1500, lead))
    return s.done()


def _multi_rows(R):
    """R rows, each with the same two columns"""
    rows = TIED_BASE + np.arange(R)
    return np.stack([np.repeat(rows, 2), np.tile(np.array([TIED_BASE + R, TIED_BASE + R + 1]), R)], axis=1)


def sel_multi(R, S=0):
    """R rows whose maximum (2) two columns attain, 8 ids per row, plus S rows with a single column at the maximum; the
    first tied pair to occur is the second column of row R // 2.  V = TIED_BASE + R + 2 (+ 2 S)."""
    tied = _multi_rows(R)
    if S:
        tied = np.concatenate([tied, _single_rows(S, TIED_BASE + R + 2)])
    s = _Stream()
    s.chunk(_filler(101))
    _rounds(s, tied, 2, 2 * (R // 2) + 1)
    return s.done()


def sel_side(hi):
    """Tied rows on both sides of row 20480 (row 20480 itself with two columns); the winner is in row 20480 (hi) or in
    row 20479."""
    tied = [(1050, 1051), (20479, 7), (20480, 20480), (20480, 255), (5000, 20480), (1040, 1041)]
    s = _Stream()
    s.chunk(_filler(4100))
    _rounds(s, tied, 3, 3 if hi else 1)
    return s.done()


SELECTION = {
    "unique": sel_unique,
    **{f"tied_{T}": functools.partial(sel_tied, T) for T in (2, 95, 96, 97)},
    **{f"multi_{R}": functools.partial(sel_multi, R) for R in (1, 2047, 2048, 2049)},
    "multi_1_single_94": functools.partial(sel_multi, 1, 94),   # 96 pairs: still listed
    "multi_1_single_95": functools.partial(sel_multi, 1, 95),   # the row scan takes the list past TIE_CAP
    # 96 listed pairs AND a multi-column row that holds the winner: the row must still be scanned at s_nt == TIE_CAP
    "multi_1_single_96": functools.partial(sel_multi, 1, 96),
    "multi_2048_single_97": functools.partial(sel_multi, 2048, 97),
    "side_hi": functools.partial(sel_side, True),
    "side_lo": functools.partial(sel_side, False),
}
# name -> (tied pairs, single-column rows, multi-column rows) the case claims
SELECTION_REGIME = {
    "unique": (1, 1, 0),
    **{f"tied_{T}": (T, T, 0) for T in (2, 95, 96, 97)},
    **{f"multi_{R}": (2 * R, 0, R) for R in (1, 2047, 2048, 2049)},
    "multi_1_single_94": (96, 94, 1),
    "multi_1_single_95": (97, 95, 1),
    "multi_1_single_96": (98, 96, 1),
    "multi_2048_single_97": (4096 + 97, 97, 2048),
    "side_hi": (6, 4, 1),
    "side_lo": (6, 4, 1),
}


# ---------------------------------------------------------------------------
# where the deciding first occurrence lies.  Every builder returns (ids, offsets, position of that occurrence).

FIRST_T = (5, 120)  # tied pairs: listed (<= TIE_CAP) / tested against the table (> TIE_CAP)


def first_at(T, where):
    """T tied pairs; the winner's first occurrence is at position `where` (filler before it, every other tied pair
    after it)."""
    s = _Stream()
    if where:
        s.chunk(_filler(where))
    at = _rounds(s, _single_rows(T), 3, T // 2)
    assert at == where
    s.chunk(_filler(777, where))
    return s.done() + (where,)


def first_tail(T):
    """The stream's LAST pair, at n - 2, is the winner's third occurrence: whoever does not count position n - 2 drops
    the winner out of the tie.  (A tie cannot be decided by a FIRST occurrence at n - 2: every other tied pair would
    have to occur first later still.  This is the case that position can make.)  The winner first occurs in tile 1."""
    tied = _single_rows(T)
    w = T // 2
    s = _Stream()
    s.chunk(_filler(4500))
    at = s.pairs(np.roll(tied, -w, axis=0))
    s.pairs(tied)
    s.chunk(_filler(700, 4500))
    s.pairs(np.delete(tied, w, axis=0))
    s.chunk(np.concatenate([_filler(2, 5200), tied[w]]))
    return s.done() + (at,)


def first_astride(T):
    """Tied pairs P = (1100, 1101) and W = (1101, 1102) among T.  W's first occurrence opens a chunk at position p, and
    the chunk before it ends in 1100: the words at p - 1 and p spell P, which occurs only later.  A sweep that forgets
    the chunk-start flag answers P."""
    tied = np.concatenate([np.array([(1100, 1101), (1101, 1102)]), _single_rows(T - 2, TIED_BASE + 10)])
    s = _Stream()
    s.chunk(_filler(4200))
    s.chunk([1105, 1100])
    at = _rounds(s, tied, 3, 1)
    s.chunk(_filler(777, 4200))
    return s.done() + (at,)


FIRST = {}
for _T in FIRST_T:
    FIRST[f"pos0_{_T}"] = functools.partial(first_at, _T, 0)
    FIRST[f"tail_{_T}"] = functools.partial(first_tail, _T)
    FIRST[f"tile0_last_word_{_T}"] = functools.partial(first_at, _T, TILE - 1)
    FIRST[f"tile256_{_T}"] = functools.partial(first_at, _T, TIE_BLOCKS * TILE + 37)   # the only streams above 100 k ids
    FIRST[f"astride_{_T}"] = functools.partial(first_astride, _T)

TIE_WINDOW = {}
for _T in FIRST_T:
    TIE_WINDOW[f"tile7_last_word_{_T}"] = functools.partial(first_at, _T, TIE_WIN * TILE - 1)
    TIE_WINDOW[f"tile8_first_word_{_T}"] = functools.partial(first_at, _T, TIE_WIN * TILE)
    TIE_WINDOW[f"tile12_{_T}"] = functools.partial(first_at, _T, 12 * TILE + 123)


@functools.lru_cache(maxsize=None)
def argmax_case(name):
    """(ids, offsets, Regime) of a selection, first-occurrence or tie_window case, built and classified once"""
    made = (SELECTION.get(name) or FIRST.get(name) or TIE_WINDOW[name])()
    ids, offsets = made[0], made[1]
    return ids, offsets, classify(ids, offsets)


# ---------------------------------------------------------------------------
# merges

MERGE_V = (300, 1921, 2049, 20481)
MERGE_IDX_BELOW = 258  # an id below every V that no stream holds


@functools.lru_cache(maxsize=None)
def merge_stream(V):
    """12501 ids over {0, 255, 256, V - 2, V - 1}.  Runs of V - 1: 11 ids across the tile boundary at 4096, 12 ids across
    the one at 8192, 7 ids cut 3 + 4 and 8 ids cut 4 + 4 by a chunk start.  (V - 2, V - 1) astride a chunk start (5000,
    5001: not a pair) and astride the tile boundary at 12288 (a pair)."""
    alphabet = np.array([0, 255, 256, V - 2, V - 1], np.int32)
    ids = alphabet[np.random.default_rng(7 * V).integers(0, 5, size=12501)]
    for lo, hi in ((4090, 4101), (8186, 8198), (6000, 6007), (7000, 7008)):
        ids[lo - 1] = ids[hi] = 0
        ids[lo:hi] = V - 1
    ids[5000], ids[5001] = V - 2, V - 1
    ids[12287], ids[12288] = V - 2, V - 1
    return ids, np.array([0, 1237, 1238, 5001, 6003, 7004, 12400], np.uint64)


def merge_cases(V):
    """(pair, idx): an a != b pair and an a == a run pair with ids at V - 1, into an id below V and into V + 1000"""
    return [(pair, idx) for idx in (MERGE_IDX_BELOW, V + 1000) for pair in ((V - 2, V - 1), (V - 1, V - 1))]


# ---------------------------------------------------------------------------
# the loop by hand

HAND_ITERS = 40
HAND_NEW = 2100  # iteration i merges into HAND_NEW + i
HAND_ALPHABET = np.array(sorted([250, 255, 256, 257, 300, 511, 512, 1023, 1024, 1025, 1500, 1919, 1920, 1921, 2047,
                                 2048, 2049, 2098, 2099] + [320 + 70 * k for k in range(22)]), np.int32)


@functools.lru_cache(maxsize=None)
def hand_stream():
    """About 17 k ids over 41 ids in [250, 2099], a chunk start every 997 ids.  Block j = 1 .. 40 is the progression 0, j,
    2j, ... modulo 41 over the alphabet: every pair of difference j once.  Twelve rounds of the blocks, each closed by a run
    of 31 x 2099; blocks 1 .. 3 are in all twelve rounds, the others in 9 to 11: the 123 pairs of difference 1 .. 3 tie at
    the top once the runs are merged, and drop out of the tie as their neighbours are merged."""
    A = len(HAND_ALPHABET)
    assert A == 41 and len(set(HAND_ALPHABET.tolist())) == A
    k = np.arange(A, dtype=np.int64)
    parts = []
    for r in range(12):
        for j in range(1, A):
            if r < (12 if j <= 3 else 11 - j % 3):
                parts.append(HAND_ALPHABET[k * j % A])
        parts.append(np.full(31, 2099, np.int32))
    ids = np.concatenate(parts).astype(np.int32)
    return ids, np.arange(0, len(ids), 997, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def hand_loop():
    """The reference loop on hand_stream(): [(pair, count, tied pairs, length after the merge)] per iteration."""
    ids, off = hand_stream()
    out = []
    for i in range(HAND_ITERS):
        st = oracle.get_stats(ids, off)
        best = max(st, key=lambda e: e[1])  # the first maximum in insertion order
        ids, off = oracle.merge_chunks(ids, off, best[0], HAND_NEW + i)
        out.append((best[0], best[1], sum(1 for e in st if e[1] == best[1]), len(ids)))
    return out
