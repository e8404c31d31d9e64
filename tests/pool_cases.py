"""Byte streams that put training at the capacity seams of the pool (k_pool.hip: pool_sel_body, pool_finish,
k_pool_sel_dp): rows a rebuild hands out, pairs it gathers, entries the pool keeps, entries located per selection and
below the walk's reach.

Every case is a small deterministic function of its form ("bare" | "body") that returns (data bytes, chunk start
offsets uint64) and is named for the branch it is meant to reach.  rebuild_view() is the rebuild rule of k_pool.hip's
header comment in plain Python, from oracle.get_stats output alone; tests/test_pool_cases_cpu.py pins that every case
has the property it is named for, tests/test_gpu_pool_seams.py trains them on the device.

No GPU, no torch: numpy and the CPU oracle.

How the streams are made.  A two-byte chunk [a, b] adds exactly one to the count of (a, b) and nothing else, so blocks
of such chunks set counts, rows (a row = a first token) and first occurrences exactly.  The bytes 0 .. 251 are split,
per family of cases, into first tokens, second tokens and a filler set: no designed pair has a == b, and none chains
onto another because no first token is a second token.
  bare   two-byte chunks only;
  body   the same pairs inside four-byte chunks [L, a, b, R], L and R from the filler set: the k-th occurrence of a
         first token a takes the k-th filler (cyclically), and the same for b, which is the most even spread there is:
         (L, a) counts ceil(occurrences of a / fillers), and the heirs (L, Z), (Z, R) of a merge count no more.  The
         merges then have neighbours, so the table update and the pool's maintenance run at the seam too.
The first occurrence of every designed pair lies in the stream's first round, whose order is a seeded shuffle:
pool_sort breaks equal counts by pair value, and a selection that skipped the locate would merge in pair order.

The head.  Merge 0 of every training run is no chain step: its selection is the general path's (it is the one merge whose
row maxima are built in full; chain steps start at merge 1).  Every stream therefore ends in HEAD = (252, 253) as two-byte chunks, once more
often than the designed maximum: it is merge 0, it has no neighbours, and what the FIRST chain step -- a rebuild: a
fresh load has no pool -- sees is the statistics after it.  case_stats() returns those, and they are what the properties
below are stated of.

The tail.  Below the designed pairs (and above the noise of a body form) every stream carries TAIL pairs in six rows
of their own, in small levels, so that a run of num_merges = 1 + designed + tail passes the seam and the pool is
maintained and rebuilt afterwards without reaching the noise.  At M = 2 the only count below the seam is 1: the bare
form's tail is one level of 36 pairs there, and the body form -- whose neighbours (L, a), (b, R) all count 1, hundreds
of them in one level, a hand-back of its own -- ends with the designed pairs.

Out of scope here: CH_EX_CAP (more than 2048 flagged rows in one rebuild) needs a vocabulary past 2300 ids with all of
it dirty, which no stream of bytes a few hundred KB long reaches; and maintenance that makes more variants than
PL_GATHER, which tests/test_gpu_chain_share_first.py and tests/test_level_model_shared_firsts.py build.
"""
import collections
import functools

import numpy as np

import oracle

# what the engine's code says (pinned against the sources in test_pool_cases_cpu.py)
PL_CAP = 256          # entries the pool holds
PL_ROWS = 128         # rows a rebuild hands to the scanning workgroups
PL_GATHER = 1024      # pairs a rebuild may gather
TIE_CAP = 96          # entries located per selection
BELOW_REACH = 16      # ... of which in levels below the walk's reach
SHIFTS = (2, 3, 4, 5, 6, 7, 8)  # candidate thresholds M - (M >> s), and M itself
CHAIN_SCAN = 127      # scanning workgroups of a rebuild (option chain_scan)
CHAIN_KCAP = 31       # most pairs of a batch (option chain_kcap; CH_KSWEEP)

HEAD = (252, 253)
N_BYTES = 252         # bytes 0 .. 251 are dealt to the three sets
TAIL = 36
TAIL_ROWS = 6
FORMS = ("bare", "body")

View = collections.namedtuple("View", "M thresholds rows picked theta pairs levels kept")


def rebuild_view(stats, n_rows=PL_ROWS):
    """What a rebuild makes of a pair table (k_pool.hip, "rebuild"): the maximum M; the eight candidate thresholds, deepest
    first (M - (M >> s) for s = 2 .. 8, then M); the rows (first tokens) whose maximum reaches each; the index of the
    threshold picked -- the deepest that at most n_rows rows reach -- or None where more rows hold the maximum itself; that
    threshold (None likewise); the pairs at or above it (at the maximum where none is picked); the sizes of their count
    levels from the top; and the entries the pool keeps of them: whole levels leave from the bottom until at most PL_CAP
    are left (0: one level larger than the pool)."""
    if not stats:
        return View(0, (), (), None, None, 0, (), 0)
    rowmax = {}
    for (a, _b), c, _f in stats:
        rowmax[a] = max(rowmax.get(a, 0), c)
    M = max(rowmax.values())
    th = tuple(M - (M >> s) for s in SHIFTS) + (M,)
    rows = tuple(sum(1 for v in rowmax.values() if v >= t) for t in th)
    picked = next((k for k in range(8) if rows[k] <= n_rows), None)
    theta = th[picked] if picked is not None else None
    cs = sorted((c for _p, c, _f in stats if c >= (theta if theta is not None else M)), reverse=True)
    levels = tuple(collections.Counter(cs)[c] for c in sorted(set(cs), reverse=True))
    kept = len(cs)
    if kept > PL_CAP:
        kept = PL_CAP
        while kept > 0 and cs[kept - 1] == cs[kept]:
            kept -= 1
    return View(M, th, rows, picked, theta, len(cs), levels, kept)


# ---------------------------------------------------------------------------
# the builder

def _rank_in_group(keys):
    """rank of every element among the earlier elements with the same key"""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    start = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    first = np.repeat(start, np.diff(np.concatenate([start, [len(sk)]])))
    out = np.empty(len(keys), np.int64)
    out[order] = np.arange(len(keys)) - first
    return out


def tail_counts(M):
    """counts of the TAIL pairs under a designed maximum M: far below M - (M >> 2), above the noise of a body form"""
    j = np.arange(TAIL)
    if M >= 256:
        return M // 2 - j // 2          # levels of 2
    if M >= 8:
        return np.maximum(2, M // 4 - j // 6)  # levels of 6; one level at 2 for M = 8
    return np.ones(TAIL, np.int64)      # M = 2: count 1, bare form only


class Case:
    """designed: [(row index, column index, count)] -- row r is first token r, column c second token n_first + c"""

    def __init__(self, name, n_first, n_second, designed, seed, doc, opts=(), tail=True):
        self.name, self.doc, self.opts, self.seed = name, doc, tuple(opts), seed
        self.n_first, self.n_second = n_first, n_second
        assert n_second >= TAIL_ROWS and n_first + TAIL_ROWS + n_second <= N_BYTES - 32
        self.fillers = np.arange(n_first + TAIL_ROWS + n_second, N_BYTES)
        d = np.asarray(designed, np.int64).reshape(-1, 3)
        assert d[:, 0].max() < n_first and d[:, 1].max() < n_second
        self.pairs = np.stack([d[:, 0], n_first + TAIL_ROWS + d[:, 1]], axis=1)
        self.counts = d[:, 2].copy()
        assert len({tuple(p) for p in self.pairs.tolist()}) == len(self.pairs)
        self.M = int(self.counts.max())
        j = np.arange(TAIL)
        self.tail_pairs = np.stack([n_first + j % TAIL_ROWS, n_first + TAIL_ROWS + (j // TAIL_ROWS) % n_second], axis=1)
        self.tail_cnt = tail_counts(self.M)
        self.with_tail = tail

    def has_tail(self, form):
        return self.with_tail and not (form == "body" and self.M < 8)

    def designed(self):
        return [tuple(p) for p in self.pairs.tolist()]

    def num_merges(self, form):
        return 1 + len(self.pairs) + (TAIL if self.has_tail(form) else 0)

    def build(self, form):
        assert form in FORMS
        pairs, counts = self.pairs, self.counts
        if self.has_tail(form):
            pairs = np.concatenate([pairs, self.tail_pairs])
            counts = np.concatenate([counts, self.tail_cnt])
        rng = np.random.default_rng(self.seed)
        first_round = rng.permutation(len(self.pairs))  # (the tail keeps its order behind it: it is no seam)
        occ = np.concatenate([first_round, np.arange(len(self.pairs), len(pairs)), np.repeat(np.arange(len(pairs)), counts - 1)])
        ab = pairs[occ]
        if form == "bare":
            body, width = ab, 2
        else:
            nf = len(self.fillers)
            L = self.fillers[(_rank_in_group(ab[:, 0]) + ab[:, 0]) % nf]
            R = self.fillers[(_rank_in_group(ab[:, 1]) + 7 * ab[:, 1]) % nf]
            body, width = np.stack([L, ab[:, 0], ab[:, 1], R], axis=1), 4
        head = np.tile(np.array(HEAD), self.M + 1)
        data = np.concatenate([body.reshape(-1), head]).astype(np.uint8)
        offs = np.concatenate([width * np.arange(len(body)), width * len(body) + 2 * np.arange(self.M + 1)])
        return data.tobytes(), offs.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def stream(name, form):
    """(data, offsets) of a case, built once"""
    return CASES[name].build(form)


def chunks_of(data, offs):
    ends = np.append(offs[1:], np.uint64(len(data))).astype(np.int64)
    return [data[int(a):int(b)] for a, b in zip(offs.astype(np.int64), ends)]


@functools.lru_cache(maxsize=None)
def case_stats(name, form):
    """oracle.get_stats after merge 0 -- the head --: what the first chain step, a rebuild, sees"""
    data, offs = stream(name, form)
    ids = np.frombuffer(data, dtype=np.uint8).astype(np.int32)
    st0 = oracle.get_stats(ids, offs)
    best = max(st0, key=lambda e: e[1])
    assert best[0] == HEAD and best[1] == CASES[name].M + 1
    ids, off = oracle.merge_chunks(ids, offs, HEAD, 256)
    return oracle.get_stats(ids, off[:-1])


def replay(data, offs, pairs):
    """(ids, chunk starts) of the resident stream after the merges, by oracle.merge_chunks"""
    ids, off = np.frombuffer(data, dtype=np.uint8).astype(np.int32), np.append(offs, np.uint64(len(data)))
    for i, p in enumerate(pairs):
        ids, off = oracle.merge_chunks(ids, off[:-1], p, 256 + i)
    return ids, sorted(set(int(off[c]) for c in range(len(off) - 1) if off[c + 1] > off[c]))


def replay_by_encode(data, offs, pairs):
    """the same by oracle.encode: one pass instead of one per merge (no chunk of these streams is empty, before or after)"""
    ids, off = oracle.encode(pairs, data, offs)
    return ids, [int(x) for x in off[:-1]]


def is_big(name):
    """the gather cases: a megabyte or two and a thousand merges -- the plain loop takes half a minute per form, one
    oracle.merge_chunks per merge seconds more"""
    return name.startswith("gather_")


@functools.lru_cache(maxsize=None)
def expected(name, form, nm=None):
    """oracle.train of a case, and the resident stream and chunk starts it leaves (its pairs replayed with
    oracle.merge_chunks): (pairs, counts, lens, ids, starts).  The gather cases take oracle.train_fast and oracle.encode
    instead, which test_pool_cases_cpu.py pins to the plain ones on these very streams."""
    data, offs = stream(name, form)
    nm = CASES[name].num_merges(form) if nm is None else nm
    # (no case is meant to run empty: raise_on_empty stays on)
    pairs, counts, lens = (oracle.train_fast if is_big(name) else oracle.train)(data, nm, offs)
    ids, starts = (replay_by_encode if is_big(name) else replay)(data, offs, pairs)
    return pairs, counts, lens, ids, starts


# ---------------------------------------------------------------------------
# the cases

CASES = {}
# name -> what rebuild_view(case_stats(...)) must report, both forms: dict of View fields (levels: a prefix)
PROPERTY = {}
# name -> "within" | "over" | None: what train_stats() must say (test_gpu_pool_seams.py); DEFERRED: the exact figure where
# the code fixes it (every merge a chain step, lean_backoff = 0: one general merge per hand-back)
CAPACITY = {}
DEFERRED = {}


def _add(case, prop, capacity, deferred=None):
    CASES[case.name] = case
    PROPERTY[case.name] = prop
    CAPACITY[case.name] = capacity
    if deferred is not None:
        DEFERRED[case.name] = deferred


def _grid(n, rows, cols):
    """n distinct (row, column) pairs over rows x cols, row-cyclic: pair k sits in row k % rows"""
    assert n <= rows * cols
    k = np.arange(n)
    return k % rows, (k // rows + k % rows) % cols


# ---- rows at the maximum.  N rows hold one pair each at M, so they tie: a level of N entries.  N > PL_ROWS: no threshold
# is picked, `ks < 0`, defer = 2.  N <= PL_ROWS: the rebuild gathers them, but a level of more than TIE_CAP entries cannot
# be located and stays without an order, K == 0, defer = 2 -- the pool is dropped, the general path merges one pair, the
# next step rebuilds: N - TIE_CAP hand-backs in all, whichever of the two branches a step takes.  So `deferred` counts
# N - 96 for 127, 128 and 129 rows alike; what tells 128 from 129 is parity (the 128th row has a scanning workgroup of its
# own at chain_scan >= 128 only: at the default 127 the gather's `j += nblk - 1` loop goes round a second time) and the
# properties pinned on the CPU.
ROWS_F, ROWS_S = 129, 16
for _N in (127, 128, 129):
    for _M, _suffix in ((512, ""), (2, "_m2")):
        _r = np.arange(_N)
        _add(Case(f"rows_{_N}{_suffix}", ROWS_F, ROWS_S, np.stack([_r, _r % ROWS_S, np.full(_N, _M)], axis=1), 100 + _N,
                  f"{_N} rows with one pair each at M = {_M}"),
             dict(M=_M, rows=(_N,) * 8, picked=0 if _N <= PL_ROWS else None, pairs=_N, levels=(_N,)),
             "over", _N - TIE_CAP)


def _rows_depth():
    """100 rows at 512; 28 rows at 480 .. 507, one pair each: 128 rows reach s = 4 (480); one row at 448: 129 reach s = 3"""
    cnt = np.concatenate([np.full(100, 512), 480 + np.arange(28), [448]])
    r = np.arange(129)
    return np.stack([r, r % ROWS_S, cnt], axis=1)


# (100 tied at M: four hand-backs by TIE_CAP before the level fits -- and after each the rebuild sees one row fewer)
_add(Case("rows_depth", ROWS_F, ROWS_S, _rows_depth(), 131, "exactly 128 rows reach M - (M >> 4), 129 reach M - (M >> 3)"),
     dict(M=512, rows=(129, 129, 128, 112, 104, 100, 100, 100), picked=2, theta=480, pairs=128, levels=(100,) + (1,) * 28),
     "over", 4)


def _rows_depth_all():
    """20 rows at 512, 108 rows at 384 .. 491: 128 rows reach even s = 2"""
    cnt = np.concatenate([np.full(20, 512), 384 + np.arange(108)])
    r = np.arange(128)
    return np.stack([r, r % ROWS_S, cnt], axis=1)


# (128 rows handed out and a top level that can be located: the one case in which a rebuild's gather covers all PL_ROWS rows
# and then selects -- with the default 127 scanning workgroups the loop over the rows goes round a second time)
_add(Case("rows_depth_all", ROWS_F, ROWS_S, _rows_depth_all(), 132, "at most 128 rows reach even M - (M >> 2): the deepest candidate"),
     dict(M=512, rows=(128, 64, 32, 20, 20, 20, 20, 20), picked=0, theta=384, pairs=128, levels=(20,) + (1,) * 108), "within")

# ---- pairs gathered: 32 rows x 32 columns (+ 1 pair in a 33rd row), levels of 8 from 512 down: level j counts 512 - j, the
# 1025th pair alone at 384 = M - (M >> 2).  Which pair sits in which level is shuffled.
GATHER_F, GATHER_S, GATHER_M = 33, 32, 512


def _gather(n):
    k = np.arange(min(n, 1024))
    row, col = k // 32, k % 32
    if n == 1025:
        row, col = np.append(row, 32), np.append(col, 0)
    level = np.arange(n) // 8
    perm = np.random.default_rng(7).permutation(1023)  # (the same places in all three cases; pairs 1023 and 1024 come last)
    place = np.concatenate([perm, np.arange(1023, n)])[:n]
    cnt = np.empty(n, np.int64)
    cnt[place] = GATHER_M - level
    return np.stack([row, col, cnt], axis=1)


for _n in (1023, 1024, 1025):
    _add(Case(f"gather_{_n}", GATHER_F, GATHER_S, _gather(_n), 200 + _n % 10,
              f"{_n} pairs at or above the threshold in {32 + (_n > 1024)} rows, levels of at most 8"),
         dict(M=512, picked=0, theta=384, pairs=_n, kept=256),
         "within" if _n <= PL_GATHER else "over", None if _n <= PL_GATHER else 1)

# ---- entries kept: levels of 3 (or 4) from 416 down over 32 rows x 10 columns
CAP_F, CAP_S, CAP_M = 32, 10, 416


def _cap(n, per_level):
    row, col = _grid(n, CAP_F, CAP_S)
    return np.stack([row, col, CAP_M - np.arange(n) // per_level], axis=1)


for _name, _n, _l, _kept in (("cap_255", 255, 3, 255), ("cap_256", 256, 3, 256), ("cap_257", 257, 3, 255),
                             ("cap_257_l4", 257, 4, 256), ("cap_300_l3", 300, 3, 255)):
    _add(Case(_name, CAP_F, CAP_S, _cap(_n, _l), 300 + _n + _l, f"{_n} pairs at or above the threshold in levels of {_l}"),
         dict(M=CAP_M, picked=0, theta=312, pairs=_n, kept=_kept, levels=(_l,) * (_n // _l)), "within")

# One level of 257: also over TIE_CAP, but pool_sel_body sorts and cuts BEFORE it looks at levels -- the `cut--` loop runs
# down to 0, "one level larger than the pool", defer = 2.  Once the general path has merged one pair the level is 256
# entries: it fits the pool and not TIE_CAP, K == 0.  257 - 96 hand-backs.
_add(Case("cap_one_level_257", CAP_F, 16, np.stack(_grid(257, CAP_F, 16) + (np.full(257, 8),), axis=1), 341,
          "a single level of 257 tied pairs in 32 rows"),
     dict(M=8, picked=0, theta=6, pairs=257, kept=0, levels=(257,)), "over", 257 - TIE_CAP)

# ---- levels located: T pairs tied at 8 in min(T, 96) rows, the next level (the tail) at 2
TIED_F, TIED_S = 96, 8


def _tied(T, M=8):
    k = np.arange(T)
    return np.stack([k % 96, (k // 96 + k % 7) % TIED_S, np.full(T, M)], axis=1)


for _T in (95, 96, 97):
    # (97: one hand-back, then 96 tied pairs are left, which are located -- 96 + 2 words fill the sharded MIN payload)
    _add(Case(f"tied_{_T}", TIED_F, TIED_S, _tied(_T), 400 + _T, f"{_T} pairs tied at the top in {min(_T, 96)} rows"),
         dict(M=8, picked=0, theta=6, pairs=_T, kept=_T, levels=(_T,)), "within" if _T <= TIE_CAP else "over",
         None if _T <= TIE_CAP else 1)

# A level of 90, then one of 7.  A batch holds at most CH_KSWEEP = 31 pairs, so the first selection's walk ends inside the top
# level: reach = 90, the level of 7 starts at reach and is asked for below it, where P + size = 97 is over 16 (and over
# TIE_CAP): it stays without an order, and the batch -- cut at 31 anyway -- cannot enter it.  The top level keeps its keys
# while it shrinks; once the walk's last entry falls into the level of 7 that level is within reach, P = 0 (a clean level is
# not counted), and it is located then.
_add(Case("tied_two_levels", TIED_F, TIED_S,
          np.concatenate([_tied(90), np.stack([np.arange(90, 96), 1 + np.arange(6), np.full(6, 7)], axis=1),
                          [[0, 7, 7]]]), 451, "a top level of 90, then a level of 7", opts=(("chain_kcap", CHAIN_KCAP),)),
     dict(M=8, picked=0, theta=6, pairs=97, kept=97, levels=(90, 7)), "within")

# ---- located below the walk's reach.  The top level is (r0, c0), (r0, c1): with chain_share_first = 0 (and in the one-launch
# and the sharded step, which never share a first token) entry 0 clashes with entry 1, reach = 2.  P counts the entries of
# EVERY level that lacks an order before a level, the top one included: seven levels of 2 below it bring P + size to exactly
# 16 at the last; a last level of 3 brings it to 17 and is left for the step that reaches it.
REACH_F, REACH_S, REACH_M = 20, 8, 32


def _below_reach(total):
    sizes = [2] * 8 if total == 16 else [2] * 7 + [3]
    rows = [0, 0] + list(range(1, sum(sizes) - 1))
    cols = [0, 1] + [r % REACH_S for r in rows[2:]]
    cnt = np.repeat(REACH_M - np.arange(len(sizes)), sizes)
    return np.stack([rows, cols, cnt], axis=1)


for _t in (16, 17):
    _add(Case(f"below_reach_{_t}", REACH_F, REACH_S, _below_reach(_t), 504,
              f"levels that lack an order total {_t} entries, the top one ends the reach", opts=(("chain_share_first", 0),)),
         dict(M=32, picked=0, theta=24, pairs=_t, kept=_t, levels=(2,) * 7 + (_t - 14,)), "within")

# cases that differ in one designed pair: (smaller, larger, the View field that tells them apart)
NEIGHBOURS = [("rows_127", "rows_128", "rows"), ("rows_128", "rows_129", "rows"), ("rows_128_m2", "rows_129_m2", "rows"),
              ("gather_1023", "gather_1024", "pairs"), ("gather_1024", "gather_1025", "pairs"),
              ("cap_255", "cap_256", "pairs"), ("cap_256", "cap_257", "pairs"),
              ("tied_95", "tied_96", "levels"), ("tied_96", "tied_97", "levels"),
              ("below_reach_16", "below_reach_17", "levels")]
# training ends inside the first batch: kmax = min(kcap, num_merges - iter) cuts the walk
MID_BATCH = ("tied_96", 1 + 10)
