"""Hand-built merge lists for encode-as-replay (api/api_encode.hip: one chunk of REPLAY_MIN_BYTES or more and a merge
list of the shape training makes is not encoded at all -- the list is replayed through the training engine, the
selections given: k_forced_sel / k_forced_pair at the end of kernels/k_chain.hip).

Pure numpy: no GPU, no synth_text.  CASES maps a name to a builder; builder(n) returns (pairs, data): an (M, 2) int32
merge list of training shape and ONE chunk of n + D bytes (D small and odd; the `collapse` family, whose lengths are
the point, excepted).  n = REPLAY_MIN_BYTES on the GPU (tests/test_gpu_replay.py), a few thousand on the CPU
(tests/test_replay_cases_cpu.py pins oracle.encode on exactly these lists first).

A replay breaks invariants that every training run keeps, and the cases are built around them:
  * counts are not monotone: a merge with no site at all can be followed by the text's most frequent pair;
  * a batch is whatever run of the list k_forced_sel's rule admits -- 31 token-disjoint merges, a cut at lane 30
    against lane 0 or lane 29, a list that ends in the middle of a run;
  * the stream can collapse to one id with merges still to go.
A merge with a == b is a BARRIER wherever the next run has to start at a known merge: k_forced_sel defers it
(K == 0), the general path merges it, and the next chain step starts right behind it.  marks(name, n) lists those
starts with the lane at which the rule must cut the run that begins there."""
import functools

import numpy as np

import oracle

REPLAY_MIN_BYTES = 1 << 20   # api_encode.hip
CH_KSWEEP = 31               # bpe_device.h: most pairs of one sweep, and the default of option chain_kcap
CH_KDENSE = 6                # k_chain.hip: most pairs of a dense step's batch
KCAPS = (1, 4, 15, 31)       # the values of option chain_kcap every case is run at
D = 3                        # bytes beyond n: small and odd
JL = ((0, 1), (0, 30), (29, 30))   # (j, l): lane l conflicts with lane j -- the first pair of lanes, the last lane
                                   # against the first, the last two lanes k_forced_sel's shuffle loop compares

LETTERS = (97, 98, 99, 100)
SPICE = tuple(range(0xA0, 0xE0))   # 64 bytes: the token-disjoint pairs of the hand-built runs are made of these
OUTSIDE = tuple(range(0x01, 0x20))  # bytes no list has in a pair
COLD = tuple(range(0xE0, 0x100)) + tuple(range(0x80, 0xA0))   # bytes no text holds


# ---------------------------------------------------------------------------
# the rules, in plain Python

def training_shape(pairs):
    """merges_training_shape (api_encode.hip): merge r is made of tokens defined before it; no pair twice"""
    pl = [(int(a), int(b)) for a, b in pairs]
    return all(0 <= a < 256 + r and 0 <= b < 256 + r for r, (a, b) in enumerate(pl)) and len(set(pl)) == len(pl)


def forced_run(pairs, start, kcap):
    """k_forced_sel: the batch of the chain step that starts at merge `start` -- the longest run of at most kcap
    merges with a != b, no token of an earlier merge of the run, no token that the run itself creates (ids from
    256 + start on).  0: the merge at `start` has a == b and goes to the general path."""
    seen, k = set(), 0
    while k < kcap and start + k < len(pairs):
        a, b = int(pairs[start + k][0]), int(pairs[start + k][1])
        if a == b or a >= 256 + start or b >= 256 + start or a in seen or b in seen:
            break
        seen.update((a, b))
        k += 1
    return k


def forced_runs(pairs, start, kcap):
    """[(first merge, run length)] of chain steps from `start` to the end of the list; a run of length 0 is one
    a == b merge handed to the general path"""
    out = []
    while start < len(pairs):
        k = forced_run(pairs, start, kcap)
        out.append((start, k))
        start += max(k, 1)
    return out


def plain_replay(pairs, data):
    """what a replay must compute: merge r applied everywhere, left to right, for r = 0 .. M - 1 (yields the stream
    before every merge, and the final one last)"""
    ids = np.frombuffer(data, dtype=np.uint8).astype(np.int32)
    for r, (a, b) in enumerate(pairs):
        yield r, ids
        ids = oracle.merge(ids, (int(a), int(b)), 256 + r)
    yield len(pairs), ids


# ---------------------------------------------------------------------------
# building blocks

class _List:
    """a merge list under construction: ids are 256 + rank, no pair twice"""

    def __init__(self):
        self.pairs = []
        self.seen = set()
        self.ladder = {c: c for c in LETTERS}   # letter -> top of its (t, t) ladder

    def add(self, a, b):
        assert (a, b) not in self.seen and max(a, b) < 256 + len(self.pairs), (a, b)
        self.seen.add((a, b))
        self.pairs.append((a, b))
        return 255 + len(self.pairs)

    def barrier(self):
        """the next a == b merge: the ladders (97, 97) -> t, (t, t) -> u, ... of the four letters in turn, so that the
        early ones walk the runs of the text and the late ones have no site"""
        c = LETTERS[sum(1 for p in self.pairs if p[0] == p[1]) % 4]
        self.ladder[c] = self.add(self.ladder[c], self.ladder[c])
        return len(self.pairs)   # the rank right behind the barrier

    def disjoint(self, rng, k, avoid=()):
        """k token-disjoint pairs of SPICE bytes, none of them in the list yet"""
        while True:
            pool = [int(x) for x in rng.permutation([s for s in SPICE if s not in avoid])]
            got = [(pool[2 * i], pool[2 * i + 1]) for i in range(k)]
            if not self.seen.intersection(got):
                return got, pool[2 * k:]

    def array(self):
        out = np.array(self.pairs, dtype=np.int32).reshape(-1, 2)
        assert training_shape(out)
        return out


def _text(rng, n, snippets=(), spice=0.3):
    """n + D bytes: runs of one of four letters (lengths geometric, one in 50 a run of 40 to 400), stretches of random
    SPICE bytes (every pair of them occurs), bytes outside every list, and the snippets -- the overlapping sites a
    case needs -- throughout"""
    units = []
    total = 0
    snippets = [bytes(s) for s in snippets]
    while total < n + D:
        kind = rng.random(256)
        lens = rng.geometric(0.4, 256)
        longs = rng.integers(40, 400, 256)
        for k, ln, lg in zip(kind, lens, longs):
            if snippets and k < 0.25:
                u = snippets[int(k * 4 * len(snippets)) % len(snippets)]
            elif k < 0.25 + spice:
                u = bytes(rng.choice(SPICE, size=int(ln) + 6).astype(np.uint8))
            elif k < 0.97:
                u = bytes([LETTERS[int(k * 1000) % 4]]) * (int(lg) if k > 0.955 else int(ln))
            else:
                u = bytes([OUTSIDE[int(k * 10000) % len(OUTSIDE)]])
            units.append(u)
            total += len(u)
    return b"".join(units)[:n + D]


# ---------------------------------------------------------------------------
# the cases: _build(name, n) -> (pairs, data, marks); marks = [(start, cut)]: the chain step that starts at merge
# `start` (right behind a barrier) must take min(kcap, cut) merges

def _disjoint_run(n):
    """40 token-disjoint byte pairs, then the tree above them (the new tokens two by two, level by level, down to one
    token).  From any start in 0 .. 9 the next 31 merges are leaves: a run of kcap pairs for every kcap."""
    rng = np.random.default_rng(11)
    L = _List()
    level = [L.add(0x30 + 2 * i, 0x31 + 2 * i) for i in range(40)]
    expand = {t: bytes([0x30 + 2 * i, 0x31 + 2 * i]) for i, t in enumerate(level)}
    levels = [level]
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level) - 1, 2):
            t = L.add(level[i], level[i + 1])
            expand[t] = expand[level[i]] + expand[level[i + 1]]
            nxt.append(t)
        if len(level) % 2:
            nxt.append(level[-1])   # the odd one out goes up a level
        level = nxt
        levels.append(level)
    assert len(L.pairs) == 79 and len(expand[level[0]]) == 80
    parts, total = [], 0
    while total < n + D:
        lv = rng.integers(0, len(levels), 512)
        pick = rng.integers(0, 1 << 30, 512)
        out = rng.random(512)
        for a, b, o in zip(lv, pick, out):
            node = levels[a][b % len(levels[a])]
            u = expand[node] + (bytes([OUTSIDE[b % len(OUTSIDE)]]) if o < 0.5 else b"")
            parts.append(u)
            total += len(u)
    return L.array(), b"".join(parts)[:n + D], []


HOT_RANK = 340   # cold_then_hot: the rank of the late hot pair


def _cold_then_hot(n):
    """Merge 0 has no site, merge 1 is the most frequent pair but one; cold and hot merges alternate up to rank 39;
    300 cold merges; at rank 340 the pair (p, q) of two bytes nothing before touches, with more than n / 4 sites.
    ((p, q) alone takes half the text, so the early hot pair has n / 6 sites: two byte pairs that share no byte cannot
    both have more than n / 4.)"""
    rng = np.random.default_rng(12)
    a, b, p, q = 0x61, 0x62, 0x70, 0x71
    fill = (0x63, 0x64, 0x65, 0x66)
    n_pq = n // 4 + 16
    n_ab = (n + D - 2 * n_pq) // 3
    units = [b"pq"] * n_pq + [bytes([a, b, fill[i]]) for i in rng.integers(0, 4, n_ab)]
    units += [bytes([OUTSIDE[i]]) for i in rng.integers(0, len(OUTSIDE), n + D - 2 * n_pq - 3 * n_ab)]
    order = rng.permutation(len(units))
    data = b"".join(units[i] for i in order)
    assert len(data) == n + D
    L = _List()
    cold_tokens = []

    def cold():
        while True:
            if cold_tokens and rng.random() < 0.2:   # a token that a cold merge made: no site either
                x, y = cold_tokens[int(rng.integers(0, len(cold_tokens)))], COLD[int(rng.integers(0, len(COLD)))]
                x, y = (x, y) if rng.random() < 0.5 else (y, x)
            else:
                x, y = (COLD[int(i)] for i in rng.integers(0, len(COLD), 2))
            if x != y and (x, y) not in L.seen:
                cold_tokens.append(L.add(x, y))
                return

    cold()                                   # rank 0: no site
    X = L.add(a, b)                          # rank 1: n / 6 sites
    hot = [(X, f) for f in fill]             # ranks 3, 5, 7, 9: Y_f = X f, a quarter of X's sites each
    Y = [256 + 3 + 2 * i for i in range(4)]
    hot += [(Y[i], Y[j]) for i in range(4) for j in range(4)][:15]   # two units side by side ((Y_0, Y_0): a == b)
    for h in hot:
        cold()
        L.add(*h)
    assert len(L.pairs) == 40
    while len(L.pairs) < HOT_RANK:
        cold()
    P = L.add(p, q)
    assert P == 256 + HOT_RANK
    L.add(P, P)                              # ... and the engine goes on from there: runs of pq pq
    cold()
    L.add(P, X)
    return L.array(), data, []


def _collapse(n, extra):
    """a run of one letter and the ladder (97, 97), (256, 256), ...: log2(n) merges are all the stream can use (it is
    one id then), four more follow"""
    k = n.bit_length() - 1
    assert n == 1 << k
    pairs = [(97, 97)] + [(256 + i, 256 + i) for i in range(k + 3)]
    return np.array(pairs, dtype=np.int32), b"a" * (n + extra), []


def collapse_ids(n, length):
    """how many ids a run of `length` letters collapses to under _collapse(n)'s list: the binary digits of the length,
    the top token (2^log2(n) letters) as often as it fits"""
    k = n.bit_length() - 1
    return (length >> k) + bin(length & ((1 << k) - 1)).count("1")


def _aa_in_run(n):
    """for kcap in KCAPS: an a == b merge at lane 0, lane 1, lane kcap - 1 and lane kcap of a run of kcap + 1
    otherwise token-disjoint merges, each run behind a barrier"""
    rng = np.random.default_rng(13)
    L = _List()
    marks = []
    L.add(LETTERS[0], LETTERS[1])   # (merge 0 is the general path's whatever it is)
    for kcap in KCAPS:
        for lane in sorted({0, 1, kcap - 1, kcap}):
            start = L.barrier()
            run, _ = L.disjoint(rng, kcap)
            for i in range(kcap + 1):
                if i == lane:
                    L.barrier()
                else:
                    L.add(*run.pop())
            marks.append((start, lane))
    return L.array(), _text(rng, n), marks


WAYS = ("aj==a", "aj==b", "bj==a", "bj==b")


def _shared_token_cut(n):
    """behind a barrier, lanes 0 .. l of token-disjoint pairs, except that lane l shares a token with lane j -- in each
    of the four ways k_forced_sel compares, for (j, l) in JL.  With lane j = (x, y), lane l = (y, z) the text holds
    x y z and w y z: both pairs merged in ONE sweep would turn x y z into x Z or leave the choice to the sweep's order;
    merge j first gives X z.  Likewise z x y for lane l = (z, x)."""
    rng = np.random.default_rng(14)
    L = _List()
    marks, snippets = [], []
    L.add(LETTERS[0], LETTERS[1])
    for j, l in JL:
        for way in WAYS:
            start = L.barrier()
            while True:
                run, rest = L.disjoint(rng, l)
                x, y = run[j]
                z, w = rest[0], rest[1]
                last = {"aj==a": (x, z), "aj==b": (z, x), "bj==a": (y, z), "bj==b": (z, y)}[way]
                if last not in L.seen:
                    break
            for pr in run:
                L.add(*pr)
            L.add(*last)
            marks.append((start, l))
            snippets += [(x, y, z), (w, y, z), (z, x, y), (z, x, w), (x, y, x, z), (z, y, x, y), (x, z, y)]
    L.barrier()
    return L.array(), _text(rng, n, snippets), marks


def _fresh_token_cut(n):
    """behind a barrier, lanes 0 .. l of token-disjoint pairs, except that lane l has the token that lane j of the same
    run creates -- as its first and as its second element, for (j, l) in JL.  The text holds x y z and z x y for lane
    j = (x, y): the new pair has sites only once merge j is done."""
    rng = np.random.default_rng(15)
    L = _List()
    marks, snippets = [], []
    L.add(LETTERS[0], LETTERS[1])
    for j, l in JL:
        for first in (True, False):
            start = L.barrier()
            run, rest = L.disjoint(rng, l)
            x, y = run[j]
            z = rest[0]   # (the pair below holds a token no earlier list entry can: it is new)
            for pr in run:
                L.add(*pr)
            t = 256 + start + j
            L.add(*((t, z) if first else (z, t)))
            marks.append((start, l))
            snippets += [(x, y, z), (z, x, y), (z, x, y, z)]
    L.barrier()
    return L.array(), _text(rng, n, snippets), marks


TAILS = (1, 3, 4, 14, 15, 30, 31)   # 1 | kcap - 1 | kcap for kcap 4, 15, 31 (kcap 1: the tails 1 and 4, among others)


def _short(n, m):
    """M = 1 and M = 2: the whole list is the general path's first merge, and one more"""
    rng = np.random.default_rng(16)
    L = _List()
    L.add(SPICE[0], SPICE[1])
    if m == 2:
        L.add(256, SPICE[2])
    return L.array(), _text(rng, n, [(SPICE[0], SPICE[1], SPICE[2])]), []


def _short_tail(n, tail):
    """a first merge, a barrier, and `tail` token-disjoint merges: the list ends in the middle of a run (or exactly at
    its end: tail == kcap) -- lanes beyond the list must not be read as merges"""
    rng = np.random.default_rng(17 + tail)
    L = _List()
    L.add(LETTERS[0], LETTERS[1])
    start = L.barrier()
    run, _ = L.disjoint(rng, tail)
    for pr in run:
        L.add(*pr)
    return L.array(), _text(rng, n), [(start, tail)]


@functools.lru_cache(maxsize=None)
def _trained():
    """oracle.train_fast of a 300 KB four-letter text, 2100 merges, re-ordered by a random topological order (every
    merge behind the merges that define its tokens) and renumbered to 256 + new rank: training shape, counts all
    over the place, ids across 1024 (CH_DCAP), 1920 (LDSD_CAP) and 2048"""
    rng = np.random.default_rng(18)
    text = bytes(97 + rng.integers(0, 4, size=300_000).astype(np.uint8))
    pairs = oracle.train_fast(text, 2100)[0]
    m = len(pairs)
    assert m == 2100
    waits = [sum(1 for t in p if t >= 256) for p in pairs]
    children = [[] for _ in range(m)]
    for r, p in enumerate(pairs):
        for t in p:
            if t >= 256:
                children[t - 256].append(r)
    ready = [r for r in range(m) if waits[r] == 0]
    new_rank = {}
    order = []
    while ready:
        i = int(rng.integers(0, len(ready)))
        ready[i], ready[-1] = ready[-1], ready[i]
        r = ready.pop()
        new_rank[r] = len(order)
        order.append(r)
        for ch in children[r]:
            waits[ch] -= 1
            if waits[ch] == 0:
                ready.append(ch)
    assert len(order) == m

    def ren(t):
        return t if t < 256 else 256 + new_rank[t - 256]
    out = np.array([(ren(pairs[r][0]), ren(pairs[r][1])) for r in order], dtype=np.int32)
    assert training_shape(out) and order != sorted(order)
    return out


def _shuffled_trained(n):
    rng = np.random.default_rng(19)   # (another text of the same alphabet than the list was trained on)
    return _trained(), bytes(97 + rng.integers(0, 4, size=n + D).astype(np.uint8)), []


_BUILDERS = {
    "disjoint_run": _disjoint_run,
    "cold_then_hot": _cold_then_hot,
    "collapse_pow2": lambda n: _collapse(n, 0),
    "collapse_plus1": lambda n: _collapse(n, 1),
    "collapse_ones": lambda n: _collapse(n, n - 1),
    "aa_in_run": _aa_in_run,
    "shared_token_cut": _shared_token_cut,
    "fresh_token_cut": _fresh_token_cut,
    "short_m1": lambda n: _short(n, 1),
    "short_m2": lambda n: _short(n, 2),
    "shuffled_trained": _shuffled_trained,
}
for _t in TAILS:
    _BUILDERS[f"short_tail{_t}"] = functools.partial(_short_tail, tail=_t)


@functools.lru_cache(maxsize=None)
def _build(name, n):
    return _BUILDERS[name](n)


def _case(name):
    return lambda n=REPLAY_MIN_BYTES: _build(name, n)[:2]


CASES = {name: _case(name) for name in _BUILDERS}


MARKED = ("aa_in_run", "shared_token_cut", "fresh_token_cut") + tuple(f"short_tail{t}" for t in TAILS)


def marks(name, n=REPLAY_MIN_BYTES):
    """[(start, cut)]: the chain step that starts at merge `start`, right behind a barrier, takes min(kcap, cut)"""
    return _build(name, n)[2]


# the merges a chain step can take at all (a != b); lists without any stay on the general path: no chain step counts
def has_chain_merges(pairs):
    return any(int(a) != int(b) for a, b in pairs[1:])


# ---------------------------------------------------------------------------
# lists that must NOT be replayed (the gate of api_encode.hip): they take the stream-wide rounds at any size

def gate_lists(n=REPLAY_MIN_BYTES):
    """{label: (pairs, merge_ids or None)} over disjoint_run's text: a pair listed twice (the last entry wins, like a
    dict: the reference's merges dict), a forward reference (merge r made of a token that merge r + 1 defines), and
    merge_ids given -- the identity and 1000 + 3 r"""
    pairs, _ = CASES["disjoint_run"](n)
    m = len(pairs)

    def insert(r, pair):   # `pair` as merge r; the tokens of the merges behind it move up by one
        rows = [(a + (a >= 256 + r), b + (b >= 256 + r)) for a, b in pairs.tolist()]
        return np.array(rows[:r] + [pair] + rows[r:], dtype=np.int32)

    # leaf 3 = (0x36, 0x37) again at rank 50: it makes 306 from there on, and token 259 -- which the tree's (258, 259)
    # waits for -- never appears
    twice = insert(50, tuple(pairs[3].tolist()))
    # rank 40 = (297, 258): token 297 is what the NEXT merge, (256, 257), makes; leaf 2 follows it in every larger node
    forward = insert(40, (297, 258))
    sparse = np.concatenate([np.arange(256), 1000 + 3 * np.arange(m)]).astype(np.int32)
    out = {
        "pair_twice": (twice, None),
        "forward_reference": (forward, None),
        "merge_ids_identity": (pairs, 256 + np.arange(m, dtype=np.int32)),
        "merge_ids_sparse": (sparse[pairs], sparse[256:]),   # (the tokens of the pairs renamed alike)
    }
    assert not training_shape(twice) and not training_shape(forward)
    assert len({tuple(p) for p in twice.tolist()}) == m and len({tuple(p) for p in forward.tolist()}) == m + 1
    assert tuple(forward[41].tolist()) == (256, 257)
    return out
