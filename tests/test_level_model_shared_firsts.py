"""CPU models of the chain steps' batch rule with SHARED FIRST TOKENS (option "chain_share_first"; k_pool.hip: pool_finish,
the mirrored maintenance; k_chain.hip: the merge pass finds a site by its pair).

The rule: walk the levels of the table from the top, inside a level in order of first occurrence; stop for good at the first
pair (x, y) with x == y, or with x a SECOND token or y a FIRST token of a pair already taken -- a pair that could chain onto a
site of the batch.  Nothing else stops the walk: a second token may come twice ((a, b), (c, b): round 6), and now a first
token too -- (a, b1), (a, b2).

Why it is exact (base.py:13-41, basic.py:31-42, regex.py:49-63): sites of (a, b1) and (a, b2) never overlap (both start on an
a, and a word has one successor); neither merge changes the other's count -- that would need b1 == a or b2 == a, which the
chain test excludes; and what a merge lowers or creates -- (L, a), (b, R) and their heirs -- chains onto the batch and stops
the walk where it stands.

Checked against the reference semantics restated with numpy (test_level_model.reference_next) on that file's streams plus
streams built to tie pairs that share a first token, at caps 4, 15 and 31; and as the pool model (test_pool_model.Pool) with
the mirrored maintenance -- an entry (x, y) has the variants ({x} + {Z_p : p ends in x}) x ({y} + {Z_q : q starts with y})
-- whose invariant (the pool is exactly the pairs that count theta or more) is asserted after every step."""
import random

import numpy as np
import pytest

import test_pool_model
from test_level_model import reference_next, streams
from test_list_model import make_stream, merge, stats_in_order, table_of, STREAMS


def batch_by_levels_shared_firsts(chunks, cap):
    """the batch the rule above takes from the current state (a lone a == b pair is a batch of one)"""
    pairs, counts = stats_in_order(chunks)
    if not pairs:
        return []
    batch, firsts, seconds = [], set(), set()
    for c in sorted(set(int(x) for x in counts), reverse=True):
        for (a, b), n in zip(pairs, counts):  # dict order = order of first occurrence
            if int(n) != c:
                continue
            if a == b or a in seconds or b in firsts:
                return batch if batch else [(a, b)]
            batch.append((a, b))
            firsts.add(a)
            seconds.add(b)
            if len(batch) == cap:
                return batch
    return batch


def fan_streams():
    """chunked streams in which pairs that share a first token tie: a few heads, each followed by one of several tails, every
    (head, tail) word repeated the same number of times; some tails are shared between heads (a first AND a second token
    twice in one batch) and some words run on into a second pair"""
    rng = random.Random(4321)
    for trial in range(60):
        heads = rng.sample(range(0, 6), rng.choice([1, 2, 3]))
        tails = rng.sample(range(6, 14), rng.choice([2, 3, 4, 5]))
        reps = rng.choice([2, 3, 3, 5])
        words = []
        for h in heads:
            for t in rng.sample(tails, rng.randint(2, len(tails))):
                w = [h, t]
                if rng.random() < 0.3:
                    w += [rng.randrange(14, 18)]
                if rng.random() < 0.15:
                    w = [rng.randrange(14, 18)] + w
                words += [np.array(w, dtype=np.int64)] * (reps if rng.random() < 0.8 else reps - 1)
        words += [np.array([rng.randrange(18) for _ in range(rng.randint(1, 5))], dtype=np.int64) for _ in range(rng.randint(0, 6))]
        rng.shuffle(words)
        yield words


def all_streams():
    yield from streams()
    yield from fan_streams()


TALLY = {}


@pytest.mark.parametrize("cap", [4, 15, 31])
def test_batches_that_share_first_tokens_are_the_reference_merges(cap):
    twice = both = 0
    for chunks in all_streams():
        next_id = 100
        for _ in range(40):
            batch = batch_by_levels_shared_firsts(chunks, cap)
            if not batch:
                break
            want, after = reference_next(chunks, len(batch), next_id)
            assert want == batch, (cap, batch, want)
            f = len({a for a, _ in batch}) < len(batch)
            s = len({b for _, b in batch}) < len(batch)
            twice += f
            both += f and s
            chunks, next_id = after, next_id + len(batch)
    TALLY[cap] = (twice, both)
    print("cap", cap, "batches that hold a first token twice:", twice, "a first and a second token twice:", both)


def test_batches_with_shared_first_tokens_did_occur():
    """(runs after the cases above in file order) the rule is exercised, not only permitted: over the cases, more than 30
    batches hold a first token twice and at least 5 share a first and a second token at once"""
    assert len(TALLY) == 3, "run together with test_batches_that_share_first_tokens_are_the_reference_merges"
    twice = sum(t for t, _ in TALLY.values())
    both = sum(b for _, b in TALLY.values())
    assert twice > 30, TALLY
    assert both >= 5, TALLY


def test_pairs_that_chain_still_end_the_batch():
    # (1, 2) and (2, 3) tie at the top, (1, 2) first: the batch is (1, 2) alone; so is (1, 2) then (4, 1)
    ids = [np.array([1, 2, 9, 2, 3, 9, 1, 2, 8, 2, 3], dtype=np.int64)]
    assert batch_by_levels_shared_firsts(ids, 8) == [(1, 2)]
    ids = [np.array([1, 2, 9, 4, 1, 9, 1, 2, 8, 4, 1, 7], dtype=np.int64)]
    assert batch_by_levels_shared_firsts(ids, 8) == [(1, 2)]
    # ... while (1, 2), (1, 3), (4, 3) go together
    ids = [np.array(w, dtype=np.int64) for w in ([1, 2], [1, 3], [4, 3])] * 3
    assert batch_by_levels_shared_firsts(ids, 8) == [(1, 2), (1, 3), (4, 3)]
    assert reference_next(ids, 3, 100)[0] == [(1, 2), (1, 3), (4, 3)]


# ---------------------------------------------------------------------------
# the pool with the mirrored maintenance

class SharedFirstPool(test_pool_model.Pool):
    """test_pool_model.Pool under the rule above: the walk lets a first token come twice, and an entry (x, y) whose y is
    the first token of SEVERAL batch pairs has a variant for each of them -- as for x and the pairs that end in it"""

    def __init__(self, *args):
        super().__init__(*args)
        self.most_variants = 0

    def batch(self, chunks, left):
        es = sorted(self.entries, key=lambda e: -e["c"])
        levels, i = [], 0
        while i < len(es):
            j = i
            while j < len(es) and es[j]["c"] == es[i]["c"]:
                j += 1
            levels.append(es[i:j])
            i = j
        kmax = min(self.cap, left)
        seen = 0
        for lv in levels:
            if seen >= kmax:
                break
            if len(lv) > 1 and (lv[0]["epoch"] == 0 or any(e["epoch"] != lv[0]["epoch"] for e in lv)):
                self.locate(chunks, lv)
            seen += len(lv)
        batch, cnts, firsts, seconds = [], [], set(), set()
        seen = 0
        for lv in levels:
            if seen >= kmax:
                break
            for e in sorted(lv, key=lambda e: e["rank"] if len(lv) > 1 else 0):
                a, b = e["pair"]
                if a == b or a in seconds or b in firsts or len(batch) >= kmax:
                    return batch, cnts, (e["pair"] if not batch else None)
                batch.append(e["pair"])
                cnts.append(e["c"])
                firsts.add(a)
                seconds.add(b)
            seen += len(lv)
        return batch, cnts, None

    def maintain(self, batch, znew, table):
        ends, starts = {}, {}
        for (a, b), z in zip(batch, znew):
            ends.setdefault(b, []).append(z)    # (several pairs of a batch may end in b)
            starts.setdefault(a, []).append(z)  # (... and several may start with a)
        taken = set(batch)
        out = []
        for e in self.entries:
            x, y = e["pair"]
            if e["pair"] in taken:
                continue
            if x not in ends and y not in starts:
                assert table.get(e["pair"], 0) == e["c"]  # untouched
                out.append(e)
                continue
            cands = [(l, r) for l in [x] + ends.get(x, []) for r in [y] + starts.get(y, [])]
            assert sum(table.get(p, 0) for p in cands) <= e["c"]
            self.most_variants = max(self.most_variants, sum(1 for p in cands if table.get(p, 0) >= self.theta))
            for p in cands:
                c = table.get(p, 0)
                if c < self.theta:
                    continue
                if c == e["c"]:  # took over every occurrence: stands where the entry stood
                    out.append(dict(pair=p, c=c, rank=e["rank"], epoch=e["epoch"]))
                    self.inherited += p != e["pair"]
                else:
                    out.append(dict(pair=p, c=c, rank=None, epoch=0))
        self.entries = out
        self.trim()


def run_pool(chunks, pool, total):
    """the pool's steps against the reference, the invariant after every step; (merges done, steps, steps whose batch held
    a first token twice)"""
    next_id, done, steps, twice = 256, 0, 0, 0
    while done < total:
        pairs, counts = stats_in_order(chunks)
        if not len(counts) or counts.max() < 2:
            break
        if not pool.entries:
            pool.rebuild(chunks)
        if len(pool.entries) > pool.capacity:  # one level larger than the pool: the general path's merge
            best = pairs[int(np.argmax(counts))]
            chunks = [merge(c, best, next_id) for c in chunks]
            next_id, done = next_id + 1, done + 1
            pool.entries = []
            continue
        batch, cnts, head_same = pool.batch(chunks, total - done)
        if not batch:  # a == b at the head: the general path's merge, the pool is void
            assert head_same is not None and head_same[0] == head_same[1]
            assert pairs[int(np.argmax(counts))] == head_same
            chunks = [merge(c, head_same, next_id) for c in chunks]
            next_id, done = next_id + 1, done + 1
            pool.entries = []
            continue
        znew = list(range(next_id, next_id + len(batch)))
        for pair, cnt, z in zip(batch, cnts, znew):
            ref_pairs, ref_counts = stats_in_order(chunks)
            j = int(np.argmax(ref_counts))
            assert ref_pairs[j] == pair and int(ref_counts[j]) == cnt, (done, pair, cnt, ref_pairs[j])
            chunks = [merge(c, pair, z) for c in chunks]
        next_id += len(batch)
        done += len(batch)
        steps += 1
        twice += len({a for a, _ in batch}) < len(batch)
        table = table_of(chunks)
        pool.maintain(batch, znew, table)
        # INVARIANT: the pool is exactly the pairs that count theta or more
        want = {p: c for p, c in table.items() if c >= pool.theta}
        have = {e["pair"]: e["c"] for e in pool.entries}
        assert have == want, (done, sorted(set(want) ^ set(have))[:4])
    return done, steps, twice


POOL_TWICE = [0]


@pytest.mark.parametrize("name,k,n", STREAMS)
@pytest.mark.parametrize("cap,capacity,depth", [(8, 96, 6), (31, 96, 6), (16, 24, 4), (31, 40, 40)])
def test_shared_first_pool_steps_are_the_references_merges(name, k, n, cap, capacity, depth):
    chunks = make_stream(name, k, n // 2, 313 * 11 + n + cap)
    done, steps, twice = run_pool(chunks, SharedFirstPool(cap, capacity, depth, random.Random(11)), 160)
    assert done > 30
    POOL_TWICE[0] += twice


def test_shared_first_pool_on_fan_streams():
    twice = 0
    for chunks in fan_streams():
        _, _, t = run_pool(list(chunks), SharedFirstPool(31, 96, 40, random.Random(5)), 60)
        twice += t
    assert twice + POOL_TWICE[0] > 30, (twice, POOL_TWICE[0])


def nine_variant_stream():
    """(p, x), (q, x), (y, r), (y, s) tie at the top -- one batch: two pairs end in x, two start with y -- and (x, y) sits in
    the pool below them, its occurrences spread over all nine of ({x, Zpx, Zqx}) x ({y, Zyr, Zys})"""
    p, q, x, y, r, s = 1, 2, 3, 4, 5, 6
    words = []
    for l in (p, q):
        for t in (r, s):
            words += [[l, x, y, t]] * 3   # (Z_l, Z_t) x 3 each
        words += [[l, x, y]] * 2          # (Z_l, y)
        words += [[l, x]] * 4
    for t in (r, s):
        words += [[x, y, t]] * 2          # (x, Z_t)
        words += [[y, t]] * 4
    words += [[x, y]] * 2                 # (x, y)
    words += [[7, 8]]                     # (a level of count 1: a pool gathered to the bottom keeps every variant)
    return [np.array(w, dtype=np.int64) for w in words], (p, q, x, y, r, s)


def test_an_entry_with_nine_variants():
    chunks, (p, q, x, y, r, s) = nine_variant_stream()
    table = table_of(chunks)
    assert table[(p, x)] == table[(q, x)] == table[(y, r)] == table[(y, s)] == 12
    assert table[(x, y)] == 3 * 4 + 2 * 2 + 2 * 2 + 2 and table[(x, y)] > 12
    # (x, y) counts MORE than the four: it is merged first and the four take over -- put it below them instead
    chunks = chunks + [np.array(w, dtype=np.int64) for w in ([p, x], [q, x], [y, r], [y, s])] * 11
    table = table_of(chunks)
    assert table[(x, y)] == 22 and table[(p, x)] == 23
    assert sorted(batch_by_levels_shared_firsts(chunks, 31)[:4]) == sorted([(p, x), (q, x), (y, r), (y, s)])
    pool = SharedFirstPool(31, 96, 40, random.Random(1))
    done, steps, twice = run_pool(chunks, pool, 16)
    assert done >= 8 and twice >= 1
    assert pool.most_variants == 9, pool.most_variants
