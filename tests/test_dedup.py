"""CPU: chunk de-duplication.  bpe_dedup_chunks against a Python Counter, and the
claim the device path rests on -- training on the distinct chunks in first-appearance order,
weighted by multiplicity (split into powers of two), gives the merges, counts and tie-breaks of
the full chunk list -- checked with a plain-Python weighted loop against the oracle."""
import collections

import numpy as np
import pytest

import oracle
from helpers import expand_weighted, hand_weighted, split_chunks, stands_for_bytes


def chunks_of(data, offs):
    ends = np.append(offs[1:], len(data)).astype(np.int64)
    return [data[int(a):int(b)] for a, b in zip(offs.astype(np.int64), ends)]


def expected_dedup(chunks):
    cnt = collections.Counter(chunks)
    out = []
    for c in dict.fromkeys(chunks):  # first-appearance order
        m, k = cnt[c], 0
        while m:
            if m & 1:
                out.append((c, k))
            m >>= 1
            k += 1
    return out, len(cnt)


def weighted_train(chunks, weights, num_merges):
    """minbpe's loop (regex.py:49-66) with `+ w` in place of `+ 1`; tests only."""
    ids = [list(c) for c in chunks]
    pairs, counts = [], []
    for i in range(num_merges):
        stats = {}
        for ch, w in zip(ids, weights):
            for p in zip(ch, ch[1:]):
                stats[p] = stats.get(p, 0) + w
        if not stats:
            break
        pair = max(stats, key=stats.get)
        pairs.append(pair)
        counts.append(stats[pair])
        new = []
        for ch in ids:
            out, j = [], 0
            while j < len(ch):
                if j + 1 < len(ch) and ch[j] == pair[0] and ch[j + 1] == pair[1]:
                    out.append(256 + i)
                    j += 2
                else:
                    out.append(ch[j])
                    j += 1
            new.append(out)
        ids = new
    return pairs, counts


def _texts(native):
    rng = np.random.default_rng(11)
    yield native.synth_text(40_000, 61).decode()
    # tiny alphabet: many ties, a == b runs, multiplicities with several set bits
    words = ["".join("ab"[int(x)] for x in rng.integers(0, 2, size=int(L))) for L in rng.integers(1, 7, size=40)]
    yield " ".join(words[int(i)] for i in rng.integers(0, len(words), size=3000))
    yield "aaaa aaaa aaaa aa aa aa aa aa a a a b bb bbb bbb bbb"
    yield "x"
    yield "solo"


@pytest.mark.parametrize("threads", [1, 3, 64])
def test_dedup_matches_counter(native, threads):
    for text in _texts(native):
        data, offs = split_chunks(text)
        d2, o2, w, nd = native.dedup_chunks(data, offs, threads)
        exp, distinct = expected_dedup(chunks_of(data, offs))
        assert [(c, int(k)) for c, k in zip(chunks_of(d2, o2), w)] == exp
        assert nd == distinct
        assert sum(len(c) << int(k) for c, k in zip(chunks_of(d2, o2), w)) == len(data)
    # large enough for the threaded path
    text = native.synth_text(1_500_000, 62).decode()
    data, offs = split_chunks(text)
    assert len(offs) > (1 << 16)
    d2, o2, w, nd = native.dedup_chunks(data, offs, threads)
    exp, distinct = expected_dedup(chunks_of(data, offs))
    assert [(c, int(k)) for c, k in zip(chunks_of(d2, o2), w)] == exp and nd == distinct


def test_dedup_edge_cases(native):
    d2, o2, w, nd = native.dedup_chunks(b"", np.empty(0, np.uint64))
    assert d2 == b"" and len(o2) == 0 and nd == 0
    # empty chunks (duplicate offsets) are chunks too: they carry no pairs
    d2, o2, w, nd = native.dedup_chunks(b"abab", np.array([0, 0, 2, 2], np.uint64))
    assert chunks_of(d2, o2) == [b"", b"ab"] and w.tolist() == [1, 1] and nd == 2
    with pytest.raises(RuntimeError):
        native.dedup_chunks(b"abc", np.array([2, 1], np.uint64))
    # offsets are checked by the thread that counts their range: a descent (or an overrun) far into a long list
    n = 200_000
    data = bytes(n)
    for t in (1, 8):
        bad = np.arange(n, dtype=np.uint64)
        bad[150_000] = 10
        with pytest.raises(RuntimeError):
            native.dedup_chunks(data, bad, t)
        bad = np.arange(n, dtype=np.uint64)
        bad[-1] = n + 5
        with pytest.raises(RuntimeError):
            native.dedup_chunks(data, bad, t)


def test_weighted_distinct_chunks_train_like_the_full_list(native):
    for text in _texts(native):
        data, offs = split_chunks(text)
        exp_pairs, exp_counts, _ = oracle.train(data, 80, offs, raise_on_empty=False)
        d2, o2, w, _ = native.dedup_chunks(data, offs)
        got_pairs, got_counts = weighted_train(chunks_of(d2, o2), [1 << int(k) for k in w], 80)
        assert got_pairs == exp_pairs and got_counts == exp_counts


def test_weighted_oracle_with_hand_set_exponents_equals_the_written_out_list():
    """oracle.train(..., weights=2^e) is the reference of the GPU tests on hand-weighted streams
    (tests/test_gpu_weighted.py).  The test above pins it for the exponents a de-duplication emits; this one for
    arbitrary ones: exponents 0..6 set by hand -- exponent 6 next to 0, one-byte chunks and empty chunks with
    exponents, chunk starts at multiples of 256, 1024 and 4096 ids, a 2500-id run of one symbol -- against the plain
    oracle on the list with every chunk written out 2^e times in place: pairs, counts, and the length of the
    written-out list after every merge."""
    data, offs, exps, edges = hand_weighted(900, 6, 6, seed=5, big_every=40)
    lens = np.diff(np.append(offs, len(data)).astype(np.int64))
    assert set(exps.tolist()) == set(range(7))
    assert edges["singles"] and all(lens[i] == 1 and exps[i] == 6 and exps[i + 1] == 0 for i in edges["singles"])
    assert edges["empties"] and all(lens[i] == 0 for i in edges["empties"])
    assert any(exps[i] > 0 for i in edges["empties"])
    assert sorted({m for m, _ in edges["aligned"]}) == [256, 1024, 4096]
    assert all(int(offs[i]) % m == 0 and offs[i] > 0 and exps[i] == 6 and exps[i - 1] == 0 for m, i in edges["aligned"])
    r = edges["run"]
    assert data[int(offs[r]):int(offs[r]) + int(lens[r])] == b"z" * 2500 and int(offs[r]) % 1024 == 900 and exps[r] == 6
    full, full_offs = expand_weighted(data, offs, exps)
    assert len(full) == stands_for_bytes(offs, exps, len(data))
    nm = 150
    want = oracle.train(full, nm, full_offs, raise_on_empty=False)
    got = oracle.train(data, nm, offs, raise_on_empty=False, weights=np.uint64(1) << exps.astype(np.uint64))
    assert len(want[0]) == nm and any(a == b for a, b in want[0])
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    py_pairs, py_counts = weighted_train(chunks_of(data, offs), [1 << int(e) for e in exps], 25)
    assert py_pairs == want[0][:25] and py_counts == want[1][:25]
