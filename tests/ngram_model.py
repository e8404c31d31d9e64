"""The definition of n-gram overlap with a reference set in Python tuples and a dict: the model every ngram
test compares with, element for element.  Not a test module.  No hashing of its own: a window is a tuple of Python
integers -- an int32 id and the int64 id of the same value are the same integer --, the index a dict from window to the
lowest position at which it starts.

    reference windows   R[i : i + w) for every reference document r and every i with roff[r] <= i, i + w <= roff[r + 1]
    low(W)              the lowest i at which the reference window W starts
    key(d)              the slice selection emits for document d with the same max_len / tail: ids[s_d : s_d + l_d],
                        l_d = len(d) or min(len(d), max_len), s_d = off[d] or off[d + 1] - l_d with tail
    hit                 a key position k with k + w <= l_d whose window key[k : k + w) is a reference window
    hits[d]             the number of hits;  first[d] = (s_d - off[d]) + the lowest hit k, or -1;
    ref_pos[d]          low(window at that first hit), or -1;  starts[p] = 1 where a hit window starts at stream position p
"""
import numpy as np

from select_model import BadOffsets, check_offsets


def _ints(ids):
    ids = np.asarray(ids)
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError("ids must be integers")
    return [int(x) for x in ids.reshape(-1)]


def _offsets(off, n):
    off = [int(x) for x in off]
    bad = check_offsets(off, n)
    if bad is not None:
        raise BadOffsets(bad)
    return off


def index(ref, roff, w):
    """(low, n_windows): low = {window: lowest start}, n_windows = the reference windows with repeats"""
    ref = _ints(ref)
    roff = _offsets(roff, len(ref))
    low, n_windows = {}, 0
    for r0, r1 in zip(roff, roff[1:]):
        for i in range(r0, r1 - w + 1):
            low.setdefault(tuple(ref[i:i + w]), i)       # (i ascends: the first one seen is the lowest)
            n_windows += 1
    return low, n_windows


def overlap(low, w, ids, off, max_len=None, tail=False):
    """(hits, first, ref_pos int64 [n_docs], starts uint8 [n], n_hit_docs) against the dict index() made"""
    ids = _ints(ids)
    off = _offsets(off, len(ids))
    n_docs = len(off) - 1
    hits = np.zeros(n_docs, np.int64)
    first = np.full(n_docs, -1, np.int64)
    ref_pos = np.full(n_docs, -1, np.int64)
    starts = np.zeros(len(ids), np.uint8)
    for d, (o0, o1) in enumerate(zip(off, off[1:])):
        l = o1 - o0 if max_len is None else min(o1 - o0, int(max_len))
        s = o1 - l if tail else o0
        for k in range(l - w + 1):
            at = low.get(tuple(ids[s + k:s + k + w]))
            if at is None:
                continue
            if hits[d] == 0:
                first[d], ref_pos[d] = (s - o0) + k, at
            hits[d] += 1
            starts[s + k] = 1
    return hits, first, ref_pos, starts, int((hits > 0).sum())


def run(ref, roff, w, ids, off, max_len=None, tail=False):
    """index() and overlap() in one: (hits, first, ref_pos, starts, n_hit_docs, n_windows, n_distinct)"""
    low, n_windows = index(ref, roff, w)
    return overlap(low, w, ids, off, max_len, tail) + (n_windows, len(low))


def stream(docs, dtype=np.int64):
    """(ids, off) of the documents laid back to back"""
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    ids = np.concatenate([np.asarray(d, dtype=dtype) for d in docs]) if docs else np.zeros(0, dtype)
    return ids.astype(dtype), off
