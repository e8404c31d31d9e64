"""The definition of span de-duplication in Python tuples and a dict: the model every dupspans test compares
with, element for element.  Not a test module.  No hashing of its own: a window is a tuple of Python integers -- an int32
id and the int64 id of the same value are the same integer --, the seen set a dict from window to the lowest absolute
position at which it starts.

    key(d)          the slice selection emits for document d with the same max_len / tail: ids[s_d : s_d + l_d],
                    l_d = len(d) or min(len(d), max_len), s_d = off[d] or off[d + 1] - l_d with tail
    windows         ids[p : p + w) for every absolute position p with s_d <= p and p + w <= s_d + l_d; a key shorter
                    than w has none
    equality        two windows are equal when they hold the same ids at their full width (two int64 ids that differ only
                    above bit 32 differ, negative ids are values like any other); windows of ALL documents are compared
    low(W)          the lowest absolute position at which a window equal to W starts, over all keys
    seen            the window at p of document d is seen if low(W) < s_d (scope "earlier document"), with `anywhere` if
                    low(W) < p (every occurrence but the stream's first)
    length[d]       l_d;  windows[d] = max(0, l_d - w + 1);  seen[d] = the seen positions
    covered[d]      the key positions i with k <= i < k + w for some seen k
    first[d]        (s_d - off[d]) + the lowest seen position relative to s_d, -1 without one
    src_pos[d]      low(W) of the window at that first seen position, -1 without one
    marks[p]        bit 0: a seen window starts at stream position p; bit 1: p is covered; 0 elsewhere
    keep            position p of [off[0], off[n_docs]) is kept iff (mask[p] & bits) != 0, with `drop` iff it is 0;
                    out = the kept ids in order, out_off[d] = the kept positions in [off[0], off[d])
"""
from collections import namedtuple

import numpy as np

from ngram_model import _ints, _offsets, stream  # noqa: F401  (stream: for the tests)

Stats = namedtuple("Stats", "length windows seen covered first src_pos marks n_docs_seen n_windows n_distinct")


def keys(off, max_len=None, tail=False):
    """[(s_d, l_d)] of the documents"""
    out = []
    for o0, o1 in zip(off, off[1:]):
        l = o1 - o0 if max_len is None else min(o1 - o0, int(max_len))
        out.append((o1 - l if tail else o0, l))
    return out


def stats(ids, off, w, max_len=None, tail=False, anywhere=False):
    """Stats of int64 [n_docs] columns, marks uint8 [n] and the three counters"""
    ids = _ints(ids)
    off = _offsets(off, len(ids))
    n_docs = len(off) - 1
    ks = keys(off, max_len, tail)
    low, n_windows = {}, 0
    for s, l in ks:
        for p in range(s, s + l - w + 1):
            low.setdefault(tuple(ids[p:p + w]), p)      # (documents and p ascend: the first one met is the lowest)
            n_windows += 1
    cols = [np.zeros(n_docs, np.int64) for _ in range(6)]
    length, windows, seen, covered, first, src_pos = cols
    first[:] = -1
    src_pos[:] = -1
    marks = np.zeros(len(ids), np.uint8)
    for d, (s, l) in enumerate(ks):
        length[d], windows[d] = l, max(0, l - w + 1)
        inside = set()
        for p in range(s, s + l - w + 1):
            at = low[tuple(ids[p:p + w])]
            if at < (p if anywhere else s):
                if seen[d] == 0:
                    first[d], src_pos[d] = p - off[d], at
                seen[d] += 1
                marks[p] |= 1
                inside.update(range(p, p + w))
        for i in inside:
            marks[i] |= 2
        covered[d] = len(inside)
    return Stats(*cols, marks, int((seen > 0).sum()), n_windows, len(low))


def keep(ids, off, mask, bits=0xFF, drop=False):
    """(the kept ids in the dtype of ids, out_off int64 [n_docs + 1])"""
    ids = np.asarray(ids)
    off = _offsets(off, len(ids))
    mask = [int(x) for x in np.asarray(mask).reshape(-1)]
    assert len(mask) == len(ids) and 1 <= bits <= 255
    kept = [p for p in range(off[0], off[-1]) if ((mask[p] & bits) != 0) != bool(drop)]
    out_off = [sum(1 for p in kept if p < o) for o in off]
    return ids[kept] if kept else ids[:0], np.asarray(out_off, np.int64)
