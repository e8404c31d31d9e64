"""The definition of the repetition statistics in Python tuples and dicts: the model every repetition test
compares with, element for element.  Not a test module.  No hashing of its own: a window is a tuple of Python integers,
the classes of a document a dict from window to the list of its starts.

    key(d)          the slice selection emits for document d with the same max_len / tail: ids[s_d : s_d + l_d],
                    l_d = len(d) or min(len(d), max_len), s_d = off[d] or off[d + 1] - l_d with tail
    windows         key[k : k + w) for every key position k with k + w <= l_d; a key shorter than w has none
    equality        two windows of the SAME document are equal when they hold the same ids at their full width (two int64
                    ids that differ only above bit 32 differ, negative ids are values like any other); windows of
                    different documents are never compared
    repeat          a position k at which a window starts that equals one starting at a lower position of the same key
    length[d]       l_d;  windows[d] = max(0, l_d - w + 1);  distinct[d] = the distinct windows = windows - repeats
    covered[d]      the key positions i with k <= i < k + w for some repeat k
    top_count[d]    the largest multiplicity of a window of the document, 0 without a window
    top_pos[d]      (s_d - off[d]) + the lowest start of the window of that multiplicity -- among several, the one whose
                    first start is lowest --, -1 without a window
    marks[p]        bit 0: a repeat starts at stream position p; bit 1: p is covered; 0 elsewhere
    flagged[d]      the Gopher rule: for some (w, t) of `top` top_count_w * w > t * length, or for some (w, t) of `dup`
                    covered_w > t * length; a document of length 0 is never flagged
"""
from collections import namedtuple

import numpy as np

from ngram_model import _ints, _offsets, stream  # noqa: F401  (stream: for the tests)

Stats = namedtuple("Stats", "length windows distinct covered top_count top_pos marks n_repeat_docs")

GOPHER_TOP = ((2, .20), (3, .18), (4, .16))
GOPHER_DUP = ((5, .15), (6, .14), (7, .13), (8, .12), (9, .11), (10, .10))


def stats(ids, off, w, max_len=None, tail=False):
    """Stats of int64 [n_docs] columns, marks uint8 [n] and the number of documents with a repeat"""
    ids = _ints(ids)
    off = _offsets(off, len(ids))
    n_docs = len(off) - 1
    cols = [np.zeros(n_docs, np.int64) for _ in range(6)]
    length, windows, distinct, covered, top_count, top_pos = cols
    top_pos[:] = -1
    marks = np.zeros(len(ids), np.uint8)
    for d, (o0, o1) in enumerate(zip(off, off[1:])):
        l = o1 - o0 if max_len is None else min(o1 - o0, int(max_len))
        s = o1 - l if tail else o0
        length[d] = l
        starts = {}
        for k in range(l - w + 1):
            starts.setdefault(tuple(ids[s + k:s + k + w]), []).append(k)   # (k ascends: the first one is the lowest)
        windows[d] = max(0, l - w + 1)
        distinct[d] = len(starts)
        inside = set()
        for ks in starts.values():
            for k in ks[1:]:
                marks[s + k] |= 1
                inside.update(range(k, k + w))
        for i in inside:
            marks[s + i] |= 2
        covered[d] = len(inside)
        if starts:
            count, first = max((len(ks), -ks[0]) for ks in starts.values())
            top_count[d], top_pos[d] = count, (s - o0) - first
    return Stats(*cols, marks, int((distinct < windows).sum()))


def _rules(top, dup):
    return [(int(w), t, True) for w, t in top] + [(int(w), t, False) for w, t in dup]


def flagged(ids, off, top=GOPHER_TOP, dup=GOPHER_DUP, max_len=None, tail=False):
    """bool [n_docs]: the rule as the package states it, both sides of every comparison in float64"""
    n_docs = len(off) - 1
    out = np.zeros(n_docs, bool)
    by_w = {}
    for w, t, is_top in _rules(top, dup):
        st = by_w.get(w)
        if st is None:
            st = by_w[w] = stats(ids, off, w, max_len, tail)
        lhs = (st.top_count * w if is_top else st.covered).astype(np.float64)
        out |= (lhs > np.float64(t) * st.length.astype(np.float64)) & (st.length > 0)
    return out
