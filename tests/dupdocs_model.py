"""The definition of exact document de-duplication in a few lines of Python: the model every dupdocs test
compares with, element for element.  Not a test module.

    key(d)     the bytes, at the width of ids, of the slice selection emits for document d with the same max_len / tail:
               ids[s_d : s_d + l_d], l_d = len(d) or min(len(d), max_len), s_d = off[d] or off[d + 1] - l_d with tail
    first[d]   the lowest e with key(e) == key(d)
    counts[d]  the number of documents with d's key where first[d] == d, 0 elsewhere
    n_distinct the number of d with first[d] == d
"""
import numpy as np

from select_model import BadOffsets, check_offsets


def keys(ids, off, max_len=None, tail=False):
    """the key of every document, as bytes"""
    ids = np.asarray(ids)
    if ids.dtype.kind not in "iu":
        ids = ids.astype(np.int64)
    off = [int(x) for x in off]
    bad = check_offsets(off, len(ids))
    if bad is not None:
        raise BadOffsets(bad)
    out = []
    for o0, o1 in zip(off, off[1:]):
        l = o1 - o0 if max_len is None else min(o1 - o0, int(max_len))
        s = o1 - l if tail else o0
        out.append(ids[s:s + l].tobytes())
    return out


def duplicates(ids, off, max_len=None, tail=False):
    """(first int64 [n_docs], counts int64 [n_docs], n_distinct)"""
    ks = keys(ids, off, max_len, tail)
    seen = {}
    first = np.zeros(len(ks), dtype=np.int64)
    counts = np.zeros(len(ks), dtype=np.int64)
    for d, k in enumerate(ks):
        first[d] = seen.setdefault(k, d)
        counts[first[d]] += 1
    return first, counts, len(seen)
