"""The definition of document selection in a few lines of NumPy: the model every select test compares with,
element for element.  Not a test module.

    off      the n_docs + 1 offsets; len(d) = off[d + 1] - off[d]
    j        a selection, d = index[j]:  l_j = len(d) if max_len is None, otherwise min(len(d), max_len);
             s_j = off[d], or off[d + 1] - l_j with tail
    out      ids[s_0 : s_0 + l_0] | ids[s_1 : s_1 + l_1] | ...
    out_offsets[j] = l_0 + ... + l_{j-1}, out_offsets[m] the total
"""
import numpy as np


class BadOffsets(ValueError):
    """offsets that descend or pass len(ids); index = the first such entry"""

    def __init__(self, index):
        super().__init__(f"doc_offsets[{index}]")
        self.index = index


class BadSelection(IndexError):
    """an index outside [0, n_docs); index = the lowest such position"""

    def __init__(self, index):
        super().__init__(f"index[{index}]")
        self.index = index


def check_offsets(off, n):
    """the first entry that is beyond n or below the one before it, or None"""
    off = [int(x) for x in off]
    for i, o in enumerate(off):
        if o > n or o < 0 or (i and o < off[i - 1]):
            return i
    return None


def select(ids, off, index, max_len=None, tail=False):
    """(out, out_offsets): out in the dtype of ids (int64 for a list), out_offsets int64 [m + 1]"""
    ids = np.asarray(ids)
    if ids.dtype.kind not in "iu":
        ids = ids.astype(np.int64)
    off = np.asarray([int(x) for x in off], dtype=np.int64)
    bad = check_offsets(off, len(ids))
    if bad is not None:
        raise BadOffsets(bad)
    n_docs = len(off) - 1
    index = [int(x) for x in np.asarray(index).reshape(-1)]
    for j, d in enumerate(index):
        if not 0 <= d < n_docs:
            raise BadSelection(j)
    idx = np.asarray(index, dtype=np.int64)
    length = off[idx + 1] - off[idx] if len(idx) else np.zeros(0, np.int64)
    if max_len is not None:
        length = np.minimum(length, int(max_len))
    start = (off[idx + 1] - length if tail else off[idx]) if len(idx) else np.zeros(0, np.int64)
    out_off = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(length, out=out_off[1:])
    # element e of selection j comes from start[j] + (e - out_off[j])
    src = np.repeat(start - out_off[:-1], length) + np.arange(out_off[-1], dtype=np.int64)
    return ids[src], out_off
