"""The definition of bpe_token_spans_resident (include/bpe_hip.h) in NumPy: a table of byte strings, the
table index of every token and optional document offsets to the two int64 [n, 2] arrays.  Written from the definition,
token by token and document by document, not from the kernels."""
import numpy as np


def is_lead(b):
    return (b & 0xC0) != 0x80


def entry_meta(entry):
    """(len, leads, cont) of one table entry"""
    leads = int(is_lead(np.frombuffer(entry, dtype=np.uint8)).sum())
    cont = 1 if len(entry) and not is_lead(entry[0]) else 0
    return len(entry), leads, cont


def spans(table, tidx, doc_offsets=None):
    """table: list of bytes; tidx: the table index of every token; doc_offsets: None (one document) or n_docs + 1
    ascending positions <= n.  Returns (byte_spans, char_spans), int64 [n, 2]; (-1, -1) outside every document."""
    meta = [entry_meta(e) for e in table]
    n = len(tidx)
    bs = np.full((n, 2), -1, dtype=np.int64)
    cs = np.full((n, 2), -1, dtype=np.int64)
    off = [0, n] if doc_offsets is None else [int(o) for o in doc_offsets]
    assert all(0 <= a <= b <= n for a, b in zip(off, off[1:])) and 0 <= off[0] <= n
    for d in range(len(off) - 1):
        B = C = 0
        for i in range(off[d], off[d + 1]):
            ln, leads, cont = meta[int(tidx[i])]
            bs[i] = (B, B + ln)
            cs[i] = (max(C - cont, 0), C + leads)
            B += ln
            C += leads
    return bs, cs


def totals(table, tidx):
    """(sum of len, sum of leads) over the whole batch"""
    meta = [entry_meta(e) for e in table]
    return sum(meta[int(t)][0] for t in tidx), sum(meta[int(t)][1] for t in tidx)


def shortest_cover(s, b0, b1):
    """(c0, c1): the shortest run of code points of s whose encoding covers bytes [b0, b1) of s.encode(), b0 < b1"""
    starts = [0]
    for ch in s:
        starts.append(starts[-1] + len(ch.encode("utf-8")))
    c0 = max(k for k in range(len(s) + 1) if starts[k] <= b0)
    c1 = min(k for k in range(len(s) + 1) if starts[k] >= b1)
    return c0, c1


def check_against_str(s, pieces, bs, cs):
    """the two properties the definition buys, for the tokens `pieces` (bytes each) of one document that decodes to s"""
    enc = s.encode("utf-8")
    assert b"".join(pieces) == enc
    starts = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum([len(ch.encode("utf-8")) for ch in s], out=starts[1:])
    for i, p in enumerate(pieces):
        b0, b1 = int(bs[i][0]), int(bs[i][1])
        c0, c1 = int(cs[i][0]), int(cs[i][1])
        assert enc[b0:b1] == p, (i, p)
        if not p:
            assert c0 == c1, (i, c0, c1)
            continue
        w0 = int(np.searchsorted(starts, b0, side="right")) - 1   # the last character that starts at or before b0
        w1 = int(np.searchsorted(starts, b1, side="left"))         # the first boundary at or after b1
        assert (c0, c1) == (w0, w1), (i, p, (c0, c1), (w0, w1))
        assert p in s[c0:c1].encode("utf-8")
