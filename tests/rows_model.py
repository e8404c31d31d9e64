"""The definition of resident training rows in a few lines of NumPy: the model every rows test compares
with, element for element.  Not a test module."""
import numpy as np


def stream_of(ids, off, sep):
    """(stream, doc_index, pos) as Python lists: seq_d = ids of document d (+ [sep]), joined"""
    stream, doc, pos = [], [], []
    for d in range(len(off) - 1):
        seq = [int(x) for x in ids[int(off[d]):int(off[d + 1])]] + ([sep] if sep is not None else [])
        stream += seq
        doc += [d] * len(seq)
        pos += list(range(len(seq)))
    return stream, doc, pos


def brute_rows(total, row_len, stride):
    """rows the model produces: a new row every `stride` positions until one reaches the end of the stream"""
    if total == 0:
        return 0
    r = 0
    while r * stride + row_len < total:
        r += 1
    return r + 1


def pack(ids, off, row_len, stride, sep, pad):
    """(rows, doc_index, pos) int64 arrays [R, row_len]"""
    stream, doc, pos = stream_of(ids, off, sep)
    T = len(stream)
    R = brute_rows(T, row_len, stride)
    q = np.arange(R, dtype=np.int64)[:, None] * stride + np.arange(row_len, dtype=np.int64)[None, :]
    q = np.where(q < T, q, T)  # position T: the pad
    take = lambda lst, fill: np.array(lst + [fill], dtype=np.int64)[q]
    return take(stream, pad), take(doc, -1), take(pos, 0)


def per_doc(ids, off, row_len, sep, pad, truncate="right", pad_side="right"):
    """(rows [n_docs, row_len], lengths [n_docs]) int64"""
    n_docs = len(off) - 1
    rows = np.full((n_docs, row_len), pad, dtype=np.int64)
    lengths = np.zeros(n_docs, dtype=np.int64)
    for d in range(n_docs):
        seq = [int(x) for x in ids[int(off[d]):int(off[d + 1])]] + ([sep] if sep is not None else [])
        kept = seq[:row_len] if truncate == "right" else seq[max(len(seq) - row_len, 0):]
        lengths[d] = len(kept)
        if kept:
            if pad_side == "right":
                rows[d, :len(kept)] = kept
            else:
                rows[d, row_len - len(kept):] = kept
    return rows, lengths
