"""The definition of segments -- the lines of every document as a stream of their own -- and of what is built on them
(DESIGN 4.14), in NumPy and plain Python: the model every segments test compares with, element for element.  Not a test
module.

    class(t)        classes[t] & 3 if 0 <= t < len(classes), the id taken as the Python integer it is; 0 otherwise
    positions       only those of [off[0], off[n_docs]) take part
    the walk        inside a document, position by position, one bit of state, FRESH or OPEN, FRESH at the document's
                    start.  A position without SKIP is content; content seen in state FRESH starts a segment; content
                    sets OPEN; BREAK sets FRESH behind the position; SKIP alone leaves the state as it is
    out             the content ids of all segments in order; with `tag` each segment is preceded by its document's number
    seg_offsets[s]  where segment s begins in out (its tag, with one); seg_offsets[n_seg] = len(out)
    seg_doc[s]      its document;  doc_seg_offsets[d] = the segments in documents below d
    src_start[s]    off[d] for the first segment of document d, else the segment's first content position
    src_end[s]      the first content position of the next segment of the same document, else off[d + 1]
    marks[p]        val[s] where start[s] <= p < end[s], else 0; entry s is bad if start[s] < 0, end[s] < start[s],
                    end[s] > n or start[s] < end[s - 1], and the first bad entry is the error
    class rule      a token whose bytes are all in b" \\t\\n\\r\\x0b\\x0c" has SKIP, a token that contains b"\\n" has BREAK
    line statistics a segment is a duplicate iff an equal one (the same content ids; the same document too, in scope
                    "in_doc") stands earlier in the stream and it has at least min_len content ids; per document: length,
                    lines, dup_lines, content, dup_content; marks: bit 0 over the source range of every duplicate segment
    flag rule       dup_lines > line_frac * lines or dup_content > content_frac * content, in float64
"""
from collections import namedtuple

import numpy as np

BREAK, SKIP, TAG_DOC = 1, 2, 1
SPACE = b" \t\n\r\x0b\x0c"

Segs = namedtuple("Segs", "out seg_offsets seg_doc doc_seg_offsets src_start src_end")
LineStats = namedtuple("LineStats", "length lines dup_lines content dup_content marks")


def class_of(t, classes):
    t = int(t)
    return int(classes[t]) & 3 if 0 <= t < len(classes) else 0


def token_classes(tokens):
    """uint8 [len(tokens)] of the class rule, tokens = the bytes of ids 0, 1, ..."""
    out = np.zeros(len(tokens), np.uint8)
    for i, tok in enumerate(tokens):
        if len(tok) and all(b in SPACE for b in tok):
            out[i] |= SKIP
        if 10 in tok:
            out[i] |= BREAK
    return out


def segment_docs(ids, off, classes=(), tag=False):
    """Segs: out in the dtype of ids, every other column int64"""
    ids = np.asarray(ids)
    vals = [int(x) for x in ids]
    off = [int(x) for x in off]
    assert all(a <= b for a, b in zip(off, off[1:])) and 0 <= off[0] and off[-1] <= len(vals)
    out, seg_offsets, seg_doc, src_start, src_end, doc_seg = [], [], [], [], [], [0]
    for d, (o0, o1) in enumerate(zip(off, off[1:])):
        fresh, n_before = True, len(seg_doc)
        for p in range(o0, o1):
            c = class_of(vals[p], classes)
            if not c & SKIP:
                if fresh:
                    if len(seg_doc) > n_before:
                        src_end.append(p)                   # closes the segment in front, of the same document
                    seg_offsets.append(len(out))
                    seg_doc.append(d)
                    src_start.append(p if len(seg_doc) - 1 > n_before else o0)
                    if tag:
                        out.append(d)
                fresh = False
                out.append(vals[p])
            if c & BREAK:
                fresh = True
        if len(seg_doc) > n_before:
            src_end.append(o1)
        doc_seg.append(len(seg_doc))
    seg_offsets.append(len(out))
    i64 = lambda x: np.asarray(x, np.int64).reshape(-1)
    return Segs(np.asarray(out, ids.dtype).reshape(-1), i64(seg_offsets), i64(seg_doc), i64(doc_seg), i64(src_start), i64(src_end))


def segment_marks(start, end, val, n):
    """(marks uint8 [n], None), or (None, the first bad entry)"""
    start, end = [int(x) for x in start], [int(x) for x in end]
    assert len(start) == len(end) == len(val)
    for s, (a, b) in enumerate(zip(start, end)):
        if a < 0 or b < a or b > n or (s > 0 and a < end[s - 1]):
            return None, s
    marks = np.zeros(n, np.uint8)
    for a, b, v in zip(start, end, val):
        marks[a:b] = int(v)
    return marks, None


def line_stats(ids, off, classes=(), scope="in_doc", min_len=1):
    """LineStats of int64 [n_docs] columns and marks uint8 [n], and the duplicate flag per segment"""
    assert scope in ("in_doc", "stream")
    ids = np.asarray(ids)
    off = [int(x) for x in off]
    n_docs = len(off) - 1
    seg = segment_docs(ids, off, classes)
    cols = [np.zeros(n_docs, np.int64) for _ in range(5)]
    length, lines, dup_lines, content, dup_content = cols
    length[:] = np.diff(np.asarray(off, np.int64))
    seen, dup = set(), []
    for s, d in enumerate(seg.seg_doc):
        body = tuple(int(x) for x in seg.out[seg.seg_offsets[s]:seg.seg_offsets[s + 1]])
        key = (int(d), body) if scope == "in_doc" else body
        is_dup = key in seen and len(body) >= min_len
        seen.add(key)
        dup.append(is_dup)
        lines[d] += 1
        content[d] += len(body)
        dup_lines[d] += is_dup
        dup_content[d] += len(body) * is_dup
    marks, bad = segment_marks(seg.src_start, seg.src_end, [int(x) for x in dup], len(ids))
    assert bad is None
    return LineStats(*cols, marks), np.asarray(dup, bool)


def flagged(stats, line_frac=.30, content_frac=.20):
    """bool [n_docs] of the flag rule"""
    return (stats.dup_lines.astype(np.float64) > np.float64(line_frac) * stats.lines.astype(np.float64)) | \
        (stats.dup_content.astype(np.float64) > np.float64(content_frac) * stats.content.astype(np.float64))
