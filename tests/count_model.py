"""The definition of bpe_count_resident and bpe_count_fold in plain Python / NumPy (no engine).  merges: the pairs in merge
order, merge r makes id 256 + r.
    bins      bin t for 0 <= t < 256 + M, then one bin per pass id in ascending order
    count     occurrences per bin; an id in no bin: BadId(its first position)
    fold      the histogram at vocab_size: from the last merge down, the count of t >= vocab_size goes to its two children
    curve     tokens at every size 256 + k -- here by expanding every id (project_model), not by folding, so that the fold
              is checked against something that is not itself"""
import numpy as np

from project_model import BadId  # noqa: F401  (raised by count)


def bins(M, pass_ids=()):
    """int64 [B]: the id each bin stands for"""
    pas = sorted(int(p) for p in pass_ids)
    assert all(not 0 <= p < 256 + M for p in pas) and len(set(pas)) == len(pas)
    return np.concatenate([np.arange(256 + M, dtype=np.int64), np.array(pas, dtype=np.int64)])


def count(ids, M, pass_ids=()):
    """int64 [B]: occurrences of every bin's id; BadId(first position whose id has no bin)"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    layout = bins(M, pass_ids)
    top = 256 + M
    dense = (ids >= 0) & (ids < top)
    out = np.zeros(len(layout), dtype=np.int64)
    out[:top] = np.bincount(ids[dense], minlength=top)
    rest = ids[~dense]
    known = np.isin(rest, layout[top:])
    if not known.all():
        raise BadId(int(np.flatnonzero(~dense)[np.flatnonzero(~known)[0]]))
    for j, p in enumerate(layout[top:].tolist()):
        out[top + j] = int(np.count_nonzero(rest == p))
    return out


def fold(counts, merges, vocab_size):
    """the histogram at vocab_size as a list of Python ints (no overflow): bins [vocab_size, 256 + M) zero, pass bins as they are"""
    h = [int(c) for c in counts]
    top = 256 + len(merges)
    assert 256 <= vocab_size <= top <= len(h)
    for t in range(top - 1, vocab_size - 1, -1):
        a, b = merges[t - 256]
        assert 0 <= a < t and 0 <= b < t, "not a merge list of the shape training makes"
        h[a] += h[t]
        h[b] += h[t]
        h[t] = 0
    return h


def expansion_lengths(merges):
    """int64 [256 + M, M + 1]: entry [t, k] = len(project_model.expand(t, merges, 256 + k)) -- E(t)'s own recursion, on
    lengths and for all sizes at once: 1 where t < 256 + k, else the sum of its children's"""
    M = len(merges)
    lens = np.ones((256 + M, M + 1), dtype=np.int64)
    k = np.arange(M + 1)
    for t in range(256, 256 + M):
        a, b = merges[t - 256]
        assert 0 <= a < t and 0 <= b < t, "not a merge list of the shape training makes"
        lens[t] = np.where(k <= t - 256, lens[a] + lens[b], 1)
        assert lens[t].max() < 2**62      # (so that no sum above has wrapped)
    return lens


def curve_by_expansion(ids, merges, pass_ids=()):
    """curve[k] = sum over the ids of len(project_model.expand(t, merges, 256 + k, pass_ids)), as Python ints: every id
    expanded on its own, nothing folded"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    M = len(merges)
    occurs = count(ids, M, pass_ids)            # (BadId for an id that does not expand)
    lens = expansion_lengths(merges).astype(object)
    dense = sum((int(c) * lens[t] for t, c in enumerate(occurs[:256 + M].tolist()) if c), np.zeros(M + 1, dtype=object))
    return [int(x) + int(occurs[256 + M:].sum()) for x in dense]
