"""The definition of bpe_project_resident in plain Python / NumPy (no engine): what a list of token ids made with 256 + M
merges looks like at vocab_size entries.  merges: the pairs in merge order, merge r makes id 256 + r.
    E(t) = [t]           if 0 <= t < vocab_size or t is a pass id
    E(t) = E(a) + E(b)   if vocab_size <= t < 256 + M and (a, b) is the pair of t
Any other id does not project: BadId(position of the first one)."""
import numpy as np


class BadId(Exception):
    """args[0] = the first position whose id does not project"""


def expansions(merges, vocab_size):
    """{id: tuple of ids below vocab_size} for every id in [vocab_size, 256 + M), children before parents"""
    merges = [tuple(int(x) for x in p) for p in merges]
    assert 256 <= vocab_size <= 256 + len(merges)
    table = {}
    for t in range(vocab_size, 256 + len(merges)):
        a, b = merges[t - 256]
        assert 0 <= a < t and 0 <= b < t, "not a merge list of the shape training makes"
        table[t] = (table[a] if a >= vocab_size else (a,)) + (table[b] if b >= vocab_size else (b,))
    return table


def expand(t, merges, vocab_size, pass_ids=()):
    """E(t) as a list, by the recursion itself (small cases: the cross-check of expansions())"""
    t = int(t)
    if 0 <= t < vocab_size or t in pass_ids:
        return [t]
    if vocab_size <= t < 256 + len(merges):
        a, b = merges[t - 256]
        return expand(a, merges, vocab_size, pass_ids) + expand(b, merges, vocab_size, pass_ids)
    raise BadId(t)


def lengths(ids, merges, vocab_size, pass_ids=()):
    """len(E(t)) of every id as int64; BadId(first bad position)"""
    table = expansions(merges, vocab_size)
    top = 256 + len(merges)
    pass_ids = set(int(p) for p in pass_ids)
    out = np.ones(len(ids), dtype=np.int64)
    for i, t in enumerate(ids):
        t = int(t)
        if vocab_size <= t < top:
            out[i] = len(table[t])
        elif not (0 <= t < vocab_size or t in pass_ids):
            raise BadId(i)
    return out


def project(ids, merges, vocab_size, pass_ids=()):
    """E(t_0) + E(t_1) + ... as a list of ints"""
    lengths(ids, merges, vocab_size, pass_ids)  # (the first bad position, before anything is made)
    table = expansions(merges, vocab_size)
    out = []
    for t in ids:
        t = int(t)
        out.extend(table.get(t, (t,)))
    return out


def doc_offsets(ids, merges, vocab_size, positions, pass_ids=()):
    """the output position of every token position (each <= len(ids); position len(ids): the total), int64"""
    cum = np.concatenate([[0], np.cumsum(lengths(ids, merges, vocab_size, pass_ids))]).astype(np.int64)
    positions = np.asarray(positions, dtype=np.int64)
    assert ((positions >= 0) & (positions <= len(ids))).all()
    return cum[positions]
