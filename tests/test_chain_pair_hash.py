"""The merge pass's pair look-up table (minbpe_amd/csrc/kernels/k_chain.hip: chain_pair_bucket, chain_hash_m2,
chain_hash_find), restated in Python: a batch's K <= 31 pairs (a, b) go into 256 buckets,

    bucket = ((umul24(a, m) + umul24(b, m2)) >> 8) & 255,    m2 = 2 m^2 + 1,

and the selection looks for a multiplier m (odd, 129 .. 255: 64 of them, two per round) under which no two pairs share a
bucket.  A batch without one takes the compare path, which is exact: what is bounded here is how often the slow path runs,
not correctness.

m2 is larger than 256 on purpose.  With both multipliers below 256 two ids that differ by one fall less than a bucket
apart, and (z, y + 1), (z + 1, y) -- consecutive new ids on both sides, the second side descending -- share a bucket under
EVERY m; 2 m^2 + 1 moves b by at least 130 buckets' worth per id.

Measured here (10^4 key sets each, ids below 32,000; share of sets with none of the 64 multipliers):
    random pairs                      K = 5: 0        K = 15: 0       K = 31: 0
    31 pairs sharing one first token  0               31 pairs sharing one second token  0
    first tokens z0 .. z0 + 30, random seconds   0    second tokens z0 .. z0 + 30, random firsts   0
    second tokens z0 .. z0 + 30 behind ONE first token   0
    first tokens z0 .. z0 + 30 before ONE second token   about 2 %  (only m separates them, and m < 256: what the table keyed
                                                          by the first token alone did with consecutive first tokens)
    both sides consecutive, ascending / one descending   0 / 0"""
import numpy as np
import pytest

N_SETS = 10_000
MULTIPLIERS = np.arange(129, 256, 2)


def umul24(x, y):
    return ((np.asarray(x, dtype=np.uint64) & 0xFFFFFF) * (np.uint64(y) & np.uint64(0xFFFFFF))) & np.uint64(0xFFFFFFFF)


def hash_m2(m):
    return 2 * m * m + 1


def bucket(a, b, m):
    return (((umul24(a, m) + umul24(b, hash_m2(m))) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)) & np.uint64(255)


def find(A, B):
    """chain_hash_find for N key sets at once (A, B: N x K): the first multiplier free of collisions, 0 = none"""
    found = np.zeros(A.shape[0], dtype=np.int64)
    for m in MULTIPLIERS:
        h = np.sort(bucket(A, B, int(m)), axis=1)
        ok = (h[:, 1:] != h[:, :-1]).all(axis=1)
        found[(found == 0) & ok] = int(m)
    return found


def check_found(A, B, found):
    """a found multiplier is free of collisions (every set, recomputed one at a time for a sample, vectorised for all)"""
    for i in np.flatnonzero(found)[:200]:
        assert len({int(bucket(a, b, int(found[i]))) for a, b in zip(A[i], B[i])}) == A.shape[1]
    idx = np.flatnonzero(found)
    for m in np.unique(found[idx]):
        rows = idx[found[idx] == m]
        h = np.sort(bucket(A[rows], B[rows], int(m)), axis=1)
        assert (h[:, 1:] != h[:, :-1]).all()


def distinct(rng, n, k):
    return np.array([rng.choice(32000, k, replace=False) for _ in range(n)], dtype=np.int64)


def random_pairs(rng, n, k):
    """n sets of k DISTINCT pairs with ids below 32,000"""
    codes = np.array([rng.choice(32000 * 32000, k, replace=False) for _ in range(n)], dtype=np.int64)
    return codes // 32000, codes % 32000


@pytest.mark.parametrize("K", [5, 15, 31])
def test_random_key_sets(K):
    rng = np.random.default_rng(100 + K)
    A, B = random_pairs(rng, N_SETS, K)
    found = find(A, B)
    check_found(A, B, found)
    miss = float((found == 0).mean())
    rounds = float(((found[found != 0] - 129) // 4).mean())
    print(f"K = {K}: share of sets without a multiplier {miss:.5f}, mean rounds before the hit {rounds:.2f}")
    assert miss <= 1e-3, miss  # (the cap is set for K = 31; smaller sets are easier and held to the same)


def structured(rng, kind, n, K=31):
    one = rng.integers(0, 32000, (n, 1))
    z0 = rng.integers(256, 31000, (n, 1)) + np.arange(K)[None, :]
    z1 = rng.integers(256, 31000, (n, 1)) + np.arange(K)[None, :]
    other = distinct(rng, n, K)
    if kind == "one_first":
        return np.broadcast_to(one, (n, K)), other
    if kind == "one_second":
        return other, np.broadcast_to(one, (n, K))
    if kind == "new_firsts":
        return z0, other
    if kind == "new_seconds":
        return other, z0
    if kind == "new_seconds_one_first":
        return np.broadcast_to(one, (n, K)), z0
    if kind == "new_firsts_one_second":
        return z0, np.broadcast_to(one, (n, K))
    if kind == "new_both":
        return z0, z1
    if kind == "new_both_descending":
        return z0, z1[:, ::-1]
    raise ValueError(kind)


# (the cap on the share of sets without a multiplier: 10^-3 where both tokens vary or the large multiplier m2 does the
# separating; consecutive first tokens before ONE second token are separated by m < 256 alone, as consecutive first tokens
# were in the table keyed by the first token -- the bucket function leaves m as it was, so that case is reported, and
# bounded only loosely: no more than one set in ten)
KINDS = [("one_first", 1e-3), ("one_second", 1e-3), ("new_firsts", 1e-3), ("new_seconds", 1e-3),
         ("new_seconds_one_first", 1e-3), ("new_firsts_one_second", 0.1), ("new_both", 1e-3), ("new_both_descending", 1e-3)]


@pytest.mark.parametrize("kind,cap", KINDS)
def test_structured_key_sets(kind, cap):
    rng = np.random.default_rng(7)
    A, B = structured(rng, kind, N_SETS)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    found = find(A, B)
    check_found(A, B, found)
    miss = float((found == 0).mean())
    print(f"{kind}: share of sets without a multiplier {miss:.5f}")
    assert miss <= cap, (kind, miss)


def test_two_small_multipliers_would_lose_descending_neighbours():
    """why m2 is large: with m2 < 256 the pairs (z, y + 1) and (z + 1, y) are less than a bucket apart under every m"""
    z, y = 1000, 2000
    apart = 0
    for m in MULTIPLIERS:
        m = int(m)
        for m2 in (m, 384 - m, 129 + ((m * 37) & 126)):
            d = (z * m + (y + 1) * m2) - ((z + 1) * m + y * m2)
            assert abs(d) < 256
        apart += int(bucket(z, y + 1, m)) != int(bucket(z + 1, y, m))
    assert apart >= 60, apart  # (... and 2 m^2 + 1 separates them under nearly every m)
