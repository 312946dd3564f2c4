"""Inputs shared by the CPU and the GPU tests of the paired k-mer test (tests/test_wilcoxon_host.py,
tests/test_gpu_wilcoxon.py): count matrices of two or three interleaved groups of one size n with counts from three ranges,
and hand-made rows.  Every builder is cached: a case is generated once per session."""
from functools import lru_cache

import numpy as np

import wilcoxon_ref as wr

# pairs per row: the smallest, both bounds of the permutation branch (13 | 14), wheat's 7, both bounds of the exact
# branch (50 | 51), both workgroup shapes (2n <= 64 | beyond), the largest
SIZES = [2, 3, 7, 8, 13, 14, 21, 50, 51, 64]
# counts are drawn from 0 .. hi - 1
RANGES = [3, 40, 100000]


@lru_cache(maxsize=None)
def case(n, hi, G, M):
    """(counts uint32 [M, G n + 2], lengths int64, groups): G groups of n chromosomes interleaved over the matrix, the list
    of the second group shuffled (pair j is the j-th entry of either list), two chromosomes that belong to no group.
    Lengths lie in [1e6, 1e7).  hi = 3: every length is 2^21, so x = count / length is exact, equal counts are equal
    values and nearly every row has zeros and ties among its differences.  hi = 40: two lengths, 2^20 and 2^21, assigned at
    random: zeros and ties in part of the rows, and group means that are exact in any summation order, as at hi = 3 (two
    groups whose means tie do so on the device and in numpy alike).  hi = 100000: distinct lengths within 10 % of each other (every group is on top in some rows): no row has a zero or a tie
    (asserted)."""
    rng = np.random.RandomState(100000 * n + 10 * (hi % 1000) + G)
    C = G * n + 2
    free = sorted(rng.choice(C, 2, replace=False).tolist())
    used = [c for c in range(C) if c not in free]
    groups = [used[g::G] for g in range(G)]
    rng.shuffle(groups[1])
    if hi == 3:
        lengths = np.full(C, 1 << 21, np.int64)
    elif hi == 40:
        lengths = rng.choice(np.array([1 << 20, 1 << 21], np.int64), C)
    else:
        lengths = rng.choice(np.arange(10**6, 10**6 + 10**5), C, replace=False).astype(np.int64)
    counts = rng.randint(0, hi, size=(M, C))
    counts[:, free] = 2**31
    if hi == 100000:
        x = counts / lengths.astype(np.float64)
        for ga in range(G):
            for gb in range(ga + 1, G):
                d = np.abs(x[:, groups[ga]] - x[:, groups[gb]])
                assert (d > 0).all() and (np.diff(np.sort(d, axis=1), axis=1) > 0).all()
    return counts.astype(np.uint32), lengths, groups


@lru_cache(maxsize=None)
def twin(n, hi, G, M):
    """the twin's result for a cached case: (top, second, p, means, stat)"""
    return wr.kmer_wilcoxon(*case(n, hi, G, M))


def pairs(n, hi, G, M):
    """[(a [R, n], b [R, n])]: the rows of a case split by the (top, second) pair the twin chose"""
    counts, lengths, groups = case(n, hi, G, M)
    top, second = twin(n, hi, G, M)[:2]
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    out = []
    for ga in range(G):
        for gb in range(G):
            sel = np.flatnonzero((top == ga) & (second == gb)) if ga != gb else []
            if len(sel):
                out.append((X[np.ix_(sel, groups[ga])], X[np.ix_(sel, groups[gb])]))
    return out


def _signed(n, neg):
    """a = 100 + d, b = 100 with d = +-(j + 1), negative where neg(j): no zero, no tie, a on top"""
    d = np.array([-(j + 1) if neg(j) else j + 1 for j in range(n)])
    assert d.sum() > 0
    return (100 + d).tolist(), [100] * n


# (what, a, b, branch, p or None, stat): counts over lengths of 1, a the top group (or tied with b)
HAND = [
    ("all d zero, n = 7", [3] * 7, [3] * 7, wr.PERM, 1.0, 0.0),
    ("all d zero, n = 14", [3] * 14, [3] * 14, wr.ASYM, float("nan"), 0.0),
    ("a == b except one pair", [3] * 6 + [5], [3] * 7, wr.PERM, 1.0, 0.0),
    ("all d positive and distinct, n = 7", list(range(11, 18)), [10] * 7, wr.EXACT, 2.0 / 2**7, 0.0),
    ("all d positive and distinct, n = 50", list(range(11, 61)), [10] * 50, wr.EXACT, 2.0 / 2**50, 0.0),
    ("n = 13, every |d| equal and nonzero", [6] * 8 + [4] * 5, [5] * 13, wr.PERM, None, 35.0),
    ("n = 14 with a single zero", [20] + [20 + j if j % 4 else 20 - j for j in range(1, 14)], [20] * 14, wr.ASYM, None, None),
    ("n = 50 without ties",) + _signed(50, lambda j: j % 3 == 0) + (wr.EXACT, None, None),
    ("n = 51 without ties",) + _signed(51, lambda j: j % 3 == 0) + (wr.ASYM, None, None),
    ("a tie group that straddles the sign", [12, 8, 12, 11, 7, 14, 15], [10] * 7, wr.PERM, None, None),
]


def hand(i):
    """(counts uint32 [3, 2n], lengths, groups): hand-made row i three times over -- as it is, with the groups' roles
    swapped (b on top), and with the pairs in reverse order -- a in the even columns, b in the odd ones"""
    a, b = HAND[i][1], HAND[i][2]
    n = len(a)
    counts = np.zeros((3, 2 * n), np.uint32)
    counts[0, 0::2], counts[0, 1::2] = a, b
    counts[1, 0::2], counts[1, 1::2] = b, a
    counts[2, 0::2], counts[2, 1::2] = a[::-1], b[::-1]
    return counts, np.ones(2 * n, np.int64), [list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2))]
