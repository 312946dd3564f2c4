"""Inputs shared by the CPU and the GPU tests of the wide rank-sum k-mer tests (tests/test_rankwide_host.py,
tests/test_gpu_rankwide.py): count matrices for a pair of group sizes under three value patterns, matrices with several
interleaved groups of very different sizes, and the twin's answers.  Every builder is cached: a case is generated once per
session and nobody writes to it."""
from functools import lru_cache

import numpy as np

import rankwide_ref as rw

# (first group, second group): just past the narrow kernel's 64; both sides of the exact rule (8 | 9) in either order; the
# padding edges of a power-of-two sort; the largest group beside the smallest; and two sizes the narrow kernel takes too
SMALL = [(65, 65), (1, 65), (65, 1), (8, 65), (9, 65), (65, 8), (3, 5), (64, 64)]
EDGES = [(255, 256), (256, 257), (257, 255)]
LARGE = [(8, 4096), (4096, 1), (4096, 4096)]
PATTERNS = ("ties", "lengths", "distinct")


def _lift(M):
    """which group a row lifts: the first in half of the rows, the second in a quarter, none in the rest (M = 1: the first)"""
    which = np.full(M, -1)
    which[: (M + 1) // 2] = 0
    which[(M + 1) // 2: (M + 1) // 2 + M // 4] = 1
    return which


@lru_cache(maxsize=None)
def size_case(n1, n2, pattern, M):
    """(counts uint32 [M, n1 + n2], lengths int64, groups): two groups in consecutive runs.
    ties      every length is 1024 (x = count / 1024 is exact) and the counts are 0..2, 0..3 in a lifted group: ties within
              and across the groups in every row; from M = 3 on the last row is all ones -- every value identical
    lengths   distinct lengths, a third of the counts zero, the others large: ties only at zero (asserted)
    distinct  every length is 1024, the first group's counts even, the second's odd, each drawn without replacement: no two
              values of a row are equal -- with a group of at most 8 the exact Mann-Whitney branch"""
    rng = np.random.RandomState((1000003 * n1 + 101 * n2 + PATTERNS.index(pattern)) % (2**31))
    C, N = n1 + n2, n1 + n2
    groups = [list(range(n1)), list(range(n1, C))]
    which = _lift(M)
    if pattern == "ties":
        lengths = np.full(C, 1024, np.int64)
        counts = rng.randint(0, 3, size=(M, C))
        for g, cols in enumerate(groups):
            counts[np.ix_(which == g, cols)] += 1
        if M >= 3:
            counts[M - 1] = 1
    elif pattern == "lengths":
        lengths = rng.choice(np.arange(10**6, 10**6 + 10**5), C, replace=False).astype(np.int64)
        counts = rng.randint(1000, 50000, size=(M, C))
        for g, cols in enumerate(groups):
            counts[np.ix_(which == g, cols)] += 20000
        counts[rng.random_sample((M, C)) < 1.0 / 3.0] = 0
        x = np.sort(counts / lengths.astype(np.float64), axis=1)
        assert ((np.diff(x, axis=1) > 0) | (x[:, 1:] == 0)).all()
    elif pattern == "distinct":
        lengths = np.full(C, 1024, np.int64)
        counts = np.empty((M, C), np.int64)
        for r in range(M):
            for g, (cols, n) in enumerate(zip(groups, (n1, n2))):
                base = N if which[r] == g else 0
                counts[r, cols] = 2 * (base + rng.choice(4 * N, n, replace=False)) + g
        assert (np.diff(np.sort(counts, axis=1), axis=1) > 0).all()
    else:
        raise ValueError(pattern)
    return counts.astype(np.uint32), lengths, groups


@lru_cache(maxsize=None)
def far_apart_case(n1, n2, M):
    """two groups whose means are far apart in every row (the first on top in the first half of the rows, the second in the
    other), ties within the groups: the narrow and the wide entry then pick the same pair whatever their order keys"""
    rng = np.random.RandomState(7 * n1 + n2)
    C = n1 + n2
    groups = [list(range(n1)), list(range(n1, C))]
    lengths = rng.choice(np.arange(10**6, 10**6 + 10**5), C, replace=False).astype(np.int64)
    counts = rng.randint(0, 40, size=(M, C))
    counts[: M // 2, :n1] += 30
    counts[M // 2:, n1:] += 30
    return counts.astype(np.uint32), lengths, groups


LAYOUT_SIZES = {3: (7, 65, 300), 5: (7, 65, 300, 8, 130)}


@lru_cache(maxsize=None)
def layout_case(G, pattern, M):
    """G groups of very different sizes whose chromosomes are interleaved over the matrix, every list in shuffled order,
    plus five chromosomes that belong to no group (their counts, 2^31, would show in every mean if they were read); the
    lifted groups move from row to row, so every group is top somewhere and the rows of one launch take different size
    pairs -- with the groups of 7 and 8, both Mann-Whitney branches under the pattern without ties"""
    sizes = LAYOUT_SIZES[G]
    rng = np.random.RandomState(G * 3 + PATTERNS.index(pattern))
    C = sum(sizes) + 5
    free = sorted(rng.choice(C, 5, replace=False).tolist())
    used = rng.permutation([c for c in range(C) if c not in free]).tolist()
    off = np.concatenate([[0], np.cumsum(sizes)])
    groups = [used[off[g]:off[g + 1]] for g in range(G)]
    lengths = np.full(C, 1024, np.int64)
    if pattern == "ties":
        counts = rng.randint(0, 3, size=(M, C))
        for r in range(M):
            counts[r, groups[r % G]] += 2
            counts[r, groups[(r // G) % G]] += 1
    elif pattern == "distinct":
        counts = np.empty((M, C), np.int64)
        for r in range(M):
            counts[r] = 8 * rng.permutation(C)           # distinct multiples of 8; the lifts below keep them apart
            counts[r, groups[r % G]] += 4 * C + 2
            counts[r, groups[(r // G) % G]] += 2 * C + 1
        inuse = np.array(sorted(used))
        assert (np.diff(np.sort(counts[:, inuse], axis=1), axis=1) > 0).all()
    else:
        raise ValueError(pattern)
    counts[:, free] = 2**31
    return counts.astype(np.uint32), lengths, groups


@lru_cache(maxsize=None)
def twin(kind, *args):
    """the twin's result for a cached case under both methods: {method: (top, second, p, means, stat)}"""
    counts, lengths, groups = {"size": size_case, "layout": layout_case, "far": far_apart_case}[kind](*args)
    return {m: rw.kmer_ranktest_wide(counts, lengths, groups, m) for m in rw.METHODS}
