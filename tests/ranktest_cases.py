"""Inputs shared by the CPU and the GPU tests of the rank-sum k-mer tests (tests/test_ranktest_host.py,
tests/test_gpu_ranktest.py): count matrices for a pair of group sizes with and without ties, matrices with several
interleaved groups, and hand-made rows.  Every builder is cached: a case is generated once per session."""
from functools import lru_cache

import numpy as np

import ranktest_ref as rr

# group sizes (first, second): both exact-branch bounds (8 | 9), the largest group, N = 2 .. 128
SIZES = [(1, 1), (1, 2), (2, 2), (3, 5), (7, 7), (8, 9), (9, 9), (8, 64), (64, 1), (64, 64)]


@lru_cache(maxsize=None)
def size_case(n1, n2, ties, M):
    """(counts uint32 [M, n1 + n2], lengths int64, groups): two groups in consecutive runs, the first lifted in half of the
    rows, the second in a quarter.  ties: every length is 1024 (x = count / 1024 is exact, so equal counts are equal
    values, and group means of equal count sums are equal in any summation order) and the counts are small: most rows
    have ties.  Otherwise the lengths are distinct and the counts positive: no two values of a row are equal (asserted)."""
    rng = np.random.RandomState(1000 * n1 + 10 * n2 + (1 if ties else 0))
    C = n1 + n2
    groups = [list(range(n1)), list(range(n1, C))]
    if ties:
        lengths = np.full(C, 1024, np.int64)
        counts = rng.poisson(4, size=(M, C))
        counts[: M // 2, :n1] += 2
        counts[M // 2: 3 * M // 4, n1:] += 2
    else:
        lengths = rng.choice(np.arange(10**6, 10**6 + 10**5), C, replace=False).astype(np.int64)
        counts = rng.randint(1, 5000, size=(M, C))
        counts[: M // 2, :n1] += 1500
        counts[M // 2: 3 * M // 4, n1:] += 1500
        x = counts / lengths.astype(np.float64)
        assert (np.diff(np.sort(x, axis=1), axis=1) > 0).all()
    return counts.astype(np.uint32), lengths, groups


@lru_cache(maxsize=None)
def layout_case(G, ties, M):
    """G groups of unequal size whose chromosomes are interleaved over the matrix, one list shuffled, chromosomes that
    belong to no group (their counts would show in every mean if they were read); the lifted group moves from row to
    row, so every group is top somewhere and the (top, second) pair varies"""
    sizes = {3: (3, 9, 12), 5: (2, 5, 9, 10, 64)}[G]
    rng = np.random.RandomState(G * 2 + (1 if ties else 0))
    C = sum(sizes) + 3
    free = sorted(rng.choice(C, 3, replace=False).tolist())
    used = rng.permutation([c for c in range(C) if c not in free]).tolist()
    off = np.concatenate([[0], np.cumsum(sizes)])
    groups = [sorted(used[off[g]:off[g + 1]]) for g in range(G)]
    rng.shuffle(groups[1])
    if ties:
        lengths = np.full(C, 1024, np.int64)
        counts = rng.poisson(5, size=(M, C))
    else:
        lengths = rng.choice(np.arange(10**6, 10**6 + 10**5), C, replace=False).astype(np.int64)
        counts = rng.randint(1, 5000, size=(M, C))
    for r in range(M):
        counts[r, groups[r % G]] *= 3
        counts[r, groups[(r // G) % G]] *= 2
    counts[:, free] = 2**31
    return counts.astype(np.uint32), lengths, groups


def hand_rows():
    """(counts, lengths, groups, what): groups of 3 and 4 over lengths of 1, the first group on top in every row"""
    rows = [
        ([5, 5, 5, 5, 5, 5, 5], "all values identical"),
        ([10, 11, 12, 1, 2, 3, 4], "perfectly separated"),
        ([12, 10, 11, 4, 1, 3, 2], "perfectly separated, unsorted"),
        ([7, 9, 10, 1, 2, 3, 7], "exactly one tie, across the groups"),
        ([9, 9, 10, 1, 2, 3, 4], "ties inside the first group only"),
        ([8, 9, 10, 2, 2, 2, 4], "ties inside the second group only"),
        ([6, 5, 4, 5, 4, 3, 2], "overlapping, two ties across"),
        ([0, 0, 1, 0, 0, 0, 0], "one value differs"),
    ]
    counts = np.array([r for r, _ in rows], np.uint32)
    return counts, np.ones(7, np.int64), [[0, 1, 2], [3, 4, 5, 6]], [w for _, w in rows]


@lru_cache(maxsize=None)
def twin(kind, *args):
    """the twin's result for a cached case under both methods: {method: (top, second, p, means, stat)}"""
    counts, lengths, groups = {"size": size_case, "layout": layout_case}[kind](*args)
    return {m: rr.kmer_ranktest(counts, lengths, groups, m) for m in rr.METHODS}
