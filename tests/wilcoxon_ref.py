"""numpy twin of subphaser_amd/csrc/sp_wilcoxon.h: the Wilcoxon signed-rank test between the top and the second subgenome
group of every k-mer row, in the header's integer formulation (zeros dropped, doubled midranks of the nonzero |d| by
counting comparisons, W2 / T / m from them) and its order of floating-point operations.  erfc is scipy's; the exact null
is counted here over Python integers by generating-function products, and the permutation counts by a subset-sum
histogram -- neither is the header's procedure."""
from fractions import Fraction
from functools import lru_cache

import numpy as np
from scipy import special

MAXG = 64
EXACT_MAX = 50
PERM_MAX = 13
EXACT, PERM, ASYM = 0, 1, 2


def rank_ints(d):
    """d: [M, n] differences.  Returns (m, W2, T, r2): m = #nonzero, r2 [M, n] the doubled midranks of the nonzero |d|
    (0 at the zeros), W2 the sum of r2 over d > 0, T = sum over the nonzero of (e^2 - 1), e the size of a value's tie
    group -- all int64."""
    d = np.asarray(d, np.float64)
    nz = d != 0
    ad = np.abs(d)
    both = nz[:, None, :] & nz[:, :, None]                    # [row, j, i]
    lt = ((ad[:, None, :] < ad[:, :, None]) & both).sum(axis=2)
    eq = ((ad[:, None, :] == ad[:, :, None]) & both).sum(axis=2)
    r2 = np.where(nz, 2 * lt + eq + 1, 0).astype(np.int64)
    W2 = np.where(d > 0, r2, 0).sum(axis=1)
    T = np.where(nz, eq * eq - 1, 0).sum(axis=1).astype(np.int64)
    return nz.sum(axis=1).astype(np.int64), W2, T, r2


@lru_cache(maxsize=None)
def exact_counts(n):
    """number of subsets of {1 .. n} with sum s, s = 0 .. n (n + 1) / 2 (Python ints): the coefficients of
    prod_i (1 + q^i)"""
    c = [1]
    for i in range(1, n + 1):
        nxt = c + [0] * i
        for s, v in enumerate(c):
            nxt[s + i] += v
        c = nxt
    return tuple(c)


def exact_table_fractions(n):
    """min(P(W <= s), P(W >= s)) as exact fractions"""
    c = exact_counts(n)
    total = 2 ** n
    le = np.cumsum(np.array(c, dtype=object)).tolist()
    return [Fraction(min(le[s], total - (le[s - 1] if s else 0)), total) for s in range(len(c))]


@lru_cache(maxsize=None)
def exact_table(n):
    return np.array([float(f) for f in exact_table_fractions(n)], np.float64)


def branch(n, m, T):
    exact = (m == n) & (T == 0) & (n <= EXACT_MAX)
    return np.where(exact, EXACT, PERM if n <= PERM_MAX else ASYM)


def stat(m, W2):
    return np.minimum(W2 / 2.0, (m * (m + 1) - W2) / 2.0)


def perm_p(n, m, W2, r2):
    """the permutation branch of one row: counts of subset sums of the nonzero doubled ranks, as Python ints"""
    hist = {0: 1}
    for r in [int(x) for x in r2 if x]:
        nxt = dict(hist)
        for s, c in hist.items():
            nxt[s + r] = nxt.get(s + r, 0) + c
        hist = nxt
    le = sum(c for s, c in hist.items() if s <= W2) << (n - m)
    ge = sum(c for s, c in hist.items() if s >= W2) << (n - m)
    return min(1.0, min(le, ge) / float(1 << n) * 2)


def asym_p(m, W2, T):
    c = m.astype(np.float64)
    r_plus = W2.astype(np.float64) / 2.0
    with np.errstate(all="ignore"):
        mn = c * (c + 1.0) * 0.25
        se = c * (c + 1.0) * (2.0 * c + 1.0)
        se = se - T.astype(np.float64) / 2.0
        se = np.sqrt(se / 24.0)
        z = (r_plus - mn) / se
        return 2.0 * (0.5 * special.erfc(np.abs(z) / 1.4142135623730951))


def rows(a, b):
    """(stat, p, branch, (m, W2, T)) of the test between the paired rows of a and b, [M, n] each"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    M, n = a.shape
    m, W2, T, r2 = rank_ints(a - b)
    br = branch(n, m, T)
    p = asym_p(m, W2, T)
    if n <= EXACT_MAX:
        ex = br == EXACT
        p[ex] = np.clip(2.0 * exact_table(n)[W2[ex] // 2], 0.0, 1.0)
    for r in np.flatnonzero(br == PERM):
        p[r] = perm_p(n, int(m[r]), int(W2[r]), r2[r])
    return stat(m, W2), p, br, (m, W2, T)


def kmer_wilcoxon(counts, lengths, groups):
    """Context.kmer_wilcoxon: (top int32 [M], second, pvals, means [M, G], stat).  x = count / length in fp64; a group's
    mean is np.sum of its values in list order / n; top and second by mean, descending, ties in group order."""
    counts = np.asarray(counts)
    X = counts.astype(np.float64) / np.asarray(lengths).astype(np.float64)
    M, G = len(counts), len(groups)
    means = np.empty((M, G))
    for r in range(M):
        for g, cols in enumerate(groups):
            means[r, g] = np.sum(np.ascontiguousarray(X[r, cols])) / len(cols)
    order = np.argsort(-means, axis=1, kind="stable") if M else np.zeros((0, G), np.int64)
    top = order[:, 0].astype(np.int32)
    second = (order[:, 1] if G > 1 else order[:, 0]).astype(np.int32)
    p, st = np.ones(M), np.full(M, np.nan)
    for ga in range(G):
        for gb in range(G):
            sel = np.flatnonzero((top == ga) & (second == gb)) if ga != gb else np.empty(0, np.int64)
            if sel.size:
                st[sel], p[sel] = rows(X[np.ix_(sel, groups[ga])], X[np.ix_(sel, groups[gb])])[:2]
    return top, second, p, means, st
