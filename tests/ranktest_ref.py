"""numpy twin of subphaser_amd/csrc/sp_ranktest.h: the Kruskal-Wallis and Mann-Whitney tests between the top and the second
subgenome group of every k-mer row, in the header's integer formulation (doubled midranks by counting comparisons, the
rank sums and the tie term from them) and its order of floating-point operations.  erfc is scipy's; the exact
Mann-Whitney null is counted here by the textbook recurrence over Python integers, not by the header's product."""
from fractions import Fraction
from functools import lru_cache

import numpy as np
from scipy import special

MAXG = 64
EXACT_MAX = 8
METHODS = ("kruskal", "mannwhitneyu")


def rank_ints(x, n1):
    """x: [M, N] pooled values, the first n1 columns the top group.  Returns (S1, S2, T) int64 [M]: the sums of the doubled
    midranks r2 = 2 #{<} + #{==} + 1 over the two groups and T = sum(e^2 - 1), e the size of a value's tie group."""
    x = np.asarray(x, np.float64)
    lt = (x[:, None, :] < x[:, :, None]).sum(axis=2)
    eq = (x[:, None, :] == x[:, :, None]).sum(axis=2)
    r2 = 2 * lt + eq + 1
    return r2[:, :n1].sum(axis=1), r2[:, n1:].sum(axis=1), (eq * eq - 1).sum(axis=1)


@lru_cache(maxsize=None)
def exact_counts(n1, n2):
    """number of arrangements of n1 + n2 distinct values with Mann-Whitney statistic u, u = 0 .. n1 n2 (Python ints):
    f(u; m, n) = f(u - n; m - 1, n) + f(u; m, n - 1) -- the largest value belongs to the first sample or to the second"""
    m, n = min(n1, n2), max(n1, n2)
    prev = [[1] for _ in range(n + 1)]                       # m = 0: one arrangement, u = 0
    for mm in range(1, m + 1):
        cur = [[1]]                                          # n = 0
        for nn in range(1, n + 1):
            f = [0] * (mm * nn + 1)
            for u, c in enumerate(prev[nn]):                 # f(u - nn; mm - 1, nn)
                f[u + nn] += c
            for u, c in enumerate(cur[nn - 1]):              # f(u; mm, nn - 1)
                f[u] += c
            cur.append(f)
        prev = cur
    return tuple(prev[n])


def exact_sf_fractions(n1, n2):
    """P(statistic >= u) as exact fractions"""
    c = exact_counts(n1, n2)
    total = sum(c)
    out, cum = [None] * len(c), 0
    for u in range(len(c) - 1, -1, -1):
        cum += c[u]
        out[u] = Fraction(cum, total)
    return out


@lru_cache(maxsize=None)
def exact_sf(n1, n2):
    """the header's table: every entry the correctly rounded quotient of two integers"""
    return np.array([float(f) for f in exact_sf_fractions(n1, n2)], np.float64)


def kruskal(n1, n2, S1, S2, T):
    """(stat, p) float64 [M]"""
    N = float(n1 + n2)
    R1, R2 = S1.astype(np.float64) / 2.0, S2.astype(np.float64) / 2.0
    ties = 1.0 - T.astype(np.float64) / (N * N * N - N)
    ssbn = R1 * R1 / float(n1) + R2 * R2 / float(n2)
    with np.errstate(all="ignore"):
        H = (12.0 / (N * (N + 1.0)) * ssbn - 3.0 * (N + 1.0)) / ties
        p = np.where(H > 0.0, special.erfc(np.sqrt(np.where(H > 0.0, H, 0.0) / 2.0)), 1.0)
    same = ties == 0.0
    return np.where(same, np.nan, H), np.where(same, 1.0, p)


def mannwhitneyu(n1, n2, S1, T):
    """(stat, p) float64 [M]"""
    N, nn = float(n1 + n2), float(n1 * n2)
    R1 = S1.astype(np.float64) / 2.0
    U1 = R1 - float(n1 * (n1 + 1)) / 2.0
    U2 = nn - U1
    U = np.maximum(U1, U2)
    with np.errstate(all="ignore"):
        s = np.sqrt(nn / 12.0 * ((N + 1.0) - T.astype(np.float64) / (N * (N - 1.0))))
        z = (U - nn / 2.0 - 0.5) / s
        p = 2.0 * (0.5 * special.erfc(z / 1.4142135623730951))
    if n1 <= EXACT_MAX or n2 <= EXACT_MAX:
        sf = exact_sf(n1, n2)
        exact = T == 0
        p = np.where(exact, 2.0 * sf[np.clip(U.astype(np.int64), 0, n1 * n2)], p)
    return U1, np.clip(p, 0.0, 1.0)


def rows(a, b, method):
    """(stat, p) of the test between the rows of a [M, n1] and b [M, n2]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n1, n2 = a.shape[1], b.shape[1]
    S1, S2, T = rank_ints(np.concatenate([a, b], axis=1), n1)
    if method == "kruskal":
        return kruskal(n1, n2, S1, S2, T)
    if method == "mannwhitneyu":
        return mannwhitneyu(n1, n2, S1, T)
    raise ValueError(method)


def kmer_ranktest(counts, lengths, groups, method):
    """Context.kmer_ranktest: (top int32 [M], second, pvals, means [M, G], stat).  x = count / length in fp64; a group's
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
    p, stat = np.ones(M), np.full(M, np.nan)
    for ga in range(G):
        for gb in range(G):
            sel = np.flatnonzero((top == ga) & (second == gb)) if ga != gb else np.empty(0, np.int64)
            if sel.size:
                stat[sel], p[sel] = rows(X[np.ix_(sel, groups[ga])], X[np.ix_(sel, groups[gb])], method)
    return top, second, p, means, stat
