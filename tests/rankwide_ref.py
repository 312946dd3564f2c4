"""numpy twin of subphaser_amd/csrc/sp_rankwide.h: the Kruskal-Wallis and Mann-Whitney tests between the top and the second
subgenome group of every k-mer row for groups of up to 4096 chromosomes.  The doubled midranks come from sorting
(np.sort of each group, np.searchsorted of every value in both sorted lists); the statistics are the header's operations
in the header's order on int64; erfc is scipy's.  The exact Mann-Whitney null is counted over Python integers and every
table entry is the correctly rounded Fraction.  means are np.mean of a group's list, top and second follow the
reference's order key -sum(x) / len(x) with Python's left-to-right sum (Cluster.py:181-183)."""
from fractions import Fraction
from functools import lru_cache

import numpy as np
from scipy import special

MAXG = 4096
EXACT_MAX = 8
METHODS = ("kruskal", "mannwhitneyu")


def rank_ints(a, b):
    """a [M, n1] the top group's values, b [M, n2] the second's.  Returns (S1, S2, T) int64 [M]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    M = len(a)
    S1, S2, T = np.zeros(M, np.int64), np.zeros(M, np.int64), np.zeros(M, np.int64)
    for r in range(M):
        sa, sb = np.sort(a[r]), np.sort(b[r])
        for x, S in ((a[r], S1), (b[r], S2)):
            lb = np.searchsorted(sa, x, "left") + np.searchsorted(sb, x, "left")
            ub = np.searchsorted(sa, x, "right") + np.searchsorted(sb, x, "right")
            eq = (ub - lb).astype(np.int64)
            S[r] = int((2 * lb.astype(np.int64) + eq + 1).sum())
            T[r] += int((eq * eq - 1).sum())
    return S1, S2, T


@lru_cache(maxsize=None)
def exact_counts(n1, n2):
    """number of arrangements with Mann-Whitney statistic u, u = 0 .. n1 n2 (Python ints, nothing wraps): the coefficients
    of the Gaussian binomial [m + n choose m]_q = prod_{i = 1..m} (1 - q^(n + i)) / (1 - q^i) as a power series modulo
    q^(m n + 1) -- all the numerator factors first, then each division as running sums along a residue class.
    (tests/ranktest_ref.py counts the same numbers by the textbook recurrence, which costs m n^2 m n steps: the host test
    compares the two at the sizes where that is affordable.)"""
    m, n = min(n1, n2), max(n1, n2)
    D = m * n
    c = np.zeros(D + 1, dtype=object)
    c[0] = 1
    for i in range(1, m + 1):
        if n + i <= D:
            c[n + i:] = c[n + i:] - c[:D + 1 - (n + i)]
    for i in range(1, m + 1):
        for r in range(i):
            c[r::i] = np.add.accumulate(c[r::i])
    return tuple(int(v) for v in c)


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
    """every entry the correctly rounded exact fraction (int / int of Python is correctly rounded)"""
    c = exact_counts(n1, n2)
    total = sum(c)
    out, cum = np.empty(len(c)), 0
    for u in range(len(c) - 1, -1, -1):
        cum += c[u]
        out[u] = cum / total
    return out


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
    if (n1 <= EXACT_MAX or n2 <= EXACT_MAX) and (T == 0).any():
        sf = exact_sf(n1, n2)
        p = np.where(T == 0, 2.0 * sf[np.clip(U.astype(np.int64), 0, n1 * n2)], p)
    return U1, np.clip(p, 0.0, 1.0)


def rows(a, b, method):
    """(stat, p) of the test between the rows of a [M, n1] and b [M, n2]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n1, n2 = a.shape[1], b.shape[1]
    S1, S2, T = rank_ints(a, b)
    if method == "kruskal":
        return kruskal(n1, n2, S1, S2, T)
    if method == "mannwhitneyu":
        return mannwhitneyu(n1, n2, S1, T)
    raise ValueError(method)


def means_top2(counts, lengths, groups):
    """(X [M, C] fp64, means [M, G], top int32 [M], second): np.mean per list; the order key -sum(x) / len(x), the sum added
    left to right from 0 (np.cumsum is sequential), descending, ties in group order (a stable sort, as sorted() is)"""
    counts = np.asarray(counts)
    X = counts.astype(np.float64) / np.asarray(lengths).astype(np.float64)
    M, G = len(counts), len(groups)
    means, key = np.empty((M, G)), np.empty((M, G))
    for g, cols in enumerate(groups):
        V = np.ascontiguousarray(X[:, cols])
        for r in range(M):
            means[r, g] = np.mean(V[r])
        key[:, g] = -(np.cumsum(V, axis=1)[:, -1] / len(cols)) if M else 0.0
    order = np.argsort(key, axis=1, kind="stable") if M else np.zeros((0, G), np.int64)
    top = order[:, 0].astype(np.int32)
    second = (order[:, 1] if G > 1 else order[:, 0]).astype(np.int32)
    return X, means, top, second


def kmer_ranktest_wide(counts, lengths, groups, method):
    """Context.kmer_ranktest_wide: (top int32 [M], second, pvals, means [M, G], stat)"""
    X, means, top, second = means_top2(counts, lengths, groups)
    M, G = len(X), len(groups)
    p, stat = np.ones(M), np.full(M, np.nan)
    for ga in range(G):
        for gb in range(G):
            sel = np.flatnonzero((top == ga) & (second == gb)) if ga != gb else np.empty(0, np.int64)
            if sel.size:
                stat[sel], p[sel] = rows(X[np.ix_(sel, groups[ga])], X[np.ix_(sel, groups[gb])], method)
    return top, second, p, means, stat
