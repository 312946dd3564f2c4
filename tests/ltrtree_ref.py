"""Plain Python twin of subphaser_amd/csrc/sp_ltrtree.h, written from the definition in its head comment (not from its code):
sketches as sorted sets, pairs as set operations on the union's first s values, neighbour joining as the scan of all live
pairs.  nj_numpy is the same procedure with the scan as one argmin over the live sub-matrix (row-major argmin = lowest i,
then lowest j, among equal Q); test_ltrtree_host.py holds it against the plain scan, and both against additive trees."""
import random

import numpy as np

M64 = (1 << 64) - 1
NONE = M64
DMAX = 1 << 40
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


class Guard(Exception):
    """an updated |D| reached 2^40"""


def mix(z):
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 & M64
    z ^= z >> 27
    z = z * 0x94d049bb133111eb & M64
    return z ^ (z >> 31)


def value(kmer):
    v = 0
    for ch in kmer:
        v = v * 4 + CODE[ch]
    return v


def hashes(seq, k):
    """the set of hashes of the valid k-mers of a string (anything but ACGT is invalid)"""
    out = set()
    for p in range(len(seq) - k + 1):
        kmer = seq[p:p + k]
        if all(ch in CODE for ch in kmer):
            rc = "".join(COMP[ch] for ch in reversed(kmer))
            out.add(mix(min(value(kmer), value(rc))))
    return out


def sketch(seq, k, s):
    """(the s entries, len)"""
    low = sorted(hashes(seq, k))[:s]
    return low + [NONE] * (s - len(low)), len(low)


def sketches(seqs, k, s):
    rows = [sketch(x, k, s) for x in seqs]
    return np.array([r[0] for r in rows], np.uint64).reshape(len(seqs), s), np.array([r[1] for r in rows], np.int32)


def pair(a, b, s):
    """a, b: the hashes of two sketches (without the unused tail): (shared, denom)"""
    sa, sb = set(a), set(b)
    first = sorted(sa | sb)[:s]
    return sum(1 for h in first if h in sa and h in sb), len(first)


def pairs(sk, ln, s):
    n = len(ln)
    rows = [[int(h) for h in sk[i][:ln[i]]] for i in range(n)]
    shared, denom = np.zeros((n, n), np.int32), np.zeros((n, n), np.int32)
    for i in range(n):
        for j in range(i, n):
            shared[i, j], denom[i, j] = shared[j, i], denom[j, i] = pair(rows[i], rows[j], s)
    return shared, denom


def nj(D, dmax=DMAX):
    """records [(i, j, D(i, j), R_i, R_j)] of a matrix given as lists of Python ints; raises Guard when an updated |D| reaches
    dmax (the definition's 2^40; tests lower it)"""
    N = len(D)
    D = [list(map(int, row)) for row in D]
    live = list(range(N))
    out = []
    while len(live) > 2:
        n = len(live)
        R = {i: sum(D[i][k] for k in live) for i in live}
        best = min(((n - 2) * D[i][j] - R[i] - R[j], i, j) for a, i in enumerate(live) for j in live[a + 1:])
        _, i, j = best
        out.append((i, j, D[i][j], R[i], R[j]))
        for k in live:
            if k != i and k != j:
                v = (D[i][k] + D[j][k] - D[i][j]) // 2
                if abs(v) >= dmax:
                    raise Guard()
                D[i][k] = D[k][i] = v
        live.remove(j)
    i, j = live
    out.append((i, j, D[i][j], 0, 0))
    return out


def nj_numpy(D, dmax=DMAX, trace=None):
    """the same records as nj(), int64 [N - 1, 5]; raises Guard; trace: a list that receives the largest updated |D| of every join"""
    D = np.array(D, np.int64)
    N = D.shape[0]
    live = np.arange(N)
    out = np.zeros((N - 1, 5), np.int64)
    big = np.int64(1) << 62
    for t in range(N - 2):
        n = len(live)
        sub = D[np.ix_(live, live)]
        R = sub.sum(axis=1)
        Q = (n - 2) * sub - R[:, None] - R[None, :]
        Q[np.tril_indices(n)] = big
        a, b = divmod(int(np.argmin(Q)), n)
        i, j = int(live[a]), int(live[b])
        out[t] = (i, j, D[i, j], R[a], R[b])
        rest = np.delete(live, [a, b])
        v = (D[i, rest] + D[j, rest] - D[i, j]) >> 1          # arithmetic shift: floor
        if trace is not None:
            trace.append(int(np.abs(v).max()) if len(v) else 0)
        if len(v) and int(np.abs(v).max()) >= dmax:
            raise Guard()
        D[i, rest] = v
        D[rest, i] = v
        live = np.delete(live, b)
    i, j = int(live[0]), int(live[1])
    out[N - 2] = (i, j, D[i, j], 0, 0)
    return out


# ---- inputs
def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return "".join(COMP.get(ch, "N") for ch in reversed(s))


def mutate(rng, s, rate):
    return "".join(rng.choice([c for c in "ACGT" if c != ch]) if ch in CODE and rng.random() < rate else ch for ch in s)


def random_matrix(seed, N, hi=1 << 31):
    rng = np.random.default_rng(seed)
    D = np.triu(rng.integers(0, hi, (N, N), dtype=np.int64), 1)
    return D + D.T


def tied_matrix(N, d=1000):
    D = np.full((N, N), d, np.int64)
    np.fill_diagonal(D, 0)
    return D


def negative_matrix(seed, N):
    """far from a tree: most distances tiny, a few huge -- the halved differences go below zero"""
    rng = np.random.default_rng(seed)
    D = np.triu(np.where(rng.random((N, N)) < 0.15, rng.integers(1 << 29, 1 << 31, (N, N)), rng.integers(0, 8, (N, N))).astype(np.int64), 1)
    return D + D.T


def random_tree(seed, N, lo=2, hi=2000):
    """a random unrooted binary tree on leaves 0 .. N - 1 with EVEN integer edge lengths: (edges [(u, v, w)], its additive
    distance matrix int64 [N, N]).  N >= 3: inner nodes N .. 2N - 3; N = 2: one edge."""
    rng = random.Random(seed)
    even = lambda: 2 * rng.randrange(lo // 2, hi // 2)
    if N == 2:
        edges = [(0, 1, even())]
    else:
        edges = [(N, 0, even()), (N, 1, even()), (N, 2, even())]
        for leaf in range(3, N):
            q = rng.randrange(len(edges))
            u, v, w = edges[q]
            mid = N + leaf - 2
            w1 = 2 * rng.randrange(1, w // 2) if w >= 4 else w       # an edge of 2 keeps its length on one side
            edges[q] = (u, mid, w1)
            edges += [(mid, v, w - w1 if w >= 4 else even()), (mid, leaf, even())]
    n_nodes = max(max(u, v) for u, v, _ in edges) + 1
    adj = [[] for _ in range(n_nodes)]
    for u, v, w in edges:
        adj[u].append((v, w))
        adj[v].append((u, w))
    D = np.zeros((N, N), np.int64)
    for src in range(N):
        dist, order = {src: 0}, [src]
        for u in order:
            for v, w in adj[u]:
                if v not in dist:
                    dist[v] = dist[u] + w
                    order.append(v)
        for dst in range(N):
            D[src, dst] = dist[dst]
    return edges, D


def guard_limit(D):
    """(limit, join, top): a guard limit that the run of D reaches, the first join that reaches it, and the largest updated |D|
    of the whole run.  The limit is the largest updated |D| of the second half of the joins without the last, so that joins
    are left to do when it fires.  N >= 6."""
    trace = []
    nj_numpy(D, trace=trace)
    limit = max(trace[len(trace) // 2:-1])
    return limit, next(t for t, v in enumerate(trace) if v >= limit), max(trace)
