"""numpy twin of subphaser_amd/csrc/sp_kpca.h: row statistics, the Gram matrix of the Z-scores in the stated chunk order,
projections and sign rows of the k-mer PCA, every sum in the header's order (np.add.accumulate is strictly left to
right; np.sum is pairwise and is not used), so that the header on the host and the kernels on the device can be
compared with `==`.  Also the host recipe of Cluster.pca on top of them (`pca`), and the test matrices."""
import numpy as np

ROWS = 1024          # SP_KP_ROWS
MAX_CHROM, MAX_COMP = 1024, 32


def _seqsum(a, axis):
    """a[0] + a[1] + ... strictly left to right along `axis`"""
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def xvals(counts, lengths):
    return np.asarray(counts, np.uint32).astype(np.float64) / np.asarray(lengths, np.int64).astype(np.float64)[None, :]


def rowstats(counts, lengths):
    """(stats [M, 2] = mean, sd; bad [M] bool)"""
    x = xvals(counts, lengths)
    C = x.shape[1]
    mean = _seqsum(x, 1) / float(C)
    d = x - mean[:, None]
    sd = np.sqrt(_seqsum(d * d, 1) / float(C))
    bad = ~(sd > 0.0) | ~np.isfinite(sd) | ~np.isfinite(mean)
    return np.stack([mean, sd], axis=1), bad


def zrows(counts, lengths, stats):
    with np.errstate(all="ignore"):
        return (xvals(counts, lengths) - stats[:, :1]) / stats[:, 1:]


def gram(counts, lengths):
    """(G [C, C], n_bad, stats): chunks of ROWS rows, rows in order inside a chunk, chunks in order"""
    stats, bad = rowstats(counts, lengths)
    z = zrows(counts, lengths, stats)
    M, C = z.shape
    G = np.zeros((C, C))
    tmp = np.empty((C, C))
    for r0 in range(0, M, ROWS):
        part = np.zeros((C, C))
        for r in range(r0, min(M, r0 + ROWS)):
            if not bad[r]:
                np.multiply.outer(z[r], z[r], out=tmp)
                part += tmp
        G += part
    low = np.tril(G)
    return low + np.tril(G, -1).T, int(bad.sum()), stats


def projections(counts, lengths, U):
    """v [M, n_comp], v[r, j] = U[0, j] z_0 + U[1, j] z_1 + ... left to right; bad [M]"""
    stats, bad = rowstats(counts, lengths)
    z = zrows(counts, lengths, stats)
    U = np.asarray(U, np.float64)
    v = np.empty((z.shape[0], U.shape[1]))
    for lo in range(0, z.shape[0], 256):
        v[lo:lo + 256] = _seqsum(U.T[None, :, :] * z[lo:lo + 256, None, :], 2)
    return v, bad


def signs(counts, lengths, U):
    """(rows [n_comp], vals [n_comp]): the good row of largest |v_j|, the lowest index on ties; (-1, 0) without one"""
    v, bad = projections(counts, lengths, U)
    ab = np.where(bad[:, None], -1.0, np.abs(v))
    rows = np.argmax(ab, axis=0).astype(np.int64)        # the first maximum
    vals = v[rows, np.arange(v.shape[1])]
    none = ab[rows, np.arange(v.shape[1])] < 0
    return np.where(none, -1, rows), np.where(none, 0.0, vals)


def pca(G, sign_vals, n_components):
    """the host part of Cluster.pca: (normalised scores [C, n], percent [n], U [C, n]); sign_vals(U) -> vals [n]"""
    w, V = np.linalg.eigh(G)
    w, V = w[::-1], V[:, ::-1]
    n = min(max(2, n_components), G.shape[0])
    U = np.ascontiguousarray(V[:, :n])
    s = np.where(np.asarray(sign_vals(U)) < 0, -1.0, 1.0)
    scores = U * np.sqrt(np.maximum(w[:n], 0.0)) * s
    with np.errstate(all="ignore"):
        return (scores - scores.mean(axis=0)) / scores.std(axis=0), 100 * w[:n] / w.sum(), U


class TwinContext:
    """a context whose PCA entries are the twin (for Cluster tests without a device)"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _host(counts):
        return counts[0] if isinstance(counts, tuple) and not isinstance(counts[0], int) else counts

    def kmer_pca_gram(self, counts, lengths, want_stats=False):
        self.calls.append(("gram", counts))
        G, n_bad, stats = gram(self._host(counts), lengths)
        return (G, n_bad, stats) if want_stats else (G, n_bad)

    def kmer_pca_signs(self, counts, lengths, U):
        self.calls.append(("signs", counts))
        return signs(self._host(counts), lengths, U)


# ------------------------------------------------------------------------------------------------ test matrices
def random_case(seed, M, C, extreme=False, bad_rows=(), dup=None):
    """counts uint32 [M, C], lengths int64 [C].  extreme: counts of 0 and 2^32 - 1 and lengths above 2^32 among them;
    bad_rows: rows made constant (all zero: x = 0 on every chromosome whatever the lengths); dup = (i, j): row j := row i"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 400, (M, C), dtype=np.int64).astype(np.uint32)
    lengths = rng.integers(10 ** 6, 10 ** 8, C, dtype=np.int64)
    if extreme:
        lengths[rng.integers(0, C)] = 2 ** 32 + 12345
        lengths[0] = 2 ** 40 + 1
        lengths[-1] = 1
        k = max(1, M // 7)
        counts[rng.integers(0, M, k), rng.integers(0, C, k)] = 2 ** 32 - 1
        counts[rng.integers(0, M, k), rng.integers(0, C, k)] = 0
        counts[M // 2, :] = 2 ** 32 - 1
        counts[M // 2, 0] = 0
    for r in bad_rows:
        counts[r] = 0
    if dup is not None:
        counts[dup[1]] = counts[dup[0]]
    return counts, lengths


def planted(seed, C, M, sizes=None, shares=(0.5, 0.3, 0.2), fold=6.0):
    """counts with planted subgenome structure: chromosomes in len(shares) groups of unequal size, every k-mer enriched
    `fold` times in one group, the groups owning unequal shares of the k-mers -- the leading eigenvalues stay apart.
    Returns (counts, lengths, group of every chromosome)."""
    rng = np.random.default_rng(seed)
    K = len(shares)
    if sizes is None:
        base = C // K
        sizes = [base + (K - 1 - g if g < K - 1 else 0) for g in range(K)]
        sizes[-1] = C - sum(sizes[:-1])
    group = np.repeat(np.arange(K), sizes)
    assert group.size == C
    lengths = rng.integers(2 * 10 ** 7, 6 * 10 ** 7, C, dtype=np.int64)
    owner = rng.choice(K, size=M, p=np.asarray(shares) / sum(shares))
    rate = rng.uniform(2e-6, 8e-6, M)[:, None] * np.where(owner[:, None] == group[None, :], fold, 1.0)
    counts = rng.poisson(rate * lengths[None, :]).astype(np.uint32)
    return counts, lengths, group
