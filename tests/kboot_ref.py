"""numpy twin of subphaser_amd/csrc/sp_kboot.h: one k-means bootstrap replicate in Gram space, written from the header's
definitions (not from its code), plus the measure that says which replicates a comparison may cover.

  gram(z, cols)          G[r] = sum_t outer(z[:, cols[r, t]], z[:, cols[r, t]]), t in draw order: `for t: G += outer`,
                         every product rounded and then added -- what the kernel must give bit for bit
  solve(G, K, seed, rep) greedy k-means++ and Lloyd on one Gram matrix -> (labels, iters, gap)

`gap` is the smallest relative margin of any decision the replicate took:
  - best against second-best distance of a point (the labels at the start and every Lloyd iteration), over the size of
    the terms the distances are made of;
  - best against the second-best potential among the trials that drew ANOTHER candidate (equal candidates are no
    decision, exactly equal potentials go to the first trial by definition), over the second-best;
  - |r - nearest running-sum boundary| / pot of every candidate draw.
A replicate is DECIDED when gap >= DECIDED: fp64 sums over at most n * C ~ 1.3e5 terms carry a relative error of about
1.4e-11, and the cut sits two orders above that.  Labels and iteration counts are compared on decided replicates only;
every test case requires that at most 1 % of its replicates are not (MAX_UNDECIDED)."""
import math

import numpy as np

DECIDED = 1e-9
MAX_UNDECIDED = 0.01
MAXIT = 300
_MASK = (1 << 64) - 1


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK
    return x ^ (x >> 31)


def u(seed, rep, i):
    """draw i of replicate `rep`: uniform in [0, 1) with 53 bits"""
    h = mix((mix((seed ^ (rep * 0xD6E8FEB86659FD93)) & _MASK) + i) & _MASK)
    return (h >> 11) * 2.0 ** -53


def trials(K):
    return 2 + int(math.floor(math.log(K)))


def gram(z, cols):
    """z: C x M, cols: R x n -> R x C x C"""
    z = np.asarray(z, np.float64)
    cols = np.asarray(cols)
    R, n = cols.shape
    C = z.shape[0]
    G = np.zeros((R, C, C))
    for t in range(n):
        zt = z[:, cols[:, t]].T                     # R x C
        G += zt[:, :, None] * zt[:, None, :]
    return G


def blobs(seed, C, K, M, noise):
    """test input: C points in K groups (point i in group i % K) over M columns, every column Z-normalised like
    Cluster.zscores; continuous noise on every point, so no two chromosomes are duplicates"""
    rng = np.random.RandomState(seed)
    x = rng.normal(size=(K, M))[np.arange(C) % K] + noise * rng.normal(size=(C, M))
    return (x - x.mean(axis=0)) / x.std(axis=0)


def _rel(best, second, scale):
    if not np.isfinite(second):
        return np.inf                               # nothing to confuse it with
    return (second - best) / scale if scale > 0 else 0.0


def solve(G, K, seed, rep):
    G = np.asarray(G, np.float64)
    C = G.shape[0]
    d = np.diag(G).copy()
    D2 = np.maximum(0.0, (d[:, None] + d[None, :]) - 2.0 * G)
    mag = d[:, None] + d[None, :] + 2.0 * np.abs(G)  # size of the terms of D2
    gap = np.inf
    T = trials(K)
    centres = [min(int(u(seed, rep, 0) * C), C - 1)]
    closest = D2[centres[0]].copy()
    pot = np.cumsum(closest)[-1]
    for c in range(1, K):
        cs = np.cumsum(closest)
        cands, pots = [], []
        for t in range(T):
            r = u(seed, rep, 1 + (c - 1) * T + t) * pot
            cands.append(min(int(np.searchsorted(cs, r, side="right")), C - 1))
            gap = min(gap, float(np.abs(cs - r).min()) / pot if pot > 0 else 0.0)
            pots.append(np.cumsum(np.minimum(closest, D2[cands[-1]]))[-1])
        best = int(np.argmin(pots))                 # the first of equal potentials
        # equal candidates are no decision; neither is an EXACT tie between two candidates: the potentials are bit-defined
        # (D2 and min from the bit-defined G, summed in index order), "the first trial wins" is part of the definition, and
        # at K = C = 3 a third of all replicates have one by symmetry (both candidates leave the same point, at the same
        # distance).  Counting them as decided puts them INTO the comparison.
        others = [p for p, cd in zip(pots, cands) if cd != cands[best] and p != pots[best]]
        if others:
            gap = min(gap, _rel(pots[best], min(others), min(others)))
        centres.append(cands[best])
        closest = np.minimum(closest, D2[cands[best]])
        pot = pots[best]
    dc = D2[:, centres]                             # C x K
    lab = dc.argmin(axis=1)
    if K > 1:
        srt = np.sort(dc, axis=1)
        sc = mag[:, centres].max(axis=1)
        gap = min(gap, min(_rel(srt[a, 0], srt[a, 1], sc[a]) for a in range(C)))
    it = 0
    while True:
        it += 1
        dist = np.full((C, K), np.inf)
        scale = np.zeros((C, K))
        for c in range(K):
            m = np.flatnonzero(lab == c)
            if m.size == 0:
                continue                            # an empty cluster stays empty
            S = np.cumsum(G[:, m], axis=1)[:, -1]
            Tc = np.cumsum(S[m])[-1]
            cnt = float(m.size)
            dist[:, c] = (d - 2.0 * S / cnt) + Tc / (cnt * cnt)
            scale[:, c] = d + np.abs(2.0 * S / cnt) + abs(Tc / (cnt * cnt))
        new = dist.argmin(axis=1)
        if K > 1:
            order = np.argsort(dist, axis=1, kind="stable")
            for a in range(C):
                b, s = order[a, 0], order[a, 1]
                gap = min(gap, _rel(dist[a, b], dist[a, s], max(scale[a, b], scale[a, s])))
        changed = bool((new != lab).any())
        lab = new
        if not changed or it >= MAXIT:
            break
    return lab.astype(np.int32), it, float(gap)


def solve_all(G, K, seed):
    """every replicate of an R x C x C stack -> (labels R x C, iters R, gaps R)"""
    out = [solve(G[r], K, seed, r) for r in range(len(G))]
    return (np.array([o[0] for o in out], np.int32).reshape(len(G), G.shape[1]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out]))


def decided(gaps):
    """mask of the decided replicates; asserts the 1 % cap of the test cases"""
    ok = np.asarray(gaps) >= DECIDED
    assert (~ok).sum() <= MAX_UNDECIDED * len(ok), "%d of %d replicates undecided by the twin" % ((~ok).sum(), len(ok))
    return ok


def bootstrap_cols(seed, M, replicates):
    """the columns Cluster.bootstrap draws: one RandomState, `replicates` indices per replicate, in stream order"""
    rng = np.random.RandomState(seed)
    return np.array([rng.randint(0, M, size=int(replicates)) for _ in range(int(replicates))], np.int64)


def support(chrs, base_labels, rep_labels):
    """the bootstrap column: percent (truncated) of replicates whose renumbered labels agree with the base assignment"""
    from subphaser_amd.cluster import relabel_by_chromosome_order
    agree = np.zeros(len(chrs), np.int64)
    for raw in rep_labels:
        agree += relabel_by_chromosome_order(chrs, raw) == np.asarray(base_labels)
    return [int(100 * a / len(rep_labels)) for a in agree.tolist()]
