"""numpy twin of subphaser_amd/csrc/sp_hclust.h: the Euclidean distance matrix summed coordinate by coordinate, left to
right, and the nearest-neighbour chain for complete linkage with the header's tie rules.  Bit for bit what the header's
host driver and the device kernels (sp_hclust.hip) produce; the tests compare with `==`."""
import numpy as np

MAX_POINTS = 16384      # SP_HC_MAXP


def dist(pts):
    """P x P: sqrt(((p_i0 - p_j0)^2 + (p_i1 - p_j1)^2) + ...), every term rounded, the sum left to right from +0"""
    pts = np.ascontiguousarray(pts, np.float64)
    P, D = pts.shape
    s = np.zeros((P, P))
    for c in range(D):
        d = pts[:, c][:, None] - pts[:, c][None, :]
        s += d * d
    return np.sqrt(s)


def chain(dmat):
    """merges (P - 1) x 4 in merge order: (x < y, height, size), raw slot ids.  dmat is not changed."""
    D = np.array(dmat, np.float64)
    P = D.shape[0]
    size = np.ones(P, np.int64)
    live = np.ones(P, bool)
    merges = np.empty((P - 1, 4))
    ch = []
    idx = np.arange(P)
    scans = 0
    for k in range(P - 1):
        if not ch:
            ch.append(int(np.flatnonzero(live)[0]))
        while True:
            x = ch[-1]
            y, cur = (ch[-2], D[x, ch[-2]]) if len(ch) > 1 else (None, np.inf)
            scans += 1
            assert scans <= 4 * P
            cand = live & (idx != x) & (D[x] < cur)
            if cand.any():
                row = np.where(cand, D[x], np.inf)
                y = int(np.argmin(row))              # the first of equal minima: the lowest index
                cur = row[y]
            assert y is not None
            if len(ch) > 1 and y == ch[-2]:
                break
            ch.append(y)
        del ch[-2:]
        if x > y:
            x, y = y, x
        merges[k] = (x, y, cur, size[x] + size[y])
        size[y] += size[x]
        size[x] = 0
        live[x] = False
        upd = live & (idx != y)
        v = np.maximum(D[upd, x], D[upd, y])
        D[upd, y] = v
        D[y, upd] = v
    return merges


def hclust(pts):
    """(merges, dist) of the points: what Context.hclust_complete(points, want_dist=True) returns"""
    d = dist(pts)
    return chain(d), d


def random_points(seed, P, D):
    return np.random.default_rng(seed).normal(size=(P, D)) * 3.0


def tied_points(seed, P, D, levels=3):
    """small-integer coordinates with duplicated points: equal distances, chains that stop on the tie rule, zero heights"""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, levels, size=(P, D)).astype(np.float64)
    if P >= 4:
        src = rng.integers(0, P, size=P // 4)
        dst = rng.integers(0, P, size=P // 4)
        pts[dst] = pts[src]
    return pts


class TwinContext:
    """stands in for the device context in CPU tests: hclust_complete from the twin, calls recorded"""

    def __init__(self):
        self.calls = []

    def hclust_complete(self, points, want_dist=False):
        points = np.ascontiguousarray(points, np.float64)
        self.calls.append(points.shape)
        m, d = hclust(points)
        return (m, d) if want_dist else m
