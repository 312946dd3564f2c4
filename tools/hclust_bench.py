#!/usr/bin/env python
"""Complete-linkage clustering of the heatmap's two axes at the size the CLI uses: Context.hclust_complete against scipy's
pdist + linkage on the same host in the same job.

    python tools/hclust_bench.py [--reps 3] [--no-scipy] [--shapes 10000x21,21x10000]

A shape is P points x D dimensions.  The points are Z-scores (per k-mer over the chromosomes, ddof = 1) of a seeded matrix
with planted subgenome structure (tests/kpca_ref.py `planted`), as Cluster.heatmap forms them: the k-mer axis is
10000 x 21, the chromosome axis its transpose.  Printed per shape: the device entry (upload, both kernels, the merges
back), its kernels alone from sp_prof_report (a run of its own with the profiler on), to_linkage on the host, scipy's pdist
and linkage, and whether the two linkages agree (ids and sizes with `==`, heights by their largest relative difference:
scipy sums its distances in another order)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kpca_ref as kp  # noqa: E402
from subphaser_amd import _native, heatmap as hm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--shapes", default="10000x21,21x10000")
    a = ap.parse_args()

    def med(f, n=a.reps):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    ctx = _native.Context(0)
    try:
        ctx.hclust_complete(np.random.default_rng(0).normal(size=(64, 8)))      # warm-up: code object
        for shape in a.shapes.split(","):
            P, D = (int(v) for v in shape.split("x"))
            N, C = max(P, D), min(P, D)
            counts, lengths, _ = kp.planted(2100, C, N)
            z = hm.zscale_columns(counts / lengths.astype(np.float64))          # C x N
            pts = np.ascontiguousarray(z.T if P >= D else z)
            assert pts.shape == (P, D) and np.isfinite(pts).all()
            print("P = %d points, D = %d dimensions: the matrix is %.1f MB" % (P, D, P * P * 8 / 1e6), flush=True)
            t_first, _ = med(lambda: ctx.hclust_complete(pts), 1)                # grows the workspace
            t_dev, merges = med(lambda: ctx.hclust_complete(pts))
            t_link, Z = med(lambda: hm.to_linkage(merges, P), 1)
            ctx.prof_enable(True)
            ctx.prof_reset()
            ctx.hclust_complete(pts)
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            print("  Context.hclust_complete %.1f ms (first call, with the workspace allocation, %.1f ms); to_linkage %.1f ms"
                  % (1e3 * t_dev, 1e3 * t_first, 1e3 * t_link))
            print("  kernels alone (device events, ms per launch): " + "; ".join(
                "%s %.3f" % (k, v["ms"] / max(1, v["calls"])) for k, v in sorted(rep.items()) if k.startswith("hc_")), flush=True)
            if not a.no_scipy:
                from scipy.cluster.hierarchy import linkage
                from scipy.spatial.distance import pdist
                t_pd, cond = med(lambda: pdist(pts), 1)
                t_lk, ref = med(lambda: linkage(cond, "complete"), 1)
                same = bool((Z[:, [0, 1, 3]] == ref[:, [0, 1, 3]]).all())
                rel = float(np.max(np.abs(Z[:, 2] - ref[:, 2]) / ref[:, 2]))
                print("  scipy pdist %.1f ms + linkage %.1f ms = %.1f ms; same tree as the device: %s; heights within %.2e (relative)"
                      % (1e3 * t_pd, 1e3 * t_lk, 1e3 * (t_pd + t_lk), same, rel), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
