#!/usr/bin/env python
"""The k-means bootstrap at wheat-like shape: the loop of scikit-learn fits (Cluster.bootstrap, engine sklearn) against one
Context.kmeans_bootstrap call on the same resampled columns.

    python tools/kboot_bench.py [--chroms 21] [--clusters 3] [--replicates 1000] [--kmers 2200000] [--reps 5] [--no-sklearn]

C x M random Z-scores with a subgenome signal (every column Z-normalised as Cluster.zscores does), R replicates of R
columns drawn like Cluster.bootstrap draws them.  Printed separately: the upload of z (C x M x 8 bytes, a device
allocation and one copy), the call with z already on the device (kernel + the copies of columns, labels and iteration
counts), the kernel alone from sp_prof_report (device events, a run of its own with the profiler on), the call with z on
the host (what Cluster.bootstrap pays: upload + kernel + release) and the host's renumbering of the R label vectors.
The two support columns are printed side by side; they are samples of one distribution, not equal."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from subphaser_amd import _native  # noqa: E402
from subphaser_amd.cluster import relabel_by_chromosome_order  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chroms", type=int, default=21)
    ap.add_argument("--clusters", type=int, default=3)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--kmers", type=int, default=2200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    C, K, R, M = a.chroms, a.clusters, a.replicates, a.kmers
    rng = np.random.default_rng(2100)
    x = rng.standard_normal((K, M))[np.arange(C) % K] + 1.5 * rng.standard_normal((C, M))
    z = np.ascontiguousarray((x - x.mean(axis=0)) / x.std(axis=0))
    del x
    chrs = ["chr%02d" % i for i in range(C)]
    base = relabel_by_chromosome_order(chrs, np.arange(C) % K)
    rs = np.random.RandomState(1)
    cols = np.array([rs.randint(0, M, size=R) for _ in range(R)], np.int64)
    print("C = %d chromosomes, K = %d, R = n = %d, M = %d k-mers: z is %.1f MB" % (C, K, R, M, z.nbytes / 1e6), flush=True)

    def med(f, n=a.reps):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts, out

    ctx = _native.Context(0)
    try:
        ctx.kmeans_bootstrap(z[:, :1000], cols % 1000, K, 1)           # warm-up: code object, workspace
        t_host, ts_host, (labels, iters) = med(lambda: ctx.kmeans_bootstrap(z, cols, K, 1))

        def upload():
            p = ctx.dev_alloc(z.nbytes)
            ctx.host_to_dev(p, z)
            return p
        ptrs = []
        t_up, ts_up, _ = med(lambda: ptrs.append(upload()))
        for p in ptrs[1:]:
            ctx.dev_free(p)
        staged = (ptrs[0], C, M)
        t_dev, ts_dev, got = med(lambda: ctx.kmeans_bootstrap(staged, cols, K, 1))
        assert got[0].tobytes() == labels.tobytes()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            ctx.kmeans_bootstrap(staged, cols, K, 1)
        rep = ctx.prof_report()["kb_bootstrap"]
        ctx.prof_enable(False)
        ctx.dev_free(ptrs[0])
    finally:
        ctx.close()
    t_rel, _, reps = med(lambda: np.array([relabel_by_chromosome_order(chrs, r) for r in labels]))
    fmt = lambda ts: " ".join("%.1f" % (1e3 * t) for t in ts)
    print("device engine, median of %d:" % a.reps)
    print("  upload of z (alloc + copy)        %8.1f ms  (%s): %.1f GB/s" % (1e3 * t_up, fmt(ts_up), z.nbytes / t_up / 1e9))
    print("  call, z on the device             %8.1f ms  (%s)" % (1e3 * t_dev, fmt(ts_dev)))
    print("  kernel kb_bootstrap alone         %8.3f ms per call (%d calls, device events)" % (rep["ms"] / rep["calls"], rep["calls"]))
    print("  call, z on the host               %8.1f ms  (%s)" % (1e3 * t_host, fmt(ts_host)))
    print("  host renumbering of %d vectors  %8.1f ms" % (R, 1e3 * t_rel))
    print("  Lloyd iterations per replicate: min %d, median %d, max %d" % (iters.min(), int(np.median(iters)), iters.max()))
    dev_bs = [int(100 * v / R) for v in (reps == base[None, :]).sum(axis=0)]
    print("  support", dev_bs)
    if a.no_sklearn:
        return
    from sklearn.cluster import KMeans
    t0 = time.perf_counter()
    sk = np.array([relabel_by_chromosome_order(chrs, KMeans(n_clusters=K, random_state=1).fit(z[:, cols[r]]).labels_)
                   for r in range(R)])
    t_sk = time.perf_counter() - t0
    print("scikit-learn loop (%d fits, gather and renumbering included): %.1f ms" % (R, 1e3 * t_sk))
    print("  support", [int(100 * v / R) for v in (sk == base[None, :]).sum(axis=0)])
    print("  device engine end to end (call with z on the host + renumbering) is %.1fx shorter" % (t_sk / (t_host + t_rel)))


if __name__ == "__main__":
    main()
