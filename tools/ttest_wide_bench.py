#!/usr/bin/env python
"""The k-mer t-test at scaffold scale: cluster.numpy_kmer_test (what Cluster.output_kmers ran for subgenomes of more than
64 chromosomes) against Context.kmer_ttest_wide on the same synthetic matrix, rows staged on the device as the CLI does.

    python tools/ttest_wide_bench.py [--rows 200000] [--chroms 3000] [--groups 3] [--reps 5] [--no-numpy]

Prints the numpy time, the wall time of a kmer_ttest_wide call (median of --reps after one warm-up; it includes the copies
of the results to the host), the two kernels' times from sp_prof_report (device events, a run of their own with the
profiler on) and the bytes by design -- M x C x 4, read once by each pass -- over those times.  It also says how far
apart the two p-value columns are and on how many rows the `ratios` columns (the means) differ in the last bits."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from subphaser_amd import _native, cluster  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--chroms", type=int, default=3000)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    M, C, G = a.rows, a.chroms, a.groups
    rng = np.random.default_rng(2000)
    lengths = rng.integers(10**6, 10**8, C)
    counts = rng.poisson(30, (M, C)).astype(np.uint32)
    per = C // G
    groups = [list(range(g * per, (g + 1) * per if g < G - 1 else C)) for g in range(G)]
    for g in range(G):                                   # every group is the top one on some rows
        counts[g::G, groups[g][0]:groups[g][-1] + 1] += 12
    print("M = %d rows, C = %d chromosomes, %d groups of %s, matrix %.2f GB (uint32)" % (
        M, C, G, sorted(set(len(g) for g in groups)), counts.nbytes / 1e9), flush=True)

    ctx = _native.Context(0)
    try:
        staged = ctx.stage_rows(counts)
        out = ctx.kmer_ttest_wide(staged, lengths, groups)           # warm-up: code objects, the workspace
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = ctx.kmer_ttest_wide(staged, lengths, groups)
            wall.append(time.perf_counter() - t0)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.reps):
            ctx.kmer_ttest_wide(staged, lengths, groups)
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        ctx.release_rows()
    finally:
        ctx.close()
    top, second, pv, means = out
    print("kmer_ttest_wide, rows staged: wall %.1f ms median of %d (%s)" % (
        1e3 * float(np.median(wall)), a.reps, " ".join("%.1f" % (1e3 * w) for w in wall)))
    tot = 0.0
    for name in ("k7_ttest_wide_means", "k7_ttest_wide_test"):
        ms = rep[name]["ms"] / rep[name]["calls"]
        tot += ms
        print("  %-20s %8.3f ms per call (%d calls): %7.1f GB/s of the M x C x 4 bytes it reads by design" % (
            name, ms, rep[name]["calls"], counts.nbytes / ms / 1e6))
    print("  both passes          %8.3f ms: %7.1f GB/s over 2 x M x C x 4 = %.2f GB" % (
        tot, 2 * counts.nbytes / tot / 1e6, 2 * counts.nbytes / 1e9))
    if a.no_numpy:
        return
    t0 = time.perf_counter()
    X = counts / lengths.astype(np.float64)
    t_x = time.perf_counter() - t0
    t0 = time.perf_counter()
    ntop, nsecond, npv, nmeans = cluster.numpy_kmer_test(X, groups)
    t_np = time.perf_counter() - t0
    print("numpy (cluster.numpy_kmer_test): %.1f s (+ %.1f s for the fp64 matrix it reads, %.2f GB)" % (t_np, t_x, X.nbytes / 1e9))
    print("  kernel wall time is %.0fx shorter" % (t_np / float(np.median(wall))))
    same = (ntop == top) & (nsecond == second)
    both = same & np.isfinite(npv) & np.isfinite(pv) & (npv > 1e-290)
    rel = np.abs(pv[both] - npv[both]) / npv[both]
    print("  top / second equal on %d of %d rows; p-values: largest relative difference %.2e on those; "
          "`ratios` differ in the last bits on %d of %d rows" % (
              int(same.sum()), M, float(rel.max()) if rel.size else 0.0, int((nmeans != means).any(axis=1).sum()), M))


if __name__ == "__main__":
    main()
