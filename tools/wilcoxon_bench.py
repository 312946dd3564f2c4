#!/usr/bin/env python
"""The paired k-mer test (Cluster.output_kmers, -test_method wilcoxon) at wheat-like shape: the device call on staged rows
against the host path on the same machine, and a worst case for the permutation branch.

    python tools/wilcoxon_bench.py [--reps 7] [--host-reps 3] [--shape 21x2200000x3] [--no-host]
                                   [--worst 26x2200000x2] [--worst-host-rows 200000]

A shape is C x M x groups (equal groups of C / groups chromosomes).  The first shape gets counts with planted subgenome
structure (tests/kpca_ref.py `planted`: Poisson counts, every k-mer enriched in one group).  Printed: staging the rows
(M x C x 4 bytes, what the CLI pays before the k-mer test anyway), Context.kmer_wilcoxon on staged rows and on host rows
(median, minimum and maximum of the repeats), the kernel alone from sp_prof_report (a run of its own with the profiler on),
cluster.numpy_kmer_test on the M x C fp64 matrix, which branch the rows took, and how far the two p-value vectors lie
apart.  The worst case has counts in 0..2 over equal lengths at 13 pairs: nearly every row has a zero or a tie and walks
all 2^m sign assignments; its host path is timed on the first --worst-host-rows rows only (it is a [rows, 2^13] matrix
product per block) and reported as such."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kpca_ref as kp  # noqa: E402
from subphaser_amd import _native, cluster  # noqa: E402


def timed(f, n):
    ts, out = [], None
    for _ in range(n):
        t0 = time.perf_counter()
        out = f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return "%.1f ms (min %.1f, max %.1f, %d calls)" % (float(np.median(ts)), min(ts), max(ts), n), out


def run(ctx, name, counts, lengths, groups, a, host_rows=None):
    M, C = counts.shape
    print("%s: C = %d chromosomes in %d groups of %d, M = %d k-mers: rows are %.1f MB"
          % (name, C, len(groups), len(groups[0]), M, counts.nbytes / 1e6), flush=True)
    ctx.kmer_wilcoxon(counts[:2000], lengths, groups)                 # warm-up: code object, workspace
    t_stage, staged = timed(lambda: ctx.stage_rows(counts), a.reps)
    print("%s: stage_rows %s" % (name, t_stage), flush=True)
    ctx.kmer_wilcoxon(staged, lengths, groups)                        # warm-up at the timed shape
    t_dev, (top, second, p, means, stat) = timed(lambda: ctx.kmer_wilcoxon(staged, lengths, groups), a.reps)
    t_up, _ = timed(lambda: ctx.kmer_wilcoxon(counts, lengths, groups), max(1, a.reps // 2))
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(a.reps):
        ctx.kmer_wilcoxon(staged, lengths, groups)
    rep = ctx.prof_report()
    ctx.prof_enable(False)
    ctx.release_rows()
    k = rep.get("k7_wilcoxon", {"ms": 0.0, "calls": 0})
    print("%s: sp_kmer_wilcoxon on staged rows %s; from host rows %s; k7_wilcoxon alone %.3f ms per launch (%d launches)"
          % (name, t_dev, t_up, k["ms"] / max(1, k["calls"]), k["calls"]), flush=True)
    print("%s: p is NaN in %d rows, 1 in %d; smallest p %.3e" % (name, int(np.isnan(p).sum()), int((p == 1).sum()),
                                                                float(np.nanmin(p))), flush=True)
    if a.no_host:
        return
    R = M if host_rows is None else min(M, host_rows)
    freqs = counts[:R] / lengths.astype(np.float64)
    t_np, (ht, hs, hp, _) = timed(lambda: cluster.numpy_kmer_test(freqs, groups, "wilcoxon"), a.host_reps)
    with np.errstate(all="ignore"):
        both = ~(np.isnan(hp) | np.isnan(p[:R]))
        rel = np.abs(p[:R][both] - hp[both]) / np.where(hp[both] > 0, hp[both], 1.0)
    print("%s: numpy_kmer_test on %d rows %s; same top/second in %d rows; NaN in the same rows: %s; p equal in %d rows; "
          "largest relative p difference %.2e" % (name, R, t_np, int(((top[:R] == ht) & (second[:R] == hs)).sum()),
                                                  bool((np.isnan(hp) == np.isnan(p[:R])).all()), int((p[:R][both] == hp[both]).sum()),
                                                  float(rel.max()) if rel.size else 0.0), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--shape", default="21x2200000x3")
    ap.add_argument("--worst", default="26x2200000x2")
    ap.add_argument("--worst-host-rows", type=int, default=200000)
    a = ap.parse_args()
    ctx = _native.Context(0)
    try:
        C, M, G = (int(v) for v in a.shape.split("x"))
        n = C // G
        assert n * G == C, "the paired test needs equal groups"
        counts, lengths, _ = kp.planted(2100, C, M, sizes=[n] * G, shares=tuple(1.0 + g for g in range(G))[::-1])
        run(ctx, "wheat shape", counts, lengths, [list(range(g * n, (g + 1) * n)) for g in range(G)], a)
        if a.worst:
            C, M, G = (int(v) for v in a.worst.split("x"))
            n = C // G
            assert n * G == C, "the paired test needs equal groups"
            counts = np.random.default_rng(13).integers(0, 3, (M, C)).astype(np.uint32)
            run(ctx, "worst case", counts, np.full(C, 1 << 21, np.int64), [list(range(g * n, (g + 1) * n)) for g in range(G)], a,
                host_rows=a.worst_host_rows)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
