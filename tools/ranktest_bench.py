#!/usr/bin/env python
"""The rank-sum k-mer tests (Cluster.output_kmers, -test_method kruskal / mannwhitneyu) at wheat-like shape: the device
call on staged rows against the host path on the same machine.

    python tools/ranktest_bench.py [--reps 5] [--host-reps 1] [--shape 21x2200000x3] [--no-host]

A shape is C x M x groups (equal groups of C / groups chromosomes).  Counts with planted subgenome structure
(tests/kpca_ref.py `planted`: Poisson counts, every k-mer enriched in one group).  Printed per method: staging the rows
(M x C x 4 bytes, what the CLI pays before the k-mer test anyway), Context.kmer_ranktest on staged rows and on host rows,
the kernel alone from sp_prof_report (a run of its own with the profiler on), cluster.numpy_kmer_test on the M x C fp64
matrix, and how far the two p-value vectors lie apart."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--shape", default="21x2200000x3")
    a = ap.parse_args()

    def med(f, n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = f()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out

    C, M, G = (int(v) for v in a.shape.split("x"))
    n = C // G
    counts, lengths, _ = kp.planted(2100, C, M, sizes=[n] * (G - 1) + [C - n * (G - 1)], shares=tuple(1.0 + g for g in range(G))[::-1])
    groups = [list(range(g * n, (g + 1) * n if g < G - 1 else C)) for g in range(G)]
    print("C = %d chromosomes in %d groups, M = %d k-mers: rows are %.1f MB" % (C, G, M, counts.nbytes / 1e6), flush=True)
    ctx = _native.Context(0)
    try:
        ctx.kmer_ranktest(counts[:2000], lengths, groups, "kruskal")                 # warm-up: code object, workspace
        t_stage, staged = med(lambda: ctx.stage_rows(counts), a.reps)
        print("stage_rows %.1f ms" % (1e3 * t_stage), flush=True)
        freqs = counts / lengths.astype(np.float64)
        for method in _native.RANKTEST_METHODS:
            t_dev, (top, second, p, means, stat) = med(lambda: ctx.kmer_ranktest(staged, lengths, groups, method), a.reps)
            t_up, _ = med(lambda: ctx.kmer_ranktest(counts, lengths, groups, method), max(1, a.reps // 2))
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(a.reps):
                ctx.kmer_ranktest(staged, lengths, groups, method)
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            k = rep.get("k7_ranktest", {"ms": 0.0, "calls": 0})
            print("%-12s sp_kmer_ranktest %.1f ms on staged rows, %.1f ms from host rows; k7_ranktest alone %.3f ms per launch"
                  % (method, 1e3 * t_dev, 1e3 * t_up, k["ms"] / max(1, k["calls"])), flush=True)
            if not a.no_host:
                t_np, (ht, hs, hp, _) = med(lambda: cluster.numpy_kmer_test(freqs, groups, method), a.host_reps)
                with np.errstate(all="ignore"):
                    rel = np.abs(p - hp) / np.where(hp > 0, hp, 1.0)
                print("%-12s numpy_kmer_test %.1f ms; same top/second in %d of %d rows; largest relative p difference %.2e; "
                      "smallest p %.2e" % (method, 1e3 * t_np, int(((top == ht) & (second == hs)).sum()), M, float(rel.max()),
                                           float(hp.min())), flush=True)
        ctx.release_rows()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
