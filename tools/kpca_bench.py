#!/usr/bin/env python
"""The k-mer PCA (Cluster.pca) at wheat-like shape and at one wide shape: the device calls and the host recipe timed apart,
against scikit-learn's PCA(svd_solver="full") on the same matrix.

    python tools/kpca_bench.py [--reps 5] [--no-sklearn] [--shapes 21x2200000x3,512x200000x8]

A shape is C x M x n_components.  Counts with planted subgenome structure (tests/kpca_ref.py `planted`: Poisson counts,
every k-mer enriched in one group of chromosomes).  Printed per shape: staging the rows (M x C x 4 bytes, what the CLI
pays before the k-mer test anyway), Context.kmer_pca_gram and kmer_pca_signs on staged rows and on host rows, their
kernels alone from sp_prof_report (a run of its own with the profiler on), the host part between them (eigh, signs,
normalisation), the numpy path of Cluster.pca (zscores, z z^T, U^T z) and scikit-learn's full solver on the Z-scores; the
largest differences of normalised scores and percentages between the three."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kpca_ref as kp  # noqa: E402
from subphaser_amd import _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--shapes", default="21x2200000x3,512x200000x8")
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
        for shape in a.shapes.split(","):
            C, M, n = (int(v) for v in shape.split("x"))
            K = 3 if C < 100 else 8
            counts, lengths, _ = kp.planted(2100, C, M, shares=tuple(1.0 + g for g in range(K))[::-1], fold=6.0)
            print("C = %d chromosomes, M = %d k-mers, %d components: rows are %.1f MB" % (C, M, n, counts.nbytes / 1e6), flush=True)
            ctx.kmer_pca_gram(counts[:2000], lengths)                               # warm-up: code object, workspace
            t_stage, staged = med(lambda: ctx.stage_rows(counts))
            t_gram, (G, n_bad) = med(lambda: ctx.kmer_pca_gram(staged, lengths))
            w, V = np.linalg.eigh(G)
            U = np.ascontiguousarray(V[:, ::-1][:, :n])
            t_signs, _ = med(lambda: ctx.kmer_pca_signs(staged, lengths, U))
            t_host, (scores, percent, _) = med(lambda: kp.pca(G, lambda U: ctx.kmer_pca_signs(staged, lengths, U)[1], n))
            t_gram_h, _ = med(lambda: ctx.kmer_pca_gram(counts, lengths), max(1, a.reps // 2))
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(a.reps):
                ctx.kmer_pca_gram(staged, lengths)
                ctx.kmer_pca_signs(staged, lengths, U)
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            ctx.release_rows()
            print("  bad rows %d; stage_rows %.1f ms; kmer_pca_gram %.1f ms staged, %.1f ms from host rows; kmer_pca_signs %.1f ms"
                  % (n_bad, 1e3 * t_stage, 1e3 * t_gram, 1e3 * t_gram_h, 1e3 * t_signs))
            print("  host part with its signs call (eigh %d x %d, normalisation) %.1f ms, of which signs %.1f ms" % (
                C, C, 1e3 * t_host, 1e3 * t_signs))
            print("  kernels alone (device events, ms per launch): " + "; ".join(
                "%s %.3f" % (k, v["ms"] / max(1, v["calls"])) for k, v in sorted(rep.items()) if k.startswith("kp_")))

            freqs = counts / lengths.astype(np.float64)

            def numpy_path():
                x = freqs.T
                z = (x - x.mean(axis=0)) / x.std(axis=0)
                Gn = z @ z.T
                return kp.pca(Gn, lambda U: (lambda v: v[np.arange(v.shape[0]), np.argmax(np.abs(v), axis=1)])(U.T @ z), n)
            t_np, (s_np, p_np, _) = med(numpy_path, max(1, a.reps // 2))
            print("  numpy path of Cluster.pca %.1f ms; against the device: scores %.2e, percentages %.2e" % (
                1e3 * t_np, np.abs(s_np - scores).max(), np.abs(p_np - percent).max()))
            if not a.no_sklearn:
                from sklearn.decomposition import PCA

                def sk():
                    x = freqs.T
                    z = (x - x.mean(axis=0)) / x.std(axis=0)
                    p = PCA(n_components=n, svd_solver="full")
                    s = p.fit_transform(z)
                    return (s - s.mean(axis=0)) / s.std(axis=0), p.explained_variance_ratio_ * 100
                t_sk, (s_sk, p_sk) = med(sk, 1)
                print("  scikit-learn PCA(svd_solver='full') with the Z-scores %.1f ms; against the device: scores %.2e, percentages %.2e"
                      % (1e3 * t_sk, np.abs(s_sk - scores).max(), np.abs(p_sk - percent).max()))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
