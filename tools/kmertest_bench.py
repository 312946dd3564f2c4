#!/usr/bin/env python
"""The per-k-mer tests of Cluster.output_kmers (-test_method) on the device against the host path on the same machine.

    python tools/kmertest_bench.py --method ttest_ind|ttest_wide|kruskal|mannwhitneyu|kruskal_wide|mannwhitneyu_wide|wilcoxon
                                   [--shape CxMxG]
                                   [--reps 7] [--host-reps 1] [--no-host] [--host-rows N] [--worst 26x2200000x2] [--json]

A shape is C chromosomes x M k-mers x G groups of C / G chromosomes (the last group takes the remainder; wilcoxon needs
equal groups).  The default is the wheat shape 21x2200000x3 with planted subgenome structure (tests/kpca_ref.py
`planted`: Poisson counts, every k-mer enriched in one group); ttest_wide defaults to the scaffold shape 3000x200000x3
(Poisson counts around 30, every group the top one on some rows), kruskal_wide and mannwhitneyu_wide to 600x200000x3, three
subgenomes of 200 scaffolds, with the same counts.  Printed: staging the rows (M x C x 4 bytes, what the
CLI pays before the k-mer test anyway), the call on staged rows and from host rows (median, minimum and maximum of the
repeats), every kernel alone from sp_prof_report (a run of its own with the profiler on), cluster.numpy_kmer_test on the
fp64 matrix (on the first --host-rows rows if given; skipped with a line when four fp64 copies of those rows exceed the
memory available) and how far the two agree: top / second, NaN positions, the largest
relative p difference, rows whose means differ in the last bits.  --worst (wilcoxon only) adds the worst case of the
permutation branch: counts in 0..2 over equal lengths at 13 pairs, where nearly every row walks all 2^m sign
assignments; its host path runs on the first 200000 rows.  --json ends with one line of the per-call times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kpca_ref as kp  # noqa: E402
from subphaser_amd import _native, cluster  # noqa: E402

# method -> (Context call, its kernels, numpy_kmer_test's method)
METHODS = {
    "ttest_ind": (lambda ctx, *a: ctx.kmer_ttest(*a), ["k7_ttest"], "ttest_ind"),
    "ttest_wide": (lambda ctx, *a: ctx.kmer_ttest_wide(*a), ["k7_ttest_wide_means", "k7_ttest_wide_test"], "ttest_ind"),
    "kruskal": (lambda ctx, *a: ctx.kmer_ranktest(*a, "kruskal"), ["k7_ranktest"], "kruskal"),
    "mannwhitneyu": (lambda ctx, *a: ctx.kmer_ranktest(*a, "mannwhitneyu"), ["k7_ranktest"], "mannwhitneyu"),
    "wilcoxon": (lambda ctx, *a: ctx.kmer_wilcoxon(*a), ["k7_wilcoxon"], "wilcoxon"),
}
for _m in ("kruskal", "mannwhitneyu"):
    METHODS[_m + "_wide"] = (lambda ctx, *a, _m=_m: ctx.kmer_ranktest_wide(*a, _m), ["k7_ttest_wide_means", "k7_ranktest_wide"], _m)
WIDE = ("ttest_wide", "kruskal_wide", "mannwhitneyu_wide")


def mem_available():
    """bytes of host memory available, or None where /proc/meminfo does not say"""
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def timed(f, n):
    ts, out = [], None
    for _ in range(n):
        t0 = time.perf_counter()
        out = f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts, out


def fmt(ts):
    return "%.1f ms (min %.1f, max %.1f, %d calls)" % (float(np.median(ts)), min(ts), max(ts), len(ts))


def case(method, shape, worst=False):
    C, M, G = (int(v) for v in shape.split("x"))
    n = C // G
    sizes = [n] * (G - 1) + [C - n * (G - 1)]
    assert method != "wilcoxon" or n * G == C, "the paired test needs equal groups"
    groups = [list(range(g * n, g * n + sizes[g])) for g in range(G)]
    if worst:
        return np.random.default_rng(13).integers(0, 3, (M, C)).astype(np.uint32), np.full(C, 1 << 21, np.int64), groups
    if method in WIDE:
        rng = np.random.default_rng(2000)
        lengths = rng.integers(10**6, 10**8, C)
        counts = rng.poisson(30, (M, C)).astype(np.uint32)
        for g in range(G):
            counts[g::G, groups[g][0]:groups[g][-1] + 1] += 12
        return counts, lengths, groups
    counts, lengths, _ = kp.planted(2100, C, M, sizes=sizes, shares=tuple(1.0 + g for g in range(G))[::-1])
    return counts, lengths, groups


def run(ctx, name, method, counts, lengths, groups, a, host_rows=None):
    call, kernels, host_method = METHODS[method]
    M, C = counts.shape
    print("%s: %s, C = %d chromosomes in %d groups of %s, M = %d k-mers: rows are %.1f MB"
          % (name, method, C, len(groups), sorted({len(g) for g in groups}), M, counts.nbytes / 1e6), flush=True)
    call(ctx, counts[:2000], lengths, groups)                         # warm-up: code object, workspace
    t_stage, staged = timed(lambda: ctx.stage_rows(counts), a.reps)
    call(ctx, staged, lengths, groups)                                # warm-up at the timed shape
    t_dev, out = timed(lambda: call(ctx, staged, lengths, groups), a.reps)
    t_up, _ = timed(lambda: call(ctx, counts, lengths, groups), max(1, a.reps // 2))
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(a.reps):
        call(ctx, staged, lengths, groups)
    rep = ctx.prof_report()
    ctx.prof_enable(False)
    ctx.release_rows()
    kern = {k: rep[k]["ms"] / max(1, rep[k]["calls"]) for k in kernels if k in rep}
    print("%s: stage_rows %s" % (name, fmt(t_stage)))
    print("%s: on staged rows %s; from host rows %s" % (name, fmt(t_dev), fmt(t_up)))
    for k, ms in kern.items():
        print("%s: %s alone %.3f ms per launch (%d launches), %.1f GB/s of the M x C x 4 bytes"
              % (name, k, ms, rep[k]["calls"], counts.nbytes / ms / 1e6), flush=True)
    top, second, p, means = out[:4]
    print("%s: p is NaN in %d rows, 1 in %d; smallest p %.3e" % (name, int(np.isnan(p).sum()), int((p == 1).sum()),
                                                                float(np.nanmin(p))), flush=True)
    times = {"name": name, "method": method, "staged_ms": t_dev, "host_rows_ms": t_up, "kernel_ms": kern}
    if a.no_host:
        return times
    R = M if host_rows is None else min(M, host_rows)
    avail = mem_available()
    if avail is not None and 4 * R * C * 8 > avail:      # the fp64 matrix, the two groups' copies, their ranks
        print("%s: numpy_kmer_test skipped: four fp64 copies of %d x %d values are %.1f GB, %.1f GB are available"
              % (name, R, C, 4 * R * C * 8 / 1e9, avail / 1e9), flush=True)
        return times
    freqs = counts[:R] / lengths.astype(np.float64)
    t_np, (ht, hs, hp, hm) = timed(lambda: cluster.numpy_kmer_test(freqs, groups, host_method), a.host_reps)
    with np.errstate(all="ignore"):
        both = ~(np.isnan(hp) | np.isnan(p[:R]))
        rel = np.abs(p[:R][both] - hp[both]) / np.where(hp[both] > 0, hp[both], 1.0)
    print("%s: numpy_kmer_test on %d rows %s; same top/second in %d rows; NaN in the same rows: %s; p equal in %d rows; "
          "largest relative p difference %.2e; means differ in the last bits on %d rows"
          % (name, R, fmt(t_np), int(((top[:R] == ht) & (second[:R] == hs)).sum()), bool((np.isnan(hp) == np.isnan(p[:R])).all()),
             int((p[:R][both] == hp[both]).sum()), float(rel.max()) if rel.size else 0.0,
             int((hm != means[:R]).any(axis=1).sum())), flush=True)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", required=True, choices=sorted(METHODS))
    ap.add_argument("--shape", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--worst", default="26x2200000x2", help="wilcoxon: CxMxG of the permutation branch's worst case ('' skips it)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    shape = a.shape or {"ttest_wide": "3000x200000x3", "kruskal_wide": "600x200000x3", "mannwhitneyu_wide": "600x200000x3"}.get(
        a.method, "21x2200000x3")
    ctx = _native.Context(0)
    try:
        times = [run(ctx, "default shape" if not a.shape else a.shape, a.method, *case(a.method, shape), a, a.host_rows)]
        if a.worst and a.method == "wilcoxon":
            times.append(run(ctx, "worst case", a.method, *case(a.method, a.worst, worst=True), a, host_rows=a.host_rows or 200000))
    finally:
        ctx.close()
    if a.json:
        print(json.dumps(times))


if __name__ == "__main__":
    main()
