#!/usr/bin/env python3
"""The list filter with passengers by passenger count (dev tool): 21 core chromosomes (7 sets x 3, synthetic bases as
wide_join_bench.py) alone, and next to P passengers (singleton lines: 1-3 kb random scaffolds that carry three copies of
one of 40 shared repeat families, so each keeps k-mers at the lower count 3).  k = 15, count engine 3 (lists) for both.
Prints the wall time of a filter call, its per-kernel ms (prof_report), the list entries and, for the passenger run,
the bytes each new kernel moves by design against its time.
usage: singleton_bench.py [core_mbases_per_chrom=20] [passengers=2000] [reps=5]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from subphaser_amd import _native
from subphaser_amd.config import sets_to_csr

MB = float(sys.argv[1]) if len(sys.argv) > 1 else 20.0
P = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
H, S, K, LOWER, SEED = 7, 3, 15, 3, 11
ARGS = (2.0, 1, 200, 1e9, 1.0)        # the CLI's defaults: -min_fold 2 -baseline 1 -q 200, ratio 1


def passengers(n, seed):
    rng = np.random.RandomState(seed)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    fams = [alpha[rng.randint(0, 4, size=int(rng.randint(100, 300)))] for _ in range(40)]
    out = []
    for _ in range(n):
        s = alpha[rng.randint(0, 4, size=int(rng.randint(1000, 3001)))].copy()
        fam, share = fams[int(rng.randint(0, 40))], s.size // 3
        for j in range(3):
            a = j * share + int(rng.randint(0, share - fam.size + 1))
            s[a:a + fam.size] = fam
        out.append(s)
    return out


def run(ctx, n_pass):
    C = H * S + n_pass
    ln = int(MB * 1e6) // 64 * 64
    labels = ["Chr%d%s" % (h + 1, "ABC"[g]) for h in range(H) for g in range(S)] + ["U%d" % (u + 1) for u in range(n_pass)]
    sgs = [[[labels[h * S + g]] for g in range(S)] for h in range(H)] + [[[lab]] for lab in labels[H * S:]]
    csr = sets_to_csr(sgs, labels)
    ctx.genome_reset(C)
    for i in range(H * S):
        p = ctx.dev_alloc(ln)
        ctx.synth_chrom(p, ln, SEED, i // S, i % S, S, i, 1 if i == 0 else 0)
        ctx.genome_add_device(i, p, ln)
        ctx.dev_free(p)
    pas = passengers(n_pass, SEED)
    for j, s in enumerate(pas):
        ctx.genome_add(H * S + j, s)
    t0 = time.perf_counter()
    ctx.count(K, LOWER, 3)
    t_count = (time.perf_counter() - t0) * 1e3
    sizes = np.array([ctx.dump_size(i) for i in range(C)], np.int64)      # list entries per chromosome
    entries = int(sizes.sum())
    res = ctx.filter(*csr, *ARGS)        # warm-up (buffers)
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        res = ctx.filter(*csr, *ARGS)
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(REPS):
        ctx.filter(*csr, *ARGS)
    ctx.prof_enable(False)
    rep = ctx.prof_report()
    per = {n: round(v["ms"] / REPS, 4) for n, v in rep.items()}        # ms per filter call
    print("C=%d core_bases=%.2fG passenger_bases=%.2fM entries=%d (passengers %d) count_ms=%.1f union/rows/hist=%s "
          "filter_wall_ms median=%.3f min=%.3f kernel_ms=%.3f kernels=%s"
          % (C, H * S * ln / 1e9, sum(s.size for s in pas) / 1e6, entries, int(sizes[H * S:].sum()), t_count, res,
             float(np.median(wall)), min(wall), sum(per.values()), per), flush=True)
    if n_pass:
        # design bytes of the new kernels (k = 15: W = 2^23 words per bitmap; E = entries of all C lists)
        W, E, nc, M = (1 << 29) // 64, entries, res[2], res[1]
        model = {
            "sps_sg_mark": E * 8 + E * 4,                # keys + at most one 4-B atomic per entry
            "sps_sg_sums": W * 8 * 2,                    # U and X read (H read and X written only when min_fold <= 0)
            "sps_sg_dir": W * 8 * 2 + W * 4 + nc * 4,    # X twice, D written, candidate slots written
            "sps_sg_tot": E * 12 + E * 8 + nc * 8,       # keys + counts, X word per entry (D only on a hit), tot atomics
            "sps_sg_rows": nc * 8,
            "sps_sg_place": nc * (8 + 4 + 4) + M * 16,
            "sps_sg_scatter": E * 12 + E * 8 + M * C * 4,
        }
        for n, b in model.items():
            if n in per and per[n] > 0:
                print("  %-15s %8.3f ms  %9.1f MB by design  %7.1f GB/s" % (n, per[n], b / 1e6, b / per[n] / 1e6), flush=True)


ctx = _native.Context(0)
try:
    run(ctx, 0)
    run(ctx, P)
finally:
    ctx.close()
