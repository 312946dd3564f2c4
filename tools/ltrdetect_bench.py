#!/usr/bin/env python
"""The de novo LTR detection (Context.ltr_seeds / ltr_hsps, ltr.chain_hsps, Context.ltr_align) on a planted synthetic
genome, on one MI355X.

    python tools/ltrdetect_bench.py [--bases 100000000] [--chroms 4] [--spacing 14000] [--repeat 7] [--seed 1] [--json FILE]

The genome is random bases on `chroms` chromosomes, loaded through genome_add, with one LTR-RT-like element every
`spacing` bases: LTRs of 120 to 1500 bases, the right one a copy of the left with 0 to 12 % substitutions and 0 to 3
indels of 1 to 9 bases, 1000 to 8000 bases between them.  Printed: the wall time of the device detection of all chromosomes
(every one of `repeat` passes after a warm one; Gbases/s from their median), its split by kernel from sp_prof_report (one
more pass; ld_sort_words, ld_sort_hsps and ld_unique are the library's kernels between two events), seeds and HSPs per Mb, the time of the host chaining, the alignment of the
candidates, and how many planted elements have a kept candidate that covers at least half of each of their LTRs.

There is nothing to compare with: no real genome and neither ltrharvest nor ltr_finder is run here; a random background
has no repeats of its own, so seeds per Mb are those of the planted elements alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from subphaser_amd import _native, ltr  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_genome(a):
    rng = np.random.default_rng(a.seed)
    per = a.bases // a.chroms
    chroms, truth = [], []
    for _ in range(a.chroms):
        s = rng.integers(0, 4, per, dtype=np.uint8)
        els = []
        for slot in range(per // a.spacing):
            left = rng.integers(0, 4, int(rng.integers(120, 1501)), dtype=np.uint8)
            right = left.copy()
            hit = np.flatnonzero(rng.random(left.size) < rng.uniform(0, 0.12))
            right[hit] = (right[hit] + rng.integers(1, 4, hit.size, dtype=np.uint8)) & 3
            for _ in range(int(rng.integers(0, 4))):
                p, n = int(rng.integers(10, right.size - 10)), int(rng.integers(1, 10))
                right = np.delete(right, slice(p, p + n)) if rng.random() < 0.5 else np.insert(right, p, rng.integers(0, 4, n, dtype=np.uint8))
            inner = int(rng.integers(1000, 8001))
            a0 = slot * a.spacing + int(rng.integers(50, a.spacing - left.size - inner - right.size - 50))
            b0 = a0 + left.size + inner
            s[a0:a0 + left.size] = left
            s[b0:b0 + right.size] = right
            els.append((a0, a0 + left.size, b0, b0 + right.size))
        chroms.append(ACGT[s])
        truth.append(els)
    return chroms, truth


def detect(ctx, n_chrom):
    out, n_seeds = [], 0
    for i in range(n_chrom):
        ns, nh = ctx.ltr_seeds(i, ltr.LTR_SEED, ltr.LTR_XDROP, ltr.LTR_MINDIST, ltr.LTR_MAXDIST, ltr.LTR_MAXLEN)
        out.append(ctx.ltr_hsps(nh))
        n_seeds += ns
    return out, n_seeds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--chroms", type=int, default=4)
    ap.add_argument("--spacing", type=int, default=14000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.repeat >= 1 and a.spacing >= 12000, "an element may span 11 100 bases"
    t0 = time.perf_counter()
    chroms, truth = make_genome(a)
    bases = int(sum(c.size for c in chroms))
    n_el = sum(map(len, truth))
    print("%.3f Gbases on %d chromosomes, %d planted elements, generated in %.1f s" % (bases / 1e9, len(chroms), n_el, time.perf_counter() - t0), flush=True)
    res = dict(bases=bases, chroms=len(chroms), elements=n_el, params={k: getattr(a, k) for k in ("spacing", "seed")})
    ctx = _native.Context(0)
    try:
        t0 = time.perf_counter()
        ctx.genome_reset(len(chroms))
        for i, c in enumerate(chroms):
            ctx.genome_add(i, c)
        ctx.sync()
        print("uploaded and packed in %.1f s" % (time.perf_counter() - t0), flush=True)
        detect(ctx, 1)                                    # warm: code objects, the sort's first call
        passes = []
        for _ in range(a.repeat):                         # (a pass ends in a device synchronise and the copy of the HSPs)
            t0 = time.perf_counter()
            hsps, n_seeds = detect(ctx, len(chroms))
            passes.append(time.perf_counter() - t0)
        res["detect_passes_s"] = [round(t, 6) for t in passes]
        res["detect_s"] = float(np.median(passes))
        ctx.prof_enable(True)
        ctx.prof_reset()
        hsps2, _ = detect(ctx, len(chroms))
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        assert all((x == y).all() for h, h2 in zip(hsps, hsps2) for x, y in zip(h, h2))
        res["kernels_ms"] = {k: round(v["ms"], 3) for k, v in sorted(rep.items()) if k.startswith("ld_")}
        n_hsps = sum(len(h[0]) for h in hsps)
        res.update(seeds=n_seeds, hsps=n_hsps, gbases_per_s=bases / res["detect_s"] / 1e9, seeds_per_mb=n_seeds / (bases / 1e6),
                   hsps_per_mb=n_hsps / (bases / 1e6))
        print("detection, %d passes: %s ms; median %.1f ms = %.2f Gbases/s; %d seeds (%.1f per Mb), %d HSPs (%.1f per Mb)" % (
            a.repeat, " ".join("%.1f" % (1e3 * t) for t in passes), 1e3 * res["detect_s"], res["gbases_per_s"], n_seeds, res["seeds_per_mb"], n_hsps,
            res["hsps_per_mb"]), flush=True)
        print("kernels, ms (second pass, device events): %s; sum %.1f ms" % (res["kernels_ms"], sum(res["kernels_ms"].values())), flush=True)
        t0 = time.perf_counter()
        cands = []
        for ci, (p0, n, d) in enumerate(hsps):
            cands += [(ci,) + c for c in ltr.candidates(ltr.chain_hsps(zip(p0.tolist(), n.tolist(), d.tolist())))]
        res.update(chain_s=time.perf_counter() - t0, candidates=len(cands))
        t0 = time.perf_counter()
        ci, a0, a1, b0, b1 = (np.array(x, np.int64) for x in zip(*cands))
        counts = ctx.ltr_align(ci.astype(np.int32), a0, a1 - a0, b0, b1 - b0, ltr.LTR_BAND)
        sims, keep, dropped = ltr.similarity(counts, ltr.LTR_SIMILAR)
        res.update(align_s=time.perf_counter() - t0, kept=len(keep), dropped=dropped)
        print("host chaining %.3f s: %d candidates; alignment %.3f s: %d kept at >= %s %%, %d outside its limits" % (
            res["chain_s"], len(cands), res["align_s"], len(keep), ltr.LTR_SIMILAR, dropped), flush=True)
        by_chrom = {}
        for i in keep:
            by_chrom.setdefault(cands[i][0], []).append(cands[i][1:])
        found, errs = 0, []
        for c, els in enumerate(truth):
            got = sorted(by_chrom.get(c, []))
            starts = np.array([g[0] for g in got] or [0])
            for e0, e1, f0, f1 in els:
                best = None
                for g in got[max(0, int(np.searchsorted(starts, e0 - 2000))):int(np.searchsorted(starts, e1))]:
                    cov = min(max(0, min(e1, g[1]) - max(e0, g[0])) / (e1 - e0), max(0, min(f1, g[3]) - max(f0, g[2])) / (f1 - f0))
                    if best is None or cov > best[0]:
                        best = (cov, max(abs(g[0] - e0), abs(g[1] - e1), abs(g[2] - f0), abs(g[3] - f1)))
                if best and best[0] >= 0.5:
                    found += 1
                    errs.append(best[1])
        errs.sort()
        res.update(found=found, boundary_err_median=errs[len(errs) // 2] if errs else None, boundary_err_p90=errs[len(errs) * 9 // 10] if errs else None)
        print("%d of %d planted elements have a kept candidate over at least half of each LTR; boundary error median %s, 90 %% %s" % (
            found, n_el, res["boundary_err_median"], res["boundary_err_p90"]), flush=True)
    finally:
        ctx.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
