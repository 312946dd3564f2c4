#!/usr/bin/env python
"""Context.ltr_align on synthetic LTR pairs, on one MI355X.

    python tools/ltralign_bench.py [--pairs 100000] [--band 64] [--min_len 100] [--max_len 7000] [--max_sub 0.15]
                                   [--max_indels 4] [--twin 12] [--seed 1] [--json FILE]

A pair is a random LTR (length uniform in min_len..max_len) and a copy with 0..max_sub substituted bases and up to
max_indels indels of 1..10 bases; the pairs are laid end to end on chromosomes of at most 256 Mbases, uploaded and packed.
Printed: the wall time of the whole call (checks, sort, upload, kernel, download), the la_align kernel from device events
(a second call), cells per second, the flags and the mean divergence; then the numpy twin (tests/ltralign_ref.py) on a
sample of the same pairs on this machine's CPU -- its answers must be the kernel's -- and the ratio of the two times per
pair.  That ratio compares one Python process with one GPU on one definition; it is not the speed-up of a run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from subphaser_amd import _native  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
CHROM_MAX = 256 << 20


def make_pairs(a):
    rng = np.random.default_rng(a.seed)
    chroms, cur, cur_len = [], [], 0
    rows = []          # chrom, a_start, a_len, b_start, b_len
    for _ in range(a.pairs):
        la = int(rng.integers(a.min_len, a.max_len + 1))
        x = rng.integers(0, 4, la, dtype=np.uint8)
        y = x.copy()
        hit = np.flatnonzero(rng.random(la) < rng.uniform(0, a.max_sub))
        y[hit] = (y[hit] + rng.integers(1, 4, hit.size, dtype=np.uint8)) & 3
        for _ in range(int(rng.integers(0, a.max_indels + 1))):
            p, n = int(rng.integers(1, max(2, y.size - 10))), int(rng.integers(1, 11))
            y = np.delete(y, slice(p, p + n)) if rng.random() < 0.5 and y.size > 4 * n else np.insert(y, p, rng.integers(0, 4, n, dtype=np.uint8))
        if cur_len + x.size + y.size > CHROM_MAX:
            chroms.append(np.concatenate(cur))
            cur, cur_len = [], 0
        rows.append((len(chroms), cur_len, x.size, cur_len + x.size, y.size))
        cur += [x, y]
        cur_len += x.size + y.size
    chroms.append(np.concatenate(cur))
    return [ACGT[c] for c in chroms], [np.asarray(col, np.int64) for col in zip(*rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--band", type=int, default=64)
    ap.add_argument("--min_len", type=int, default=100)
    ap.add_argument("--max_len", type=int, default=7000)
    ap.add_argument("--max_sub", type=float, default=0.15)
    ap.add_argument("--max_indels", type=int, default=4)
    ap.add_argument("--twin", type=int, default=12, help="pairs the numpy twin is timed on (0: none)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    chroms, cols = make_pairs(a)
    bases = int(sum(c.size for c in chroms))
    print("%d pairs, %.3f Gbases on %d chromosomes, generated in %.1f s" % (a.pairs, bases / 1e9, len(chroms), time.perf_counter() - t0), flush=True)
    la, lb = cols[2], cols[4]
    width = np.abs(lb - la) + 2 * a.band + 1
    cells = int((np.minimum(la, lb) * width).sum())          # band cells, to first order
    res = dict(pairs=a.pairs, band=a.band, bases=bases, band_cells=cells, params={k: getattr(a, k) for k in ("min_len", "max_len", "max_sub", "max_indels", "seed")})
    ctx = _native.Context(0)
    try:
        t0 = time.perf_counter()
        ctx.genome_reset(len(chroms))
        for i, c in enumerate(chroms):
            ctx.genome_add(i, c)
        ctx.sync()
        print("uploaded and packed in %.1f s" % (time.perf_counter() - t0), flush=True)
        ctx.ltr_align(*[c[:64] for c in cols], a.band)       # warm: code object
        t0 = time.perf_counter()
        out = ctx.ltr_align(*cols, a.band)
        res["call_s"] = time.perf_counter() - t0
        ctx.prof_enable(True)
        ctx.prof_reset()
        out2 = ctx.ltr_align(*cols, a.band)
        rep = ctx.prof_report()
        ctx.prof_enable(False)
        assert (out == out2).all()
        res["kernel_s"] = rep["la_align"]["ms"] / 1e3
        flags = out[:, 5]
        ok = (flags & 6) == 0
        div = out[ok, 2] / np.maximum(1, out[ok, 1] + out[ok, 2])
        res.update(edge=int((flags & 1 != 0).sum()), band_too_wide=int((flags & 2 != 0).sum()), too_long=int((flags & 4 != 0).sum()),
                   mean_div=float(div.mean()), cells_per_s=cells / res["kernel_s"])
        print("whole call %.3f s; la_align kernel %.3f s (%.1f us per pair, %.2f Gcells/s); edge %d, band too wide %d, too long %d; mean div %.4f" % (
            res["call_s"], res["kernel_s"], 1e6 * res["kernel_s"] / a.pairs, res["cells_per_s"] / 1e9, res["edge"], res["band_too_wide"], res["too_long"],
            res["mean_div"]), flush=True)
        if a.twin:
            import ltralign_ref as lr
            pick = np.random.default_rng(a.seed + 1).choice(a.pairs, size=min(a.twin, a.pairs), replace=False)
            codes = {}
            t0 = time.perf_counter()
            for i in pick.tolist():
                c = int(cols[0][i])
                if c not in codes:
                    codes[c] = lr.encode(bytes(chroms[c]))
                want = lr.align(codes[c][cols[1][i]:cols[1][i] + la[i]], codes[c][cols[3][i]:cols[3][i] + lb[i]], a.band)
                assert tuple(out[i].tolist()) == want, (i, out[i].tolist(), want)
            twin_s = (time.perf_counter() - t0) / pick.size
            sample_share = float((la[pick] + lb[pick]).sum() / (la + lb).sum())       # the twin's time goes with la + lb
            res.update(twin_pairs=int(pick.size), twin_s_per_pair=twin_s, twin_equal=True,
                       ratio=twin_s * pick.size / (res["kernel_s"] * sample_share))
            print("twin: %d pairs, all equal to the kernel's, %.2f s per pair; ratio of the times for the same pairs (kernel time by share of la + lb): %.0f" % (
                pick.size, twin_s, res["ratio"]), flush=True)
    finally:
        ctx.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
