#!/usr/bin/env python
"""The LTR tree (Context.ltr_sketch, ltr_sketch_pairs, nj_tree; subphaser_amd/ltrtree.py) on planted families, on one MI355X.

    python tools/ltrtree_bench.py [--n 1000 4096] [--length 6000] [--families 40] [--div 0.08] [--k 13] [--s 1024]
                                  [--repeat 3] [--loop_max 1000] [--sweep 32 64 128 256 512 1000] [--seed 1] [--json FILE]

The genome is one synthetic chromosome per 256 elements: every element is its family's random ancestor of `length` bases
with `div` substitutions per base, every second one reverse-complemented, 200 random bases between two elements.  Printed
per N: the wall time of the three entries (the median of `repeat` calls after a warm one; nj_tree under either driver, above 2000 slots one cold call of the launches' driver alone --
the looping workgroup only up to --loop_max slots, because its time grows with N^3 on one compute unit), the time of the
host steps between and behind them (distance units, rooting, newick), their sum, one pass of the stage's tree step as
Pipeline._ltr_tree runs it (ltrtree.build and the newick text, timed as one piece: stage_pass_s), and how
many families are one clade of the tree.  --sweep times both neighbour-joining drivers on the first N elements' matrix for
the crossover.

There is nothing to compare with: no iqtree, FastTree or mafft is run here, and the families are synthetic."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from subphaser_amd import _native, ltrtree  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_genome(a, n):
    rng = np.random.default_rng(a.seed)
    anc = [rng.integers(0, 4, a.length, dtype=np.uint8) for _ in range(a.families)]
    chroms, el, fams = [], [], []
    for c0 in range(0, n, 256):
        parts, at = [], 0
        for e in range(c0, min(n, c0 + 256)):
            gap = rng.integers(0, 4, 200, dtype=np.uint8)
            x = anc[e % a.families].copy()
            hit = np.flatnonzero(rng.random(x.size) < a.div)
            x[hit] = (x[hit] + rng.integers(1, 4, hit.size, dtype=np.uint8)) & 3
            if e & 1:
                x = 3 - x[::-1]
            parts += [gap, x]
            el.append((len(chroms), at + 200, at + 200 + x.size))
            fams.append(e % a.families)
            at += 200 + x.size
        chroms.append(ACGT[np.concatenate(parts + [rng.integers(0, 4, 200, dtype=np.uint8)])])
    return chroms, el, fams


def timed(fn, repeat):
    """median of `repeat` calls after a warm one; repeat = 0: the one cold call"""
    if repeat == 0:
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def clades(records, fams):
    sp = ltrtree.splits(ltrtree.unrooted_edges(records), len(fams))
    everyone, ok = set(range(len(fams))), 0
    for f in set(fams):
        side = frozenset(i for i, x in enumerate(fams) if x == f)
        ok += side in sp or frozenset(everyone - side) in sp
    return ok, len(set(fams))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--length", type=int, default=6000)
    ap.add_argument("--families", type=int, default=40)
    ap.add_argument("--div", type=float, default=0.08)
    ap.add_argument("--k", type=int, default=ltrtree.TREE_K)
    ap.add_argument("--s", type=int, default=ltrtree.TREE_SKETCH)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--loop_max", type=int, default=1000)
    ap.add_argument("--sweep", type=int, nargs="*", default=[32, 64, 128, 256, 512, 1000])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _native.Context(0)
    res = {"args": vars(a), "sizes": [], "sweep": []}
    for n in a.n:
        chroms, el, fams = make_genome(a, n)
        ctx.genome_reset(len(chroms))
        for i, c in enumerate(chroms):
            ctx.genome_add(i, c)
        chrom, start, end = (np.array(x) for x in zip(*el))
        t_sk, (sk, ln) = timed(lambda: ctx.ltr_sketch(chrom, start, end, a.k, a.s), a.repeat)
        t_pr, (sh, dn) = timed(lambda: ctx.ltr_sketch_pairs(sk, ln), a.repeat)
        t0 = time.perf_counter()
        D = ltrtree.distance_matrix(sh, dn, a.k, a.s)
        t_units = time.perf_counter() - t0
        row = {"n": n, "bases": int((end - start).sum()), "sketch_s": t_sk, "pairs_s": t_pr, "units_s": t_units}
        rec = None
        for mode, name in ((2, "nj_launches_s"), (1, "nj_loop_s")):
            if mode == 1 and n > a.loop_max:
                row[name] = None
                continue
            ctx.nj_set_mode(mode)
            row[name], rec = timed(lambda: ctx.nj_tree(D), 0 if n > 2000 else a.repeat)
        ctx.nj_set_mode(0)
        if n > 2000:      # one cold call is all a size this slow gets: the default driver is the launches' here
            row["nj_default_s"] = row["nj_launches_s"]
        else:
            row["nj_default_s"], rec = timed(lambda: ctx.nj_tree(D), a.repeat)
        t0 = time.perf_counter()
        text = ltrtree.tree_text(rec, ["e%d" % i for i in range(n)])
        row["newick_s"] = time.perf_counter() - t0
        row["tree_step_s"] = t_sk + t_pr + t_units + row["nj_default_s"] + row["newick_s"]
        # the stage's tree step as the stage runs it, in one pass: ltrtree.build (the three entries and the distance units) and
        # the newick text
        t0 = time.perf_counter()
        rec2, _ = ltrtree.build(ctx, chrom, start, end, a.k, a.s)
        ltrtree.tree_text(rec2, ["e%d" % i for i in range(n)])
        row["stage_pass_s"] = time.perf_counter() - t0
        row["family_clades"] = "%d of %d" % clades(rec, fams)
        row["newick_bytes"] = len(text)
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        if n == a.n[0]:
            for m in a.sweep:
                if m > n:
                    continue
                sub = np.ascontiguousarray(D[:m, :m])
                out = {"n": m}
                for mode, name in ((1, "loop_s"), (2, "launches_s")):
                    ctx.nj_set_mode(mode)
                    out[name], _ = timed(lambda: ctx.nj_tree(sub), a.repeat)
                ctx.nj_set_mode(0)
                res["sweep"].append(out)
                print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
