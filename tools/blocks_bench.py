#!/usr/bin/env python
"""Homoeologous blocks on the synthetic genomes of bench.py, on one MI355X.

    python tools/blocks_bench.py [--config wheat|peanut|ara|small|tiny] [--scale 1.0] [--block_k 21] [--block_sample 4]
                                 [--block_bin 50000] [--block_votes 5] [--block_gap 5] [--min_block 100000] [--json FILE]

The chromosomes are generated in HBM (sp_synth_chrom: homoeologous copies of one backbone with 8 % substitutions, so the
whole of every homoeologous pair is collinear by construction) and packed; nothing is counted.  Printed: the index build
per chromosome (wall, and its kernels from the device events of a second build), the pair call per pair (wall and the
bk_pair kernel), anchors and spilled windows per pair, the share of every A chromosome that the blocks cover at the given
parameters, and the wall time of blocks.run over the whole pair list, indexes included."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from subphaser_amd import _native, blocks as bl  # noqa: E402
from subphaser_amd.synth import SynthGenome  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="wheat")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--block_k", type=int, default=bl.BLOCK_K)
    ap.add_argument("--block_sample", type=int, default=bl.BLOCK_SAMPLE)
    ap.add_argument("--block_bin", type=int, default=bl.BLOCK_BIN)
    ap.add_argument("--block_votes", type=int, default=bl.BLOCK_VOTES)
    ap.add_argument("--block_gap", type=int, default=bl.BLOCK_GAP)
    ap.add_argument("--min_block", type=int, default=bl.MIN_BLOCK)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    gen = SynthGenome(a.config, a.scale)
    ctx = _native.Context(0)
    res = dict(config=a.config, scale=a.scale, params={k: getattr(a, k) for k in ("block_k", "block_sample", "block_bin", "block_votes", "block_gap", "min_block")},
               chromosomes=len(gen.chroms), bases=gen.total_bases, index=[], pairs=[])
    try:
        t0 = time.perf_counter()
        ctx.genome_reset(len(gen.chroms))
        for i, c in enumerate(gen.chroms):
            p = ctx.dev_alloc(max(c["length"], 1))
            ctx.synth_chrom(p, c["length"], gen.seed, c["set_id"], c["sg_id"], gen.S, c["chrom_id"], c["exchange"])
            ctx.genome_add_device(i, p, c["length"])
            ctx.sync()
            ctx.dev_free(p)
        print("%s-like genome: %d chromosomes, %.3f Gbases, generated and packed in %.1f s" % (
            a.config, len(gen.chroms), gen.total_bases / 1e9, time.perf_counter() - t0), flush=True)
        lengths = [c["length"] for c in gen.chroms]
        where = {lab: i for i, lab in enumerate(gen.labels)}
        groups = bl.pair_list(gen.sgs)
        kb, s, bin_size = a.block_k, a.block_sample, a.block_bin

        # ---- per chromosome and per pair, one config line at a time (the indexes of a line are released after it)
        for group in groups:
            chroms = sorted({where[c] for pair in group for c in pair})
            for i in chroms:
                t0 = time.perf_counter()
                n_sampled, n_single = ctx.blocks_index(i, kb, s)
                wall = time.perf_counter() - t0
                ctx.blocks_release(i)
                ctx.prof_enable(True)
                ctx.prof_reset()
                ctx.blocks_index(i, kb, s)
                rep = ctx.prof_report()
                ctx.prof_enable(False)
                ent = dict(chrom=gen.labels[i], length=lengths[i], n_sampled=n_sampled, n_single=n_single, wall_ms=1e3 * wall,
                           kernels_ms={k: v["ms"] for k, v in rep.items() if k.startswith("bk_")})
                res["index"].append(ent)
                print("index %-8s %11d bases: %9d sampled, %9d single-copy; %.1f ms wall; kernels %s" % (
                    ent["chrom"], ent["length"], n_sampled, n_single, ent["wall_ms"],
                    ", ".join("%s %.2f ms" % kv for kv in sorted(ent["kernels_ms"].items()))), flush=True)
            for c1, c2 in group:
                ia, ib = where[c1], where[c2]
                ctx.blocks_pair(ia, ib, kb, s, bin_size)      # warm: output buffers
                t0 = time.perf_counter()
                win_b, opp, votes, total, n_anch, n_spill = ctx.blocks_pair(ia, ib, kb, s, bin_size, want_spilled=True)
                wall = time.perf_counter() - t0
                ctx.prof_enable(True)
                ctx.prof_reset()
                ctx.blocks_pair(ia, ib, kb, s, bin_size)
                rep = ctx.prof_report()
                ctx.prof_enable(False)
                blocks = bl.walk(win_b, opp, votes, lengths[ia], lengths[ib], bin_size, a.block_votes, a.block_gap, a.min_block)
                cov = sum(b[1] - b[0] for b in blocks)
                ent = dict(a=c1, b=c2, anchors=n_anch, spilled_windows=n_spill, called=int((votes >= a.block_votes).sum()), windows=len(votes),
                           blocks=len(blocks), inverted=sum(b[4] == "-" for b in blocks), covered=cov, covered_share=cov / max(1, lengths[ia]),
                           wall_ms=1e3 * wall, bk_pair_ms=rep.get("bk_pair", {}).get("ms"))
                res["pairs"].append(ent)
                print("pair %s - %s: %d anchors, %d / %d windows called, %d spilled, %d blocks (%d inverted), %.1f %% of %s covered; "
                      "%.1f ms wall, bk_pair %.2f ms" % (c1, c2, n_anch, ent["called"], ent["windows"], n_spill, len(blocks), ent["inverted"],
                                                         100 * ent["covered_share"], c1, ent["wall_ms"], ent["bk_pair_ms"] or float("nan")), flush=True)
            for i in chroms:
                ctx.blocks_release(i)

        # ---- the stage as the pipeline runs it
        t0 = time.perf_counter()
        out = bl.run(ctx, groups, gen.labels, lengths, kb, s, bin_size, a.block_votes, a.block_gap, a.min_block)
        res["stage_wall_s"] = time.perf_counter() - t0
        res["stage_pairs"] = sum(map(len, out))
        print("stage: %d pairs, indexes included, in %.3f s" % (res["stage_pairs"], res["stage_wall_s"]))
        w = np.array([p["wall_ms"] for p in res["pairs"]])
        x = np.array([e["wall_ms"] for e in res["index"]])
        c = np.array([p["covered_share"] for p in res["pairs"]])
        print("index build: median %.1f ms, max %.1f ms; pair call: median %.1f ms, max %.1f ms; coverage of A: min %.1f %%, median %.1f %%" % (
            np.median(x), x.max(), np.median(w), w.max(), 100 * c.min(), 100 * np.median(c)))
    finally:
        ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
