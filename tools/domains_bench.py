#!/usr/bin/env python
"""Context.dom_search on synthetic profiles and synthetic inner sequences, on one MI355X.

    python tools/domains_bench.py [--elements 10000] [--profiles 300] [--min_m 80] [--max_m 450] [--min_len 1000]
                                  [--max_len 10000] [--planted 0.1] [--slice 1000] [--seed 1] [--json profiles/domains_bench.json]

Nobody here has REXdb: the profile set is ASSUMED to look like its plant set as TEsorter ships it -- a few hundred
profiles (300 by default) of 80..450 nodes (uniform), each built from a random consensus protein with 0.8 on the consensus
residue and HMMER-like gap transitions (tests/domains_ref.py: consensus_profile).  The inner sequences are uniform random
DNA of min_len..max_len bases; a share `planted` of them carries the back-translation of one profile's consensus.  No real
database, no real genome and no hmmscan are involved.

Printed and written: DP cells (residues of the six frames x nodes of all profiles), the wall time of the calls (`slice`
elements each; checks, item sort, upload, kernels, download), the kernels from device events of the same pass: dm_translate, dm_search (+ dm_search_wide), dm_pick; cells per second by both
clocks; how many planted domains are the hit of their profile; and the NULL distribution -- over the unplanted elements,
the best score per node in bits per profile-length bucket (median, 99th, 99.9th percentile, maximum), and the share of
(element, profile) pairs that pass the default filters (coverage >= 20 %, >= 0.5 bit per node)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import domains_ref as dr  # noqa: E402
from subphaser_amd import _native  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
BUCKETS = ((1, 99), (100, 199), (200, 299), (300, 2048))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=10000)
    ap.add_argument("--profiles", type=int, default=300)
    ap.add_argument("--min_m", type=int, default=80)
    ap.add_argument("--max_m", type=int, default=450)
    ap.add_argument("--min_len", type=int, default=1000)
    ap.add_argument("--max_len", type=int, default=10000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--slice", type=int, default=1000, help="elements per call")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rng, nrng = random.Random(a.seed), np.random.default_rng(a.seed)
    t0 = time.perf_counter()
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, rng.randint(a.min_m, a.max_m)), name="p%d" % q) for q in range(a.profiles)]
    cons = ["".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs]
    Ms = np.array([p["M"] for p in profs], np.int64)
    lens = nrng.integers(a.min_len, a.max_len + 1, a.elements)
    parts, start, planted = [], [], {}
    pos = 0
    for e, n in enumerate(lens.tolist()):
        x = ACGT[nrng.integers(0, 4, n, dtype=np.uint8)]
        if rng.random() < a.planted:
            q = rng.randrange(a.profiles)
            dom = np.frombuffer(dr.back_translate(rng, cons[q]).encode(), np.uint8)
            if dom.size + 20 < n:
                at = rng.randrange(0, n - dom.size)
                x = x.copy()
                x[at:at + dom.size] = dom
                planted[e] = q
        parts.append(x)
        start.append(pos)
        pos += n
    chrom = np.concatenate(parts)
    start = np.array(start, np.int64)
    end = start + lens
    residues = int(sum(dr_nres(int(n)) for n in lens))
    cells = residues * int(Ms.sum())
    print("%d elements (%.1f Mbases), %d profiles of %d..%d nodes (%d in all): %.3e DP cells; generated in %.1f s" % (
        a.elements, pos / 1e6, a.profiles, Ms.min(), Ms.max(), Ms.sum(), cells, time.perf_counter() - t0), flush=True)
    res = dict(elements=a.elements, profiles=a.profiles, nodes=int(Ms.sum()), bases=int(pos), residues=residues, cells=cells,
               params={k: getattr(a, k) for k in ("min_m", "max_m", "min_len", "max_len", "planted", "slice", "seed")})
    tab = dr.tables(profs)
    ctx = _native.Context(0)
    try:
        ctx.genome_reset(1)
        ctx.genome_add(0, chrom)
        ctx.sync()
        z = np.zeros(a.elements, np.int32)
        ctx.dom_search(z[:2], start[:2], start[:2] + 30, *tab)       # warm: code objects
        # one pass, `slice` elements per call; the device events are recorded on the stream without a wait, so the same
        # pass gives both clocks
        ctx.prof_enable(True)
        ctx.prof_reset()
        out, res["call_s"] = np.empty((a.elements, a.profiles, 6), np.int32), 0.0
        for lo in range(0, a.elements, a.slice):
            hi = min(a.elements, lo + a.slice)
            t0 = time.perf_counter()
            out[lo:hi] = ctx.dom_search(z[lo:hi], start[lo:hi], end[lo:hi], *tab)
            res["call_s"] += time.perf_counter() - t0
            print("elements %d..%d done, %.1f s so far" % (lo, hi, res["call_s"]), flush=True)
        rep = ctx.prof_report()
        ctx.prof_enable(False)
    finally:
        ctx.close()
    ms = {k: v["ms"] for k, v in rep.items() if k.startswith("dm_")}
    search_s = (ms.get("dm_search", 0.0) + ms.get("dm_search_wide", 0.0)) / 1e3
    res.update(kernel_ms=ms, translate_s=ms.get("dm_translate", 0.0) / 1e3, search_s=search_s, pick_s=ms.get("dm_pick", 0.0) / 1e3,
               cells_per_s_events=cells / max(search_s, 1e-9), cells_per_s_wall=cells / res["call_s"])
    print("the calls %.2f s (%.2f Gcells/s); kernels by device events: translate %.4f s, search %.2f s (%.2f Gcells/s), pick %.4f s" % (
        res["call_s"], res["cells_per_s_wall"] / 1e9, res["translate_s"], search_s, res["cells_per_s_events"] / 1e9, res["pick_s"]), flush=True)
    # the planted domains
    ok = sum(1 for e, q in planted.items() if out[e, q, 5] - out[e, q, 4] + 1 >= 0.9 * Ms[q])
    res.update(planted=len(planted), planted_found=ok)
    print("%d of %d planted domains are the hit of their profile over >= 90 %% of its nodes" % (ok, len(planted)), flush=True)
    # the null: unplanted elements
    null = np.array([e for e in range(a.elements) if e not in planted], np.int64)
    per_node = out[null, :, 0].astype(np.float64) / (256.0 * Ms[None, :])
    cov = 100.0 * (out[null, :, 5] - out[null, :, 4] + 1) / Ms[None, :]
    res["null"] = []
    for lo, hi in BUCKETS:
        sel = (Ms >= lo) & (Ms <= hi)
        if not sel.any() or null.size == 0:
            continue
        v, c = per_node[:, sel].ravel(), cov[:, sel].ravel()
        row = dict(m_lo=lo, m_hi=hi, profiles=int(sel.sum()), pairs=int(v.size), median=float(np.median(v)), p99=float(np.percentile(v, 99)),
                   p999=float(np.percentile(v, 99.9)), max=float(v.max()), pass_score=float((v >= 0.5).mean()),
                   pass_both=float(((v >= 0.5) & (c >= 20.0)).mean()))
        res["null"].append(row)
        print("null, M %4d..%4d (%3d profiles, %d pairs): bits per node median %.3f, 99 %% %.3f, 99.9 %% %.3f, max %.3f; >= 0.5: %.2e, and coverage >= 20 %%: %.2e" % (
            lo, hi, row["profiles"], row["pairs"], row["median"], row["p99"], row["p999"], row["max"], row["pass_score"], row["pass_both"]), flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def dr_nres(n):
    return sum((n - f % 3) // 3 for f in range(6))


if __name__ == "__main__":
    main()
