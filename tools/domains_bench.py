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
(element, profile) pairs that pass the default filters (coverage >= 20 %, >= 0.5 bit per node).

    python tools/domains_bench.py --prefilter [--elements 400] [--planted 0.5] ...

The ungapped prefilter (Context.dom_ssv, Context.dom_search(prefilter=)) on the same assumed profiles.  The planted copies
are DIVERGED here: the consensus with 0, 10, 20 or 30 % of its residues substituted and 0 to 3 single-residue indels, then
back-translated (an exact copy is one ungapped segment, which an ungapped filter cannot lose).  Printed and written:
  (a) the null distribution of ssv in bits over the (frame, profile) items of the unplanted elements, by profile-length class
      and frame-length class (median, 98th, 99th, 99.9th percentile, maximum);
  (b) per divergence class, the planted domains the unfiltered search finds (the hit of their profile over >= 50 % of its nodes);
  (c) for thresholds of 8..30 whole bits: the null pass rate, the found planted domains whose winning frame the filter
      drops, by divergence class, and the wall time of the filtered call against the unfiltered call on the same elements;
      the time of dm_ssv by device events, and its cells per second beside dm_search's.
The rule for domains.PREFILTER_BITS: the smallest whole number of bits at which at most 2 % of the null items pass."""
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
    ap.add_argument("--prefilter", action="store_true", help="the ungapped prefilter: null, diverged copies, threshold sweep")
    a = ap.parse_args()
    if a.prefilter:
        return prefilter_mode(a)
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


DIVERGENCE = (0, 10, 20, 30)
SWEEP = (8, 30)      # whole bits
FRAME_CLASSES = ((1, 999), (1000, 1999), (2000, 21845))


def diverged(rng, protein, sub_pct, indels):
    out = [rng.choice([b for b in dr.AA if b != a]) if rng.random() < sub_pct / 100.0 else a for a in protein]
    for _ in range(indels):
        at = rng.randrange(5, len(out) - 5)
        if rng.random() < 0.5:
            out.insert(at, rng.choice(dr.AA))
        else:
            del out[at]
    return "".join(out)


def prefilter_mode(a):
    rng, nrng = random.Random(a.seed), np.random.default_rng(a.seed)
    t0 = time.perf_counter()
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, rng.randint(a.min_m, a.max_m)), name="p%d" % q) for q in range(a.profiles)]
    cons = ["".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs]
    Ms = np.array([p["M"] for p in profs], np.int64)
    lens = nrng.integers(a.min_len, a.max_len + 1, a.elements)
    parts, start, planted, pos = [], [], {}, 0
    for e, n in enumerate(lens.tolist()):
        x = ACGT[nrng.integers(0, 4, n, dtype=np.uint8)]
        if rng.random() < a.planted:
            q, sub, indels = rng.randrange(a.profiles), rng.choice(DIVERGENCE), rng.randrange(4)
            dom = np.frombuffer(dr.back_translate(rng, diverged(rng, cons[q], sub, indels)).encode(), np.uint8)
            if dom.size + 20 < n:
                at = rng.randrange(0, n - dom.size)
                x = x.copy()
                x[at:at + dom.size] = dom
                planted[e] = (q, sub, indels)
        parts.append(x)
        start.append(pos)
        pos += n
    chrom = np.concatenate(parts)
    start = np.array(start, np.int64)
    end = start + lens
    residues = int(sum(dr_nres(int(n)) for n in lens))
    cells = residues * int(Ms.sum())
    print("%d elements (%.1f Mbases), %d planted, %d profiles of %d..%d nodes (%d in all): %.3e DP cells; generated in %.1f s" % (
        a.elements, pos / 1e6, len(planted), a.profiles, Ms.min(), Ms.max(), Ms.sum(), cells, time.perf_counter() - t0), flush=True)
    res = dict(mode="prefilter", elements=a.elements, profiles=a.profiles, nodes=int(Ms.sum()), bases=int(pos), residues=residues, cells=cells,
               planted=len(planted), params={k: getattr(a, k) for k in ("min_m", "max_m", "min_len", "max_len", "planted", "seed")})
    tab = dr.tables(profs)
    z = np.zeros(a.elements, np.int32)
    ctx = _native.Context(0)

    def timed(call):
        ctx.prof_reset()
        t = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t
        return out, wall, {k: v["ms"] / 1e3 for k, v in ctx.prof_report().items() if k.startswith("dm_")}
    try:
        ctx.genome_reset(1)
        ctx.genome_add(0, chrom)
        ctx.sync()
        ctx.dom_search(z[:2], start[:2], start[:2] + 30, *tab, prefilter=0, stats={})      # warm: code objects
        ctx.dom_ssv(z[:2], start[:2], start[:2] + 30, *tab)
        ctx.prof_enable(True)
        ssv, ssv_wall, ev = timed(lambda: ctx.dom_ssv(z, start, end, *tab))
        res.update(ssv_call_s=ssv_wall, ssv_kernel_s=ev.get("dm_ssv", 0.0), ssv_cells_per_s=cells / max(ev.get("dm_ssv", 0.0), 1e-9))
        print("dom_ssv: the call %.3f s, dm_ssv by device events %.4f s: %.1f Gcells/s" % (ssv_wall, res["ssv_kernel_s"], res["ssv_cells_per_s"] / 1e9), flush=True)
        plain, plain_wall, ev = timed(lambda: ctx.dom_search(z, start, end, *tab))
        search_s = ev.get("dm_search", 0.0) + ev.get("dm_search_wide", 0.0)
        res.update(search_call_s=plain_wall, search_kernel_s=search_s, search_cells_per_s=cells / max(search_s, 1e-9))
        print("dom_search: the call %.2f s, dm_search by device events %.2f s: %.1f Gcells/s" % (plain_wall, search_s, res["search_cells_per_s"] / 1e9), flush=True)
        # (a) the null
        null = np.array([e for e in range(a.elements) if e not in planted], np.int64)
        nres = np.array([[(n - f % 3) // 3 for f in range(6)] for n in lens[null].tolist()], np.int64)      # [null, 6]
        bits = ssv[null].astype(np.float64) / 256.0                                                          # [null, P, 6]
        live = np.broadcast_to((nres > 0)[:, None, :], bits.shape)
        res["null"] = []
        for mlo, mhi in BUCKETS:
            for flo, fhi in FRAME_CLASSES:
                sel = live & ((Ms >= mlo) & (Ms <= mhi))[None, :, None] & ((nres >= flo) & (nres <= fhi))[:, None, :]
                if not sel.any():
                    continue
                v = bits[sel]
                row = dict(m_lo=mlo, m_hi=mhi, res_lo=flo, res_hi=fhi, items=int(v.size), median=float(np.median(v)), p98=float(np.percentile(v, 98)),
                           p99=float(np.percentile(v, 99)), p999=float(np.percentile(v, 99.9)), max=float(v.max()))
                res["null"].append(row)
                print("null, M %4d..%4d, %5d..%5d residues (%8d items): ssv bits median %.2f, 98 %% %.2f, 99 %% %.2f, 99.9 %% %.2f, max %.2f" % (
                    mlo, mhi, flo, fhi, row["items"], row["median"], row["p98"], row["p99"], row["p999"], row["max"]), flush=True)
        null_bits = bits[live]
        # (b) the planted domains the unfiltered search finds, and the ssv of their winning frame
        found = {d: [] for d in DIVERGENCE}      # divergence -> ssv bits of the winning frame
        n_planted = {d: 0 for d in DIVERGENCE}
        for e, (q, sub, indels) in planted.items():
            n_planted[sub] += 1
            if plain[e, q, 5] - plain[e, q, 4] + 1 >= 0.5 * Ms[q]:
                found[sub].append(ssv[e, q, plain[e, q, 1]] / 256.0)
        res["planted_by_divergence"] = {str(d): dict(planted=n_planted[d], found=len(found[d]), min_ssv_bits=float(min(found[d])) if found[d] else None)
                                        for d in DIVERGENCE}
        print("planted / found without the filter (lowest ssv of a winning frame, bits), by divergence: " + ", ".join(
            "%d %%: %d / %d (%.1f)" % (d, n_planted[d], len(found[d]), min(found[d]) if found[d] else float("nan")) for d in DIVERGENCE), flush=True)
        # (c) the sweep
        res["sweep"], rule = [], None
        for T in range(SWEEP[0], SWEEP[1] + 1):
            stats = {}
            out, wall, ev = timed(lambda: ctx.dom_search(z, start, end, *tab, prefilter=T * 256, stats=stats))
            rate = float((null_bits >= T).mean())
            lost = {d: int(sum(b < T for b in found[d])) for d in DIVERGENCE}
            same = int(sum((out[e, q] == plain[e, q]).all() for e, (q, _, _) in planted.items()))
            row = dict(bits=T, null_pass=rate, lost={str(d): lost[d] for d in DIVERGENCE}, planted_unchanged=same, items=stats["items"], passed=stats["passed"],
                       call_s=wall, ratio=wall / plain_wall, ssv_s=ev.get("dm_ssv", 0.0), search_s=ev.get("dm_search", 0.0) + ev.get("dm_search_wide", 0.0))
            res["sweep"].append(row)
            if rule is None and rate <= 0.02:
                rule = T
            print("T = %2d bits: null pass %.4f %%, all items passed %.4f %%; lost %s; the call %.3f s = %.4f of the unfiltered (dm_ssv %.4f s, dm_search %.3f s)" % (
                T, 1e2 * rate, 1e2 * stats["passed"] / max(stats["items"], 1), " ".join("%d%%:%d/%d" % (d, lost[d], len(found[d])) for d in DIVERGENCE), wall,
                row["ratio"], row["ssv_s"], row["search_s"]), flush=True)
        res["rule_bits"] = rule
        print("the rule (smallest whole number of bits with a null pass rate <= 2 %%): %s" % rule, flush=True)
        ctx.prof_enable(False)
    finally:
        ctx.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def dr_nres(n):
    return sum((n - f % 3) // 3 for f in range(6))


if __name__ == "__main__":
    main()
