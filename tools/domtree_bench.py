#!/usr/bin/env python
"""The device calls of the domain trees (-ltr_domtree) on synthetic families, on one MI355X: Context.dom_align,
aln_pairs and nj_tree, each kernel by the device events of sp_prof_report.

    python tools/domtree_bench.py [--elements 1000] [--nodes 150 250 120] [--families 8] [--family_sub 0.25]
                                  [--member_sub 0.05] [--pad 32] [--seed 1] [--json profiles/domtree_bench.json]

Nobody here has REXdb: the three profiles are ASSUMED to look like an INT, an RT and an RH profile of its plant set (150, 250
and 120 nodes by default), each built from a random consensus protein with 0.8 on the consensus residue and HMMER-like gap
transitions (tests/domains_ref.py: consensus_profile), as tools/domains_bench.py assumes them.  An element is three domains
in frame 0 of one inner sequence; a family substitutes `family_sub` of the consensus residues, a member `member_sub` more.
No real database, no real genome and no mafft / trimal / iqtree run are involved.

Printed and written: per kernel milliseconds (da_residues, da_fill + da_fill_wide, da_trace, da_pairs, the nj_* kernels), the
cells per second of da_fill, the same of dm_search over the same windows' intervals and profiles, the share of da_trace in
the alignment, the wall time of each call, and how many families are one clade of the tree."""
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
from subphaser_amd import _native, domtree, ltrtree  # noqa: E402


def variant(rng, protein, rate):
    return "".join(rng.choice([a for a in dr.AA if a != c]) if rng.random() < rate else c for c in protein)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1000)
    ap.add_argument("--nodes", type=int, nargs="+", default=[150, 250, 120])
    ap.add_argument("--families", type=int, default=8)
    ap.add_argument("--family_sub", type=float, default=0.25)
    ap.add_argument("--member_sub", type=float, default=0.05)
    ap.add_argument("--pad", type=int, default=domtree.PAD)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rng = random.Random(a.seed)
    t0 = time.perf_counter()
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, M), name="d%d" % q) for q, M in enumerate(a.nodes)]
    cons = ["".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs]
    fams = [[variant(rng, c, a.family_sub) for c in cons] for _ in range(a.families)]
    spacer, D = 12, len(profs)
    parts, start, end, family, items, pos = [], [], [], [], [], 0
    for e in range(a.elements):
        f = e % a.families
        res_at, prot = 0, ""
        wins = []
        for d in range(D):
            dom = variant(rng, fams[f][d], a.member_sub)
            head = dr.rand_protein(rng, spacer)
            wins.append((res_at + spacer, res_at + spacer + len(dom) - 1))
            prot += head + dom
            res_at += spacer + len(dom)
        prot += dr.rand_protein(rng, spacer)
        dna = dr.back_translate(rng, prot)
        parts.append(dna)
        start.append(pos)
        pos += len(dna)
        end.append(pos)
        family.append(f)
        n_res = len(prot)
        for d, (i_s, i_e) in enumerate(wins):
            items.append((e, 0) + domtree.window(i_s, i_e, n_res, a.pad) + (d,))
    chrom = "".join(parts)
    el, fr, i0, i1, pr = (np.array(c) for c in zip(*items))
    start, end = np.array(start, np.int64), np.array(end, np.int64)
    place = (np.zeros(len(items), np.int32), start[el], end[el], fr.astype(np.int32), i0.astype(np.int32), i1.astype(np.int32))
    Ms = np.array(a.nodes, np.int64)
    cells = int(((i1 - i0 + 1) * Ms[pr]).sum())
    print("%d elements x %d domains (%d..%d nodes) in %d families, %.2f Mbases: %d items, %.3e cells; generated in %.1f s" % (
        a.elements, D, Ms.min(), Ms.max(), a.families, pos / 1e6, len(items), cells, time.perf_counter() - t0), flush=True)
    res = dict(elements=a.elements, nodes=a.nodes, items=len(items), cells=cells,
               params={k: getattr(a, k) for k in ("families", "family_sub", "member_sub", "pad", "seed")})
    tab = dr.tables(profs)
    ctx = _native.Context(0)
    try:
        ctx.genome_reset(1)
        ctx.genome_add(0, chrom)
        ctx.sync()
        ctx.dom_align(*(p[:2] for p in place), pr[:2].astype(np.int32), *tab)      # warm: code objects
        ctx.aln_pairs(np.zeros((2, 8), np.uint8))
        ctx.nj_tree(np.array([[0, 1], [1, 0]], np.int64))
        ctx.dom_search(place[0][:2], place[1][:2], place[2][:2], *tab)
        ctx.prof_enable(True)
        ctx.prof_reset()
        t0 = time.perf_counter()
        hit, col, coff = ctx.dom_align(*place, pr.astype(np.int32), *tab)
        res["align_call_s"] = time.perf_counter() - t0
        pep, poff = ctx.dom_peptide(*place)
        t0 = time.perf_counter()
        blocks = [[] for _ in range(D)]
        for q in range(len(items)):
            blocks[q % D].append(domtree.row_string(col[int(coff[q]):int(coff[q + 1])].tolist(), int(i0[q]), pep[int(poff[q]):int(poff[q + 1])]))
        desc, records, dropped = domtree.cat_rows(list(range(a.elements)), blocks, unique=True)
        trimmed = domtree.trim([r for _, r in records], domtree.OCCUPANCY)
        rows = domtree.encode(trimmed)
        res["rows_host_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        same, both = ctx.aln_pairs(rows)
        res["pairs_call_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        Dm = domtree.distance_matrix(same, both)
        res["distance_host_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        rec = np.asarray(ctx.nj_tree(Dm), np.int64)
        res["nj_call_s"] = time.perf_counter() - t0
        # the search over the same windows, as intervals of their own, and the same profiles: its cells per second
        w_start, w_end = place[1] + 3 * i0, place[1] + 3 * (i1 + 1)
        t0 = time.perf_counter()
        ctx.dom_search(place[0][::D], w_start[::D], w_end[::D], *tab)
        res["search_call_s"] = time.perf_counter() - t0
        rep = ctx.prof_report()
        ctx.prof_enable(False)
    finally:
        ctx.close()
    ms = {k: v["ms"] for k, v in rep.items() if k.startswith(("da_", "dm_", "nj_"))}
    fill = ms.get("da_fill", 0.0) + ms.get("da_fill_wide", 0.0)
    trace = ms.get("da_trace", 0.0)
    search_cells = int(sum(sum((int(n) - f % 3) // 3 for f in range(6)) for n in (w_end[::D] - w_start[::D])) * int(Ms.sum()))
    search = ms.get("dm_search", 0.0) + ms.get("dm_search_wide", 0.0)
    nj = sum(v for k, v in ms.items() if k.startswith("nj_"))
    res.update(kernel_ms=ms, rows=len(records), columns=int(rows.shape[1]), dropped=dropped, fill_cells_per_s=cells / max(fill / 1e3, 1e-9),
               search_cells=search_cells, search_cells_per_s=search_cells / max(search / 1e3, 1e-9),
               trace_share=trace / max(fill + trace + ms.get("da_residues", 0.0), 1e-9), nj_ms=nj)
    print("align: residues %.3f ms, fill %.3f ms (%.2f Gcells/s), trace %.3f ms (%.1f %% of the three); the call %.3f s" % (
        ms.get("da_residues", 0.0), fill, res["fill_cells_per_s"] / 1e9, trace, 100 * res["trace_share"], res["align_call_s"]), flush=True)
    print("search of the same windows: %.3f ms (%.2f Gcells/s)" % (search, res["search_cells_per_s"] / 1e9), flush=True)
    print("pairs: %d rows x %d columns, da_pairs %.3f ms; the call %.3f s; distances on the host %.3f s" % (
        len(records), rows.shape[1], ms.get("da_pairs", 0.0), res["pairs_call_s"], res["distance_host_s"]), flush=True)
    print("neighbour joining: kernels %.3f ms; the call %.3f s" % (nj, res["nj_call_s"]), flush=True)
    # the planted families as clades
    fam_of = [family[e] for e, _ in records]
    splits = set(ltrtree.splits(ltrtree.unrooted_edges(rec), len(records)))
    every = frozenset(range(len(records)))
    ok = 0
    for f in range(a.families):
        leaves = frozenset(q for q, x in enumerate(fam_of) if x == f)
        ok += bool(leaves) and (leaves in splits or every - leaves in splits or len(leaves) in (len(records), len(records) - 1, 1))
    res.update(families_as_clades=ok)
    print("%d of %d families are one clade of the tree" % (ok, a.families), flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
