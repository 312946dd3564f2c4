#!/usr/bin/env python3
"""Generate tests/golden/golden_ltr.json.gz by IMPORTING the reference's LTR module here.

Run where the reference checkout that gen_golden.py points at exists:

    python tests/golden/gen_golden_ltr.py

The reference is imported unmodified, with the stand-ins of gen_golden.py for the third-party packages this image lacks.
What runs is LTR.LTRHarvest (the `.scn` reader), group_resolve_overlaps / resolve_overlaps, LTRHarvestRecord.estimate_age,
plot_insert_age up to its R script (the `.data` and `.summary` files; Rscript is absent and its failure is ignored),
summary_ltr_time, Seqs.map_kmer3(chunk=False) on the FASTA of the elements, Circos.stack_matrix and Stats.enrich_ltr.
The fixture holds inputs (the `.scn` text, the seed of the toy genome, the labelled k-mers) and recorded results only."""
import gzip
import io
import itertools
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts oracle/, tests/ and the repository on sys.path)
import pyoracle as po  # noqa: E402
from toygenome import make_toy_genome  # noqa: E402

K, MU, SEED = 15, 13e-9, 7


def scn_text(toy):
    """records tiling A1, B1, A2, hand-placed ones there and on B2 (and one unknown sequence): 1-based, both ends included"""
    rng = np.random.RandomState(5)
    lines = ["# LTR_pp", "#start end len lLTR_str lLTR_end lLTR_len rLTR_str rLTR_end rLTR_len similarity seqid chr"]

    def rec(chrom, start, length, lltr, rltr, sim, nr=0, source=None, element_len=None):
        end = start + length - 1
        f = [start, end, element_len or length, start, start + lltr - 1, lltr, end - rltr + 1, end, rltr, sim, nr, chrom]
        lines.append(" ".join(map(str, f)) + (" #" + source if source else ""))

    for nr, chrom in enumerate(("A1", "B1", "A2")):
        n = len(toy["seqs"][chrom])
        pos = 300
        while pos + 4000 < n:
            length = int(rng.randint(1200, 3000))
            lltr = int(rng.randint(100, 400))
            sim = [100, 100.0, 99.9, 98.5, 97.31, 95.0, 90.2, 85.0][int(rng.randint(0, 8))]
            rec(chrom, pos, length, lltr, lltr + int(rng.randint(-5, 6)), sim, nr, source="ltr_harvest" if rng.randint(2) else None)
            pos += length + int(rng.randint(50, 900))
    a1 = len(toy["seqs"]["A1"])
    rec("A1", 1000, 2000, 200, 200, 91.0, 0)                      # overlaps its neighbours: decided by length
    rec("A1", 1000, 2000, 200, 200, 91.0, 0, source="ltr_finder")      # equal to the last
    rec("A1", 1000, 2500, 210, 190, 92.0, 0)                      # equal start, another end
    rec("A1", 5000, 1500, 150, 150, 20.0, 0)                      # div = 0.8
    rec("A1", 5050, 1500, 150, 150, 25.0, 0)
    rec("A1", 5100, 1400, 150, 150, 25.1, 0)
    rec("A1", a1 - 2999, 3000, 300, 300, 99.0, 0)                 # ends on the last base
    rec("A1", 1, 1800, 120, 130, 96.0, 0)                         # starts on the first
    rec("B1", 9000, 2000, 250, 250, 94.0, 1, element_len=2600)    # the length column is what overlaps are judged by
    rec("scaffold9", 100, 2000, 200, 200, 95.0, 7)
    rec("B1", 20000, 2000, 200, 200, 93.0, 1)                     # B1 again: another run of its own
    rec("B1", 20150, 1800, 200, 200, 93.0, 1)                     # 90 % overlap
    rec("B1", 21900, 1000, 120, 120, 93.0, 1)                     # 10 %: not above max_ovl
    rec("B1", 22790, 1100, 120, 120, 88.0, 1)                     # just above
    rec("B2", 1000, 1500, 150, 150, 20.0, 3)                      # div = 0.8
    rec("B2", 4000, 1500, 150, 150, 25.0, 3)                      # div = 0.75, the boundary
    rec("B2", 7000, 1400, 150, 150, 25.1, 3)                      # div just below
    rec("B2", 10000, 1400, 150, 150, 100, 3)                      # no divergence
    return "\n".join(lines) + "\n"


def main():
    tmp = tempfile.mkdtemp(prefix="sp_golden_ltr_")
    gg.install_standins(tmp)
    import logging
    logging.disable(logging.CRITICAL)
    from subphaser import LTR, Circos, Seqs, Stats  # noqa

    toy = make_toy_genome(seed=SEED)
    seqs = {lab: toy["seqs"][lab] for lab in toy["labels"]}
    d_sg = dict(toy["sg_assigned"])
    sg_names = sorted(set(d_sg.values()))

    # labelled k-mers: repeated in A2 and absent from B2 -> SG1, and the other way round; every third one (the last quarter
    # of A1 carries B's repeats: potential exchanges)
    def kmers(lab):
        keys, counts = po.count(seqs[lab], K, 1)
        return {po.decode(k_, K): int(c) for k_, c in zip(keys.tolist(), counts.tolist())}
    ka, kb = kmers("A2"), kmers("B2")
    d_kmers = {}
    for mine, other, sg in ((ka, kb, "SG1"), (kb, ka, "SG2")):
        for kmer in sorted(x for x, c in mine.items() if c >= 4 and x not in other)[::3]:
            d_kmers[kmer] = sg

    # Cluster.output_kmers hands map_kmer3 every labelled k-mer on both strands (Cluster.py:175); the fixture keeps one
    comp = str.maketrans("ACGT", "TGCA")
    both = dict(d_kmers)
    both.update({kmer.translate(comp)[::-1]: sg for kmer, sg in d_kmers.items()})

    text = scn_text(toy)
    scn = os.path.join(tmp, "LTR.scn")
    open(scn, "w").write(text)
    ltrs = list(LTR.LTRHarvest(scn))
    out = {"seed": SEED, "k": K, "mu": MU, "scn": text, "d_sg": d_sg, "sg_names": sg_names,
           "kmers": sorted(d_kmers.items()),
           "records": [[r.id, r.start, r.end, r.element_len, r.lltr, r.rltr, r.lltr_e, r.rltr_s, r.similarity, r.seq_nr, r.seq_id]
                       for r in ltrs]}
    known = [r for r in ltrs if r.seq_id in seqs]
    resolved = LTR.group_resolve_overlaps(known)
    # equal starts come out of a set in hash order: every run (itertools.groupby, as group_resolve_overlaps) sorted by the full key
    by_run = []
    for _, items in itertools.groupby(known, key=lambda x: x.seq_id):
        by_run += sorted(LTR.resolve_overlaps(list(items)), key=lambda r: (r.start, r.end, r.lltr_e, r.rltr_s))
    assert sorted(r.id for r in by_run) == sorted(r.id for r in resolved) and len(by_run) == len(resolved)
    resolved = by_run
    out["resolved"] = [r.id for r in resolved]
    out["ages"] = [r.estimate_age(mu=MU) for r in resolved]

    fa = os.path.join(tmp, "LTR.filtered.LTR.fa")
    with open(fa, "w") as f:
        for r in resolved:
            f.write(">{}\n{}\n".format(r.id, r.get_full_seq(d_seqs=seqs)))
    buf = io.StringIO()
    Seqs.map_kmer3([fa], both, fout=buf, k=K, ncpu=1, bin_size=10000000, sg_names=sg_names, chunk=False, log=False, method="map")
    out["bin_count"] = buf.getvalue()
    ltr_map = os.path.join(tmp, "x.ltr.bin.count")
    open(ltr_map, "w").write(buf.getvalue())
    bins, counts = Circos.stack_matrix(ltr_map, window_size=100000000)
    buf = io.StringIO()
    d_enriched, d_exchange = Stats.enrich_ltr(buf, d_sg, counts, colnames=sg_names, rownames=bins, max_pval=0.05, ncpu=1)
    out["enrich"] = buf.getvalue()
    out["d_enriched"], out["d_exchange"] = d_enriched, d_exchange

    class Colors:
        colors_r = "c('red','blue','grey')"
    out["insert"] = {}
    for excl in (False, True):
        for nonspec in (False, True):
            prefix = os.path.join(tmp, "x.ltr.insert.%d%d" % (excl, nonspec))
            try:
                LTR.plot_insert_age(resolved, d_enriched, prefix, shared={}, exclude_exchanges=excl, d_exchange=d_exchange,
                                    non_specific=nonspec, mu=MU, figfmt="pdf", sg_color=Colors())
            except Exception as e:      # Rscript: the two text files are complete before it is started
                print("plot_insert_age stopped after the text files:", repr(e)[:200])
            out["insert"]["%d%d" % (excl, nonspec)] = {"data": open(prefix + ".data").read(), "summary": open(prefix + ".summary").read()}
    d_data = {"SG2": [0.5, 1.25, 3.0], "SG1": [2.0], "non-specific": [0.0, 0.0, 7.5, 0.125]}
    buf = io.StringIO()
    d_info = LTR.summary_ltr_time(d_data, buf)
    out["summary_hand"] = {"d_data": d_data, "text": buf.getvalue(), "d_info": d_info}

    path = os.path.join(HERE, "golden_ltr.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print("wrote", path, os.path.getsize(path), "bytes;", len(ltrs), "records,", len(resolved), "resolved,", len(d_kmers), "k-mers,",
          len(d_enriched), "enriched,", sum(v == "yes" for v in d_exchange.values()), "exchanges")


if __name__ == "__main__":
    main()
