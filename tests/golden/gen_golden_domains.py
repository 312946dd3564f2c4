#!/usr/bin/env python3
"""Generate tests/golden/golden_domains.json.gz by IMPORTING the reference's LTR module and its copy of TEsorter here.

Run where the reference checkout that gen_golden.py points at exists:

    python tests/golden/gen_golden_domains.py

The reference is imported unmodified, with the stand-ins of gen_golden.py for the third-party packages this image lacks.
What runs is LTRHarvestRecord.get_int_seq (the interval the inner sequence is cut at), group_resolve_overlaps on records
some of which a classification calls complete, TEsorter's parse_hmmname and
Classifier.classify (with classify_element, identify_rexdb and _parse_rexdb) on hand-made domain lists written as the
`.dom.gff3` lines hmm2best writes.  The fixture holds inputs (the `.scn` lines, the domain lists) and recorded results only."""
import gzip
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts oracle/, tests/ and the repository on sys.path)

COPIA, GYPSY = "Class_I/LTR/Ty1_copia/", "Class_I/LTR/Ty3_gypsy/"


def _genes(prefix, clade, ty, genes):
    return ["%s%s:%s-%s" % (prefix, clade, ty, g) for g in genes]


# name -> (strands, profile names in gff order): an element's lines are sorted by start, so the order IS the position
CASES = {
    "single_clade": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT", "INT", "RT", "RH"])),
    "complete_gypsy": ("+", _genes(GYPSY, "chromovirus/Tekay", "Ty3", ["GAG", "PROT", "RT", "RH", "INT"])),
    "incomplete_copia": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG", "INT", "RT"])),
    "disordered_copia": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT", "RT", "INT", "RH"])),
    "incomplete_gypsy": ("+", _genes(GYPSY, "non-chromovirus/OTA/Athila", "Ty3", ["PROT", "RT", "RH"])),
    "gypsy_arh_chdii": ("+", _genes(GYPSY, "chromovirus/CRM", "Ty3", ["GAG", "PROT", "RT", "RH", "aRH", "INT", "CHDII"])),
    "majority": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT", "INT"]) + _genes(COPIA, "Ivana", "Ty1", ["RT"])),
    "majority_second": ("+", _genes(COPIA, "Ivana", "Ty1", ["GAG"]) + _genes(COPIA, "Ale", "Ty1", ["PROT", "INT", "RT"])),
    "tie_two_two": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT"]) + _genes(COPIA, "Ivana", "Ty1", ["INT", "RT"])),
    "clade_mixture": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG"]) + _genes(COPIA, "Ivana", "Ty1", ["RT"])),
    "three_clades": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG"]) + _genes(COPIA, "Ivana", "Ty1", ["PROT", "INT"]) + _genes(COPIA, "Tork", "Ty1", ["RT", "RH"])),
    "superfamily_mixture": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG"]) + _genes(GYPSY, "chromovirus/Tekay", "Ty3", ["RT"])),
    "order_mixture": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG"]) + ["Class_I/LINE:LINE-RT"]),
    "order_mixture_majority": ("+", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT"]) + ["Class_I/LINE:LINE-RT"]),
    "minus_strand": ("-", _genes(COPIA, "Ale", "Ty1", ["RH", "RT", "INT", "PROT", "GAG"])),
    "minus_strand_forward_order": ("-", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT", "INT", "RT", "RH"])),
    "mixed_strands": ("+-+", _genes(COPIA, "Ale", "Ty1", ["GAG", "PROT", "INT"])),
    "line": ("+", ["Class_I/LINE:LINE-RT", "Class_I/LINE:LINE-ENDO"]),
    "class_ii": ("+", ["Class_II/Subclass_1/TIR/hAT:hAT-TPase"]),
    "class_ii_short": ("+", ["Class_II/Subclass_2/Helitron:Helitron-HEL1", "Class_II/Subclass_2/Helitron:Helitron-HEL2"]),
    "pararetrovirus": ("+", ["Class_I/pararetrovirus:pararetrovirus-RT", "Class_I/pararetrovirus:pararetrovirus-RH"]),
    "retrovirus_na": ("+", ["NA:Retrovirus-RH"]),
    "bel_pao": ("+", _genes("Class_I/LTR/", "Bel-Pao", "Bel-Pao", ["GAG", "PROT", "RT", "RH", "INT"])),
    "retrovirus": ("+", _genes("Class_I/LTR/", "Retrovirus", "Retrovirus", ["RT", "RH"])),
    "ty_clade": ("+", ["Class_I/LTR/Ty1_copia:Ty1-RT", "Class_I/LTR/Ty1_copia:Ty1-RH"]),
    "ty_outgroup": ("+", ["Class_I/LTR/Ty3_gypsy/Ty3-outgroup:Ty3-RT"]),
    "dirs": ("+", ["Class_I/DIRS:DIRS-RT"]),
}
NAMES = sorted({n for _, names in CASES.values() for n in names})

SCN = ["10 2009 2000 10 209 200 1810 2009 200 95.00 0 chrA",
       "1 900 900 1 120 120 771 900 130 88.10 0 chrA",
       "301 1300 1000 301 400 100 1201 1300 100 100.00 1 chrB"]


# overlapping records of one sequence: (start, length, complete?) -- a complete one beats a longer incomplete one
OVERLAPS = [(100, 2000, False), (600, 1500, True), (1900, 3000, False), (6000, 1000, True), (6100, 1500, True), (8000, 900, False),
            (8100, 2000, False), (8200, 500, True), (12000, 1000, True), (12950, 1000, False), (12990, 3000, False)]


def main():
    tmp = tempfile.mkdtemp(prefix="sp_golden_dom_")
    gg.install_standins(tmp)
    import logging
    logging.disable(logging.CRITICAL)
    from subphaser import LTR  # noqa
    from subphaser.api.TEsorter import app  # noqa

    # the interval of the inner sequence: get_int_seq on a list of positions, so that the slice names its own interval
    inner = []
    for line in SCN:
        rec = LTR.LTRHarvestRecord(line)
        got = rec.get_int_seq(seq=list(range(2500)))
        inner.append({"line": line, "id": rec.id, "first": got[0], "last": got[-1], "length": len(got)})

    recs = []
    for start, length, complete in OVERLAPS:
        end = start + length - 1
        rec = LTR.LTRHarvestRecord(" ".join(map(str, [start, end, length, start, start + 99, 100, end - 99, end, 100, 90.0, 0, "chrA"])))
        if complete:
            rec.completed = "yes"
        recs.append(rec)
    overlaps = {"records": [list(o) for o in OVERLAPS], "kept": [r.id for r in LTR.group_resolve_overlaps(recs)]}

    parsed = {n: list(app.parse_hmmname(n, db="rexdb")) for n in NAMES}

    gff = os.path.join(tmp, "cases.dom.gff3")
    with open(gff, "w") as f:
        for q, (case, (strands, names)) in enumerate(CASES.items()):
            lid = "chr%d:%d-%d:%d-%d" % (q % 3, 100 + q, 9000 + q, 300 + q, 8700 + q)
            for j, name in enumerate(names):
                gene, clade = app.parse_hmmname(name, db="rexdb")
                domain = gene.split("-")[1]
                domain = {"aRH": "RH", "TPase": "INT"}.get(domain, domain)
                strand = strands[j % len(strands)]
                gid = "%s|%s" % (app.format_gff_id(lid), name)
                attr = "ID={};Name={}-{};gene={};clade={};coverage=90.0;evalue=1e-20;probability=0.9".format(gid, clade, domain, domain, clade)
                f.write("\t".join(map(str, ["chr%d" % (q % 3), "TEsorter", "CDS", 400 + 500 * j, 800 + 500 * j, 1.5, strand, j % 3, attr])) + "\n")
    out = io.StringIO()
    rows = [[c.id, c.order, c.superfamily, c.clade, c.completed, c.strand, c.domains] for c in app.Classifier(gff=gff, db="rexdb", fout=out).classify()]
    assert len(rows) == len(CASES)
    fixture = {"inner": inner, "overlaps": overlaps, "names": parsed, "gff": open(gff).read(), "cases": list(CASES), "rows": rows, "cls_text": out.getvalue()}
    path = os.path.join(HERE, "golden_domains.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(fixture, sort_keys=True).encode())
    print("wrote %s (%d bytes): %d classifier rows, %d names, %d intervals" % (path, os.path.getsize(path), len(rows), len(parsed), len(inner)))


if __name__ == "__main__":
    main()
