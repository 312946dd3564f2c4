"""CPU: the host side of the LTR-RT classification (subphaser_amd/domains.py): the HMMER3 reader and its integer conversion
on files written here, name parsing, the choice per domain, the filters at their thresholds, the coordinates, the writers,
and the restated classifier against the reference's own rows (tests/golden/golden_domains.json.gz, recorded by
tests/golden/gen_golden_domains.py from the reference's copy of TEsorter) with `==`."""
import gzip
import io
import json
import math
import os
import random

import numpy as np
import pytest

import domains_ref as dr
from subphaser_amd import domains as dm
from subphaser_amd import ltr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden_dom():
    with gzip.open(os.path.join(HERE, "golden", "golden_domains.json.gz")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def profs():
    rng = random.Random(4)
    return [dr.consensus_profile(rng, dr.rand_protein(rng, M), name=name)
            for M, name in ((7, "Class_I/LTR/Ty1_copia/Ale:Ty1-RT"), (1, "PF00078"), (12, "Class_I/LTR/Ty3_gypsy/chromovirus/Tekay:Ty3-INT"))]


# ------------------------------------------------------------------------------------------------ the reader
def test_read_hmm_variants_agree(tmp_path, profs):
    got = []
    for q, kw in enumerate((dict(), dict(compo=False), dict(annot=False), dict(version="HMMER3/b [3.0 | March 2010]", annot=False, compo=False))):
        p = tmp_path / ("v%d.hmm" % q)
        p.write_text(dr.hmm_text(profs, **kw))
        got.append(dm.read_hmm(str(p)))
    a = got[0]
    assert a.names == [p["name"] for p in profs] and a.M == [7, 1, 12] and len(a) == 3
    assert a.moff.tolist() == [0, 7, 8, 20] and a.emis.shape == (20, 22) and a.trans.shape == (20, 7)
    assert a.entry.tolist() == [dr.entry_score(M) for M in (7, 1, 12)] == [-1231, 0, -1609]
    for b in got[1:]:
        assert b.names == a.names and all((x == y).all() for x, y in zip(a.tables(), b.tables()))
    # `*`: the last node's m->d and d->d
    assert a.trans[6, dm_idx("MD")] == dm.NEG and a.trans[6, dm_idx("DD")] == dm.NEG and a.trans[19, dm_idx("DD")] == dm.NEG
    assert (a.emis[:, 20] == 0).all() and (a.emis[:, 21] == -2048).all()
    # the text rounds -ln p to five decimals: the tables are the twin's to within one unit, and mostly equal
    want = np.concatenate([p["emis"] for p in profs])
    assert np.abs(a.emis - want).max() <= 1 and (a.emis == want).mean() > 0.95
    assert np.abs(a.trans - np.concatenate([p["trans"] for p in profs])).max() <= 1
    assert dm.BACKGROUND == dr.BACKGROUND and abs(sum(dm.BACKGROUND.values()) - 1.0) < 1e-12


def dm_idx(name):
    return ["MM", "MI", "MD", "IM", "II", "DM", "DD"].index(name)


def test_integer_conversion_on_hand_values():
    ln2 = math.log(2)
    assert dm.trans_score(0.0) == 0 and dm.trans_score(ln2) == -256 and dm.trans_score(None) == dm.NEG == -(1 << 20)
    assert dm.trans_score(0.69315) == -256 and dm.trans_score(3 * ln2 + 0.001) == -768
    assert dm.trans_score(0.5 * ln2 / 256) == 0 and dm.trans_score(1.5 * ln2 / 256 + 1e-9) == -2        # halves round up
    # an emission equal to the background scores 0; p = 1 scores -log2 q
    assert dm.emis_score(math.log(61 / 4), "A") == 0 and dm.emis_score(2.72458, "A") == 0
    assert dm.emis_score(0.0, "W") == 1518 and dm.emis_score(0.0, "L") == math.floor(math.log2(61 / 6) * 256 + 0.5) == 857
    assert dm.emis_score(None, "C") == dm.NEG
    assert [dm.entry_score(M) for M in (1, 2, 3, 2048)] == [0, -406, -662, math.floor(math.log2(2 / (2048 * 2049)) * 256 + 0.5)]
    assert [dm.CODONS[a] for a in "LSRAGPTVICDEFHKNQYMW"] == [6] * 3 + [4] * 5 + [3] + [2] * 9 + [1] * 2 and sum(dm.CODONS.values()) == 61


def _lines(profs):
    return dr.hmm_text(profs[:1]).split("\n")


@pytest.mark.parametrize("name, edit, line, expected", [
    ("no_header", lambda L: L[1:], 1, "first line of a profile"),
    ("dna", lambda L: [x.replace("ALPH  amino", "ALPH  DNA") for x in L], 9, "ALPH  amino"),
    ("no_alph", lambda L: [x for x in L if not x.startswith("ALPH")], 8, "ALPH  amino"),
    ("no_leng", lambda L: [x for x in L if not x.startswith("LENG")], 8, "LENG"),
    ("leng_text", lambda L: [x.replace("LENG  7", "LENG  seven") for x in L], 4, "LENG <integer>"),
    ("no_name", lambda L: [x for x in L if not x.startswith("NAME")], 8, "NAME"),
    ("letters", lambda L: [x.replace("A        C        D", "C        A        D") for x in L], 9, "20 letters"),
    ("node_number", lambda L: L[:16] + [L[16].replace("      2 ", "      3 ", 1)] + L[17:], 17, "match line of node 2 of 7"),
    ("few_values", lambda L: L[:14] + [" ".join(L[14].split()[:15])] + L[15:], 15, "insert emissions of node 1"),
    ("few_transitions", lambda L: L[:15] + [" ".join(L[15].split()[:6])] + L[16:], 16, "transitions of node 1 (7 values)"),
    ("bad_number", lambda L: L[:13] + [L[13].replace(L[13].split()[3], "abc", 1)] + L[14:], 14, "match emissions of node 1"),
    ("nan", lambda L: L[:15] + [L[15].replace(L[15].split()[0], "nan", 1)] + L[16:], 16, "finite"),
    ("negative", lambda L: L[:15] + [L[15].replace(L[15].split()[0], "-0.5", 1)] + L[16:], 34, "probabilities"),
    ("no_end", lambda L: L[:34] + ["HMMER3/f"] + L[35:], 35, "`//` after node 7"),
    ("truncated", lambda L: L[:20], 21, "file ends where the insert line of node 3"),
    ("truncated_header", lambda L: L[:5], 6, "file ends where the `HMM` line"),
    ("end_in_header", lambda L: L[:5] + ["//"], 6, "`HMM` line before the end"),
    ("empty", lambda L: [], 1, "holds none"),
])
def test_read_hmm_malformed(tmp_path, profs, name, edit, line, expected):
    L = _lines(profs)
    assert L[12].split()[0] != "COMPO" and L[10].split()[0] == "COMPO" and L[13].split()[0] == "1" and L[34] == "//"
    p = tmp_path / (name + ".hmm")
    p.write_text("\n".join(edit(L)))
    with pytest.raises(ValueError) as e:
        dm.read_hmm(str(p))
    msg = str(e.value)
    assert msg.startswith("%s:%d:" % (p, line)) and expected in msg, msg


# ------------------------------------------------------------------------------------------------ names
def test_names_are_the_references(golden_dom):
    for name, (gene, clade) in golden_dom["names"].items():
        g, c, d, full = dm.parse_name(name)
        assert (g, c) == (gene, clade) and full == name.split(":")[0]
        assert d == {"aRH": "RH", "TPase": "INT"}.get(gene.split("-")[1], gene.split("-")[1])
    assert dm.parse_name("Class_I/LTR/Ty3_gypsy/chromovirus/Tekay:Ty3-RT") == ("Ty3-RT", "Tekay", "RT", "Class_I/LTR/Ty3_gypsy/chromovirus/Tekay")
    assert dm.parse_name("Class_I/LTR/Ty3_gypsy/chromovirus/CRM:Ty3-aRH")[2] == "RH" and dm.parse_name("Class_II/Subclass_1/TIR/hAT:hAT-TPase")[2] == "INT"
    assert dm.parse_name("PF00078") == ("PF00078",) * 4
    assert dm.format_gff_id("a|b;c=d:1-2") == "a_b_c_d:1-2"


# ------------------------------------------------------------------------------------------------ hits
def _profiles(names, Ms):
    return dm.Profiles(names, [np.zeros((M, 22)) for M in Ms], [np.zeros((M, 7)) for M in Ms])


def test_the_best_profile_per_domain_and_the_filters():
    P = _profiles(["x/Ale:Ty1-RT", "x/Ivana:Ty1-RT", "x/Tork:Ty1-RT", "x/Ale:Ty1-INT", "x/CRM:Ty3-aRH", "x/CRM:Ty3-RH"], [10, 20, 30, 11, 8, 16])
    ids, n = ["chr1:1000-2000:1100-1900"], [800]
    none = [-(1 << 31), 0, 0, 0, 0, 0]
    # RT: 2000 / 10 = 200 per node against 4100 / 20 = 205 and 6150 / 30 = 205: the second wins, the third ties and loses
    hits = np.array([[[2000, 0, 0, 9, 1, 10], [4100, 1, 5, 24, 1, 20], [6150, 2, 7, 36, 1, 30], none, none, none]], np.int32)
    d = dm.best_domains(ids, n, hits, P)
    assert [(x.profile, x.gene, x.clade, x.raw) for x in d] == [("x/Ivana:Ty1-RT", "RT", "Ivana", 4100)]
    assert d[0].score == 0.8 and d[0].coverage == 100.0 and (d[0].start, d[0].end, d[0].strand, d[0].frame) == (1016, 1075, "+", 1)
    hits[0, 2, 0] = 6151                                   # 6151 * 20 > 4100 * 30
    assert dm.best_domains(ids, n, hits, P)[0].profile == "x/Tork:Ty1-RT"
    # aRH counts as RH: one line for the two
    hits[0, 4], hits[0, 5] = [1100, 3, 0, 7, 1, 8], [2100, 3, 0, 15, 1, 16]
    assert sorted(x.profile for x in dm.best_domains(ids, n, hits, P)) == ["x/CRM:Ty3-aRH", "x/Tork:Ty1-RT"]
    # coverage exactly at 20 %: 2 of 10 nodes pass, 2 of 11 do not, and the threshold moves with the option
    hits[:] = none
    hits[0, 0], hits[0, 3] = [5000, 0, 0, 1, 4, 5], [5000, 0, 0, 1, 4, 5]
    assert [x.profile for x in dm.best_domains(ids, n, hits, P)] == ["x/Ale:Ty1-RT"]
    assert len(dm.best_domains(ids, n, hits, P, min_cov=18.0)) == 2 and len(dm.best_domains(ids, n, hits, P, min_cov=20.1)) == 0
    # score exactly at 0.5 bit per node: 1280 of 10 nodes passes, 1279 does not
    hits[0, 0], hits[0, 3] = [1280, 0, 0, 9, 1, 10], [1407, 0, 0, 9, 1, 11]
    assert [x.profile for x in dm.best_domains(ids, n, hits, P)] == ["x/Ale:Ty1-RT"]
    hits[0, 0, 0], hits[0, 3, 0] = 1279, 1408
    assert [x.profile for x in dm.best_domains(ids, n, hits, P)] == ["x/Ale:Ty1-INT"]
    assert len(dm.best_domains(ids, n, hits, P, min_score=0.499)) == 2


def test_coordinates_on_both_strands():
    eid = "chr1:1000-2000:1100-1900"
    assert dm.coordinates(eid, 1, 2, 4, 100) == ("chr1", 999 + 8, 999 + 16, "+", 1)
    assert dm.coordinates(eid, 0, 0, 0, 100) == ("chr1", 1000, 1002, "+", 0)
    assert dm.coordinates(eid, 4, 2, 4, 100) == ("chr1", 999 + 85, 999 + 93, "-", 1)
    assert dm.coordinates(eid, 3, 0, 0, 100) == ("chr1", 999 + 98, 999 + 100, "-", 0)
    assert dm.coordinates("elem", 5, 0, 1, 9) == ("elem", 2, 7, "-", 2)           # no coordinates in the id: relative to the sequence
    # the bases the coordinates name translate to the residues of the hit, on either strand
    seq = dr.rand_dna(random.Random(2), 100)
    for f in range(6):
        _, a, b, strand, fr = dm.coordinates("elem", f, 2, 4, 100)
        cut = seq[a - 1:b] if strand == "+" else dr.revcomp(seq[a - 1:b])
        assert fr == f % 3 and dr.translate(cut, 0) == dr.translate(seq, f)[2:5]


# ------------------------------------------------------------------------------------------------ the classifier
def _golden_domains(golden_dom):
    out = []
    for line in golden_dom["gff"].splitlines():
        f = line.split("\t")
        at = dict(kv.split("=", 1) for kv in f[8].split(";"))
        d = dm.Domain()
        d.element, d.profile = "|".join(at["ID"].split("|")[:-1]), at["ID"].split("|")[-1]
        _, d.clade, d.gene, d.full = dm.parse_name(d.profile)
        d.seqid, d.start, d.end, d.score, d.strand, d.frame, d.coverage, d.raw = f[0], int(f[3]), int(f[4]), float(f[5]), f[6], int(f[7]), 90.0, 0
        assert (d.gene, d.clade) == (at["gene"], at["clade"])
        out.append(d)
    return out


def test_the_classifier_is_the_references(golden_dom):
    doms = _golden_domains(golden_dom)
    rows = dm.classify(doms)
    assert len(rows) == len(golden_dom["cases"]) == 27
    for case, got, want in zip(golden_dom["cases"], rows, golden_dom["rows"]):
        assert got == want, case
    out = io.StringIO()
    dm.write_cls(out, rows)
    assert out.getvalue() == golden_dom["cls_text"]
    res = {c: r for c, r in zip(golden_dom["cases"], rows)}
    assert res["majority_second"][3] == "mixture" and res["majority"][3] == "Ale"          # the insertion-order quirk
    assert res["minus_strand"][4:6] == ["yes", "-"] and res["mixed_strands"][5] == "?" and res["ty_clade"][3] == "unknown"
    assert dm.parse_rexdb("PF00078") == ("Unknown", "unknown")


def test_gff_lines(golden_dom):
    doms = _golden_domains(golden_dom)[:3]
    out = io.StringIO()
    dm.write_gff(out, doms)
    lines = out.getvalue().splitlines()
    assert len(lines) == 3
    f = lines[0].split("\t")
    assert len(f) == 9 and f[:5] == ["chr0", "subphaser_amd", "CDS", "400", "800"] and f[6:8] == ["+", "0"]
    assert f[8] == "ID=chr0:100-9000:300-8700|Class_I/LTR/Ty1_copia/Ale:Ty1-GAG;Name=Ale-GAG;gene=GAG;clade=Ale;coverage=90.0;score=1.5"
    # what the reference's reader takes from such a line is what went in
    at = dict(kv.split("=", 1) for kv in f[8].split(";"))
    assert "|".join(at["ID"].split("|")[:-1]) == doms[0].element and at["ID"].split("|")[-1].split(":")[0] == doms[0].full


def test_inner_interval_is_get_int_seqs(golden_dom, tmp_path):
    p = tmp_path / "x.scn"
    p.write_text("".join(r["line"] + "\n" for r in golden_dom["inner"]))
    for rec, want in zip(ltr.read_scn(str(p)), golden_dom["inner"]):
        a, b = dm.inner_interval(rec)
        assert rec.id == want["id"] and (a, b - 1, b - a) == (want["first"], want["last"], want["length"])


def test_a_complete_element_beats_an_overlapping_incomplete_one(golden_dom, tmp_path):
    """group_resolve_overlaps with the keys of the complete records: the reference's rows"""
    lines, done = [], []
    for start, length, complete in golden_dom["overlaps"]["records"]:
        end = start + length - 1
        lines.append(" ".join(map(str, [start, end, length, start, start + 99, 100, end - 99, end, 100, 90.0, 0, "chrA"])))
        done.append(complete)
    p = tmp_path / "o.scn"
    p.write_text("\n".join(lines) + "\n")
    recs = ltr.read_scn(str(p))
    completed = {r.key for r, c in zip(recs, done) if c}
    assert [r.id for r in ltr.group_resolve_overlaps(recs, completed)] == golden_dom["overlaps"]["kept"]
    assert [r.id for r in ltr.group_resolve_overlaps(recs)] != golden_dom["overlaps"]["kept"]          # the rule matters on these records
    assert [r.id for r in ltr.group_resolve_overlaps(recs, set())] == [r.id for r in ltr.group_resolve_overlaps(recs)]
