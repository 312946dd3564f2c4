"""Pipeline.stage_ltr under -ltr_hmm without a GPU: the oracle context of test_pipeline_ltrtree.py with the twin
(tests/domains_ref.py) behind dom_search.  The filter with and without -all_ltr, -intact_ltr, the two files and their
checkpoints, the Clade column of `.ltr.tree.map`, the error without the entry, the closing note, and that nothing changes
while the flag is off."""
import logging
import os
import random
import re

import numpy as np
import pytest

import domains_ref as dr
from test_pipeline_ltrdetect import LABELS, _run, with_ctx  # noqa: F401  (fixture)
from test_pipeline_ltrdetect import D_SG, K, _pipe
from test_pipeline_ltrtree import _TreeCtx
from subphaser_amd import domains, pipeline, seqs

COPIA = ["Class_I/LTR/Ty1_copia/Ale:Ty1-%s" % g for g in ("GAG", "PROT", "INT", "RT", "RH")]
GYPSY = ["Class_I/LTR/Ty3_gypsy/chromovirus/Tekay:Ty3-%s" % g for g in ("GAG", "PROT", "RT", "RH", "INT")]
M = 40


class _DomCtx(_TreeCtx):
    memo = {}
    profs = None      # the twin's tables of the file the run reads: the world sets them

    def dom_search(self, chrom, start, end, moff, emis, trans, entry):
        self.calls.append(("dom", len(chrom), len(entry)))
        assert [p["M"] for p in self.profs] == np.diff(moff).tolist()
        for p, a, b in zip(self.profs, moff[:-1], moff[1:]):      # the reader's integers, not the generator's
            if not (p["emis"] == emis[a:b]).all() or not (p["trans"] == trans[a:b]).all():
                p["emis"], p["trans"] = np.array(emis[a:b]), np.array(trans[a:b])
                self.memo.clear()
        return dr.search([self._seq(c)[a:b] for c, a, b in zip(map(int, chrom), map(int, start), map(int, end))], self.profs, self.memo)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """four chromosomes of 12 kb with three elements each: a Copia-like one (five domains of clade Ale, forward), a decoy
    without domains, a Gypsy-like one (five domains of clade Tekay, on the reverse strand).  The 15-mers of the left LTRs
    are the subgenome-specific k-mers."""
    rng = random.Random(17)
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, M), name=n) for n in COPIA + GYPSY]
    cons = {p["name"]: "".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs}
    hmm = tmp_path_factory.mktemp("hmm") / "toy.hmm"
    hmm.write_text(dr.hmm_text(profs))
    chroms, d_kmers, scn, kinds = [], {}, [], {}
    for ci, lab in enumerate(LABELS):
        s, pos = "", 0
        for kind in ("copia", "decoy", "gypsy"):
            s += dr.rand_dna(rng, 700)
            ltr_ = dr.rand_dna(rng, 180)
            d_kmers.update({ltr_[i:i + K]: D_SG[lab] for i in range(len(ltr_) - K + 1)})
            if kind == "decoy":
                inner = dr.rand_dna(rng, 700)
            else:
                inner = dr.rand_dna(rng, 20) + "".join(dr.back_translate(rng, cons[n]) + dr.rand_dna(rng, 12) for n in (COPIA if kind == "copia" else GYPSY))
                if kind == "gypsy":
                    inner = dr.revcomp(inner)
            start = len(s) + 1
            s += ltr_ + inner + ltr_
            end = len(s)
            scn.append(" ".join(map(str, [start, end, end - start + 1, start, start + 179, 180, end - 179, end, 180, "100.00", ci, lab])))
            kinds["%s:%d-%d:%d-%d" % (lab, start, end, start + 179, end - 179)] = kind
        chroms.append(s + dr.rand_dna(rng, 12000 - len(s)))
    scn_file = hmm.parent / "toy.scn"
    scn_file.write_text("\n".join(scn) + "\n")
    kl = seqs.KmerLabels.from_dict(d_kmers, ["SG1", "SG2"], K)

    def make(cls):
        ctx = cls()
        ctx.genome_reset(len(LABELS))
        for i, s in enumerate(chroms):
            ctx.genome_add(i, s)
        ctx.k, ctx.calls = K, []
        if cls is _DomCtx:
            cls.profs = profs
        return ctx
    return chroms, kl, make, str(hmm), str(scn_file), kinds


def _dom_run(tmp, world, caplog, with_ctx, cls=_DomCtx, **over):
    opts = dict(ltr_denovo=False, ltr_scn=world[4], ltr_hmm=world[3])
    opts.update(over)
    p, lay = _pipe(tmp, **opts)
    ctx = world[2](cls)
    log = _run(p, lay, world, ctx, caplog, with_ctx)
    for _, _, done in p._background:
        done()
    return p, lay, ctx, log


def _cls_rows(lay):
    rows = [r.split("\t") for r in open(lay.out("ltr.cls.tsv")).read().splitlines()]
    assert rows[0] == ["#TE", "Order", "Superfamily", "Clade", "Complete", "Strand", "Domains"]
    return rows[1:]


def _ids(lay, ext):
    return [r.split("\t")[0] for r in open(lay.out(ext)).read().splitlines()[1:]]


def test_classification_filters_the_decoys(tmp_path, world, caplog, with_ctx):
    kinds = world[5]
    p, lay, ctx, log = _dom_run(tmp_path / "hmm", world, caplog, with_ctx)
    for ext in ("ltr.dom.gff3", "ltr.cls.tsv"):
        assert os.path.exists(lay.out(ext)) and os.path.exists(lay.ckp(lay.out(ext))), ext
    rows = _cls_rows(lay)
    good = sorted(i for i, k in kinds.items() if k != "decoy")
    assert sorted(r[0] for r in rows) == good and len(good) == 8
    for r in rows:
        if kinds[r[0]] == "copia":
            assert r[1:6] == ["LTR", "Copia", "Ale", "yes", "+"] and r[6] == "GAG|Ale PROT|Ale INT|Ale RT|Ale RH|Ale"
        else:
            assert r[1:6] == ["LTR", "Gypsy", "Tekay", "yes", "-"] and r[6] == "GAG|Tekay PROT|Tekay RT|Tekay RH|Tekay INT|Tekay"
    gff = [line.split("\t") for line in open(lay.out("ltr.dom.gff3")).read().splitlines()]
    assert len(gff) == 40 and all(len(f) == 9 and f[1:3] == ["subphaser_amd", "CDS"] for f in gff)
    assert gff == sorted(gff, key=lambda f: (f[0], f[8].split(";")[0][3:].rsplit("|", 1)[0], int(f[3])))
    assert all(float(f[5]) > 2.0 and "coverage=100.0" in f[8] for f in gff)
    assert ("dom", 12, 10) in ctx.calls and sum(c[0] == "dom" for c in ctx.calls) == 1
    assert "12 LTRs read from `%s`" % world[4] in log and "10 profiles of 40-40 nodes read from `%s`" % world[3] in log
    assert "By the device domain search, 8 (66.7%) are classified as LTRs, of which 8 (100.0%) are intact with complete protein domains" in log
    assert "After filtering, 8 / 12 (66.7%) LTRs retained" in log
    assert not any("no classification" in m for m in log)
    assert sorted(_ids(lay, "ltr.identity.tsv")) == good and set(_ids(lay, "ltr.bin.count")) <= set(good)


def test_all_ltr_keeps_them_and_intact_ltr_changes_nothing(tmp_path, world, caplog, with_ctx):
    kinds = world[5]
    p0, lay0, _, log0 = _dom_run(tmp_path / "plain", world, caplog, with_ctx)
    p, lay, ctx, log = _dom_run(tmp_path / "all", world, caplog, with_ctx, all_ltr=True)
    assert "After filtering, 12 / 12 (100.0%) LTRs retained" in log and sorted(_ids(lay, "ltr.identity.tsv")) == sorted(kinds)
    assert open(lay.out("ltr.cls.tsv")).read() == open(lay0.out("ltr.cls.tsv")).read()
    assert "By the device domain search, 8 (66.7%) are classified as LTRs, of which 8 (100.0%) are intact with complete protein domains" in log
    p2, lay2, _, log2 = _dom_run(tmp_path / "intact", world, caplog, with_ctx, intact_ltr=True, tesorter_options="-db rexdb-plant")
    assert sum(m.startswith("-intact_ltr changes nothing, as in the reference") for m in log2) == 1
    assert sum(m.startswith("-tesorter_options -db rexdb-plant: TEsorter is not run") for m in log2) == 1
    for ext in ("ltr.cls.tsv", "ltr.dom.gff3", "ltr.identity.tsv", "ltr.enrich", "ltr.insert.data"):
        assert open(lay2.out(ext)).read() == open(lay0.out(ext)).read(), ext
    # thresholds nothing reaches: no domain, no LTR, and the zero counts are guarded
    p3, lay3, _, log3 = _dom_run(tmp_path / "strict", world, caplog, with_ctx, ltr_dom_score=50.0)
    assert _cls_rows(lay3) == [] and open(lay3.out("ltr.dom.gff3")).read() == ""
    assert "By the device domain search, 0 (0.0%) are classified as LTRs, of which 0 (0.0%) are intact with complete protein domains" in log3
    assert "After filtering, 0 / 12 (0.0%) LTRs retained" in log3


def test_tree_map_has_the_clades(tmp_path, world, caplog, with_ctx):
    kinds = world[5]
    p, lay, ctx, log = _dom_run(tmp_path / "tree", world, caplog, with_ctx, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64)
    rows = [r.split("\t") for r in open(lay.out("ltr.tree.map")).read().splitlines()]
    assert rows[0] == ["label", "Clade", "Subgenome"] and len(rows) >= 5
    assert [r[1] for r in rows[1:]] == [{"copia": "Ale", "gypsy": "Tekay"}[kinds[r[0]]] for r in rows[1:]]
    assert {r[1] for r in rows[1:]} == {"Ale", "Tekay"}
    assert any(m.endswith("(midpoint-rooted; one tree; the Clade column is the domain classification's)") for m in log)
    # under -all_ltr a decoy in the tree is `unknown`
    p2, lay2, _, _ = _dom_run(tmp_path / "tree_all", world, caplog, with_ctx, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64, all_ltr=True)
    rows2 = [r.split("\t") for r in open(lay2.out("ltr.tree.map")).read().splitlines()[1:]]
    assert {r[1] for r in rows2 if kinds[r[0]] == "decoy"} == {"unknown"} and {r[1] for r in rows2} == {"Ale", "Tekay", "unknown"}


def test_long_inner_sequences_are_left_unclassified(tmp_path, world, caplog, with_ctx, monkeypatch):
    monkeypatch.setattr(domains, "MAX_LEN", 700)       # the decoys' inner sequences have 701 bases (get_int_seq ends on the right LTR's first base)
    p, lay, ctx, log = _dom_run(tmp_path / "long", world, caplog, with_ctx, all_ltr=True)
    assert "4 LTR-RTs with an inner sequence above 700 bases are left unclassified" in log and ("dom", 8, 10) in ctx.calls
    assert len(_cls_rows(lay)) == 8 and "After filtering, 12 / 12 (100.0%) LTRs retained" in log


def test_errors_come_before_anything_is_written(tmp_path, world, caplog, with_ctx):
    with pytest.raises(RuntimeError, match="-ltr_hmm needs a context with dom_search .*no CPU engine"):
        _dom_run(tmp_path / "none", world, caplog, with_ctx, cls=_TreeCtx)
    assert os.listdir(str(tmp_path / "none")) == []
    bad = tmp_path / "bad.hmm"
    bad.write_text("HMMER3/f\nNAME x\nLENG 3\nALPH amino\n//\n")
    with pytest.raises(ValueError, match=r"bad.hmm:5: expected the `HMM` line"):
        _dom_run(tmp_path / "bad", world, caplog, with_ctx, ltr_hmm=str(bad))
    assert os.listdir(str(tmp_path / "bad")) == []


def test_flag_off_changes_nothing(tmp_path, world, caplog, with_ctx):
    p, lay, ctx, log_today = _dom_run(tmp_path / "today", world, caplog, with_ctx, ltr_hmm=None, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64)
    p2, lay2, ctx2, log_off = _dom_run(tmp_path / "off", world, caplog, with_ctx, ltr_hmm=None, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64,
                                       ltr_dom_cov=55.0, ltr_dom_score=3.0, intact_ltr=True, tesorter_options="-db x", all_ltr=True)
    strip = lambda log, root: [re.sub(r"\d+\.\d+ s", "T s", m).replace(str(root), "") for m in log]
    assert strip(log_off, tmp_path / "off") == strip(log_today, tmp_path / "today")
    assert sorted(os.listdir(lay2.root)) == sorted(os.listdir(lay.root)) and not any("dom" in f or "cls" in f for f in os.listdir(lay.root))
    for f in os.listdir(lay.root):
        if not f.endswith((".ok", ".png")):
            assert open(os.path.join(lay.root, f)).read() == open(os.path.join(lay2.root, f)).read(), f
    assert not [c for c in ctx2.calls if c[0] == "dom"]
    # the lines of today, byte for byte
    assert "12 LTRs read from `%s`; no classification: every record is used, as under -all_ltr" % world[4] in log_today
    assert "After filtering, 12 / 12 (100.0%) LTRs retained" in log_today
    assert "LTR tree -> `run.ltr.tree.nwk` (midpoint-rooted; one tree, no clades: nothing is classified)" in log_today
    assert {r.split("\t")[1] for r in open(lay.out("ltr.tree.map")).read().splitlines()[1:]} == {"unknown"}


def test_closing_note(monkeypatch, caplog):
    def run(built, **flags):
        opts = dict(outdir="o", tmpdir="t", disable_circos=True, disable_blocks=True)
        opts.update(flags)
        p = pipeline.Pipeline.bare(**opts)

        class _C:
            d_sg, sg_names = {}, []
        monkeypatch.setattr(pipeline, "Layout", lambda *a: "lay")
        monkeypatch.setattr(p, "stage_ingest", lambda lay: (["f"], ["c"], {"c": 1}, {}), raising=False)
        monkeypatch.setattr(p, "stage_count_filter", lambda *a: None, raising=False)
        monkeypatch.setattr(p, "stage_cluster", lambda *a: (_C(), None), raising=False)
        monkeypatch.setattr(p, "stage_windows", lambda *a: None, raising=False)
        monkeypatch.setattr(p, "stage_ltr", lambda *a: setattr(p, "_ltr_tree_built", built), raising=False)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            p._run()
        return [r.getMessage() for r in caplog.records]
    assert run(False, ltr_scn="x.scn", ltr_hmm="r.hmm") == [
        "Of modules 3-4, LTR detection, the LTR trees and the circos figure are not part of this build; the classification is this "
        "build's own Viterbi domain search (-ltr_hmm), not TEsorter's hmmscan; run the reference on the outputs above for them"]
    assert run(True, ltr_denovo=True, ltr_tree=True, ltr_hmm="r.hmm") == [
        "Of modules 3-4, the circos figure is not part of this build; the classification is this build's own Viterbi domain search "
        "(-ltr_hmm), not TEsorter's hmmscan (the LTR-RTs are this build's own detection, not ltr_finder's or ltrharvest's); the tree of "
        "-ltr_tree is this build's own (sketches and neighbour joining), not the reference's domain trees; run the reference on the "
        "outputs above for it"]
    # without the flag: today's text
    assert run(False, ltr_scn="x.scn") == [
        "Of modules 3-4, LTR detection, TEsorter classification, the LTR trees and the circos figure are not "
        "part of this build; run the reference on the outputs above for them"]


def test_cli_options():
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config"])
    assert (args.ltr_hmm, args.ltr_dom_cov, args.ltr_dom_score) == (None, 20.0, 0.5)
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_denovo", "-ltr_hmm", "rexdb.hmm", "-ltr_dom_cov", "30", "-ltr_dom_score", "1.5"])
    assert (args.ltr_hmm, args.ltr_dom_cov, args.ltr_dom_score) == ("rexdb.hmm", 30.0, 1.5)
    assert pipeline.option_defaults()["ltr_hmm"] is None and pipeline.Pipeline.ltr_dom_cov == 20.0
