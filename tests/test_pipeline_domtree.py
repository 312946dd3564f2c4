"""Pipeline.stage_ltr under -ltr_domtree without a GPU: the context of test_pipeline_domains.py with the twins
(tests/domalign_ref.py) behind dom_align, dom_peptide and aln_pairs, on a world enlarged to two planted families per
superfamily.  Every file and checkpoint, each planted family as one clade of its tree, fewer than 4 rows, -ltr_domains RT
alone, -disable_ltrtree, the command-line error without -ltr_hmm, the error without the entries, the closing note, and that
nothing changes while the flag is off."""
import logging
import os
import random
import re

import numpy as np
import pytest

import domalign_ref as da
import domains_ref as dr
from test_pipeline_domains import COPIA, GYPSY, M, _DomCtx, _dom_run
from test_pipeline_ltrdetect import D_SG, K, LABELS, with_ctx  # noqa: F401  (fixture)
from subphaser_amd import domtree, ltrtree, pipeline, seqs

FAMILIES = ("copiaA", "copiaB", "gypsyA", "gypsyB")
TREE_EXT = ("aln", "map", "aln.trimmed", "aln.rooted.tre")


class _DomTreeCtx(_DomCtx):
    trees = None

    def _items(self, chrom, start, end, frame, i0, i1):
        seqs_ = [self._seq(c)[a:b] for c, a, b in zip(map(int, chrom), map(int, start), map(int, end))]
        return seqs_, [(q, int(f), int(x), int(y)) for q, (f, x, y) in enumerate(zip(frame, i0, i1))]

    def dom_align(self, chrom, start, end, frame, i0, i1, prof, moff, emis, trans, entry):
        self.calls.append(("dom_align", len(chrom)))
        assert [p["M"] for p in self.profs] == np.diff(moff).tolist() and all((p["emis"] == emis[a:b]).all() for p, a, b in zip(self.profs, moff[:-1], moff[1:]))
        seqs_, items = self._items(chrom, start, end, frame, i0, i1)
        return da.align_items(seqs_, [it + (int(p),) for it, p in zip(items, prof)], self.profs)

    def dom_peptide(self, chrom, start, end, frame, i0, i1):
        self.calls.append(("dom_peptide", len(chrom)))
        seqs_, items = self._items(chrom, start, end, frame, i0, i1)
        pep = [da.window_residues(seqs_[q], f, x, y) for q, f, x, y in items]
        return np.array([c for p in pep for c in p], np.uint8), np.concatenate(([0], np.cumsum([len(p) for p in pep]))).astype(np.int64)

    def aln_pairs(self, rows):
        self.calls.append(("aln_pairs",) + tuple(rows.shape))
        return da.aln_pairs(rows)

    def nj_tree(self, dist):
        rec = super().nj_tree(dist)
        self.trees.append(np.array(rec))
        return rec


def _variant(rng, protein, rate):
    return "".join(rng.choice([a for a in dr.AA if a != c]) if rng.random() < rate else c for c in protein)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """four chromosomes of 12 kb with four elements each: one of each of two Copia-like families (clade Ale, forward) and of two
    Gypsy-like families (clade Tekay, reverse strand).  A family is the consensus of the five profiles with a quarter of the
    residues substituted, the same in all its members; a member adds two substitutions of its own per domain.  The 15-mers of
    the left LTRs are the subgenome-specific k-mers: 8 Copia and 8 Gypsy elements, 4 per family."""
    rng = random.Random(23)
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, M), name=n) for n in COPIA + GYPSY]
    cons = {p["name"]: "".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs}
    hmm = tmp_path_factory.mktemp("domtree") / "toy.hmm"
    hmm.write_text(dr.hmm_text(profs))
    fam = {f: {n: _variant(rng, cons[n], 0.25) for n in (COPIA if f.startswith("copia") else GYPSY)} for f in FAMILIES}
    chroms, d_kmers, scn, kinds = [], {}, [], {}
    for ci, lab in enumerate(LABELS):
        s = ""
        for f in FAMILIES:
            s += dr.rand_dna(rng, 700)
            ltr_ = dr.rand_dna(rng, 180)
            d_kmers.update({ltr_[i:i + K]: D_SG[lab] for i in range(len(ltr_) - K + 1)})
            names = COPIA if f.startswith("copia") else GYPSY
            member = {}
            for n in names:
                p = list(fam[f][n])
                for at in rng.sample(range(M), 2):
                    p[at] = rng.choice([a for a in dr.AA if a != p[at]])
                member[n] = "".join(p)
            inner = dr.rand_dna(rng, 20) + "".join(dr.back_translate(rng, member[n]) + dr.rand_dna(rng, 12) for n in names)
            if f.startswith("gypsy"):
                inner = dr.revcomp(inner)
            start = len(s) + 1
            s += ltr_ + inner + ltr_
            end = len(s)
            scn.append(" ".join(map(str, [start, end, end - start + 1, start, start + 179, 180, end - 179, end, 180, "100.00", ci, lab])))
            kinds["%s:%d-%d:%d-%d" % (lab, start, end, start + 179, end - 179)] = f
        chroms.append(s + dr.rand_dna(rng, 12000 - len(s)))
    scn_file = hmm.parent / "toy.scn"
    scn_file.write_text("\n".join(scn) + "\n")
    kl = seqs.KmerLabels.from_dict(d_kmers, ["SG1", "SG2"], K)

    def make(cls):
        ctx = cls()
        ctx.genome_reset(len(LABELS))
        for i, s in enumerate(chroms):
            ctx.genome_add(i, s)
        ctx.k, ctx.calls, ctx.trees = K, [], []
        if issubclass(cls, _DomCtx):
            _DomCtx.profs = profs
            _DomCtx.memo.clear()
        return ctx
    return chroms, kl, make, str(hmm), str(scn_file), kinds


def _tree_run(tmp, world, caplog, with_ctx, cls=_DomTreeCtx, **over):
    opts = dict(ltr_domtree=True, subsample=1000, bootstrap_seed=None)
    opts.update(over)
    return _dom_run(tmp, world, caplog, with_ctx, cls=cls, **opts)


def _fasta(path):
    recs = open(path).read().split(">")[1:]
    return [(r.split("\n")[0], r.split("\n")[1]) for r in recs]


def _label(eid):
    return domtree.format_id_for_iqtree(eid)


def test_every_file_and_each_family_a_clade(tmp_path, world, caplog, with_ctx):
    kinds = world[5]
    p, lay, ctx, log = _tree_run(tmp_path / "on", world, caplog, with_ctx)
    listed = [r.split("\t")[0] for r in open(lay.out("ltr.insert.data")).read().splitlines()[1:]]
    assert sorted(listed) == sorted(kinds) and len(listed) == 16
    # `.ltr.cls.pep`: one record per line of the gff, in its order, the peptide of the hit
    gff = [line.split("\t") for line in open(lay.out("ltr.dom.gff3")).read().splitlines()]
    pep = _fasta(lay.out("ltr.cls.pep"))
    assert os.path.exists(lay.ckp(lay.out("ltr.cls.pep"))) and len(pep) == len(gff) == 80
    for (head, seq), f in zip(pep, gff):
        rid, cid, did = re.match(r"^(\S+)#(\S+)#(\S+)$", head.split()[0]).groups()
        assert kinds[rid].startswith("copia") == (cid == "LTR/Copia/Ale") and cid in ("LTR/Copia/Ale", "LTR/Gypsy/Tekay")
        assert head.split(" ", 1)[1] == f[8] and did == re.search(r"gene=([^;\s]+)", f[8]).group(1) + "|" + re.search(r"clade=([^;\s]+)", f[8]).group(1)
        assert 8 <= len(seq) <= 60 and set(seq) <= set(dr.AA)      # (a local hit of 20 % of the nodes at least; it may hold inserted residues)
    for sf, fams in (("Copia", FAMILIES[:2]), ("Gypsy", FAMILIES[2:])):
        base = "ltr.LTR_%s." % sf
        for ext in TREE_EXT:
            assert os.path.exists(lay.out(base + ext)) and os.path.exists(lay.ckp(lay.out(base + ext))), (sf, ext)
        assert os.path.exists(lay.out(base + "tree.png"))
        members = [i for i in listed if kinds[i] in fams]
        rows = [r.split("\t") for r in open(lay.out(base + "map")).read().splitlines()]
        assert rows[0] == ["label", "Clade", "Subgenome"]
        assert [r[0] for r in rows[1:]] == [_label(i) for i in members]
        assert {r[1] for r in rows[1:]} == {"Ale" if sf == "Copia" else "Tekay"}
        assert [r[2] for r in rows[1:]] == [D_SG[i.split(":")[0]] for i in members]
        aln, trimmed = _fasta(lay.out(base + "aln")), _fasta(lay.out(base + "aln.trimmed"))
        assert [h for h, _ in aln] == ["%s genes:3 sites:120 blocks:[40, 40, 40]" % _label(i) for i in members] == [h for h, _ in trimmed]
        assert all(len(s) == 120 and set(s) <= set(dr.AA + "-") for _, s in aln) and len({s for _, s in aln}) == 8
        assert [s for _, s in trimmed] == domtree.trim([s for _, s in aln], 50)
        # the rows are the members' own peptides on the common profile's nodes: the first block is INT
        by_id = {}
        for (head, seq), f in zip(pep, gff):
            by_id.setdefault(head.split("#")[0], {})[re.search(r"gene=([^;\s]+)", f[8]).group(1)] = seq
        for (h, s), i in zip(aln, members):
            # the common profile is every member's own winner and the window holds its hit: a block is the hit's peptide on its
            # nodes -- its residues in order, without the inserted ones
            for q, d in enumerate(("INT", "RT", "RH")):
                block, rest = s[40 * q:40 * q + 40].replace("-", ""), iter(by_id[i][d])
                assert len(block) >= 8 and all(c in rest for c in block), (i, d, block, by_id[i][d])
        # each planted family is one clade
        rec = ctx.trees[0 if sf == "Copia" else 1]
        splits = set(ltrtree.splits(ltrtree.unrooted_edges(rec), 8))
        for fam in fams:
            leaves = frozenset(q for q, i in enumerate(members) if kinds[i] == fam)
            assert len(leaves) == 4 and (leaves in splits or frozenset(range(8)) - leaves in splits), (fam, sorted(map(sorted, splits)))
        tre = open(lay.out(base + "aln.rooted.tre")).read()
        assert tre == ltrtree.tree_text(rec, [_label(i) for i in members]) + "\n" and tre.count(",") == 7
    widths = [len(_fasta(lay.out("ltr.LTR_%s.aln.trimmed" % sf))[0][1]) for sf in ("Copia", "Gypsy")]
    assert all(100 <= w <= 120 for w in widths)
    assert [c for c in ctx.calls if c[0] in ("dom_align", "aln_pairs", "nj")] == [x for w in widths for x in (("dom_align", 24), ("aln_pairs", 8, w), ("nj", 8))]
    for line in ("Extracting and aligning protein domain sequences of LTR/Copia", "8 sequences contain INT domains",
                 "8 sequences contain all ['INT', 'RT', 'RH'] domains", "8 (100.0%) unique alignments retained"):
        assert log.count(line) == (2 if "Copia" not in line else 1), line
    assert p._ltr_domtrees_built == ("Copia", "Gypsy")      # (the closing note is _run's: test_closing_note)


def test_fewer_than_four_rows_give_no_tree(tmp_path, world, caplog, with_ctx):
    p, lay, ctx, log = _tree_run(tmp_path / "few", world, caplog, with_ctx, subsample=3)
    assert log.count("Subsample 3 / 8 (37.50%)") == 2
    assert "LTR_Copia: 3 aligned rows, fewer than 4: no tree" in log and "LTR_Gypsy: 3 aligned rows, fewer than 4: no tree" in log
    for sf in ("Copia", "Gypsy"):
        assert len(_fasta(lay.out("ltr.LTR_%s.aln" % sf))) == 3 and len(open(lay.out("ltr.LTR_%s.map" % sf)).read().splitlines()) == 4
        assert not os.path.exists(lay.out("ltr.LTR_%s.aln.trimmed" % sf)) and not os.path.exists(lay.out("ltr.LTR_%s.aln.rooted.tre" % sf))
    assert not [c for c in ctx.calls if c[0] in ("aln_pairs", "nj")] and p._ltr_domtrees_built == ()
    # a domain nothing has: nothing is selected, the files are empty but for the map's header
    p2, lay2, ctx2, log2 = _tree_run(tmp_path / "none", world, caplog, with_ctx, ltr_domains=["RT", "CHD"])
    assert "0 sequences contain CHD domains" in log2 and "0 sequences contain all ['RT', 'CHD'] domains" in log2
    assert open(lay2.out("ltr.LTR_Copia.aln")).read() == "" and not [c for c in ctx2.calls if c[0] == "dom_align"]


def test_ltr_domains_rt_alone(tmp_path, world, caplog, with_ctx):
    p, lay, ctx, log = _tree_run(tmp_path / "rt", world, caplog, with_ctx, ltr_domains=["RT"], trimal_options="-gt 0.5")
    aln = _fasta(lay.out("ltr.LTR_Gypsy.aln"))
    assert len(aln) == 8 and all(h.endswith(" genes:1 sites:40 blocks:[40]") and len(s) == 40 for h, s in aln)
    assert ("dom_align", 8) in ctx.calls and ("aln_pairs", 8, 40) in ctx.calls and p._ltr_domtrees_built == ("Copia", "Gypsy")
    assert sum(m.startswith("-trimal_options -gt 0.5: trimal is not run") for m in log) == 1


def test_disable_ltrtree_wins(tmp_path, world, caplog, with_ctx):
    p, lay, ctx, log = _tree_run(tmp_path / "off", world, caplog, with_ctx, disable_ltrtree=True)
    assert "-disable_ltrtree: the domain trees of -ltr_domtree are not built" in log
    assert not any("LTR_" in f or "cls.pep" in f for f in os.listdir(lay.root)) and not [c for c in ctx.calls if c[0].startswith(("dom_", "aln_"))]


def test_errors_come_before_anything_is_written(tmp_path, world, caplog, with_ctx):
    with pytest.raises(SystemExit):
        pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_scn", "x.scn", "-ltr_domtree"])
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_scn", "x.scn", "-ltr_domtree", "-ltr_hmm", "r.hmm", "-ltr_tree_occupancy", "60"])
    assert args.ltr_domtree and (args.ltr_tree_occupancy, args.ltr_tree_overlap) == (60, 20)
    assert pipeline.option_defaults()["ltr_domtree"] is False and pipeline.Pipeline.ltr_tree_occupancy == 50
    with pytest.raises(ValueError, match="-ltr_domtree builds its trees from the domains of the classification"):
        _tree_run(tmp_path / "nohmm", world, caplog, with_ctx, ltr_hmm=None)
    assert os.listdir(str(tmp_path / "nohmm")) == []
    with pytest.raises(RuntimeError, match="-ltr_domtree needs a context with dom_align, dom_peptide, aln_pairs and nj_tree .*no CPU engine"):
        _tree_run(tmp_path / "none", world, caplog, with_ctx, cls=_DomCtx)
    assert os.listdir(str(tmp_path / "none")) == []


def test_flag_off_changes_nothing(tmp_path, world, caplog, with_ctx):
    """the files of a run without the flag are those of a run with it (the new ones apart), byte for byte, and the options
    that belong to the flag change neither a file nor a log line while it is off"""
    p1, lay1, ctx1, log_on = _tree_run(tmp_path / "on", world, caplog, with_ctx, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64)
    p0, lay0, ctx0, log_off = _tree_run(tmp_path / "off", world, caplog, with_ctx, ltr_domtree=False, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64)
    p2, lay2, ctx2, log_off2 = _tree_run(tmp_path / "off2", world, caplog, with_ctx, ltr_domtree=False, ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64,
                                         ltr_tree_occupancy=90, ltr_tree_overlap=3, ltr_domains=["RT"])
    strip = lambda log, root: [re.sub(r"\d+\.\d+ s", "T s", m).replace(str(root), "") for m in log]
    new = lambda f: "LTR_" in f or "cls.pep" in f
    assert sorted(os.listdir(lay0.root)) == sorted(f for f in os.listdir(lay1.root) if not new(f)) and any(new(f) for f in os.listdir(lay1.root))
    for f in os.listdir(lay0.root):
        if not f.endswith((".ok", ".png")):
            assert open(os.path.join(lay0.root, f)).read() == open(os.path.join(lay1.root, f)).read(), f
    assert not [c for c in ctx0.calls if c[0].startswith(("dom_align", "dom_peptide", "aln_"))]
    # off, with the flag's options set: the same lines but for -ltr_tree's own warning about -ltr_domains
    assert [m for m in strip(log_off2, tmp_path / "off2") if not m.startswith("-ltr_domains")] == strip(log_off, tmp_path / "off")
    # on: the lines of a run without the flag are all there, in order
    on = strip(log_on, tmp_path / "on")
    it = iter(on)
    assert all(m in it for m in strip(log_off, tmp_path / "off"))


def test_closing_note(monkeypatch, caplog):
    def run(built, dom, **flags):
        opts = dict(outdir="o", tmpdir="t", disable_circos=True, disable_blocks=True)
        opts.update(flags)
        p = pipeline.Pipeline.bare(**opts)

        class _C:
            d_sg, sg_names = {}, []

        def stage(*a):
            p._ltr_tree_built, p._ltr_domtrees_built = built, dom
        monkeypatch.setattr(pipeline, "Layout", lambda *a: "lay")
        monkeypatch.setattr(p, "stage_ingest", lambda lay: (["f"], ["c"], {"c": 1}, {}), raising=False)
        monkeypatch.setattr(p, "stage_count_filter", lambda *a: None, raising=False)
        monkeypatch.setattr(p, "stage_cluster", lambda *a: (_C(), None), raising=False)
        monkeypatch.setattr(p, "stage_windows", lambda *a: None, raising=False)
        monkeypatch.setattr(p, "stage_ltr", stage, raising=False)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            p._run()
        return [r.getMessage() for r in caplog.records]
    assert run(False, ("Copia", "Gypsy"), ltr_scn="x.scn", ltr_hmm="r.hmm", ltr_domtree=True) == [
        "Of modules 3-4, LTR detection and the circos figure are not part of this build; the classification is this build's own Viterbi "
        "domain search (-ltr_hmm), not TEsorter's hmmscan; the domain trees of -ltr_domtree (Copia, Gypsy) are built and are this build's own "
        "(profile alignment, Kimura distances, neighbour joining), not mafft / trimal / iqtree trees; run the reference on the outputs above "
        "for them"]
    # no domain tree was built: the text of a run without the flag
    assert run(False, (), ltr_scn="x.scn", ltr_hmm="r.hmm", ltr_domtree=True) == [
        "Of modules 3-4, LTR detection, the LTR trees and the circos figure are not part of this build; the classification is this "
        "build's own Viterbi domain search (-ltr_hmm), not TEsorter's hmmscan; run the reference on the outputs above for them"]


def test_map_lists_the_elements_left_out_for_their_window(tmp_path, world, caplog, with_ctx, monkeypatch):
    """an element whose window is above the limit is in no alignment, but `.map` lists every selected element, as the
    reference's does (the limit is lowered: the world's windows have about 100 residues)"""
    monkeypatch.setattr(domtree, "MAX_WIN", 103)
    p, lay, ctx, log = _tree_run(tmp_path / "win", world, caplog, with_ctx)
    n_out = 0
    for sf in ("Copia", "Gypsy"):
        left = [int(m.split()[1]) for m in log if m.startswith("LTR_%s: " % sf) and "window above 103 residues are left out" in m]
        left = left[0] if left else 0
        n_out += left
        assert len(open(lay.out("ltr.LTR_%s.map" % sf)).read().splitlines()) == 1 + 8
        assert len(_fasta(lay.out("ltr.LTR_%s.aln" % sf))) == 8 - left
    assert 1 <= n_out < 16
