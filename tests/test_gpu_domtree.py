"""GPU: the LTR stage under -ltr_domtree with the real library.

On the world of tests/test_pipeline_domtree.py every file of the domain trees (and the classification they start from)
equals the twin-context run's byte for byte; there the stage is run as the CPU tests run it (Pipeline.stage_ltr on the
world's chromosomes and k-mer labels): the world's random chromosomes carry no k-mer signal for the stages in front of it.
On the toy genome with planted elements main() runs from the command line to the files, and the rows of the `.aln` files
equal those of the twin path.

No kernel of sp_domalign.hip caps its grid (items, items, tiles of the pair triangle), so there is no SP_CU_LIMIT case."""
import os

import pytest

from test_pipeline_domains import _dom_run
from test_pipeline_domtree import _DomTreeCtx, world  # noqa: F401  (fixture)
from test_pipeline_ltrdetect import K, LABELS, with_ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
FILES = ["ltr.dom.gff3", "ltr.cls.tsv", "ltr.cls.pep", "ltr.insert.data"] + [
    "ltr.LTR_%s.%s" % (sf, ext) for sf in ("Copia", "Gypsy") for ext in ("aln", "map", "aln.trimmed", "aln.rooted.tre")]


def test_stage_files_equal_the_twin_run(gpu_ctx, tmp_path, world, caplog, with_ctx):
    opts = dict(ltr_domtree=True, subsample=1000, bootstrap_seed=None)
    p0, lay0, ctx0, log0 = _dom_run(tmp_path / "twin", world, caplog, with_ctx, cls=_DomTreeCtx, **opts)
    # the real context with the world's genome loaded and counted (the label set needs k)
    chroms = world[0]
    gpu_ctx.genome_reset(len(LABELS))
    for i, s in enumerate(chroms):
        gpu_ctx.genome_add(i, s)
    gpu_ctx.count(K, 1, 0)
    real_world = (world[0], world[1], lambda cls: gpu_ctx) + tuple(world[3:])
    p1, lay1, ctx1, log1 = _dom_run(tmp_path / "real", real_world, caplog, with_ctx, cls=None, **opts)
    assert p0._ltr_domtrees_built == p1._ltr_domtrees_built == ("Copia", "Gypsy")
    for ext in FILES:
        assert os.path.getsize(lay1.out(ext)) > 0 and open(lay1.out(ext)).read() == open(lay0.out(ext)).read(), ext
        assert ext == "ltr.insert.data" or os.path.exists(lay1.ckp(lay1.out(ext))), ext      # (`.insert.data` has none: its summary has)
    for sf in ("Copia", "Gypsy"):
        assert os.path.exists(lay1.out("ltr.LTR_%s.tree.png" % sf))
    dom = lambda log: [m for m in log if ("sequences contain" in m and m.endswith("domains")) or "unique alignments" in m or "is aligned to profile" in m]
    assert dom(log1) == dom(log0) and len(dom(log0)) == 16


def test_cli_denovo_with_domain_trees(gpu_ctx, toy, tmp_path, caplog):
    """main() with -ltr_denovo -ltr_hmm -ltr_domtree on the toy genome: six planted LTR-RTs per chromosome, Copia-like and
    Gypsy-like in turn, each with two domains (INT, RT) that differ from the consensus in three residues of their own.  The
    rows of the `.aln` files are those of the twin path: the records of the `.scn`, the twin's search of their inner
    sequences, the common profile, the window of the own hit +- 32 residues, the twin's alignment.  `.map`, `.cls.pep`, the
    tree files and the closing note are checked against what the run itself selected."""
    import random
    import re

    import domalign_ref as da
    import domains_ref as dr
    import ltr_cases
    from subphaser_amd import domains, domtree, ltr
    from test_gpu_domains import CLI_NAMES
    from test_gpu_ltrdetect import _cli
    rng = random.Random(43)
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, 40), name=n) for n in CLI_NAMES]
    cons = ["".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs]
    labels = toy["labels"]
    seqs, _, elements = ltr_cases.plant_elements({lab: str(toy["seqs"][lab]) for lab in labels}, labels, per_chrom=6)
    for q, (lab, start, end, lltr, rltr) in enumerate(elements):
        pair = cons[:2] if q % 2 == 0 else cons[2:]
        own = []
        for c in pair:
            c = list(c)
            for at in rng.sample(range(5, 35), 3):
                c[at] = rng.choice([a for a in dr.AA if a != c[at]])
            own.append("".join(c))
        dom = dr.back_translate(rng, own[0]) + dr.rand_dna(rng, 15) + dr.back_translate(rng, own[1])
        if q % 2:
            dom = dr.revcomp(dom)
        at = start - 1 + lltr + 40
        assert at + len(dom) < end - rltr - 40
        seqs[lab] = seqs[lab][:at] + dom + seqs[lab][at + len(dom):]
    hmm = tmp_path / "toy.hmm"
    hmm.write_text(dr.hmm_text(profs))
    base, log = _cli(gpu_ctx, toy, seqs, tmp_path / "domtree", caplog,
                     ["-ltr_denovo", "-ltr_maxdist", "2600", "-ltr_hmm", str(hmm), "-ltr_domtree", "-ltr_domains", "INT", "RT"])
    # the twin path up to the hits
    P = domains.read_hmm(str(hmm))
    twins = [dr.make_profile(M, P.emis[a:a + M], P.trans[a:a + M], entry=e, name=n) for M, a, e, n in zip(P.M, P.moff.tolist(), P.entry.tolist(), P.names)]
    recs = {domains.format_gff_id(r.id): r for r in ltr.read_scn(base + ".ltr.scn")}
    gff = [line.split("\t") for line in open(base + ".ltr.dom.gff3").read().splitlines()]
    pep = [(r.split("\n")[0], r.split("\n")[1]) for r in open(base + ".ltr.cls.pep").read().split(">")[1:]]
    assert len(pep) == len(gff) > 0 and all(h.split(" ", 1)[1] == f[8] and re.match(r"^\S+#LTR/(Copia/Ale|Gypsy/Tekay)#\S+\|\S+$", h.split()[0])
                                            for (h, _), f in zip(pep, gff))
    listed = [r.split("\t")[0] for r in open(base + ".ltr.insert.data").read().splitlines()[1:]]
    cls = {r.split("\t")[0]: r.split("\t") for r in open(base + ".ltr.cls.tsv").read().splitlines()[1:]}
    n_rows, built = 0, []
    for sf, (p_int, p_rt) in (("Copia", (0, 1)), ("Gypsy", (3, 2))):
        want_ids = [i for i in listed if cls.get(i, [None] * 3)[2] == sf and {"INT", "RT"} <= {d.split("|")[0].split("-")[-1] for d in cls[i][6].split()}]
        rows = [r.split("\t") for r in open("%s.ltr.LTR_%s.map" % (base, sf)).read().splitlines()]
        assert rows[0] == ["label", "Clade", "Subgenome"] and [r[0] for r in rows[1:]] == [domtree.format_id_for_iqtree(i) for i in want_ids]
        want_rows = []
        for i in want_ids:
            r = recs[i]
            a, b = domains.inner_interval(r)
            inner = seqs[r.seq_id][a:b]
            blocks = ""
            for p in (p_int, p_rt):
                s, f, i_s, i_e, _, _ = dr.element(inner, twins[p])
                i0, i1 = domtree.window(i_s, i_e, len(dr.translate(inner, f)))
                res = da.window_residues(inner, f, i0, i1)
                _, col, _ = da.align(res, i0, twins[p])
                blocks += domtree.row_string(col, i0, res)
            want_rows.append((domtree.format_id_for_iqtree(i), blocks))
        desc, kept, dropped = domtree.cat_rows([n for n, _ in want_rows], [[b[:40] for _, b in want_rows], [b[40:] for _, b in want_rows]])
        aln = [(r.split("\n")[0], r.split("\n")[1]) for r in open("%s.ltr.LTR_%s.aln" % (base, sf)).read().split(">")[1:]]
        assert aln == [("%s %s" % (n, desc), row) for n, row in kept], sf
        n_rows += len(aln)
        has_tree = os.path.exists("%s.ltr.LTR_%s.aln.rooted.tre" % (base, sf))
        assert has_tree == (len(aln) >= 4)
        if has_tree:
            built.append(sf)
            assert open("%s.ltr.LTR_%s.aln.rooted.tre" % (base, sf)).read().count(",") == len(aln) - 1
            assert os.path.exists("%s.ltr.LTR_%s.aln.trimmed" % (base, sf))
    assert n_rows >= 1
    note = [m for m in log if m.startswith("Of modules 3-4")]
    assert len(note) == 1 and (("the domain trees of -ltr_domtree (%s) are built" % ", ".join(built)) in note[0]) == bool(built)
