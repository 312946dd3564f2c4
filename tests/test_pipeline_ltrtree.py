"""Pipeline.stage_ltr under -ltr_tree without a GPU: the oracle context of test_pipeline_ltrdetect.py with the twin
(tests/ltrtree_ref.py) behind the three new methods.  The three files, the subsample rule, the "fewer than 4" and "too long"
lines, -disable_ltrtree, the closing note with and without a tree, and that nothing changes while the flag is off."""
import logging
import os
import re

import numpy as np
import pytest

import ltrtree_ref as lt
from test_pipeline_ltrdetect import LABELS, _Cl, _DetectCtx, _pipe, _run, with_ctx, world  # noqa: F401  (fixtures)
from subphaser_amd import ltrtree, pipeline

TREE_FILES = ("ltr.tree.nwk", "ltr.tree.map", "ltr.tree.png")


class _TreeCtx(_DetectCtx):
    def _seq(self, c):
        return bytes(self.seqs[c]).decode()

    def ltr_sketch(self, chrom, start, end, k, s):
        self.calls.append(("sketch", len(chrom), k, s))
        return lt.sketches([self._seq(c)[a:b] for c, a, b in zip(map(int, chrom), map(int, start), map(int, end))], k, s)

    def ltr_sketch_pairs(self, sketch, length):
        self.calls.append(("pairs", len(length)))
        return lt.pairs(sketch, length, sketch.shape[1])

    def nj_tree(self, dist):
        self.calls.append(("nj", dist.shape[0]))
        self.last_dist = np.array(dist)
        return lt.nj_numpy(dist)


def _tree_run(tmp, world, caplog, with_ctx, cls=_TreeCtx, **over):
    opts = dict(ltr_tree=True, ltr_tree_k=13, ltr_tree_sketch=64, subsample=1000, bootstrap_seed=None)
    opts.update(over)
    p, lay = _pipe(tmp, **opts)
    ctx = world[2](cls)
    log = _run(p, lay, world, ctx, caplog, with_ctx)
    for _, _, done in p._background:
        done()
    return p, lay, ctx, log


def _listed(lay):
    return [r.split("\t")[:2] for r in open(lay.out("ltr.insert.data")).read().splitlines()[1:]]


def test_the_three_files(tmp_path, world, caplog, with_ctx):
    p, lay, ctx, log = _tree_run(tmp_path / "tree", world, caplog, with_ctx)
    listed = _listed(lay)
    assert len(listed) >= 8
    for ext in TREE_FILES[:2]:
        assert os.path.exists(lay.out(ext)) and os.path.exists(lay.ckp(lay.out(ext))), ext
    rows = [r.split("\t") for r in open(lay.out("ltr.tree.map")).read().splitlines()]
    assert rows[0] == ["label", "Clade", "Subgenome"] and [[r[0], r[2]] for r in rows[1:]] == listed and {r[1] for r in rows[1:]} == {"unknown"}
    n = len(listed)
    assert [c for c in ctx.calls if c[0] in ("sketch", "pairs", "nj")] == [("sketch", n, 13, 64), ("pairs", n), ("nj", n)]
    D = ctx.last_dist
    assert D.dtype == np.int64 and (D == D.T).all() and (np.diag(D) == 0).all() and D.min() >= 0 and D.max() < 1 << 31
    assert open(lay.out("ltr.tree.nwk")).read() == ltrtree.tree_text(lt.nj_numpy(D), [x[0] for x in listed]) + "\n"
    assert any(m.startswith("LTR tree of %d elements (k = 13, 64 hashes): sketches " % n) for m in log)
    assert p._ltr_tree_built is True
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert os.path.exists(lay.out("ltr.tree.png")) and os.path.getsize(lay.out("ltr.tree.png")) > 1000


def test_subsample_and_fewer_than_four(tmp_path, world, caplog, with_ctx):
    p0, lay0, _, _ = _tree_run(tmp_path / "all", world, caplog, with_ctx)
    listed = _listed(lay0)
    n = len(listed)
    p, lay, ctx, log = _tree_run(tmp_path / "five", world, caplog, with_ctx, subsample=5, bootstrap_seed=3)
    assert "LTR tree: 5 of the %d subgenome-specific elements are kept (-subsample; at most 4096 in one tree)" % n in log
    rows = [r.split("\t")[0] for r in open(lay.out("ltr.tree.map")).read().splitlines()[1:]]
    assert rows == [listed[q][0] for q in ltrtree.choose(n, 5, 3)] and ("nj", 5) in ctx.calls
    p2, lay2, _, _ = _tree_run(tmp_path / "seed0", world, caplog, with_ctx, subsample=5)      # no seed given: 0
    assert [r.split("\t")[0] for r in open(lay2.out("ltr.tree.map")).read().splitlines()[1:]] == [listed[q][0] for q in ltrtree.choose(n, 5, 0)]
    p3, lay3, ctx3, log3 = _tree_run(tmp_path / "all0", world, caplog, with_ctx, subsample=0)  # 0 means all
    assert ("nj", n) in ctx3.calls and not any("are kept" in m for m in log3)
    p4, lay4, ctx4, log4 = _tree_run(tmp_path / "three", world, caplog, with_ctx, subsample=3)
    assert "LTR tree: 3 subgenome-specific elements, fewer than 4: no tree" in log4 and p4._ltr_tree_built is False
    assert not any(os.path.exists(lay4.out(ext)) for ext in TREE_FILES) and not [c for c in ctx4.calls if c[0] == "nj"]


def test_too_long_elements_are_left_out(tmp_path, world, caplog, with_ctx, monkeypatch):
    p0, lay0, _, _ = _tree_run(tmp_path / "all", world, caplog, with_ctx)
    lens = {r.id: r.end - r.start for r in pipeline.ltr_mod.read_scn(lay0.out("ltr.scn"))}
    listed = [x[0] for x in _listed(lay0)]
    cut = sorted(lens[i] for i in listed)[-3]              # the two longest go
    monkeypatch.setattr(ltrtree, "MAX_LEN", cut)
    p, lay, ctx, log = _tree_run(tmp_path / "cut", world, caplog, with_ctx)
    gone = [i for i in listed if lens[i] > cut]
    assert 1 <= len(gone) <= 2 and "LTR tree: %d elements above %d bases are left out" % (len(gone), cut) in log
    assert [r.split("\t")[0] for r in open(lay.out("ltr.tree.map")).read().splitlines()[1:]] == [i for i in listed if i not in gone]


def test_disable_wins_and_a_context_without_the_entries(tmp_path, world, caplog, with_ctx):
    p, lay, ctx, log = _tree_run(tmp_path / "off", world, caplog, with_ctx, cls=_DetectCtx, disable_ltrtree=True)
    assert log.count("-disable_ltrtree: the LTR tree of -ltr_tree is not built") == 1 and p._ltr_tree_built is False
    assert not any(os.path.exists(lay.out(ext)) for ext in TREE_FILES) and os.path.exists(lay.out("ltr.insert.data"))
    with pytest.raises(RuntimeError, match="-ltr_tree needs a context with ltr_sketch, ltr_sketch_pairs and nj_tree .*no CPU engine"):
        _tree_run(tmp_path / "none", world, caplog, with_ctx, cls=_DetectCtx)
    assert not os.path.exists(os.path.join(str(tmp_path / "none"), "run.ltr.scn"))


def test_flag_off_changes_nothing(tmp_path, world, caplog, with_ctx):
    p, lay = _pipe(tmp_path / "today")                      # as the existing tests build it: none of the new attributes
    log_today = _run(p, lay, world, world[2](_TreeCtx), caplog, with_ctx)
    for _, _, done in p._background:
        done()
    p2, lay2, ctx2, log_off = _tree_run(tmp_path / "off", world, caplog, with_ctx, ltr_tree=False, ggtree_options="x", tree_method="iqtree")
    strip = lambda log, root: [re.sub(r"\d+\.\d+ s", "T s", m).replace(str(root), "") for m in log]
    assert strip(log_off, tmp_path / "off") == strip(log_today, tmp_path / "today")
    assert not any(os.path.exists(lay2.out(ext)) for ext in TREE_FILES) and not [c for c in ctx2.calls if c[0] in ("sketch", "pairs", "nj")]
    assert sorted(os.listdir(lay2.root)) == sorted(os.listdir(lay.root))
    # with the flag on, the options of the reference's tree programs are warned about
    p3, lay3, ctx3, log3 = _tree_run(tmp_path / "warn", world, caplog, with_ctx, ggtree_options="x", tree_method="iqtree")
    assert sum("no alignment or tree program is run" in m for m in log3) == 2


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
    # the five texts, byte for byte
    assert run(True, ltr_denovo=True, ltr_tree=True) == [
        "Of modules 3-4, TEsorter classification and the circos figure are not part of this build "
        "(the LTR-RTs are this build's own detection, not ltr_finder's or ltrharvest's); the tree of -ltr_tree is this build's own "
        "(sketches and neighbour joining), not the reference's domain trees; run the reference on the outputs above for them"]
    assert run(True, ltr_scn="x.scn", ltr_tree=True) == [
        "Of modules 3-4, LTR detection, TEsorter classification and the circos figure are not part of this build; the tree of "
        "-ltr_tree is this build's own (sketches and neighbour joining), not the reference's domain trees; run the reference on the "
        "outputs above for them"]
    # no tree built (flag off, disabled, or fewer than 4 elements)
    assert run(False, ltr_denovo=True, ltr_tree=True) == [
        "Of modules 3-4, TEsorter classification, the LTR trees and the circos figure are not part of this build "
        "(the LTR-RTs are this build's own detection, not ltr_finder's or ltrharvest's); run the reference on "
        "the outputs above for them"]
    assert run(False, ltr_scn="x.scn") == [
        "Of modules 3-4, LTR detection, TEsorter classification, the LTR trees and the circos figure are not "
        "part of this build; run the reference on the outputs above for them"]
    # no LTR stage: neither -ltr_scn nor -ltr_denovo, or -disable_ltr; nothing once -disable_circos is given too
    for flags in (dict(), dict(disable_circos=False, disable_ltr=True, ltr_scn="x.scn")):
        assert run(False, **flags) == [
            "Modules 3-4 (LTR, circos) are not part of this build; run the reference on the "
            "outputs above, or pass -disable_ltr -disable_circos to silence this note"]
    assert run(False, disable_ltr=True, ltr_denovo=True) == []


def test_option_record_is_the_parsers():
    """every option has ONE default, the `CLI` table's: a pipeline built without the parser reads what the parser would give"""
    args = vars(pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config"]))      # no -pre: outdir and tmpdir are not rewritten
    record = pipeline.option_defaults()
    assert set(record) == set(args)
    p = pipeline.Pipeline.bare()
    for dest in sorted(set(args) - {"genomes", "sg_cfgs"}):
        assert record[dest] == args[dest] and type(record[dest]) is type(args[dest]), dest
        assert getattr(p, dest) == args[dest] and getattr(pipeline.Pipeline, dest) == args[dest], dest      # the class's, not a copy
    assert (p._background, p.d_targets, p._ltr_tree_built) == ([], {}, False)
    assert pipeline.Pipeline.bare(colors="red,#00ff00").colors == ["red", "#00ff00"] and p.colors is None


def test_cli_options():
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config"])
    assert (args.ltr_tree, args.ltr_tree_k, args.ltr_tree_sketch, args.subsample, args.disable_ltrtree) == (False, 13, 1024, 1000, False)
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_denovo", "-ltr_tree", "-ltr_tree_k", "15", "-ltr_tree_sketch", "256", "-subsample", "0"])
    assert (args.ltr_tree, args.ltr_tree_k, args.ltr_tree_sketch, args.subsample) == (True, 15, 256, 0)
