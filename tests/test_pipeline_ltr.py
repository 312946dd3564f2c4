"""Pipeline.stage_ltr without a GPU: the CPU oracle context answers the map and the enrichment, the twin
(tests/ltralign_ref.py) answers ltr_align.  Inputs and the reference's outputs are those of tests/golden/golden_ltr.json.gz:
`.ltr.bin.count`, `.ltr.insert.data` and `.ltr.insert.summary` must be the reference's files byte for byte under
-ltr_identity scn, `.ltr.enrich` its calls; under -ltr_identity align the files must be what ltr.py makes of the twin's counts."""
import gzip
import io
import json
import logging
import os

import numpy as np
import pytest

import ltralign_ref as lr
from oracle_ctx import OracleContext
from subphaser_amd import ltr, pipeline, runtime, seqs
from toygenome import make_toy_genome

HERE = os.path.dirname(os.path.abspath(__file__))


class _AlignCtx(OracleContext):
    """the oracle context plus ltr_align from the twin (one twin run per distinct call, shared by the tests)"""
    cache = {}

    def ltr_align(self, chrom, a_start, a_len, b_start, b_len, band):
        key = (tuple(map(int, chrom)), tuple(map(int, a_start)), tuple(map(int, a_len)), tuple(map(int, b_start)), tuple(map(int, b_len)), band)
        if key not in self.cache:
            text = [bytes(s).decode() for s in self.seqs]
            self.cache[key] = lr.align_intervals(text, chrom, a_start, a_len, b_start, b_len, band)
        self.calls.append(band)
        return self.cache[key].copy()


@pytest.fixture(scope="module")
def world():
    with gzip.open(os.path.join(HERE, "golden", "golden_ltr.json.gz"), "rt") as f:
        gold = json.load(f)
    toy = make_toy_genome(seed=gold["seed"])
    labels = toy["labels"]

    def make(cls):
        ctx = cls()
        ctx.genome_reset(len(labels))
        for i, lab in enumerate(labels):
            ctx.genome_add(i, toy["seqs"][lab])
        ctx.k = gold["k"]
        ctx.calls = []
        return ctx
    kl = seqs.KmerLabels.from_dict(dict(map(tuple, gold["kmers"])), gold["sg_names"], gold["k"])
    return gold, labels, make, kl


class _Lay:
    def __init__(self, root):
        self.root = str(root)

    def out(self, ext):
        return os.path.join(self.root, "run." + ext)

    def ckp(self, name):
        return os.path.join(self.root, os.path.basename(name) + ".ok")


class _Cl:
    def __init__(self, gold):
        self.d_sg, self.sg_names = dict(gold["d_sg"]), list(gold["sg_names"])


@pytest.fixture
def with_ctx():
    old = runtime._ctx
    yield runtime.set_context
    runtime._ctx = old


def _pipe(tmp_path, gold, scn_text=None, **over):
    scn = tmp_path / "LTR.scn"
    scn.write_text(gold["scn"] if scn_text is None else scn_text)
    opts = dict(ltr_scn=str(scn), mu=gold["mu"], figfmt="png")
    opts.update(over)
    p = pipeline.Pipeline.bare(**opts)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    return p, _Lay(out)


def _run(p, lay, world, ctx, caplog, with_ctx, kl=None):
    gold, labels = world[:2]
    kl = world[3] if kl is None else kl
    with_ctx(ctx)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_ltr(lay, labels, _Cl(gold), kl)
    return [r.getMessage() for r in caplog.records]


def _read(lay, ext):
    with open(lay.out(ext)) as f:
        return f.read()


def _resolved(gold, tmp_path):
    recs = ltr.read_scn(str(tmp_path / "LTR.scn"))
    return ltr.group_resolve_overlaps([r for r in recs if r.seq_id in gold["d_sg"]])


def _twin_counts(world, ltrs, band):
    gold, labels, make, _ = world
    ctx = make(_AlignCtx)
    a0, la, b0, lb = ltr.ltr_intervals(ltrs)
    return ctx.ltr_align([labels.index(r.seq_id) for r in ltrs], a0, la, b0, lb, band)


def _enrich_rows(text):
    rows = [line.split("\t") for line in text.splitlines()]
    return [(r[0], r[1], r[3], r[4]) for r in rows], [[float(r[2]), float(r[5])] for r in rows[1:]]


def test_scn_identity_is_the_reference(tmp_path, world, caplog, with_ctx):
    gold, labels, make, _ = world
    p, lay = _pipe(tmp_path, gold, ltr_identity="scn")
    ctx = make(_AlignCtx)
    log = _run(p, lay, world, ctx, caplog, with_ctx)
    assert _read(lay, "ltr.bin.count") == gold["bin_count"]
    assert _read(lay, "ltr.insert.data") == gold["insert"]["00"]["data"]
    assert _read(lay, "ltr.insert.summary") == gold["insert"]["00"]["summary"]
    got, want = _enrich_rows(_read(lay, "ltr.enrich")), _enrich_rows(gold["enrich"])
    assert got[0] == want[0]                                     # ids, calls, counts, exchanges
    np.testing.assert_allclose(got[1], want[1], rtol=1e-6, atol=1e-300)
    # the identity table: the alignment is reported beside the file's similarity, the ages are the file's
    ltrs = _resolved(gold, tmp_path)
    counts = _twin_counts(world, ltrs, 64)
    want = io.StringIO()
    ltr.write_identity(want, ltrs, counts, [1 - r.similarity / 100 for r in ltrs], gold["ages"])
    assert _read(lay, "ltr.identity.tsv") == want.getvalue()
    assert ctx.calls == [64]
    for ext in ("ltr.bin.count", "ltr.enrich", "ltr.identity.tsv", "ltr.insert.summary"):
        assert os.path.exists(lay.ckp(lay.out(ext)))
    n_sig = len(gold["d_enriched"])
    assert "{} significant subgenome-specific LTR-RTs".format(n_sig) in log
    per_sg = sorted(set(gold["d_enriched"].values()))
    at = log.index("{} significant subgenome-specific LTR-RTs".format(n_sig))
    assert log[at + 1:at + 1 + len(per_sg)] == ["\t{} {}-specific LTR-RTs".format(list(gold["d_enriched"].values()).count(sg), sg) for sg in per_sg]
    assert "1 LTRs lie on sequences that are not target chromosomes: skipped" in log
    assert sum("every record is used, as under -all_ltr" in m for m in log) == 1
    assert any(m.startswith("A rough estimation of the divergence–hybridization period: ") for m in log)
    assert not any("take the similarity of the file" in m for m in log)
    # the two figures are queued for the main thread and optional
    (name, wait, done), = p._background
    assert name == lay.out("ltr.insert.density.png")
    wait()
    done()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    for fig in (name, lay.out("ltr.insert.histo.png")):
        with open(fig, "rb") as f:
            assert f.read(4) == b"\x89PNG"


def _expected_files(world, tmp_path, lay, band, mode, excl=False, nonspec=False):
    """what ltr.py makes of the twin's counts, given the stage's own `.ltr.enrich`"""
    gold = world[0]
    ltrs = _resolved(gold, tmp_path)
    counts = _twin_counts(world, ltrs, band)
    divs, fell = ltr.divergences(ltrs, counts, mode)
    ages = [ltr.estimate_age(d, gold["mu"]) for d in divs]
    ident, data, summary = io.StringIO(), io.StringIO(), io.StringIO()
    ltr.write_identity(ident, ltrs, counts, divs, ages)
    d_data, _, _ = ltr.write_insert_data(data, ltrs, ages, gold["d_enriched"], gold["d_exchange"], exclude_exchanges=excl, non_specific=nonspec)
    ltr.summary_ltr_time(d_data, summary)
    return counts, fell, ident.getvalue(), data.getvalue(), summary.getvalue()


def test_align_identity(tmp_path, world, caplog, with_ctx):
    gold, labels, make, _ = world
    p, lay = _pipe(tmp_path, gold)
    log = _run(p, lay, world, make(_AlignCtx), caplog, with_ctx)
    counts, fell, ident, data, summary = _expected_files(world, tmp_path, lay, 64, "align")
    assert fell == 0 and not (counts[:, 5] & (lr.F_BAND | lr.F_LEN)).any()
    assert _read(lay, "ltr.bin.count") == gold["bin_count"]
    assert _read(lay, "ltr.identity.tsv") == ident
    assert _read(lay, "ltr.insert.data") == data and data != gold["insert"]["00"]["data"]
    assert _read(lay, "ltr.insert.summary") == summary
    assert [line.split("\t")[:2] for line in data.splitlines()] == [line.split("\t")[:2] for line in gold["insert"]["00"]["data"].splitlines()]
    assert any(m.startswith("%d LTR pairs aligned (band 64)" % len(counts)) for m in log)
    assert not any("take the similarity of the file" in m for m in log)


def test_pairs_that_are_not_aligned_take_the_files_similarity(tmp_path, world, caplog, with_ctx):
    gold, labels, make, _ = world
    p, lay = _pipe(tmp_path, gold, ltr_band=512)             # 2 * 512 + 1 diagonals: wider than the kernel's band for every pair
    log = _run(p, lay, world, make(_AlignCtx), caplog, with_ctx)
    n = len(gold["resolved"])
    assert "{} LTR pairs without an aligned substitution column or outside the limits of the alignment take the similarity of the file".format(n) in log
    assert _read(lay, "ltr.insert.data") == gold["insert"]["00"]["data"]
    assert _read(lay, "ltr.insert.summary") == gold["insert"]["00"]["summary"]
    flags = {line.split("\t")[7] for line in _read(lay, "ltr.identity.tsv").splitlines()[1:]}
    assert flags == {str(lr.F_BAND)}


def test_context_without_ltr_align_falls_back_to_scn(tmp_path, world, caplog, with_ctx):
    gold, labels, make, _ = world
    p, lay = _pipe(tmp_path, gold)
    log = _run(p, lay, world, make(OracleContext), caplog, with_ctx)
    assert sum(m == "this context has no ltr_align: -ltr_identity scn is used" for m in log) == 1
    assert _read(lay, "ltr.insert.data") == gold["insert"]["00"]["data"]
    assert _read(lay, "ltr.insert.summary") == gold["insert"]["00"]["summary"]
    rows = [line.split("\t") for line in _read(lay, "ltr.identity.tsv").splitlines()[1:]]
    assert len(rows) == len(gold["resolved"]) and all(r[2:8] == ["NA"] * 6 for r in rows)
    assert [float(r[9]) for r in rows] == gold["ages"]


@pytest.mark.parametrize("excl,nonspec", [(True, False), (False, True), (True, True)])
def test_exclude_exchanges_and_non_specific(tmp_path, world, caplog, with_ctx, excl, nonspec):
    gold, labels, make, _ = world
    p, lay = _pipe(tmp_path, gold, ltr_identity="scn", exclude_exchanges=excl, non_specific=nonspec)
    log = _run(p, lay, world, make(OracleContext), caplog, with_ctx)
    want = gold["insert"]["%d%d" % (excl, nonspec)]
    assert _read(lay, "ltr.insert.data") == want["data"] and _read(lay, "ltr.insert.summary") == want["summary"]
    n_yes = sum(gold["d_exchange"][i] == "yes" for i in gold["d_enriched"])
    assert ("{} potentially exchanged LTR-RTs are excluded".format(n_yes) in log) == excl


def test_ids_before_renaming_are_taken(tmp_path, world, caplog, with_ctx):
    gold, labels, make, _ = world
    rows = [line if line.startswith("#") else line.split() for line in gold["scn"].splitlines()]
    text = "".join(r + "\n" if isinstance(r, str) else " ".join(r[:11] + ["chr_a1" if r[11] == "A1" else r[11]] + r[12:]) + "\n" for r in rows)
    assert "chr_a1" in text
    p, lay = _pipe(tmp_path, gold, scn_text=text, ltr_identity="scn", d_targets={"chr_a1": "A1", "scaffold9": "scaffold9"})
    _run(p, lay, world, make(OracleContext), caplog, with_ctx)
    assert _read(lay, "ltr.bin.count") == gold["bin_count"]
    assert _read(lay, "ltr.insert.data") == gold["insert"]["00"]["data"]


def test_no_enriched_element_no_plots(tmp_path, world, caplog, with_ctx):
    gold, labels, make, kl = world
    p, lay = _pipe(tmp_path, gold, scn_text="100 2100 2001 100 300 201 1900 2100 201 95.5 0 A3\n")
    none = seqs.KmerLabels.from_dict({}, gold["sg_names"], gold["k"])      # no subgenome-specific k-mer: no element is mapped
    log = _run(p, lay, world, make(_AlignCtx), caplog, with_ctx, kl=none)
    assert _read(lay, "ltr.bin.count") == "#chrom\tstart\tend\tSG1\tSG2\n"
    assert "0 significant subgenome-specific LTR-RTs" in log
    assert "Because of none subgenome-specific LTR-RTs, plots of LTR-RTs are skipped." in log
    assert not os.path.exists(lay.out("ltr.insert.data")) and not p._background
    assert len(_read(lay, "ltr.identity.tsv").splitlines()) == 2


def test_errors_and_skips(tmp_path, world, caplog, with_ctx, monkeypatch):
    gold, labels, make, _ = world
    # the raw 11-column format
    p, lay = _pipe(tmp_path, gold, scn_text="100 2100 2001 100 300 201 1900 2100 201 95.5 0\n")
    with_ctx(make(_AlignCtx))
    with pytest.raises(ValueError, match="column 12, the sequence id, is missing"):
        p.stage_ltr(lay, labels, _Cl(gold), world[3])
    # an element off its chromosome is named
    p, lay = _pipe(tmp_path, gold, scn_text="100 999999 2001 100 300 201 1900 999999 201 95.5 0 A1\n")
    with pytest.raises(ValueError, match="A1:100-999999:300-999799 does not lie on its chromosome"):
        p.stage_ltr(lay, labels, _Cl(gold), world[3])
    # a multi-rank run
    p, lay = _pipe(tmp_path, gold)
    monkeypatch.setenv("WORLD_SIZE", "2")
    log = _run(p, lay, world, make(_AlignCtx), caplog, with_ctx)
    assert log == ["LTR stage skipped: it runs on one GPU, this is a run of 2 ranks"]
    assert os.listdir(lay.root) == []


def test_switches_that_skip_the_stage(monkeypatch, caplog):
    """the stage follows the feature and block stages; it needs -ltr_scn and runs unless -just_core or -disable_ltr"""
    def run(**flags):
        opts = dict(outdir="o", tmpdir="t", custom_features=["f.bed"], ltr_scn="x.scn")
        opts.update(flags)
        p = pipeline.Pipeline.bare(**opts)
        order = []

        class _C:
            d_sg, sg_names = {}, []
        monkeypatch.setattr(pipeline, "Layout", lambda *a: "lay")
        monkeypatch.setattr(p, "stage_ingest", lambda lay: (order.append("ingest"), (["f"], ["c"], {"c": 1}, {}))[1], raising=False)
        monkeypatch.setattr(p, "stage_count_filter", lambda *a: order.append("count"), raising=False)
        monkeypatch.setattr(p, "stage_cluster", lambda *a: (order.append("cluster"), (_C(), None))[1], raising=False)
        for name in ("windows", "features", "blocks", "ltr"):
            monkeypatch.setattr(p, "stage_" + name, lambda *a, name=name: order.append(name), raising=False)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            p._run()
        return order, [r.getMessage() for r in caplog.records]
    order, log = run()
    assert order == ["ingest", "count", "cluster", "windows", "features", "blocks", "ltr"]
    assert len(log) == 1 and log[0].startswith("Of modules 3-4, LTR detection, TEsorter classification, the LTR trees and the circos figure")
    assert run(disable_ltr=True)[0] == ["ingest", "count", "cluster", "windows", "features", "blocks"]
    assert run(ltr_scn=None)[0] == ["ingest", "count", "cluster", "windows", "features", "blocks"]
    assert run(ltr_scn=None)[1][0].startswith("Modules 3-4 (LTR, circos) are not part of this build")
    assert run(just_core=True)[0] == ["ingest", "count", "cluster"]
    order, log = run(disable_circos=True)
    assert order == ["ingest", "count", "cluster", "windows", "features", "ltr"] and len(log) == 1 and log[0].startswith("Of modules 3-4, ")


def test_cli_options():
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config"])
    assert (args.ltr_scn, args.ltr_identity, args.ltr_band) == (None, "align", 64)
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_scn", "tmp/LTR.scn", "-ltr_identity", "scn", "-ltr_band", "16",
                                  "-mu", "7e-9", "-exclude_exchanges", "-non_specific"])
    assert (args.ltr_scn, args.ltr_identity, args.ltr_band, args.mu) == ("tmp/LTR.scn", "scn", 16, 7e-9)
    assert args.exclude_exchanges and args.non_specific
    with pytest.raises(SystemExit):
        pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_identity", "blast"])
