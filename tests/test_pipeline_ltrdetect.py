"""Pipeline.stage_ltr under -ltr_denovo without a GPU: the CPU oracle context answers the map and the enrichment, the twins
answer the device entries -- tests/ltrdetect_ref.py behind ltr_seeds / ltr_hsps, tests/ltralign_ref.py behind ltr_align.
The written `.ltr.scn` must be what ltr.py makes of the twins' answers, and the stage must go on from its records exactly
as it does from a file: a second run that reads the `.scn` through -ltr_scn writes the same downstream files."""
import io
import logging
import os
import random

import numpy as np
import pytest

import ltralign_ref as lr
import ltrdetect_cases as lc
import ltrdetect_ref as ld
from oracle_ctx import OracleContext
from subphaser_amd import ltr, pipeline, runtime, seqs

K = 15
LABELS = ["A1", "A2", "B1", "B2"]
D_SG = {"A1": "SG1", "A2": "SG1", "B1": "SG2", "B2": "SG2"}
DOWNSTREAM = ("ltr.bin.count", "ltr.enrich", "ltr.identity.tsv", "ltr.insert.data", "ltr.insert.summary")


class _DetectCtx(OracleContext):
    """the oracle context plus the three device entries of the LTR stage, from the twins"""
    cache = {}

    def ltr_seeds(self, chrom, seed_len, xdrop, dmin, dmax, maxlen):
        key = (bytes(self.seqs[chrom]), seed_len, xdrop, dmin, dmax, maxlen)
        if key not in self.cache:
            self.cache[key] = ld.hsps(key[0], seed_len, xdrop, dmin, dmax, maxlen)
        n_seeds, self.last = self.cache[key]
        self.calls.append(("seeds", chrom, seed_len, xdrop, dmin, dmax, maxlen))
        return n_seeds, len(self.last)

    def ltr_hsps(self, n):
        assert n == len(self.last)
        cols = list(zip(*self.last)) if self.last else [(), (), ()]
        return tuple(np.array(c, np.int32) for c in cols)

    def ltr_align(self, chrom, a_start, a_len, b_start, b_len, band):
        key = (tuple(bytes(s) for s in self.seqs), tuple(map(int, chrom)), tuple(map(int, a_start)), tuple(map(int, a_len)), tuple(map(int, b_start)),
               tuple(map(int, b_len)), band)
        if key not in self.cache:
            self.cache[key] = lr.align_intervals([bytes(s).decode() for s in self.seqs], chrom, a_start, a_len, b_start, b_len, band)
        self.calls.append(("align", len(chrom), band))
        return self.cache[key].copy()


@pytest.fixture(scope="module")
def world():
    """four chromosomes of 30 kb, four elements each; the 15-mers of the left LTRs are the subgenome-specific k-mers of
    the subgenome their chromosome belongs to"""
    rng = random.Random(31)
    chroms, d_kmers = [], {}
    for lab in LABELS:
        s = lc.rand_seq(rng, 30_000)
        for e in range(4):
            left = lc.rand_seq(rng, rng.randrange(150, 500))
            d_kmers.update({left[i:i + K]: D_SG[lab] for i in range(len(left) - K + 1)})
            right = lc.mutate(rng, left, rng.uniform(0, 0.06), rng.randrange(0, 2))
            a0 = 1500 + 7000 * e + rng.randrange(0, 500)
            s = lc.put(lc.put(s, a0, left), a0 + len(left) + rng.randrange(1500, 4000), right)
        chroms.append(s)
    kl = seqs.KmerLabels.from_dict(d_kmers, ["SG1", "SG2"], K)

    def make(cls):
        ctx = cls()
        ctx.genome_reset(len(LABELS))
        for i, s in enumerate(chroms):
            ctx.genome_add(i, s)
        ctx.k = K
        ctx.calls = []
        return ctx
    return chroms, kl, make


class _Lay:
    def __init__(self, root):
        self.root = str(root)
        os.makedirs(self.root, exist_ok=True)

    def out(self, ext):
        return os.path.join(self.root, "run." + ext)

    def ckp(self, name):
        return os.path.join(self.root, os.path.basename(name) + ".ok")


class _Cl:
    d_sg, sg_names = dict(D_SG), ["SG1", "SG2"]


@pytest.fixture
def with_ctx():
    old = runtime._ctx
    yield runtime.set_context
    runtime._ctx = old


def _pipe(root, **over):
    opts = dict(ltr_denovo=True, figfmt="png")
    opts.update(over)
    return pipeline.Pipeline.bare(**opts), _Lay(root)


def _run(p, lay, world, ctx, caplog, with_ctx):
    with_ctx(ctx)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_ltr(lay, LABELS, _Cl(), world[1])
    return [r.getMessage() for r in caplog.records]


def expected_scn(chroms, band=64, L=20, X=20, dmin=1000, dmax=15000, minlen=100, maxlen=7000, similar=85.0, indel=32, join=200, labels=LABELS,
                 align=lr.align_intervals):
    """(the `.scn` text, seeds, HSPs, chains, candidates, kept) from the twins and ltr.py, put together here once more"""
    n_seeds = n_hsps = n_chains = 0
    cands = []
    for ci, s in enumerate(chroms):
        ns, hsps = ld.hsps(s, L, X, dmin, dmax, maxlen)
        chains = ltr.chain_hsps(hsps, indel, join)
        n_seeds, n_hsps, n_chains = n_seeds + ns, n_hsps + len(hsps), n_chains + len(chains)
        cands += [(ci,) + c for c in ltr.candidates(chains, minlen, maxlen, dmin, dmax)]
    recs = []
    if cands:
        counts = align(chroms, [c[0] for c in cands], [c[1] for c in cands], [c[2] - c[1] for c in cands], [c[3] for c in cands],
                                    [c[4] - c[3] for c in cands], band)
        for c, row in zip(cands, np.asarray(counts).tolist()):
            m, x, g = row[1:4]
            if not row[5] & (lr.F_BAND | lr.F_LEN) and m + x + g and 100 * m / (m + x + g) >= similar:
                recs.append(ltr.Record.from_coords(labels[c[0]], c[0], c[1], c[2], c[3], c[4], 100 * m / (m + x + g)))
    buf = io.StringIO()
    ltr.write_scn(buf, recs)
    return buf.getvalue(), n_seeds, n_hsps, n_chains, len(cands), len(recs)


def test_denovo_stage_writes_the_scn_and_goes_on_as_from_a_file(tmp_path, world, caplog, with_ctx):
    chroms, kl, make = world
    p, lay = _pipe(tmp_path / "denovo")
    ctx = make(_DetectCtx)
    log = _run(p, lay, world, ctx, caplog, with_ctx)
    text, n_seeds, n_hsps, n_chains, n_cand, n_kept = expected_scn(chroms)
    assert n_kept >= 16 and n_cand >= n_kept                       # the planted elements at least
    scn = open(lay.out("ltr.scn")).read()
    assert scn == text and os.path.exists(lay.ckp(lay.out("ltr.scn")))
    assert len(ltr.read_scn(lay.out("ltr.scn"))) == n_kept
    # one detection per chromosome with the defaults, one alignment call for all candidates, one for the kept elements
    assert [c for c in ctx.calls if c[0] == "seeds"] == [("seeds", i, 20, 20, 1000, 15000, 7000) for i in range(4)]
    assert [c for c in ctx.calls if c[0] == "align"][0] == ("align", n_cand, 64) and len([c for c in ctx.calls if c[0] == "align"]) == 2
    assert any(m.startswith("%d seeds, %d extended seeds (HSPs), %d chains, %d candidates on 4 chromosomes in " % (n_seeds, n_hsps, n_chains, n_cand)) for m in log)
    assert any(m.startswith("%d candidates aligned (band 64) in " % n_cand) and m.endswith("; %d with similarity >= 85.0" % n_kept) for m in log)
    assert any(m.startswith("%d LTR-RTs detected, written to `%s`" % (n_kept, lay.out("ltr.scn"))) for m in log)
    assert any("no TSD or motif search" in m for m in log)
    assert not any("LTRs read from" in m for m in log)
    for ext in DOWNSTREAM:
        assert os.path.exists(lay.out(ext)), ext
    rows = open(lay.out("ltr.enrich")).read().splitlines()[1:]
    assert sum(r.split("\t")[1] in ("SG1", "SG2") for r in rows) >= 8
    # the same records through -ltr_scn: the same files
    p2, lay2 = _pipe(tmp_path / "fromfile", ltr_denovo=False, ltr_scn=lay.out("ltr.scn"))
    ctx2 = make(_DetectCtx)
    log2 = _run(p2, lay2, world, ctx2, caplog, with_ctx)
    assert not [c for c in ctx2.calls if c[0] == "seeds"] and "%d LTRs read from `%s`; no classification: every record is used, as under -all_ltr" % (
        n_kept, lay.out("ltr.scn")) in log2
    for ext in DOWNSTREAM:
        assert open(lay2.out(ext)).read() == open(lay.out(ext)).read(), ext
    assert not os.path.exists(lay2.out("ltr.scn"))


def test_options_reach_the_detector(tmp_path, world, caplog, with_ctx):
    chroms, kl, make = world
    opts = dict(ltr_seed=14, ltr_mindist=1200, ltr_maxdist=9000, ltr_minlen=150, ltr_maxlen=2000, ltr_xdrop=10, ltr_similar=97.0, ltr_chain_indel=8,
                ltr_chain_join=50, ltr_band=16)
    p, lay = _pipe(tmp_path / "opts", **opts)
    ctx = make(_DetectCtx)
    _run(p, lay, world, ctx, caplog, with_ctx)
    assert [c for c in ctx.calls if c[0] == "seeds"] == [("seeds", i, 14, 10, 1200, 9000, 2000) for i in range(4)]
    text = expected_scn(chroms, band=16, L=14, X=10, dmin=1200, dmax=9000, minlen=150, maxlen=2000, similar=97.0, indel=8, join=50)[0]
    assert open(lay.out("ltr.scn")).read() == text and text != expected_scn(chroms)[0]
    p, lay = _pipe(tmp_path / "bad", ltr_minlen=500, ltr_maxlen=400)
    with pytest.raises(ValueError, match="-ltr_minlen 500"):
        _run(p, lay, world, make(_DetectCtx), caplog, with_ctx)


def test_nothing_detected(tmp_path, world, caplog, with_ctx):
    chroms, kl, make = world
    p, lay = _pipe(tmp_path / "none", ltr_similar=100.5)
    log = _run(p, lay, world, make(_DetectCtx), caplog, with_ctx)
    assert open(lay.out("ltr.scn")).read() == ltr.SCN_HEADER and ltr.read_scn(lay.out("ltr.scn")) == []
    assert any(m.startswith("0 LTR-RTs detected") for m in log) and "0 significant subgenome-specific LTR-RTs" in log
    assert not os.path.exists(lay.out("ltr.insert.data"))


def test_no_cpu_detector_and_ranks(tmp_path, world, caplog, with_ctx, monkeypatch):
    chroms, kl, make = world
    p, lay = _pipe(tmp_path / "plain")
    with_ctx(make(OracleContext))
    with pytest.raises(RuntimeError, match="-ltr_denovo needs a context with ltr_seeds, ltr_hsps and ltr_align .*no CPU detector"):
        p.stage_ltr(lay, LABELS, _Cl(), kl)
    assert not os.path.exists(lay.out("ltr.scn"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    log = _run(p, lay, world, make(_DetectCtx), caplog, with_ctx)
    assert log == ["LTR stage skipped: it runs on one GPU, this is a run of 2 ranks"] and os.listdir(lay.root) == []


def test_switches(monkeypatch, caplog):
    def run(**flags):
        opts = dict(outdir="o", tmpdir="t", disable_circos=True)
        opts.update(flags)
        p = pipeline.Pipeline.bare(**opts)
        order = []

        class _C:
            d_sg, sg_names = {}, []
        monkeypatch.setattr(pipeline, "Layout", lambda *a: "lay")
        monkeypatch.setattr(p, "stage_ingest", lambda lay: (["f"], ["c"], {"c": 1}, {}), raising=False)
        monkeypatch.setattr(p, "stage_count_filter", lambda *a: None, raising=False)
        monkeypatch.setattr(p, "stage_cluster", lambda *a: (_C(), None), raising=False)
        for name in ("windows", "features", "blocks", "ltr"):
            monkeypatch.setattr(p, "stage_" + name, lambda *a, name=name: order.append(name), raising=False)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            p._run()
        return order, [r.getMessage() for r in caplog.records]
    order, log = run(ltr_denovo=True)
    assert order == ["windows", "ltr"] and len(log) == 1
    assert log[0].startswith("Of modules 3-4, TEsorter classification, the LTR trees and the circos figure are not part of this build")
    assert "LTR detection" not in log[0]
    order, log = run(ltr_scn="x.scn")
    assert order == ["windows", "ltr"] and log[0].startswith("Of modules 3-4, LTR detection, TEsorter classification, the LTR trees and the circos figure")
    order, log = run()
    assert order == ["windows"] and log[0].startswith("Modules 3-4 (LTR, circos) are not part of this build")
    assert run(ltr_denovo=True, disable_ltr=True)[0] == ["windows"]
    assert run(ltr_denovo=True, just_core=True)[0] == []


def test_cli_options():
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config"])
    assert args.ltr_denovo is False and args.ltr_scn is None
    assert (args.ltr_seed, args.ltr_mindist, args.ltr_maxdist, args.ltr_minlen, args.ltr_maxlen) == (20, 1000, 15000, 100, 7000)
    assert (args.ltr_xdrop, args.ltr_similar, args.ltr_chain_indel, args.ltr_chain_join, args.ltr_band) == (20, 85, 32, 200, 64)
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_denovo", "-ltr_seed", "16", "-ltr_mindist", "500", "-ltr_maxdist", "20000", "-ltr_minlen",
                                  "80", "-ltr_maxlen", "5000", "-ltr_xdrop", "12", "-ltr_similar", "90.5", "-ltr_chain_indel", "10", "-ltr_chain_join", "99"])
    assert args.ltr_denovo is True
    assert (args.ltr_seed, args.ltr_mindist, args.ltr_maxdist, args.ltr_minlen, args.ltr_maxlen) == (16, 500, 20000, 80, 5000)
    assert (args.ltr_xdrop, args.ltr_similar, args.ltr_chain_indel, args.ltr_chain_join) == (12, 90.5, 10, 99)


def test_denovo_and_scn_exclude_each_other(capsys):
    with pytest.raises(SystemExit):
        pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_denovo", "-ltr_scn", "tmp/LTR.scn"])
    assert "-ltr_denovo detects the LTR-RTs, -ltr_scn reads them from a file" in capsys.readouterr().err
    for flag in ("-ltr_seed", "-ltr_similar", "-ltr_chain_join"):
        with pytest.raises(SystemExit):
            pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", flag, "x"])
