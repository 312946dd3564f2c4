"""Cluster.heatmap and the pipeline's heatmap step without a GPU: the numpy twin (tests/hclust_ref.py) stands in for the
kernels behind a recording context.  The engine choice and its log line, the sample, the ddof = 1 Z-scores, the TSV, `NA`
labels, the colour panel, the figure, and the CLI options around it."""
import logging
import os

import numpy as np
import pytest

import hclust_ref as hc
from subphaser_amd import _native, cluster, heatmap as hm, kmer as kmerlib
from subphaser_amd.seqs import KmerLabels
from test_kpca_host import planted_case

SIZE = 150


class _Mat:
    pass


class _NoEntry:
    pass


def _matrix(ctx, rows=600, constant=()):
    counts, lengths, group, _ = planted_case("C12")
    counts = counts[:rows].copy()
    for r in constant:
        counts[r] = 0
    M, C = counts.shape
    mat = _Mat()
    mat.labels = ["c%04d" % i for i in range(C)]
    mat.k = 15
    mat.keys = np.arange(M, dtype=np.uint64) * np.uint64(7919) + np.uint64(11)
    mat.counts, mat.lengths = counts, lengths
    mat.freqs = counts / lengths.astype(np.float64)
    mat.ctx = ctx
    return mat, {c: "SG%d" % (g + 1) for c, g in zip(mat.labels, group.tolist())}


def _cluster(ctx, seed=5, **kw):
    mat, sg = _matrix(ctx, **kw)
    return cluster.Cluster(mat, n_clusters=3, sg_assigned=sg, seed=seed), mat


def _labels(mat, rows, names=("SG1", "SG2", "SG3")):
    rows = np.asarray(rows)
    return KmerLabels(kmerlib.canonical(mat.keys[rows], mat.k), (rows % len(names)).astype(np.uint8), list(names), mat.k)


def _log(caplog, level=None):
    return [r.getMessage() for r in caplog.records
            if r.getMessage().startswith("heatmap") and (level is None or r.levelno == level)]


def _scipy(z):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    return linkage(pdist(np.ascontiguousarray(z.T)), "complete"), linkage(pdist(z), "complete")


def test_device_engine_is_chosen_and_is_the_twin(caplog):
    from scipy.cluster.hierarchy import leaves_list
    ctx = hc.TwinContext()
    cl, mat = _cluster(ctx)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        assert cl.heatmap(None, size=SIZE) is None
    assert cl.heatmap_engine == "device" and ctx.calls == [(SIZE, 12), (12, SIZE)]
    msgs = _log(caplog)
    assert len(msgs) == 2 and "left out" in msgs[0] and "on the device" in msgs[1]
    z = cl.heatmap_z
    assert (cl.heatmap_col_linkage == hm.to_linkage(hc.hclust(z.T)[0], SIZE)).all()
    assert (cl.heatmap_row_linkage == hm.to_linkage(hc.hclust(z)[0], 12)).all()
    assert (cl.heatmap_kmer_order == leaves_list(cl.heatmap_col_linkage)).all()
    assert (cl.heatmap_chrom_order == hm.reorder(cl.heatmap_row_linkage, z.mean(axis=1))).all()
    assert sorted(cl.heatmap_chrom_order.tolist()) == list(range(12))
    # scipy on its own distances: the same trees up to the rounding of pdist (tests/test_hclust_host.py derives the bound)
    col, row = _scipy(z)
    tol = lambda D: (D + 2) * 2.0 ** -52
    assert (np.abs(cl.heatmap_col_linkage[:, 2] - col[:, 2]) <= tol(12) * col[:, 2]).all()
    assert (np.abs(cl.heatmap_row_linkage[:, 2] - row[:, 2]) <= tol(SIZE) * row[:, 2]).all()


def test_kmer_mat_file_takes_scipy(tmp_path, caplog):
    mat, sg = _matrix(None)
    path = tmp_path / "x.kmer.mat"
    with open(path, "w") as f:
        f.write("\t".join(["kmer"] + mat.labels) + "\n")
        for km, row in zip(kmerlib.decode_many(mat.keys, mat.k), mat.freqs.tolist()):
            f.write("\t".join([km] + [repr(v) for v in row]) + "\n")
    a = cluster.Cluster(str(path), n_clusters=3, sg_assigned=sg, seed=5)
    b = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg, seed=5)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        a.heatmap(None, outtsv=str(tmp_path / "a.tsv"), size=SIZE)
        b.heatmap(None, outtsv=str(tmp_path / "b.tsv"), size=SIZE)
    assert a.heatmap_engine == b.heatmap_engine == "scipy"
    assert sum("no device context" in m and m.endswith("using scipy") for m in _log(caplog)) == 2
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes()
    col, row = _scipy(a.heatmap_z)
    assert (a.heatmap_col_linkage == col).all() and (a.heatmap_row_linkage == row).all()


def test_context_without_the_entry_takes_scipy(caplog):
    cl, _ = _cluster(_NoEntry())
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.heatmap(None, size=SIZE)
    assert cl.heatmap_engine == "scipy" and any("no device context" in m for m in _log(caplog))


def test_more_points_than_the_device_takes_goes_to_scipy(caplog, monkeypatch):
    """the limit is lowered instead of sampling 16385 k-mers: what is tested is the comparison, and scipy on 16385 points
    takes a gigabyte"""
    ctx = hc.TwinContext()
    cl, _ = _cluster(ctx)
    monkeypatch.setattr(_native, "HCLUST_MAX_POINTS", SIZE - 1)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.heatmap(None, size=SIZE)
    assert cl.heatmap_engine == "scipy" and ctx.calls == []
    assert any("{} k-mers x 12 chromosomes".format(SIZE) in m and str(SIZE - 1) in m for m in _log(caplog))
    monkeypatch.setattr(_native, "HCLUST_MAX_POINTS", SIZE)
    cl.heatmap(None, size=SIZE)
    assert cl.heatmap_engine == "device" and len(ctx.calls) == 2


def test_sample_is_sorted_seeded_and_skips_constant_rows(caplog):
    constant = (0, 17, 599)
    cl, mat = _cluster(hc.TwinContext(), constant=constant)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.heatmap(None, size=SIZE)
    rows = cl.heatmap_rows
    assert len(rows) == SIZE and (np.diff(rows) > 0).all() and not set(rows.tolist()) & set(constant)
    assert _log(caplog)[0].startswith("heatmap: 3 of 600 k-mers left out")
    good = np.array([r for r in range(600) if r not in constant])
    assert (rows == good[hm.sample_rows(597, SIZE, 5)]).all()
    again, _ = _cluster(hc.TwinContext(), constant=constant)
    again.heatmap(None, size=SIZE)
    other, _ = _cluster(hc.TwinContext(), seed=6, constant=constant)
    other.heatmap(None, size=SIZE)
    assert (again.heatmap_rows == rows).all() and (other.heatmap_rows != rows).any()
    # all rows when the pool is not larger than the sample
    cl.heatmap(None, size=597)
    assert (cl.heatmap_rows == good).all()
    cl.heatmap(None, size=10000)
    assert (cl.heatmap_rows == good).all()


def test_zscores_use_the_sample_variance():
    cl, mat = _cluster(hc.TwinContext())
    cl.heatmap(None, size=SIZE)
    x = mat.freqs[cl.heatmap_rows]
    z = ((x - x.mean(axis=1, keepdims=True)) / np.sqrt(x.var(axis=1, ddof=1, keepdims=True))).T
    assert cl.heatmap_z.shape == (12, SIZE) and (cl.heatmap_z == z).all()
    assert np.abs(cl.heatmap_z.var(axis=0, ddof=1) - 1).max() < 1e-12 and np.abs(cl.heatmap_z.mean(axis=0)).max() < 1e-12
    assert np.abs(cl.zscores()[:, cl.heatmap_rows] - cl.heatmap_z).max() > 1e-3       # zscores() is ddof = 0: not this


def test_tsv_shape_round_trip_and_na(tmp_path):
    cl, mat = _cluster(hc.TwinContext())
    cl.heatmap(None, size=SIZE)                                # to learn the sample
    labelled = cl.heatmap_rows[::3]
    labels = _labels(mat, labelled)
    out = tmp_path / "h.tsv"
    cl.heatmap(labels, outtsv=str(out), size=SIZE)
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 1 + SIZE + 1
    head = lines[0].split("\t")
    assert head[:2] == ["#kmer", "subgenome"] and head[2:] == [cl.chrs[i] for i in cl.heatmap_chrom_order]
    kmers = kmerlib.decode_many(mat.keys[cl.heatmap_rows], mat.k)
    want_sg = {int(r): "SG%d" % (int(r) % 3 + 1) for r in labelled}
    n_na = 0
    for j, line in zip(cl.heatmap_kmer_order.tolist(), lines[1:]):
        t = line.split("\t")
        assert len(t) == 2 + 12 and t[0] == kmers[j]
        assert t[1] == want_sg.get(int(cl.heatmap_rows[j]), "NA")
        n_na += t[1] == "NA"
        assert [float(v) for v in t[2:]] == cl.heatmap_z[cl.heatmap_chrom_order, j].tolist()      # repr: an exact round trip
    assert n_na == SIZE - len(labelled)
    cl.heatmap(None, outtsv=str(out), size=SIZE)
    assert all(l.split("\t")[1] == "NA" for l in out.read_text().split("\n")[1:-1])


def test_colour_panels(tmp_path):
    pytest.importorskip("matplotlib")
    cl, mat = _cluster(hc.TwinContext())
    for panel in (("blue", "yellow"), ("green", "black", "red"), "#0000ff,#ffffff,#ff0000"):
        fig = tmp_path / ("p%d.png" % len(os.listdir(tmp_path)))
        cl.heatmap(_labels(mat, np.arange(0, 600, 2)), outfig=str(fig), size=SIZE, heatmap_colors=panel)
        assert fig.stat().st_size > 1000 and fig.read_bytes()[:4] == b"\x89PNG"
    lv = hm.color_levels(("green", "black", "red"), 100)
    assert lv.shape == (100, 3) and lv[0].tolist() == [0.0, 0.5019607843137255, 0.0] and lv[-1].tolist() == [1.0, 0.0, 0.0]
    assert lv[49].max() < 0.02 and lv[50].max() < 0.02
    for bad in (("a", "b", "c", "d"), ("red",), ()):
        with pytest.raises(ValueError, match="2 or 3 colours"):
            cl.heatmap(None, size=SIZE, heatmap_colors=bad)


def test_figure_under_agg_and_deferred(tmp_path):
    matplotlib = pytest.importorskip("matplotlib")
    cl, mat = _cluster(hc.TwinContext())
    later = tmp_path / "later.png"
    write = cl.heatmap(_labels(mat, np.arange(0, 600, 5)), outfig=str(later), size=SIZE, colors="#ff0000,#00ff00,#0000ff",
                       defer=True)
    assert callable(write) and not later.exists()
    write()
    assert later.stat().st_size > 1000 and later.read_bytes()[:4] == b"\x89PNG"
    assert matplotlib.get_backend().lower() == "agg"


def test_too_few_kmers_or_chromosomes_is_a_skip(caplog, tmp_path):
    cl, _ = _cluster(hc.TwinContext(), rows=5, constant=(0, 1, 2, 3))
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        assert cl.heatmap(None, outtsv=str(tmp_path / "x.tsv"), size=SIZE) is None
    assert cl.heatmap_engine is None and any(m.startswith("heatmap skipped") for m in _log(caplog))
    assert not (tmp_path / "x.tsv").exists()


# ------------------------------------------------------------------------------------------------- the pipeline
class _Lay:
    def __init__(self, d):
        self.d = str(d)

    def out(self, name):
        return os.path.join(self.d, "t." + name)

    def ckp(self, path):
        return path + ".ok"


def _pipeline(**kw):
    from subphaser_amd import pipeline
    opts = dict(nsg=3, replicates=0, bootstrap_seed=1, figfmt="png", heatmap_size=SIZE)
    opts.update(kw)
    return pipeline.Pipeline.bare(**opts)


def test_option_is_parsed():
    from subphaser_amd import pipeline
    base = ["-i", "g.fa", "-c", "sg.cfg"]
    assert pipeline.makeArgparse(base).heatmap_size == 10000
    args = pipeline.makeArgparse(base + ["-heatmap_size", "500", "-heatmap_colors", "blue", "white"])
    assert args.heatmap_size == 500 and list(args.heatmap_colors) == ["blue", "white"]
    assert pipeline.makeArgparse(base + ["-heatmap_size", "0"]).heatmap_size == 0


def test_stage_cluster_draws_the_heatmap_after_output_kmers(tmp_path, caplog, monkeypatch):
    events = []
    real_kmers, real_heatmap = cluster.Cluster.output_kmers, cluster.Cluster.heatmap

    def output_kmers(self, *a, **kw):
        events.append("output_kmers")
        return real_kmers(self, *a, **kw)

    def heatmap(self, kmer_labels, *a, **kw):
        events.append(("heatmap", kmer_labels))
        return real_heatmap(self, kmer_labels, *a, **kw)
    monkeypatch.setattr(cluster.Cluster, "output_kmers", output_kmers)
    monkeypatch.setattr(cluster.Cluster, "heatmap", heatmap)
    ctx = hc.TwinContext()
    mat, sg = _matrix(ctx)
    p = _pipeline()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl, labels = p.stage_cluster(_Lay(tmp_path), mat, sg)
    assert [e if isinstance(e, str) else e[0] for e in events] == ["output_kmers", "heatmap"] and events[1][1] is labels
    assert cl.heatmap_engine == "device" and len(ctx.calls) == 2
    tsv = tmp_path / "t.kmer.mat.heatmap.tsv"
    assert tsv.exists() and (tmp_path / "t.kmer.mat.heatmap.tsv.ok").exists()
    sgs = {l.split("\t")[1] for l in tsv.read_text().split("\n")[1:-1]}
    assert sgs <= {"SG1", "SG2", "SG3", "NA"} and sgs & {"SG1", "SG2", "SG3"}       # planted k-mers are significant
    assert not (tmp_path / "t.kmer.mat.png").exists()             # the figure waits for the background queue
    p._finish_background()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / "t.kmer.mat.png").stat().st_size > 1000 and (tmp_path / "t.kmer.mat.png.ok").exists()


def test_size_zero_skips_and_options_warn(tmp_path, caplog):
    cl, _ = _cluster(hc.TwinContext())
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        _pipeline(heatmap_size=0, heatmap_options="Rowv=FALSE")._heatmap(_Lay(tmp_path), cl, None)
    assert os.listdir(tmp_path) == [] and any("heatmap skipped: -heatmap_size 0" in m for m in _log(caplog))
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "-heatmap_options" in warned[0] and "Rowv=FALSE" in warned[0]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        _pipeline()._heatmap(_Lay(tmp_path), cl, None)
    assert not [r for r in caplog.records if r.levelno == logging.WARNING]
    assert (tmp_path / "t.kmer.mat.heatmap.tsv").exists()


def test_only_a_wrong_colour_count_stops_the_run(tmp_path, caplog):
    cl, _ = _cluster(hc.TwinContext())
    with pytest.raises(ValueError, match="2 or 3 colours"):
        _pipeline(heatmap_colors=("a", "b", "c", "d"))._heatmap(_Lay(tmp_path), cl, None)

    class Broken:
        def hclust_complete(self, points, want_dist=False):
            raise RuntimeError("boom")
    cl2, _ = _cluster(Broken())
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        _pipeline()._heatmap(_Lay(tmp_path), cl2, None)
    assert any("heatmap not written: boom" in r.getMessage() for r in caplog.records)
    assert not (tmp_path / "t.kmer.mat.heatmap.tsv.ok").exists()

    class One:
        chrs = ["only"]
    _pipeline()._heatmap(_Lay(tmp_path), One(), None)
    assert not (tmp_path / "t.kmer.mat.heatmap.tsv").exists()
