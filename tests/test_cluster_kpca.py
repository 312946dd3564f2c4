"""Cluster.pca with stub contexts (no GPU): the numpy twin (tests/kpca_ref.py) stands in for the kernels.  The engine
choice and its log line, `.kmer.mat` input and wide matrices on the numpy path, the ValueError on a constant k-mer, the
clamp of n_components, the TSV, the figure, and stage_cluster calling pca before the staged rows are released."""
import logging
import os

import numpy as np
import pytest

import kpca_ref as kp
from subphaser_amd import cluster, kmer as kmerlib
from test_kpca_host import TOL, planted_case, sklearn_pca


class _Mat:
    pass


class _NoEntry:
    pass


def _matrix(ctx, name="C12", counts=None, lengths=None):
    if counts is None:
        counts, lengths, group, _ = planted_case(name)
    else:
        group = np.arange(counts.shape[1]) % 3
    M, C = counts.shape
    mat = _Mat()
    mat.labels = ["c%04d" % i for i in range(C)]
    mat.k = 15
    mat.keys = np.arange(M, dtype=np.uint64)
    mat.counts, mat.lengths = counts, lengths
    mat.freqs = counts / lengths.astype(np.float64)
    mat.ctx = ctx
    return mat, {c: "SG%d" % (g + 1) for c, g in zip(mat.labels, group.tolist())}


def _log(caplog):
    return [r.getMessage() for r in caplog.records if r.getMessage().startswith("k-mer PCA")]


def test_device_engine_is_chosen_and_is_the_twin(caplog):
    ctx = kp.TwinContext()
    mat, sg = _matrix(ctx)
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        assert cl.pca(n_components=3) is None
    assert cl.pca_engine == "device" and [c[0] for c in ctx.calls] == ["gram", "signs"]
    assert all(c[1] is mat.counts for c in ctx.calls)               # no staged rows: the host matrix
    msgs = _log(caplog)
    assert len(msgs) == 1 and "on the device" in msgs[0] and "staged" not in msgs[0]
    G, _ = ctx.kmer_pca_gram(mat.counts, mat.lengths)
    scores, percent, _ = kp.pca(G, lambda U: kp.signs(mat.counts, mat.lengths, U)[1], 3)
    assert (cl.pca_scores == scores).all() and (cl.pca_percent == percent).all()
    ref_scores, ref_percent = sklearn_pca(mat.freqs, 3)
    assert np.abs(cl.pca_scores - ref_scores).max() <= TOL and np.abs(cl.pca_percent - ref_percent).max() <= TOL


def test_staged_rows_are_used_when_present(caplog):
    ctx = kp.TwinContext()
    mat, sg = _matrix(ctx)
    mat.counts_dev = (mat.counts, mat.counts.shape[0], mat.counts.shape[1])     # what stage_rows returns, a host array for a pointer
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.pca()
    assert all(c[1] is mat.counts_dev for c in ctx.calls) and "(staged rows)" in _log(caplog)[0]
    assert cl.pca_scores.shape == (12, 2)


@pytest.mark.parametrize("ctx,why", [(None, "no device context"), (_NoEntry(), "no device context")])
def test_numpy_path_without_the_entries(caplog, ctx, why):
    mat, sg = _matrix(ctx)
    dev = cluster.Cluster(_matrix(kp.TwinContext())[0], n_clusters=3, sg_assigned=sg)
    dev.pca(n_components=3)
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.pca(n_components=3)
    msgs = _log(caplog)
    assert cl.pca_engine == "numpy" and len(msgs) == 1 and why in msgs[0] and msgs[0].endswith("using numpy")
    assert np.abs(cl.pca_scores - dev.pca_scores).max() <= TOL and np.abs(cl.pca_percent - dev.pca_percent).max() <= TOL


def test_kmer_mat_file_takes_the_numpy_path_with_equal_files(tmp_path, caplog):
    """the matrix written as `.kmer.mat` text (repr floats: an exact round trip) and read back has no counts: numpy, and
    the same TSV as the matrix in memory gives on the numpy path, byte for byte"""
    mat, sg = _matrix(None)
    path = tmp_path / "x.kmer.mat"
    kmers = kmerlib.decode_many(mat.keys, mat.k)
    with open(path, "w") as f:
        f.write("\t".join(["kmer"] + mat.labels) + "\n")
        for km, row in zip(kmers, mat.freqs.tolist()):
            f.write("\t".join([km] + [repr(v) for v in row]) + "\n")
    a = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    b = cluster.Cluster(str(path), n_clusters=3, sg_assigned=sg)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        a.pca(outtsv=str(tmp_path / "a.tsv"), n_components=3)
        b.pca(outtsv=str(tmp_path / "b.tsv"), n_components=3)
    assert a.pca_engine == b.pca_engine == "numpy" and len(_log(caplog)) == 2
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes()


def test_wider_than_the_device_limit_falls_to_numpy(caplog):
    ctx = kp.TwinContext()
    counts, lengths = kp.random_case(5, 40, 1025)
    mat, sg = _matrix(ctx, counts=counts, lengths=lengths)
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.pca()
    assert cl.pca_engine == "numpy" and ctx.calls == [] and "1025 chromosomes" in _log(caplog)[0]
    assert cl.pca_scores.shape == (1025, 2)


@pytest.mark.parametrize("ctx", [kp.TwinContext(), None], ids=["device", "numpy"])
def test_constant_kmer_is_a_value_error(ctx):
    counts, lengths, _, _ = planted_case("C12")
    counts = counts.copy()
    counts[7] = 0                                # x = 0 on every chromosome: sd = 0
    mat, sg = _matrix(ctx, counts=counts, lengths=lengths)
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    with pytest.raises(ValueError, match="Input contains NaN or infinity"):
        cl.pca()


@pytest.mark.parametrize("asked,C,kept", [(1, 12, 2), (0, 12, 2), (2, 12, 2), (5, 12, 5), (40, 12, 12), (3, 2, 2)])
def test_n_components_is_clamped(asked, C, kept):
    counts, lengths, _, _ = planted_case("C12")
    mat, sg = _matrix(kp.TwinContext(), counts=counts[:, :C], lengths=lengths[:C])
    cl = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg)
    cl.pca(n_components=asked)
    assert cl.pca_scores.shape == (C, kept) and cl.pca_percent.shape == (kept,)
    assert (np.diff(cl.pca_percent) <= 0).all() and cl.pca_percent.sum() <= 100 + 1e-9


def test_tsv_format(tmp_path):
    mat, sg = _matrix(kp.TwinContext())
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    out = tmp_path / "p.kmer_pca.tsv"
    cl.pca(outtsv=str(out), n_components=3)
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 2 + 12 + 1
    assert lines[0] == "#" + "\t".join("PC%d=%r%%" % (j + 1, float(p)) for j, p in enumerate(cl.pca_percent))
    assert lines[1] == "#chrom\tsubgenome\tPC1\tPC2\tPC3"
    for c, row, line in zip(cl.chrs, cl.pca_scores, lines[2:]):
        t = line.split("\t")
        assert t[:2] == [c, cl.d_sg[c]] and [float(v) for v in t[2:]] == row.tolist()      # repr: an exact round trip


def test_figure_is_written_and_can_be_deferred(tmp_path):
    pytest.importorskip("matplotlib")
    mat, sg = _matrix(kp.TwinContext())
    cl = cluster.Cluster(mat, n_clusters=3, sg_assigned=sg)
    fig = tmp_path / "p.kmer_pca.png"
    cl.pca(outfig=str(fig), n_components=3, colors="#ff0000,#00ff00,#0000ff")
    assert fig.stat().st_size > 1000 and fig.read_bytes()[:4] == b"\x89PNG"
    later = tmp_path / "later.png"
    write = cl.pca(outfig=str(later), defer=True)
    assert callable(write) and not later.exists()
    write()
    assert later.stat().st_size > 1000


class _Lay:
    def __init__(self, d):
        self.d = str(d)

    def out(self, name):
        return os.path.join(self.d, "t." + name)

    def ckp(self, path):
        return path + ".ok"


class _StagingTwin(kp.TwinContext):
    """records the order of PCA calls and of the release of the staged rows"""

    def __init__(self):
        super().__init__()
        self.events = []

    def stage_rows(self, counts):
        self.events.append("stage")
        return (counts, counts.shape[0], counts.shape[1])

    def release_rows(self):
        self.events.append("release")

    def kmer_pca_gram(self, counts, lengths, want_stats=False):
        self.events.append("gram staged" if isinstance(counts, tuple) else "gram host")
        return super().kmer_pca_gram(counts, lengths, want_stats)


def _pipeline(nsg=3):
    from subphaser_amd import pipeline
    return pipeline.Pipeline.bare(nsg=nsg, replicates=0, bootstrap_seed=1, figfmt="png")


def test_stage_cluster_runs_pca_before_the_rows_are_released(tmp_path, caplog):
    ctx = _StagingTwin()
    mat, sg = _matrix(ctx)
    mat.counts_dev = ctx.stage_rows(mat.counts)
    p = _pipeline()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl, _ = p.stage_cluster(_Lay(tmp_path), mat, sg)
    assert ctx.events.index("gram staged") < ctx.events.index("release") and "gram host" not in ctx.events
    assert cl.pca_engine == "device" and cl.pca_scores.shape == (12, 3)
    tsv = tmp_path / "t.kmer_pca.tsv"
    assert tsv.exists() and (tmp_path / "t.kmer_pca.tsv.ok").exists()
    assert not (tmp_path / "t.kmer_pca.png").exists()             # the figure waits for the background queue
    p._finish_background()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    else:
        assert (tmp_path / "t.kmer_pca.png").stat().st_size > 1000 and (tmp_path / "t.kmer_pca.png.ok").exists()


def test_stage_cluster_survives_a_pca_failure_but_not_bad_input(tmp_path, caplog):
    class Broken(_StagingTwin):
        def kmer_pca_signs(self, counts, lengths, U):
            raise RuntimeError("boom")
    mat, sg = _matrix(Broken())
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        _pipeline().stage_cluster(_Lay(tmp_path), mat, sg)
    assert any("k-mer PCA not written: boom" in r.getMessage() for r in caplog.records)
    assert (tmp_path / "t.chrom-subgenome.tsv").exists() and (tmp_path / "t.sig.kmer-subgenome.tsv").exists()
    assert not (tmp_path / "t.kmer_pca.tsv.ok").exists()
    counts, lengths, _, _ = planted_case("C12")
    counts = counts.copy()
    counts[0] = 0
    mat, sg = _matrix(_StagingTwin(), counts=counts, lengths=lengths)
    d2 = tmp_path / "bad"
    d2.mkdir()
    with pytest.raises(ValueError, match="Input contains NaN or infinity"):
        _pipeline().stage_cluster(_Lay(d2), mat, sg)
    assert (d2 / "t.chrom-subgenome.tsv").exists()                # written before the PCA: still there


def test_single_chromosome_is_skipped(tmp_path, caplog):
    from subphaser_amd import pipeline

    class One:
        chrs = ["only"]
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        _pipeline()._pca(_Lay(tmp_path), One())
    assert any("k-mer PCA skipped" in r.getMessage() for r in caplog.records) and os.listdir(tmp_path) == []
