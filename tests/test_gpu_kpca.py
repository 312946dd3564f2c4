"""GPU: the k-mer PCA kernels (sp_kpca.hip: kp_rowstats, kp_gram, kp_gram_sum, kp_signs; Context.kmer_pca_gram /
kmer_pca_signs) against the numpy twin (tests/kpca_ref.py) with `==`: row statistics, the Gram matrix, the bad-row count,
sign rows and values; rows from a host pointer and staged on the device; the error codes; Cluster.pca through the real
context against its numpy path; the CLI on the toy genome.

Tolerance of the two comparisons that are not bit for bit: TOL of tests/test_kpca_host.py (100 x the measured
twin-vs-scikit-learn difference on the planted matrices).  The device path IS the twin (same bits into the same eigh), so
device against numpy is twin against numpy."""
import ctypes
import logging

import numpy as np
import pytest

import kpca_ref as kp
from subphaser_amd import _native, cluster
from test_kpca_host import TOL, planted_case

pytestmark = pytest.mark.gpu

R = kp.ROWS
_twin = {}


def _case(C, M, extreme=False, bad=(), dup=None):
    """inputs and the twin's answers, computed once per shape and left unchanged"""
    key = (C, M, extreme, bad, dup)
    if key not in _twin:
        counts, lengths = kp.random_case(1000 * C + M % 997, M, C, extreme, bad, dup)
        G, n_bad, stats = kp.gram(counts, lengths)
        for a in (counts, lengths, G, stats):
            a.setflags(write=False)
        _twin[key] = (counts, lengths, G, n_bad, stats)
    return _twin[key]


def _check_gram(ctx, counts, lengths, G, n_bad, stats, staged):
    rows = ctx.stage_rows(counts) if staged else counts
    try:
        g, nb, st = ctx.kmer_pca_gram(rows, lengths, want_stats=True)
        g2, nb2 = ctx.kmer_pca_gram(rows, lengths)
    finally:
        if staged:
            ctx.release_rows()
    assert (st == stats).all(), np.argwhere(st != stats)[:5]
    assert nb == nb2 == n_bad
    assert (g == G).all(), np.argwhere(g != G)[:5]
    assert g2.tobytes() == g.tobytes()


@pytest.mark.parametrize("M", [1, R - 1, R, R + 1, 3 * R + 7])
@pytest.mark.parametrize("C", [2, 3, 21, 33, 64, 65, 128, 129])
def test_gram_and_stats_are_the_twin(gpu_ctx, C, M):
    counts, lengths, G, n_bad, stats = _case(C, M)
    _check_gram(gpu_ctx, counts, lengths, G, n_bad, stats, staged=False)
    _check_gram(gpu_ctx, counts, lengths, G, n_bad, stats, staged=True)


def test_gram_at_the_chromosome_limit(gpu_ctx):
    counts, lengths, G, n_bad, stats = _case(1024, R + 1)
    _check_gram(gpu_ctx, counts, lengths, G, n_bad, stats, staged=True)


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
def test_extreme_counts_and_bad_rows_in_three_chunks(gpu_ctx, staged):
    M = 3 * R + 7
    bad = (3, R + 500, M - 1)                  # the first, a middle and the last chunk
    counts, lengths, G, n_bad, stats = _case(21, M, True, bad, (10, M - 2))
    assert counts.max() == 2 ** 32 - 1 and counts.min() == 0 and lengths.max() > 2 ** 32 and n_bad == 3
    _check_gram(gpu_ctx, counts, lengths, G, n_bad, stats, staged)
    # the rows are skipped: every good row adds z . z = C to the trace
    assert np.isfinite(G).all() and abs(np.trace(G) - 21 * (M - 3)) <= 4 * 21 * M * 2.0 ** -52 * 21


@pytest.mark.parametrize("n_comp", [1, 2, 32])
@pytest.mark.parametrize("C,M", [(21, 3 * R + 7), (129, R + 1), (2, 1)])
def test_sign_rows_are_the_twin(gpu_ctx, C, M, n_comp):
    counts, lengths = _case(C, M)[:2]
    U = np.random.default_rng(n_comp).normal(size=(C, n_comp))
    rows, vals = gpu_ctx.kmer_pca_signs(counts, lengths, U)
    trows, tvals = kp.signs(counts, lengths, U)
    assert rows.dtype == np.int64 and (rows == trows).all() and (vals == tvals).all()
    staged = gpu_ctx.stage_rows(counts)
    try:
        rows2, vals2 = gpu_ctx.kmer_pca_signs(staged, lengths, U)
    finally:
        gpu_ctx.release_rows()
    assert (rows2 == rows).all() and (vals2 == vals).all()


def test_sign_row_ties_and_the_last_row(gpu_ctx):
    C, M = 21, 3 * R + 7
    counts, lengths = _case(C, M)[:2]
    U = np.random.default_rng(77).normal(size=(C, 2))
    base, _ = kp.signs(counts, lengths, U)
    # the maximal row of component 0 duplicated further down, and in another workgroup: the lowest index wins
    dup = counts.copy()
    later = [int(base[0]) + 1, M - 5] if base[0] < M - 6 else [M - 1]
    dup[later] = counts[base[0]]
    rows, vals = gpu_ctx.kmer_pca_signs(dup, lengths, U)
    trows, tvals = kp.signs(dup, lengths, U)
    assert (rows == trows).all() and (vals == tvals).all() and rows[0] == base[0]
    # the maximal row of component 1 moved to the last row of the last chunk
    last = counts.copy()
    last[[int(base[1]), M - 1]] = counts[[M - 1, int(base[1])]]
    rows, vals = gpu_ctx.kmer_pca_signs(last, lengths, U)
    trows, tvals = kp.signs(last, lengths, U)
    assert (rows == trows).all() and (vals == tvals).all() and rows[1] == M - 1


def test_all_rows_bad(gpu_ctx):
    counts, lengths = np.zeros((R + 3, 5), np.uint32), np.arange(1, 6, dtype=np.int64)
    G, n_bad = gpu_ctx.kmer_pca_gram(counts, lengths)
    assert n_bad == R + 3 and (G == 0).all()
    rows, vals = gpu_ctx.kmer_pca_signs(counts, lengths, np.ones((5, 3)))
    assert (rows == -1).all() and (vals == 0).all()


def _raw(ctx, which, C, M, n_comp=2, zero_len=False):
    counts = np.ones((max(M, 1), max(C, 1)), np.uint32)
    lengths = np.full(max(C, 1), 1000, np.int64)
    if zero_len:
        lengths[-1] = 0
    vp = ctypes.c_void_p
    if which == "gram":
        gram, n_bad = np.full((max(C, 1), max(C, 1)), -7.0), ctypes.c_int64(-7)
        rc = ctx.L.sp_kmer_pca_gram(ctx.h, vp(counts.ctypes.data), M, C, vp(lengths.ctypes.data), vp(gram.ctypes.data),
                                    ctypes.byref(n_bad), None)
        return rc, (gram == -7).all() and n_bad.value == -7
    U = np.ones((max(C, 1), max(n_comp, 1)))
    rows, vals = np.full(max(n_comp, 1), -7, np.int64), np.full(max(n_comp, 1), -7.0)
    rc = ctx.L.sp_kmer_pca_signs(ctx.h, vp(counts.ctypes.data), M, C, vp(lengths.ctypes.data), vp(U.ctypes.data), n_comp,
                                 vp(rows.ctypes.data), vp(vals.ctypes.data))
    return rc, (rows == -7).all() and (vals == -7).all()


@pytest.mark.parametrize("which,C,M,n_comp,zero_len,code", [
    ("gram", 1, 10, 2, False, _native.SP_EINVAL), ("signs", 1, 10, 2, False, _native.SP_EINVAL),
    ("gram", 5, 0, 2, False, _native.SP_EINVAL), ("signs", 5, 0, 2, False, _native.SP_EINVAL),
    ("signs", 5, 10, 33, False, _native.SP_EINVAL), ("signs", 5, 10, 0, False, _native.SP_EINVAL),
    ("gram", 1025, 3, 2, False, _native.SP_EUNSUP), ("signs", 1025, 3, 2, False, _native.SP_EUNSUP),
    ("gram", 5, 10, 2, True, _native.SP_EINVAL), ("signs", 5, 10, 2, True, _native.SP_EINVAL)])
def test_error_codes(gpu_ctx, which, C, M, n_comp, zero_len, code):
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        rc, untouched = _raw(gpu_ctx, which, C, M, n_comp, zero_len)
        launched = gpu_ctx.prof_report()
    finally:
        gpu_ctx.prof_enable(False)
    assert rc == code, gpu_ctx.L.sp_last_error(gpu_ctx.h)
    assert untouched and not any(k.startswith("kp_") for k in launched)      # nothing launched, nothing written
    assert ("sp_kmer_pca_" + which).encode() in gpu_ctx.L.sp_last_error(gpu_ctx.h)


def test_binding_raises_value_error(gpu_ctx):
    with pytest.raises(ValueError, match="sp_kmer_pca_gram"):
        gpu_ctx.kmer_pca_gram(np.ones((4, 1025), np.uint32), np.ones(1025, np.int64))
    with pytest.raises(ValueError, match="sp_kmer_pca_signs"):
        gpu_ctx.kmer_pca_signs(np.ones((4, 5), np.uint32), np.ones(5, np.int64), np.ones((5, 33)))


class _Mat:
    pass


@pytest.mark.parametrize("name", ["C12", "C21"])
def test_cluster_pca_device_against_numpy(gpu_ctx, name, caplog):
    counts, lengths, group, freqs = planted_case(name)
    sg = {}
    mats = []
    for ctx in (gpu_ctx, None):
        mat = _Mat()
        mat.labels = ["c%03d" % i for i in range(counts.shape[1])]
        mat.k, mat.keys = 15, np.arange(counts.shape[0], dtype=np.uint64)
        mat.counts, mat.lengths, mat.freqs, mat.ctx = counts, lengths, freqs, ctx
        mats.append(mat)
        sg = {c: "SG%d" % (g + 1) for c, g in zip(mat.labels, group.tolist())}
    dev = cluster.Cluster(mats[0], n_clusters=3, sg_assigned=sg)
    host = cluster.Cluster(mats[1], n_clusters=3, sg_assigned=sg)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        dev.pca(n_components=3)
        host.pca(n_components=3)
    assert dev.pca_engine == "device" and host.pca_engine == "numpy"
    ds, dp = np.abs(dev.pca_scores - host.pca_scores).max(), np.abs(dev.pca_percent - host.pca_percent).max()
    print("%s: device against numpy: scores %.2e, percentages %.2e" % (name, ds, dp))
    assert ds <= TOL and dp <= TOL
    # and the device path is the twin's recipe to the bit
    G, _, _ = kp.gram(counts, lengths)
    scores, percent, _ = kp.pca(G, lambda U: kp.signs(counts, lengths, U)[1], 3)
    assert (dev.pca_scores == scores).all() and (dev.pca_percent == percent).all()


def test_cli_writes_the_pca(gpu_ctx, toy, tmp_path, caplog):
    """The toy genome through the CLI: `.kmer_pca.tsv` and the figure appear next to the other outputs, the PCA ran on the
    device from the staged rows, and the coordinates agree with the numpy path on the run's own `.kmer.mat`.
    Margin over TOL for the trip through the text file: none.  The matrix is written with the shortest digits that read
    back to the same double (repr), so the numpy path starts from the bits count / length the device divides out itself;
    what remains is the difference of the two summation orders, which TOL covers (the toy's eigenvalues are further
    apart, relative to the largest, than the planted matrices' on which TOL was measured: 9e-3 against 4e-5)."""
    from subphaser_amd import pipeline, runtime
    fa = tmp_path / "toy.fa"
    with open(fa, "w") as f:
        for lab in toy["labels"]:
            f.write(">%s\n%s\n" % (lab, toy["seqs"][lab]))
    cfg = tmp_path / "sg.config"
    cfg.write_text("\n".join("\t".join(",".join(u) for u in sg) for sg in toy["sgs"]) + "\n")
    asg = tmp_path / "assigned.tsv"
    asg.write_text("".join("%s\t%s\n" % kv for kv in toy["sg_assigned"].items()))
    out, tmpd = tmp_path / "out", tmp_path / "tmp"
    old = runtime._ctx
    runtime.set_context(gpu_ctx)
    try:
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-sg_assigned", str(asg), "-q", "30", "-k", "15", "-o", str(out),
                           "-tmpdir", str(tmpd), "-window_size", "2500", "-disable_ltr", "-disable_circos", "-figfmt", "png",
                           "-replicates", "20", "-bootstrap_seed", "1"])
    finally:
        runtime._ctx = old
    log = [r.getMessage() for r in caplog.records if r.getMessage().startswith("k-mer PCA")]
    assert any("on the device (staged rows)" in m for m in log) and not any("using numpy" in m for m in log)
    base = str(out / "k15_q30_f2")
    lines = open(base + ".kmer_pca.tsv").read().rstrip("\n").split("\n")
    K = len(set(toy["sg_assigned"].values()))
    assert lines[0].startswith("#PC1=") and lines[1].split("\t") == ["#chrom", "subgenome"] + ["PC%d" % (j + 1) for j in range(max(2, K))]
    percent = np.array([float(t.split("=")[1].rstrip("%")) for t in lines[0][1:].split("\t")])
    got = {t[0]: (t[1], [float(v) for v in t[2:]]) for t in (l.split("\t") for l in lines[2:])}
    ref = cluster.Cluster(base + ".kmer.mat", n_clusters=K, sg_assigned=dict(toy["sg_assigned"]))
    ref.pca(n_components=K)
    assert ref.pca_engine == "numpy" and list(got) == ref.chrs
    assert [got[c][0] for c in ref.chrs] == [ref.d_sg[c] for c in ref.chrs]
    scores = np.array([got[c][1] for c in ref.chrs])
    ds, dp = np.abs(scores - ref.pca_scores).max(), np.abs(percent - ref.pca_percent).max()
    print("toy CLI: device against numpy on the written matrix: scores %.2e, percentages %.2e" % (ds, dp))
    assert ds <= TOL and dp <= TOL
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    with open(base + ".kmer_pca.png", "rb") as f:
        assert f.read(4) == b"\x89PNG"
