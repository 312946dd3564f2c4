"""GPU: the k-means bootstrap kernel (sp_kboot.hip: kb_bootstrap, Context.kmeans_bootstrap) against the numpy twin
(tests/kboot_ref.py): the Gram matrices bit for bit, labels and iteration counts on every replicate the twin calls decided
(at most 1 % of a case may be undecided); the error codes; a matrix staged on the device; the CLI and Cluster with
bootstrap_engine = device."""
import ctypes
import io
import logging

import numpy as np
import pytest

import kboot_ref as kr
from subphaser_amd import _native, cluster

pytestmark = pytest.mark.gpu

TILE = 32      # SP_KB_TILE: columns staged per chunk

# C, K, n, R, M -- the kernel has one instance for C <= 32, one for C <= 64, one for C <= 128
CASES = {
    "minimum_one_column_matrix": (2, 2, 1, 1, 1),
    "minimum_many_workgroups": (2, 2, TILE - 1, 600, 50),
    "every_point_a_centre": (3, 3, TILE, 600, 40),
    "typical": (21, 3, 1000, 600, 5000),
    "last_of_first_instance": (32, 5, TILE + 1, 4, 200),
    "first_of_second_instance": (33, 4, TILE + 1, 5, 200),
    "mid": (64, 7, TILE + 1, 20, 300),
    "first_of_third_instance": (65, 5, TILE - 1, 3, 300),
    "limit": (128, 32, 1000, 3, 2000),
    "limit_one_replicate_one_tile": (128, 32, TILE, 1, 500),
    "one_cluster": (21, 1, TILE, 4, 100),
    "one_cluster_at_limit": (128, 1, TILE - 1, 2, 100),
}


def _case(name):
    C, K, n, R, M = CASES[name]
    i = sorted(CASES).index(name)
    z = kr.blobs(200 + i, C, max(K, 2), M, noise=0.8) if M > 1 else np.array([[1.0], [-1.0]])
    cols = np.random.RandomState(i).randint(0, M, size=(R, n)).astype(np.int64)
    if n >= 8:                      # the first and the last column, and one column several times
        cols[0, 0], cols[0, 1], cols[-1, -1] = 0, M - 1, M - 1
        cols[0, 2:6] = cols[0, 6]
    return z, cols, K, 0xC0FFEE + 977 * i


def _check(gpu_ctx, z, cols, K, seed):
    labels, iters, gram = gpu_ctx.kmeans_bootstrap(z, cols, K, seed, want_gram=True)
    R, C = cols.shape[0], z.shape[0]
    assert labels.shape == (R, C) and labels.dtype == np.int32 and iters.shape == (R,) and gram.shape == (R, C, C)
    G = kr.gram(z, cols)
    assert gram.tobytes() == G.tobytes(), np.argwhere(gram != G)[:5]
    rl, ri, gaps = kr.solve_all(G, K, seed)
    ok = kr.decided(gaps)
    print("%d of %d decided, smallest gap %.1e, iterations %d..%d" % (int(ok.sum()), R, float(gaps.min()), int(ri.min()),
                                                                     int(ri.max())))
    assert (iters[ok] == ri[ok]).all(), np.nonzero(iters != ri)[0][:5]
    assert (labels[ok] == rl[ok]).all(), np.nonzero((labels != rl).any(axis=1))[0][:5]
    assert (labels >= 0).all() and (labels < K).all() and (iters >= 1).all() and (iters <= kr.MAXIT).all()
    plain = gpu_ctx.kmeans_bootstrap(z, cols, K, seed)          # without the Gram copies: the same fits
    assert plain[0].tobytes() == labels.tobytes() and plain[1].tobytes() == iters.tobytes()
    return labels, iters, gram


@pytest.mark.parametrize("name", sorted(CASES))
def test_kboot_against_twin(gpu_ctx, name):
    z, cols, K, seed = _case(name)
    labels, iters, _ = _check(gpu_ctx, z, cols, K, seed)
    if K == 1:
        assert (labels == 0).all() and (iters == 1).all()
    if name == "typical":
        assert cols.min() == 0 and cols.max() == z.shape[1] - 1 and (cols[0, 2:7] == cols[0, 6]).all()


def test_kboot_seed_and_replicate_select_the_stream(gpu_ctx):
    """the same columns in every replicate: the replicate index alone varies the draws; another seed, other draws"""
    z = kr.blobs(5, 21, 3, 400, noise=3.0)
    cols = np.tile(np.random.RandomState(5).randint(0, 400, size=(1, 64)), (40, 1)).astype(np.int64)
    a, _, _ = _check(gpu_ctx, z, cols, 3, 1)
    b, _, _ = _check(gpu_ctx, z, cols, 3, 2)
    assert len({r.tobytes() for r in a}) > 1 and a.tobytes() != b.tobytes()


def test_kboot_staged_matrix(gpu_ctx):
    z, cols, K, seed = _case("mid")
    host = gpu_ctx.kmeans_bootstrap(z, cols, K, seed, want_gram=True)
    z = np.ascontiguousarray(z)
    ptr = gpu_ctx.dev_alloc(z.nbytes)
    try:
        gpu_ctx.host_to_dev(ptr, z)
        dev = gpu_ctx.kmeans_bootstrap((ptr, z.shape[0], z.shape[1]), cols, K, seed, want_gram=True)
    finally:
        gpu_ctx.dev_free(ptr)
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()


def _raw(ctx, z, cols, K):
    z, cols = np.ascontiguousarray(z, np.float64), np.ascontiguousarray(cols, np.int64)
    (C, M), (R, n) = z.shape, cols.shape
    labels, iters = np.full((R, C), -7, np.int32), np.full(R, -7, np.int32)
    vp = ctypes.c_void_p
    rc = ctx.L.sp_kmeans_bootstrap(ctx.h, vp(z.ctypes.data), C, M, vp(cols.ctypes.data), R, n, K, ctypes.c_uint64(1),
                                   vp(labels.ctypes.data), vp(iters.ctypes.data), None)
    return rc, labels, iters


@pytest.mark.parametrize("C,K,bad,code", [(129, 3, None, _native.SP_EUNSUP), (40, 33, None, _native.SP_EUNSUP),
                                          (3, 4, None, _native.SP_EINVAL), (3, 0, None, _native.SP_EINVAL),
                                          (21, 3, 50, _native.SP_EINVAL), (21, 3, -1, _native.SP_EINVAL)])
def test_kboot_error_codes(gpu_ctx, C, K, bad, code):
    M = 50
    z = np.random.RandomState(C).normal(size=(C, M))
    cols = np.random.RandomState(K).randint(0, M, size=(6, 40))
    if bad is not None:
        cols[5, 39] = bad                       # the last index of the last replicate
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        rc, labels, iters = _raw(gpu_ctx, z, cols, K)
        launched = gpu_ctx.prof_report()
    finally:
        gpu_ctx.prof_enable(False)
    assert rc == code, gpu_ctx.L.sp_last_error(gpu_ctx.h)
    assert "kb_bootstrap" not in launched and (labels == -7).all() and (iters == -7).all()      # nothing launched
    with pytest.raises(ValueError, match="sp_kmeans_bootstrap"):
        gpu_ctx.kmeans_bootstrap(z, cols, K, 1)


def test_kboot_no_columns(gpu_ctx):
    rc, _, _ = _raw(gpu_ctx, np.ones((3, 5)), np.zeros((4, 0), np.int64), 2)
    assert rc == _native.SP_EINVAL


class _Mat:
    pass


def _matrix(ctx, C, M, seed):
    rng = np.random.default_rng(seed)
    mat = _Mat()
    mat.labels = ["c%03d" % i for i in range(C)]
    mat.k = 15
    mat.keys = np.arange(M, dtype=np.uint64)
    mat.counts = rng.integers(1, 50, (M, C)).astype(np.uint32)
    mat.counts[:, : C // 2] += rng.integers(0, 30, (M, 1)).astype(np.uint32)
    mat.lengths = rng.integers(10 ** 6, 10 ** 7, C)
    mat.freqs = mat.counts / mat.lengths.astype(np.float64)
    mat.ctx = ctx
    return mat, {c: ("SG1" if i < C // 2 else "SG2") for i, c in enumerate(mat.labels)}


def test_cluster_device_engine_is_the_twin(gpu_ctx):
    """Cluster(bootstrap_engine="device"): the columns of RandomState(seed), the seed as the kernel's, the twin's support"""
    mat, sg = _matrix(gpu_ctx, 12, 300, 3)
    cl = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=100, seed=9, bootstrap_engine="device")
    z = cl.zscores()
    rl, _, gaps = kr.solve_all(kr.gram(z, kr.bootstrap_cols(9, z.shape[1], 100)), 2, 9)
    assert kr.decided(gaps).all()
    assert [cl.d_bs[c] for c in cl.chrs] == kr.support(cl.chrs, cl.labels, rl)
    assert cl.bootstrap_labels.shape == (100, 12) and 0 <= cl.mean_adjusted_rand_score <= 1 and 0 <= cl.mean_v_measure_score <= 1


def test_cluster_unsupported_shape_falls_back(gpu_ctx, caplog):
    mat, sg = _matrix(gpu_ctx, 130, 200, 4)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        dev = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=20, seed=5, bootstrap_engine="device")
    assert sum("using scikit-learn" in r.getMessage() for r in caplog.records) == 1
    ref = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=20, seed=5)
    assert dev.d_bs == ref.d_bs and (dev.bootstrap_labels == ref.bootstrap_labels).all()
    assert dev.mean_adjusted_rand_score == ref.mean_adjusted_rand_score


def test_cli_device_engine(gpu_ctx, toy, tmp_path, caplog):
    """`-bootstrap_engine device -bootstrap_seed 1` on the toy genome: the bootstrap column of `.chrom-subgenome.tsv` is the
    one derived from the twin on the `.kmer.mat` the run wrote, and the log holds the reference's Bootstrap line"""
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
                           "-replicates", "200", "-bootstrap_engine", "device", "-bootstrap_seed", "1"])
    finally:
        runtime._ctx = old
    log = [r.getMessage() for r in caplog.records]
    assert sum(m.startswith("Bootstrap: mean Adjusted Rand-Index: ") and "; mean V-measure score: " in m for m in log) == 1
    assert not any("using scikit-learn" in m for m in log)
    base = str(out / "k15_q30_f2")
    got = [l.split("\t") for l in open(base + ".chrom-subgenome.tsv").read().strip().split("\n")[1:]]
    ref = cluster.Cluster(base + ".kmer.mat", n_clusters=2, sg_assigned=dict(toy["sg_assigned"]))       # no bootstrap: z and labels
    z = ref.zscores()
    K = len(set(toy["sg_assigned"].values()))
    rl, _, gaps = kr.solve_all(kr.gram(z, kr.bootstrap_cols(1, z.shape[1], 200)), K, 1)
    kr.decided(gaps)
    want = dict(zip(ref.chrs, kr.support(ref.chrs, ref.labels, rl)))
    assert len(got) == len(want) and {c: int(b) for c, _, b in got} == want
