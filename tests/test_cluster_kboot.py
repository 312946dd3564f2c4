"""Cluster.bootstrap's two engines, with stub contexts (no GPU): the default keeps the loop of scikit-learn fits and its
support column; bootstrap_engine="device" hands Context.kmeans_bootstrap the columns that loop would have drawn and the
seed, renumbers every replicate and counts agreement; outside the kernel's limits it logs one line and takes the loop.
Both engines log the reference's `Bootstrap: mean Adjusted Rand-Index ...` line (Cluster.py:108-111)."""
import logging

import numpy as np
import pytest

import kboot_ref as kr
from subphaser_amd import cluster


class _Mat:
    pass


class _Twin:
    """a context whose kmeans_bootstrap is the numpy twin"""

    def __init__(self):
        self.calls = []

    def kmeans_bootstrap(self, z, cols, K, seed, want_gram=False):
        self.calls.append((z, cols, K, seed))
        labels, iters, _ = kr.solve_all(kr.gram(z, cols), K, seed)
        return labels, iters


class _NoEntry:
    pass


def _matrix(ctx, C=12, M=300, seed=3):
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


def _loop(cl, replicates, seed):
    """the bootstrap as it was before there were engines"""
    z = cl.zscores()
    rng = np.random.RandomState(seed)
    agree = np.zeros(len(cl.chrs), np.int64)
    reps = []
    for _ in range(replicates):
        cols = rng.randint(0, z.shape[1], size=replicates)
        reps.append(cluster.relabel_by_chromosome_order(cl.chrs, cl._kmeans(z[:, cols]).labels_))
        agree += reps[-1] == cl.labels
    return {c: int(100 * a / replicates) for c, a in zip(cl.chrs, agree.tolist())}, np.array(reps)


def test_default_engine_is_the_sklearn_loop(caplog):
    from sklearn import metrics
    ctx = _Twin()
    mat, sg = _matrix(ctx)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=30, seed=4)
    assert cl.bootstrap_engine == "sklearn" and ctx.calls == []
    d_bs, reps = _loop(cl, 30, 4)
    assert cl.d_bs == d_bs and (cl.bootstrap_labels == reps).all()
    ari = np.mean([metrics.adjusted_rand_score(cl.labels, r) for r in reps])
    vms = np.mean([metrics.v_measure_score(cl.labels, r) for r in reps])
    assert abs(cl.mean_adjusted_rand_score - ari) < 1e-12 and abs(cl.mean_v_measure_score - vms) < 1e-12
    line = "Bootstrap: mean Adjusted Rand-Index: {:.4f}; mean V-measure score: {:.4f}".format(
        cl.mean_adjusted_rand_score, cl.mean_v_measure_score)
    assert [r.getMessage() for r in caplog.records].count(line) == 1


def test_no_bootstrap_no_scores():
    mat, sg = _matrix(_Twin())
    cl = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg)
    assert set(cl.d_bs.values()) == {"NA"} and not hasattr(cl, "mean_adjusted_rand_score")


def test_device_engine_columns_seed_and_support(caplog):
    ctx = _Twin()
    mat, sg = _matrix(ctx)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=50, seed=6, bootstrap_engine="device")
    assert len(ctx.calls) == 1                                  # one call for all replicates
    z, cols, K, seed = ctx.calls[0]
    assert (z == cl.zscores()).all() and K == 2 and seed == 6
    assert cols.shape == (50, 50) and cols.dtype == np.int64 and (cols == kr.bootstrap_cols(6, z.shape[1], 50)).all()
    labels, _, _ = kr.solve_all(kr.gram(z, cols), 2, 6)
    assert [cl.d_bs[c] for c in cl.chrs] == kr.support(cl.chrs, cl.labels, labels)
    msgs = [r.getMessage() for r in caplog.records]
    assert sum(m.startswith("Bootstrap: mean Adjusted Rand-Index: ") for m in msgs) == 1
    assert not any("using scikit-learn" in m for m in msgs)


def test_device_engine_without_a_seed_draws_one():
    seeds = []
    for _ in range(2):
        ctx = _Twin()
        mat, sg = _matrix(ctx)
        cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=5, seed=None, bootstrap_engine="device")
        seeds.append(ctx.calls[0][3])
    assert all(isinstance(s, int) and 0 <= s < 2 ** 64 for s in seeds) and seeds[0] != seeds[1]


@pytest.mark.parametrize("ctx,C,why", [(_Twin(), 130, "130 chromosomes in 2 clusters"), (_NoEntry(), 12, "no device context"),
                                       (None, 12, "no device context")])
def test_device_engine_falls_back_outside_its_limits(caplog, ctx, C, why):
    mat, sg = _matrix(ctx, C=C)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl = cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=10, seed=8, bootstrap_engine="device")
    msgs = [r.getMessage() for r in caplog.records if "using scikit-learn" in r.getMessage()]
    assert len(msgs) == 1 and why in msgs[0]
    assert getattr(ctx, "calls", []) == []
    assert cl.d_bs == _loop(cl, 10, 8)[0]


def test_device_engine_more_clusters_than_the_kernel_takes(caplog):
    ctx = _Twin()
    mat, _ = _matrix(ctx, C=70)
    sg = {c: "SG%02d" % (i % 33) for i, c in enumerate(mat.labels)}
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cluster.Cluster(mat, n_clusters=33, sg_assigned=sg, bootstrap=True, replicates=3, seed=8, bootstrap_engine="device")
    assert ctx.calls == [] and sum("70 chromosomes in 33 clusters" in r.getMessage() for r in caplog.records) == 1


def test_device_engine_refuses_a_matrix_that_is_not_finite():
    ctx = _Twin()
    mat, sg = _matrix(ctx)
    mat.counts[7] = 5
    mat.freqs[7] = 0.5                    # a constant column: its Z-scores are 0 / 0
    with pytest.raises(ValueError, match="NaN"):
        cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap=True, replicates=5, seed=1, bootstrap_engine="device")
    assert ctx.calls == []


def test_engine_names():
    mat, sg = _matrix(None)
    with pytest.raises(ValueError, match="bootstrap_engine"):
        cluster.Cluster(mat, n_clusters=2, sg_assigned=sg, bootstrap_engine="gpu")
    from subphaser_amd.pipeline import makeArgparse
    assert makeArgparse("-i g.fa -c sg.cfg".split()).bootstrap_engine == "sklearn"
    assert makeArgparse("-i g.fa -c sg.cfg -bootstrap_engine device".split()).bootstrap_engine == "device"
    with pytest.raises(SystemExit):
        makeArgparse("-i g.fa -c sg.cfg -bootstrap_engine cuda".split())
