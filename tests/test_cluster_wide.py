"""Cluster.output_kmers' choice between the three k-mer t-tests, with stub contexts (no GPU): k7_ttest up to 64 chromosomes
per subgenome, the wide kernels (Context.kmer_ttest_wide) above that when the context has them, numpy otherwise; the
rows the pipeline staged on the device are handed to the kernel that runs and released on every route."""
import io

import numpy as np
import pytest

from subphaser_amd import cluster

M = 120


class _Mat:
    pass


def _np_test(counts, lengths, groups):
    """a stand-in result with the shapes and the decisions of the kernels (the values are not what these tests check)"""
    X = np.asarray(counts, np.float64) / np.asarray(lengths, np.float64)
    means = np.stack([X[:, g].mean(axis=1) for g in groups], axis=1)
    order = np.argsort(-means, axis=1, kind="stable")
    return order[:, 0].astype(np.int32), order[:, 1].astype(np.int32), np.full(len(X), 0.01), means


class _Narrow:
    """a context that has only the 64-chromosome kernel"""

    def __init__(self, host_counts):
        self.host_counts = host_counts
        self.calls = []
        self.released = 0

    def _rows(self, counts):
        return self.host_counts if isinstance(counts, tuple) else counts

    def kmer_ttest(self, counts, lengths, groups):
        assert max(len(g) for g in groups) <= cluster.TTEST_MAX_GROUP
        self.calls.append(("narrow", counts))
        return _np_test(self._rows(counts), lengths, groups)

    def release_rows(self):
        self.released += 1


class _Wide(_Narrow):
    def kmer_ttest_wide(self, counts, lengths, groups):
        assert max(len(g) for g in groups) > cluster.TTEST_MAX_GROUP
        self.calls.append(("wide", counts))
        return _np_test(self._rows(counts), lengths, groups)


def _cluster(na, ctx_type, staged):
    rng = np.random.default_rng(na)
    C = na + 5
    mat = _Mat()
    mat.labels = ["c%03d" % i for i in range(C)]
    mat.k = 15
    mat.keys = rng.integers(0, 4 ** 15, M, dtype=np.int64).astype(np.uint64)
    mat.counts = rng.integers(0, 50, (M, C)).astype(np.uint32)
    mat.counts[:, :na] += rng.integers(0, 30, (M, 1)).astype(np.uint32)
    mat.lengths = rng.integers(10 ** 6, 10 ** 7, C)
    mat.freqs = mat.counts / mat.lengths.astype(np.float64)
    mat.ctx = ctx_type(mat.counts)
    if staged:
        mat.counts_dev = (0xdead0000, M, C)        # what Context.stage_rows returns: (device pointer, M, C)
    sg = {c: ("SG1" if i < na else "SG2") for i, c in enumerate(mat.labels)}
    return cluster.Cluster(mat, n_clusters=2, sg_assigned=sg), mat


@pytest.mark.parametrize("staged", [False, True])
def test_group_of_65_takes_the_wide_kernel_once(staged):
    cl, mat = _cluster(65, _Wide, staged)
    buf = io.StringIO()
    labels = cl.output_kmers(buf, max_pval=1.0)
    assert [c[0] for c in mat.ctx.calls] == ["wide"]
    got = mat.ctx.calls[0][1]
    if staged:
        assert got == (0xdead0000, M, 70)
        assert mat.ctx.released == 1 and cl._counts_dev is None
    else:
        assert got is mat.counts and mat.ctx.released == 0
    assert len(buf.getvalue().splitlines()) == M + 1 and len(labels.keys) == M


@pytest.mark.parametrize("staged", [False, True])
def test_group_of_64_stays_with_the_narrow_kernel(staged):
    cl, mat = _cluster(64, _Wide, staged)
    cl.output_kmers(io.StringIO(), max_pval=1.0)
    assert [c[0] for c in mat.ctx.calls] == ["narrow"]
    assert mat.ctx.released == (1 if staged else 0)
    if staged:
        assert mat.ctx.calls[0][1] == (0xdead0000, M, 69) and cl._counts_dev is None


@pytest.mark.parametrize("staged", [False, True])
def test_context_without_the_wide_kernel_takes_numpy(staged):
    from scipy import stats as st
    cl, mat = _cluster(65, _Narrow, staged)
    buf = io.StringIO()
    cl.output_kmers(buf, max_pval=1.0)
    assert mat.ctx.calls == []
    assert mat.ctx.released == (1 if staged else 0)        # nobody reads the staged rows: they must not stay on the device
    if staged:
        assert cl._counts_dev is None
    rows = buf.getvalue().splitlines()[1:]
    assert len(rows) == M
    p = np.array([float(r.split("\t")[2]) for r in rows])
    ref = st.ttest_ind(mat.freqs[:, :65], mat.freqs[:, 65:], axis=1).pvalue
    assert np.allclose(p, ref, rtol=1e-9, atol=0)


def test_kernel_error_still_releases_the_staged_rows():
    class _Failing(_Wide):
        def kmer_ttest_wide(self, counts, lengths, groups):
            raise MemoryError("sp_kmer_ttest_wide: a workspace of 1 bytes does not fit on the device")

    cl, mat = _cluster(65, _Failing, True)
    with pytest.raises(MemoryError):
        cl.output_kmers(io.StringIO(), max_pval=1.0)
    assert mat.ctx.released == 1 and cl._counts_dev is None


def test_group_beyond_the_wide_limit_takes_numpy(monkeypatch):
    monkeypatch.setattr(cluster, "TTEST_WIDE_MAX_GROUP", 70)
    cl, mat = _cluster(71, _Wide, True)
    cl.output_kmers(io.StringIO(), max_pval=1.0)
    assert mat.ctx.calls == [] and mat.ctx.released == 1
