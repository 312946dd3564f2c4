"""Cluster.output_kmers' choice for test_method = kruskal and mannwhitneyu, with stub contexts (no GPU): the device entry
(Context.kmer_ranktest) when the context has it, the integer counts and lengths are there, M > 0 and no subgenome has more
than RANKTEST_MAX_GROUP chromosomes; the numpy / scipy path with one log line otherwise; wilcoxon and ttest_ind never
reach the entry; the rows the pipeline staged on the device are released on every route.  The stub answers with the numpy
twin (tests/ranktest_ref.py), so the two routes must also write the same k-mers."""
import io
import logging

import numpy as np
import pytest

import hp_reference as hr
import ranktest_ref as rr
from subphaser_amd import _native, cluster

M = 60
METHODS = ("kruskal", "mannwhitneyu")


class _Mat:
    pass


class _NoEntry:
    """a context from before the rank-sum kernel: only the t-test"""

    def __init__(self, host_counts):
        self.host_counts = host_counts
        self.calls = []
        self.released = 0

    def _rows(self, counts):
        return self.host_counts if isinstance(counts, tuple) else counts

    def kmer_ttest(self, counts, lengths, groups):
        self.calls.append(("ttest", counts, None))
        top, second, p, means, _ = rr.kmer_ranktest(self._rows(counts), lengths, groups, "kruskal")
        return top, second, p, means

    def release_rows(self):
        self.released += 1


class _Rank(_NoEntry):
    def kmer_ranktest(self, counts, lengths, groups, method):
        assert max(len(g) for g in groups) <= _native.RANKTEST_MAX_GROUP
        self.calls.append(("rank", counts, method))
        return rr.kmer_ranktest(self._rows(counts), lengths, groups, method)


def _cluster(na, ctx_type, staged, nb=5, m=M):
    rng = np.random.default_rng(na)
    C = na + nb
    mat = _Mat()
    mat.labels = ["c%03d" % i for i in range(C)]
    mat.k = 15
    mat.keys = rng.integers(0, 4 ** 15, m, dtype=np.int64).astype(np.uint64)
    mat.counts = rng.integers(0, 50, (m, C)).astype(np.uint32)
    mat.counts[:, :na] += rng.integers(0, 30, (m, 1)).astype(np.uint32)
    mat.lengths = rng.integers(10 ** 6, 10 ** 7, C)
    mat.freqs = mat.counts / mat.lengths.astype(np.float64)
    mat.ctx = ctx_type(mat.counts)
    if staged:
        mat.counts_dev = (0xdead0000, m, C)        # what Context.stage_rows returns: (device pointer, M, C)
    sg = {c: ("SG1" if i < na else "SG2") for i, c in enumerate(mat.labels)}
    return cluster.Cluster(mat, n_clusters=2, sg_assigned=sg), mat


def _host_lines(caplog):
    return [r.getMessage() for r in caplog.records if "on the host" in r.getMessage()]


def _rows_of(text):
    return [l.split("\t") for l in text.splitlines()[1:]]


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_device_entry_is_taken(method, staged, caplog):
    cl, mat = _cluster(6, _Rank, staged)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = cl.output_kmers(buf, max_pval=1.0, test_method=method)
    assert [(c[0], c[2]) for c in mat.ctx.calls] == [("rank", method)]
    got = mat.ctx.calls[0][1]
    if staged:
        assert got == (0xdead0000, M, 11) and mat.ctx.released == 1 and cl._counts_dev is None
    else:
        assert got is mat.counts and mat.ctx.released == 0
    assert _host_lines(caplog) == []
    assert len(_rows_of(buf.getvalue())) == M and len(labels.keys) == M
    # the same k-mers, subgenomes and p-values as the numpy / scipy route writes
    cl2, mat2 = _cluster(6, _NoEntry, False)
    ref = io.StringIO()
    cl2.output_kmers(ref, max_pval=1.0, test_method=method)
    a, b = _rows_of(buf.getvalue()), _rows_of(ref.getvalue())
    assert [r[:2] for r in a] == [r[:2] for r in b]
    assert hr.tail_ok([float(r[2]) for r in a], [float(r[2]) for r in b]).all()


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_group_of_65_takes_numpy_and_says_so(method, staged, caplog):
    cl, mat = _cluster(65, _Rank, staged, m=12)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(buf, max_pval=1.0, test_method=method)
    assert mat.ctx.calls == []
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    lines = _host_lines(caplog)
    assert len(lines) == 1 and method in lines[0] and "65" in lines[0] and "64" in lines[0]
    assert len(_rows_of(buf.getvalue())) == 12


def test_group_of_64_is_taken():
    cl, mat = _cluster(64, _Rank, True, m=12)
    cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="kruskal")
    assert [c[0] for c in mat.ctx.calls] == ["rank"] and mat.ctx.released == 1


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_context_without_the_entry_takes_numpy_and_says_so(method, staged, caplog):
    cl, mat = _cluster(6, _NoEntry, staged)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method=method)
    assert mat.ctx.calls == []
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    lines = _host_lines(caplog)
    assert len(lines) == 1 and method in lines[0] and "no device context" in lines[0]


@pytest.mark.parametrize("method", METHODS)
def test_kmer_mat_file_takes_numpy_and_says_so(method, tmp_path, caplog):
    _, mat = _cluster(4, _Rank, False, nb=4, m=20)
    path = tmp_path / "toy.kmer.mat"
    from subphaser_amd import kmer as kmerlib
    kmers = kmerlib.decode_many(mat.keys, mat.k)
    with open(path, "w") as f:
        f.write("\t".join(["kmer"] + mat.labels) + "\n")
        for km, row in zip(kmers, mat.freqs.tolist()):
            f.write("\t".join([km] + [repr(v) for v in row]) + "\n")
    sg = {c: ("SG1" if i < 4 else "SG2") for i, c in enumerate(mat.labels)}
    cl = cluster.Cluster(str(path), n_clusters=2, sg_assigned=sg)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(buf, max_pval=1.0, test_method=method)
    assert len(_host_lines(caplog)) == 1 and method in _host_lines(caplog)[0]
    assert len(_rows_of(buf.getvalue())) == len(cl.keys) > 0
    p = np.array([float(r[2]) for r in _rows_of(buf.getvalue())])
    X = cl.raw_data
    assert (p == cluster.numpy_kmer_test(X, [[0, 1, 2, 3], [4, 5, 6, 7]], method)[2]).all()


def test_matrix_without_counts_takes_numpy(caplog):
    cl, mat = _cluster(6, _Rank, False)
    cl._counts = None
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="kruskal")
    assert mat.ctx.calls == [] and len(_host_lines(caplog)) == 1 and "counts" in _host_lines(caplog)[0]


@pytest.mark.parametrize("staged", [False, True])
def test_wilcoxon_and_ttest_never_reach_the_entry(staged, caplog):
    for method, expect in (("wilcoxon", []), ("ttest_ind", ["ttest"])):
        cl, mat = _cluster(6, _Rank, staged, nb=6)
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            cl.output_kmers(io.StringIO(), max_pval=1.0, test_method=method)
        assert [c[0] for c in mat.ctx.calls] == expect
        assert mat.ctx.released == (1 if staged else 0)
    assert _host_lines(caplog) == []


def test_entry_error_still_releases_the_staged_rows():
    class _Failing(_Rank):
        def kmer_ranktest(self, counts, lengths, groups, method):
            raise MemoryError("sp_kmer_ranktest: a workspace of 1 bytes does not fit on the device")

    cl, mat = _cluster(6, _Failing, True)
    with pytest.raises(MemoryError):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="mannwhitneyu")
    assert mat.ctx.released == 1 and cl._counts_dev is None


def test_no_rows_takes_numpy():
    cl, mat = _cluster(6, _Rank, False)
    cl.raw_data, cl.keys = cl.raw_data[:0], cl.keys[:0]
    labels = cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="kruskal")
    assert mat.ctx.calls == [] and len(labels.keys) == 0
