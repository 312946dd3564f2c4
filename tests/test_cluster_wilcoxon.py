"""Cluster.output_kmers' choice for test_method = wilcoxon, with stub contexts (no GPU): the device entry
(Context.kmer_wilcoxon) when the context has it, the integer counts and lengths are there, M > 0 and all subgenomes have one
size n with 2 <= n <= WILCOXON_MAX_GROUP; the numpy / scipy path with one log line otherwise, silently when the context has
no such entry; the rows the pipeline staged on the device are released on every route.  The stub answers with the numpy
twin (tests/wilcoxon_ref.py), so the two routes must also write the same k-mers."""
import io
import logging

import numpy as np
import pytest

import hp_reference as hr
import wilcoxon_ref as wr
from subphaser_amd import _native, cluster

M = 60


class _Mat:
    pass


class _NoEntry:
    """a context from before the paired kernel: the t-test and the rank-sum tests"""

    def __init__(self, host_counts):
        self.host_counts = host_counts
        self.calls = []
        self.released = 0

    def _rows(self, counts):
        return self.host_counts if isinstance(counts, tuple) else counts

    def kmer_ttest(self, counts, lengths, groups):
        self.calls.append(("ttest", counts))
        raise AssertionError("the t-test entry under test_method = wilcoxon")

    def kmer_ranktest(self, counts, lengths, groups, method):
        self.calls.append(("rank", counts))
        raise AssertionError("the rank-sum entry under test_method = wilcoxon")

    def release_rows(self):
        self.released += 1


class _Wx(_NoEntry):
    def kmer_wilcoxon(self, counts, lengths, groups):
        sizes = {len(g) for g in groups}
        assert len(sizes) == 1 and 2 <= min(sizes) <= _native.WILCOXON_MAX_GROUP
        self.calls.append(("wilcoxon", counts))
        return wr.kmer_wilcoxon(self._rows(counts), lengths, groups)


def _cluster(na, ctx_type, staged, nb=None, m=M, hi=50):
    nb = na if nb is None else nb
    rng = np.random.default_rng(na)
    C = na + nb
    mat = _Mat()
    mat.labels = ["c%03d" % i for i in range(C)]
    mat.k = 15
    mat.keys = rng.integers(0, 4 ** 15, m, dtype=np.int64).astype(np.uint64)
    mat.counts = rng.integers(0, hi, (m, C)).astype(np.uint32)
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


def test_the_binding_declares_the_entry():
    assert _native.WILCOXON_MAX_GROUP == 64 and "sp_kmer_wilcoxon" in _native.SYMBOLS
    assert callable(getattr(_native.Context, "kmer_wilcoxon"))
    assert "wilcoxon" not in _native.RANKTEST_METHODS


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("na", [6, 14])
def test_device_entry_is_taken(na, staged, caplog):
    cl, mat = _cluster(na, _Wx, staged)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = cl.output_kmers(buf, max_pval=1.0, test_method="wilcoxon")
    assert [c[0] for c in mat.ctx.calls] == ["wilcoxon"]
    got = mat.ctx.calls[0][1]
    if staged:
        assert got == (0xdead0000, M, 2 * na) and mat.ctx.released == 1 and cl._counts_dev is None
    else:
        assert got is mat.counts and mat.ctx.released == 0
    assert _host_lines(caplog) == []
    assert len(_rows_of(buf.getvalue())) == M and len(labels.keys) == M
    # the same k-mers, subgenomes and p-values as the numpy / scipy route writes
    cl2, mat2 = _cluster(na, _NoEntry, False)
    ref = io.StringIO()
    cl2.output_kmers(ref, max_pval=1.0, test_method="wilcoxon")
    assert mat2.ctx.calls == []
    a, b = _rows_of(buf.getvalue()), _rows_of(ref.getvalue())
    assert [r[:2] for r in a] == [r[:2] for r in b]
    assert hr.tail_ok([float(r[2]) for r in a], [float(r[2]) for r in b]).all()


def test_the_two_routes_keep_the_same_kmers_with_ties_and_nan():
    """counts in 0..2 over equal lengths at 14 pairs: ties everywhere, and rows whose differences are all zero have p = NaN
    on both routes and are kept by both"""
    out = []
    for ctx_type in (_Wx, _NoEntry):
        cl, mat = _cluster(14, ctx_type, False, hi=3)
        mat.counts[:] = np.random.default_rng(5).integers(0, 3, mat.counts.shape)
        mat.counts[:4] = 1
        cl._lengths = mat.lengths = np.full(28, 1 << 21)
        cl.raw_data = mat.counts / mat.lengths.astype(np.float64)
        buf = io.StringIO()
        cl.output_kmers(buf, max_pval=0.3, test_method="wilcoxon")
        out.append(_rows_of(buf.getvalue()))
        assert [c[0] for c in mat.ctx.calls] == (["wilcoxon"] if ctx_type is _Wx else [])
    a, b = out
    assert 4 < len(a) < M and [r[:2] for r in a] == [r[:2] for r in b]
    pa, pb = np.array([float(r[2]) for r in a]), np.array([float(r[2]) for r in b])
    assert np.isnan(pa[:4]).all() and (np.isnan(pa) == np.isnan(pb)).all()
    assert hr.tail_ok(pa[~np.isnan(pa)], pb[~np.isnan(pb)]).all()


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("na,nb,words", [(1, 1, ("1", "2 to 64")), (65, 65, ("65", "2 to 64"))])
def test_unsupported_size_takes_the_host_and_says_so(na, nb, words, staged, caplog):
    cl, mat = _cluster(na, _Wx, staged, nb=nb, m=6)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(buf, max_pval=1.0, test_method="wilcoxon")
    assert len(_rows_of(buf.getvalue())) == 6
    assert mat.ctx.calls == []
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    lines = _host_lines(caplog)
    assert len(lines) == 1 and lines[0].startswith("k-mer test (wilcoxon) on the host: ")
    assert all(w in lines[0] for w in words)


@pytest.mark.parametrize("staged", [False, True])
def test_unequal_sizes_reach_scipy_which_raises(staged, caplog):
    cl, mat = _cluster(6, _Wx, staged, nb=5, m=6)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        with pytest.raises(ValueError):
            cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="wilcoxon")
    assert mat.ctx.calls == [] and mat.ctx.released == (1 if staged else 0)
    lines = _host_lines(caplog)
    assert len(lines) == 1 and lines[0].startswith("k-mer test (wilcoxon) on the host: ") and "5, 6" in lines[0]


def test_matrix_without_counts_takes_the_host(caplog):
    cl, mat = _cluster(6, _Wx, False)
    cl._counts = None
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="wilcoxon")
    lines = _host_lines(caplog)
    assert mat.ctx.calls == [] and len(lines) == 1 and "counts" in lines[0] and "(wilcoxon)" in lines[0]


def test_no_rows_takes_the_host(caplog):
    cl, mat = _cluster(6, _Wx, False)
    cl.raw_data, cl.keys = cl.raw_data[:0], cl.keys[:0]
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="wilcoxon")
    assert mat.ctx.calls == [] and len(labels.keys) == 0
    assert len(_host_lines(caplog)) == 1 and "no k-mers" in _host_lines(caplog)[0]


@pytest.mark.parametrize("staged", [False, True])
def test_context_without_the_entry_stays_silent(staged, caplog):
    cl, mat = _cluster(6, _NoEntry, staged)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(buf, max_pval=1.0, test_method="wilcoxon")
    assert mat.ctx.calls == [] and _host_lines(caplog) == []
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    assert len(_rows_of(buf.getvalue())) == M


def test_other_methods_never_reach_the_entry():
    for method in ("ttest_ind", "kruskal", "mannwhitneyu"):
        cl, mat = _cluster(6, _Wx, False)
        with pytest.raises(AssertionError, match="under test_method = wilcoxon"):
            cl.output_kmers(io.StringIO(), max_pval=1.0, test_method=method)
        assert [c[0] for c in mat.ctx.calls] == ["ttest" if method == "ttest_ind" else "rank"]


def test_entry_error_still_releases_the_staged_rows():
    class _Failing(_Wx):
        def kmer_wilcoxon(self, counts, lengths, groups):
            raise MemoryError("sp_kmer_wilcoxon: a workspace of 1 bytes does not fit on the device")

    cl, mat = _cluster(6, _Failing, True)
    with pytest.raises(MemoryError):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="wilcoxon")
    assert mat.ctx.released == 1 and cl._counts_dev is None
