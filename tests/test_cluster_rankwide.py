"""Cluster.output_kmers' choice between the two rank-sum engines for test_method = kruskal and mannwhitneyu, with stub
contexts (no GPU):
  groups <= 64                                      Context.kmer_ranktest, as before
  65 .. 4096, a context with kmer_ranktest_wide      that entry, no "on the host" line
  65 .. 4096, a context with kmer_ranktest alone     numpy / scipy, one line naming 65 and 64
  above 4096                                         numpy / scipy, one line naming the size and 4096
The rows the pipeline staged on the device are released on every route, also when the entry raises.  The stubs answer with
the numpy twins, so the device route and the host route must write the same k-mers."""
import io
import logging

import numpy as np
import pytest

import hp_reference as hr
import ranktest_ref as rr
import rankwide_ref as rw
from subphaser_amd import _native, cluster

METHODS = ("kruskal", "mannwhitneyu")


class _Mat:
    pass


class _Narrow:
    """a context from before the wide kernel"""

    def __init__(self, host_counts):
        self.host_counts = host_counts
        self.calls = []
        self.released = 0

    def _rows(self, counts):
        return self.host_counts if isinstance(counts, tuple) else counts

    def kmer_ranktest(self, counts, lengths, groups, method):
        assert max(len(g) for g in groups) <= _native.RANKTEST_MAX_GROUP
        self.calls.append(("rank", counts, method))
        return rr.kmer_ranktest(self._rows(counts), lengths, groups, method)

    def release_rows(self):
        self.released += 1


class _Wide(_Narrow):
    def kmer_ranktest_wide(self, counts, lengths, groups, method):
        assert max(len(g) for g in groups) <= _native.RANKTEST_WIDE_MAX_GROUP
        self.calls.append(("wide", counts, method))
        return rw.kmer_ranktest_wide(self._rows(counts), lengths, groups, method)


def _cluster(na, ctx_type, staged, nb=5, m=12):
    rng = np.random.default_rng(na)
    C = na + nb
    mat = _Mat()
    mat.labels = ["c%04d" % i for i in range(C)]
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


def test_the_limit_and_the_engine_list():
    assert _native.RANKTEST_WIDE_MAX_GROUP == 4096
    for m in METHODS:
        assert [e[0] for e in cluster.KMER_ENGINES[m]] == ["kmer_ranktest", "kmer_ranktest_wide"]
    assert "sp_kmer_ranktest_wide" in _native.SYMBOLS


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_small_groups_keep_the_narrow_entry(method, staged, caplog):
    cl, mat = _cluster(64, _Wide, staged)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method=method)
    assert [(c[0], c[2]) for c in mat.ctx.calls] == [("rank", method)]
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    assert _host_lines(caplog) == []


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("na", [65, 300])
def test_wide_groups_take_the_wide_entry(na, method, staged, caplog):
    cl, mat = _cluster(na, _Wide, staged)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = cl.output_kmers(buf, max_pval=1.0, test_method=method)
    assert [(c[0], c[2]) for c in mat.ctx.calls] == [("wide", method)]
    got = mat.ctx.calls[0][1]
    if staged:
        assert got == (0xdead0000, 12, na + 5) and mat.ctx.released == 1 and cl._counts_dev is None
    else:
        assert got is mat.counts and mat.ctx.released == 0
    assert _host_lines(caplog) == []
    assert len(_rows_of(buf.getvalue())) == 12 and len(labels.keys) == 12
    # the same k-mers, subgenomes and p-values as the numpy / scipy route writes
    cl2, mat2 = _cluster(na, _Narrow, False)
    ref = io.StringIO()
    cl2.output_kmers(ref, max_pval=1.0, test_method=method)
    assert mat2.ctx.calls == []
    a, b = _rows_of(buf.getvalue()), _rows_of(ref.getvalue())
    assert [r[:2] for r in a] == [r[:2] for r in b]
    assert hr.tail_ok([float(r[2]) for r in a], [float(r[2]) for r in b]).all()


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_context_without_the_wide_entry_takes_numpy_and_names_64(method, staged, caplog):
    cl, mat = _cluster(65, _Narrow, staged)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(buf, max_pval=1.0, test_method=method)
    assert mat.ctx.calls == []
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    lines = _host_lines(caplog)
    assert len(lines) == 1 and method in lines[0] and "65" in lines[0] and "64" in lines[0] and "4096" not in lines[0]
    assert len(_rows_of(buf.getvalue())) == 12


@pytest.mark.parametrize("staged", [False, True])
def test_above_4096_takes_numpy_and_names_the_size(staged, caplog):
    cl, mat = _cluster(4097, _Wide, staged, m=4)
    buf = io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(buf, max_pval=1.0, test_method="kruskal")
    assert mat.ctx.calls == []
    assert mat.ctx.released == (1 if staged else 0) and getattr(cl, "_counts_dev", None) is None
    lines = _host_lines(caplog)
    assert len(lines) == 1 and "kruskal" in lines[0] and "4097" in lines[0] and "4096" in lines[0]
    assert len(_rows_of(buf.getvalue())) == 4


def test_group_of_4096_is_taken():
    cl, mat = _cluster(4096, _Wide, True, m=2)
    cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="kruskal")
    assert [c[0] for c in mat.ctx.calls] == ["wide"] and mat.ctx.released == 1


@pytest.mark.parametrize("method", METHODS)
def test_entry_error_still_releases_the_staged_rows(method):
    class _Failing(_Wide):
        def kmer_ranktest_wide(self, counts, lengths, groups, method):
            raise MemoryError("sp_kmer_ranktest_wide: a workspace of 1 bytes does not fit on the device")

    cl, mat = _cluster(66, _Failing, True)
    with pytest.raises(MemoryError):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method=method)
    assert mat.ctx.released == 1 and cl._counts_dev is None


def test_context_without_any_entry_says_so(caplog):
    class _None(_Narrow):
        kmer_ranktest = None

    cl, mat = _cluster(66, _None, True)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.output_kmers(io.StringIO(), max_pval=1.0, test_method="mannwhitneyu")
    lines = _host_lines(caplog)
    assert len(lines) == 1 and "no device context" in lines[0] and mat.ctx.released == 1
