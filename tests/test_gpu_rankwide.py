"""GPU: the rank-sum k-mer tests for subgenomes of 65 .. 4096 chromosomes (sp_rankwide.hip: k7_ranktest_wide behind
k7_ttest_wide_means, Context.kmer_ranktest_wide) for test_method = kruskal and mannwhitneyu, against the numpy twin of the
header (tests/rankwide_ref.py) and against the host path the CLI took at these sizes (cluster.numpy_kmer_test):

  twin        top, second and means bytes ==, stat == (NaN where NaN), p within hp_reference.tail_ok (relative 1e-10 on
              [1e-290, 0.5], absolute 1e-13 above)
  host path   the same top / second, p within tail_ok
  narrow      at (3, 5) and (64, 64), on rows whose group means are far apart: stat and p bytes == Context.kmer_ranktest
The kernel takes one workgroup per row, so M only sets the grid: M = 1, 70 and 3 (the 64-KiB rows).  Sizes and value
patterns are those of tests/rankwide_cases.py; then matrices of three and five interleaved groups, staged rows, a group
alone, the entry conditions and Cluster.output_kmers on a matrix with two subgenomes of 66 chromosomes."""
import ctypes
import io
import logging

import numpy as np
import pytest

import hp_reference as hr
import rankwide_cases as rc
import rankwide_ref as rw
from subphaser_amd import _native, cluster

pytestmark = pytest.mark.gpu


def _same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def _check(gpu_ctx, counts, lengths, groups, ref, stage=False, host=True):
    """both methods on one matrix; returns {method: (top, second, p, means, stat)}"""
    out = {}
    M = len(counts)
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    for m in rw.METHODS:
        got = gpu_ctx.kmer_ranktest_wide(counts, lengths, groups, m)
        top, second, p, means, stat = got
        assert top.shape == second.shape == p.shape == stat.shape == (M,) and means.shape == (M, len(groups))
        assert top.dtype == second.dtype == np.int32 and p.dtype == stat.dtype == means.dtype == np.float64
        rt, rs, rp, rm, rst = ref[m]
        assert means.tobytes() == rm.tobytes(), (m, np.argwhere(means != rm)[:5])
        assert (top == rt).all() and (second == rs).all(), (m, np.nonzero((top != rt) | (second != rs))[0][:5])
        assert _same(stat, rst), (m, np.nonzero(~((stat == rst) | (np.isnan(stat) & np.isnan(rst))))[0][:5])
        ok = hr.tail_ok(p, rp)
        assert ok.all(), (m, [(r, p[r], rp[r]) for r in np.nonzero(~ok)[0][:5]])
        if host:
            ht, hs, hp, _ = cluster.numpy_kmer_test(X, groups, m)
            assert (top == ht).all() and (second == hs).all(), (m, np.nonzero((top != ht) | (second != hs))[0][:5])
            ok = hr.tail_ok(p, hp)
            assert ok.all(), (m, [(r, p[r], hp[r]) for r in np.nonzero(~ok)[0][:5]])
        if stage:
            staged = gpu_ctx.stage_rows(counts)
            try:
                again = gpu_ctx.kmer_ranktest_wide(staged, lengths, groups, m)
            finally:
                gpu_ctx.release_rows()
            for a, b in zip(got, again):
                assert a.tobytes() == b.tobytes(), m
        out[m] = got
    return out


@pytest.mark.parametrize("pattern", rc.PATTERNS)
@pytest.mark.parametrize("n1,n2", rc.SMALL + rc.EDGES)
def test_group_sizes(gpu_ctx, n1, n2, pattern):
    counts, lengths, groups = rc.size_case(n1, n2, pattern, 70)
    out = _check(gpu_ctx, counts, lengths, groups, rc.twin("size", n1, n2, pattern, 70))
    top, second, p, means, stat = out["kruskal"]
    assert set(top.tolist()) == {0, 1}                   # both orders of the pair are met
    if pattern == "ties":
        assert np.isnan(stat[69]) and p[69] == 1.0 and out["mannwhitneyu"][2][69] == 1.0      # every value identical


@pytest.mark.parametrize("pattern", rc.PATTERNS)
@pytest.mark.parametrize("n1,n2", rc.LARGE)
def test_large_groups(gpu_ctx, n1, n2, pattern):
    counts, lengths, groups = rc.size_case(n1, n2, pattern, 3)
    _check(gpu_ctx, counts, lengths, groups, rc.twin("size", n1, n2, pattern, 3))


@pytest.mark.parametrize("pattern", rc.PATTERNS)
@pytest.mark.parametrize("n1,n2", [(65, 65), (8, 65), (257, 255)])
def test_one_row(gpu_ctx, n1, n2, pattern):
    counts, lengths, groups = rc.size_case(n1, n2, pattern, 1)
    _check(gpu_ctx, counts, lengths, groups, rc.twin("size", n1, n2, pattern, 1))


def test_the_exact_branch_is_reached():
    """the condition on the inputs: rows without ties beside a group of at most 8, on both sides of the rule"""
    for n1, n2, exact in ((8, 65, True), (65, 8, True), (8, 4096, True), (9, 65, False)):
        counts, lengths, groups = rc.size_case(n1, n2, "distinct", 70 if n2 < 4096 else 3)
        x = np.sort(counts / lengths.astype(np.float64), axis=1)
        assert (np.diff(x, axis=1) > 0).all() and (min(n1, n2) <= rw.EXACT_MAX) == exact


@pytest.mark.parametrize("n1,n2", [(3, 5), (64, 64)])
def test_same_bytes_as_the_narrow_entry(gpu_ctx, n1, n2):
    counts, lengths, groups = rc.far_apart_case(n1, n2, 70)
    ref = rc.twin("far", n1, n2, 70)
    out = _check(gpu_ctx, counts, lengths, groups, ref)
    for m in rw.METHODS:
        top, second, p, means, stat = out[m]
        nt, ns, np_, nmeans, nstat = gpu_ctx.kmer_ranktest(counts, lengths, groups, m)
        assert (top == nt).all() and (second == ns).all() and set(top.tolist()) == {0, 1}
        assert stat.tobytes() == nstat.tobytes() and p.tobytes() == np_.tobytes(), m


@pytest.mark.parametrize("pattern", ["ties", "distinct"])
@pytest.mark.parametrize("G", [3, 5])
def test_interleaved_groups(gpu_ctx, G, pattern):
    counts, lengths, groups = rc.layout_case(G, pattern, 70)
    assert counts.shape[1] > sum(len(g) for g in groups) and len({len(g) for g in groups}) == G
    assert all(np.any(np.diff(g) < 0) for g in groups if len(g) > 7)      # unsorted lists
    out = _check(gpu_ctx, counts, lengths, groups, rc.twin("layout", G, pattern, 70))
    top, second = out["mannwhitneyu"][:2]
    pairs = set(zip(top.tolist(), second.tolist()))
    assert len(set(top.tolist())) == G and len(pairs) > G
    assert any((b, a) in pairs for a, b in pairs)        # both orders of at least one pair
    small = {g for g in range(G) if len(groups[g]) <= rw.EXACT_MAX}
    assert any(a in small or b in small for a, b in pairs) and any(a not in small and b not in small for a, b in pairs)


def test_staged_rows_give_the_same_bytes(gpu_ctx):
    for args in ((65, 8, "distinct", 70), (256, 257, "ties", 70), (4096, 4096, "lengths", 3)):
        counts, lengths, groups = rc.size_case(*args)
        _check(gpu_ctx, counts, lengths, groups, rc.twin("size", *args), stage=True, host=False)
    counts, lengths, groups = rc.layout_case(5, "distinct", 70)
    _check(gpu_ctx, counts, lengths, groups, rc.twin("layout", 5, "distinct", 70), stage=True, host=False)


def test_one_group(gpu_ctx):
    counts = np.arange(700, dtype=np.uint32).reshape(10, 70)
    lengths = np.full(70, 7, np.int64)
    groups = [list(range(69, 2, -1))]
    for m in rw.METHODS:
        top, second, p, means, stat = gpu_ctx.kmer_ranktest_wide(counts, lengths, groups, m)
        rt, rs, rp, rm, rst = rw.kmer_ranktest_wide(counts, lengths, groups, m)
        assert (top == 0).all() and (second == 0).all() and (p == 1.0).all() and np.isnan(stat).all()
        assert means.tobytes() == rm.tobytes()


def test_entry_conditions(gpu_ctx):
    C = 4100
    counts = np.ones((3, C), np.uint32)
    lengths = np.full(C, 1000, np.int64)
    with pytest.raises(ValueError, match="sp_kmer_ranktest_wide.*4097.*4096"):
        gpu_ctx.kmer_ranktest_wide(counts, lengths, [list(range(4097)), [4098, 4099]], "kruskal")
    gpu_ctx.kmer_ranktest_wide(counts, lengths, [list(range(4096)), [4098, 4099]], "kruskal")
    with pytest.raises(ValueError, match="sp_kmer_ranktest_wide.*method 2"):
        gpu_ctx.kmer_ranktest_wide(counts, lengths, [[0, 1], [2, 3]], 2)
    with pytest.raises(ValueError, match="method must be one of"):
        gpu_ctx.kmer_ranktest_wide(counts, lengths, [[0, 1], [2, 3]], "wilcoxon")
    zero = lengths.copy()
    zero[C - 1] = 0
    with pytest.raises(ValueError, match="sp_kmer_ranktest_wide.*chromosome 4099 has length 0"):
        gpu_ctx.kmer_ranktest_wide(counts, zero, [[0, 1], [2, 3]], "mannwhitneyu")
    with pytest.raises(ValueError, match="sp_kmer_ranktest_wide.*out of range"):
        gpu_ctx.kmer_ranktest_wide(counts, lengths, [[0, 1], [2, C]], "mannwhitneyu")
    for m in rw.METHODS:
        top, second, p, means, stat = gpu_ctx.kmer_ranktest_wide(np.zeros((0, C), np.uint32), lengths, [[0, 1], [2, 3, 4]], m)
        assert top.shape == second.shape == p.shape == stat.shape == (0,) and means.shape == (0, 2)


def test_error_codes_and_null_pointers(gpu_ctx):
    vp = ctypes.c_void_p
    C = 4100
    counts, lengths = np.ones((2, C), np.uint32), np.full(C, 9, np.int64)
    gch = np.arange(C, dtype=np.int32)
    big, ok, empty = np.array([0, 4097, 4099], np.int32), np.array([0, 70, 73], np.int32), np.array([0, 70, 70], np.int32)
    top, sec, p, means = np.empty(2, np.int32), np.empty(2, np.int32), np.empty(2), np.empty((2, 2))
    ptr = lambda a: vp(a.ctypes.data)

    def call(c=counts, l=lengths, off=ok, method=0, t=top, M=2):
        return gpu_ctx.L.sp_kmer_ranktest_wide(gpu_ctx.h, c if isinstance(c, vp) else ptr(c) if c is not None else None, M, C,
                                               ptr(l) if l is not None else None, 2, ptr(off), ptr(gch), method,
                                               ptr(t) if t is not None else None, ptr(sec), ptr(p), ptr(means), None)
    assert call() == _native.SP_OK                                         # stat may be NULL
    assert call(method=2) == _native.SP_EINVAL and call(method=-1) == _native.SP_EINVAL
    assert call(c=None) == _native.SP_EINVAL and call(l=None) == _native.SP_EINVAL and call(t=None) == _native.SP_EINVAL
    assert call(off=empty) == _native.SP_EINVAL
    assert b"sp_kmer_ranktest_wide" in gpu_ctx.L.sp_last_error(gpu_ctx.h)
    assert call(off=big) == _native.SP_EUNSUP
    assert b"4097" in gpu_ctx.L.sp_last_error(gpu_ctx.h)
    # rows that claim to be 2^38 on the device: the workspace, 10 TB, cannot be had -- SP_ENOMEM with its size, and
    # nothing is launched; with a group of 4097 the same call is refused before it asks for any memory
    staged = gpu_ctx.stage_rows(counts)
    try:
        assert call(c=vp(staged[0]), M=2 ** 38) == _native.SP_ENOMEM
        msg = gpu_ctx.L.sp_last_error(gpu_ctx.h)
        assert b"sp_kmer_ranktest_wide" in msg and b"bytes" in msg and b"274877906944 rows" in msg
        assert call(c=vp(staged[0]), M=2 ** 38, off=big) == _native.SP_EUNSUP
        assert call(c=vp(staged[0])) == _native.SP_OK                      # the context goes on
    finally:
        gpu_ctx.release_rows()


# ---- through Cluster.output_kmers: two subgenomes of 66 chromosomes
MAX_PVAL = 0.05


class _Mat:
    pass


@pytest.fixture(scope="module")
def toy_matrix(gpu_ctx):
    rng = np.random.default_rng(66)
    M, C = 400, 132
    mat = _Mat()
    mat.labels = ["c%03d" % i for i in range(C)]
    mat.k = 15
    mat.keys = np.unique(rng.integers(0, 4 ** 15, 2 * M, dtype=np.int64))[:M].astype(np.uint64)
    mat.counts = rng.poisson(6, (M, C)).astype(np.uint32)
    lift = rng.integers(0, 3, M)                         # a third of the rows each: first subgenome, second, neither
    mat.counts[lift == 0, :66] += rng.integers(1, 4, (int((lift == 0).sum()), 1)).astype(np.uint32)
    mat.counts[lift == 1, 66:] += rng.integers(1, 4, (int((lift == 1).sum()), 1)).astype(np.uint32)
    mat.lengths = rng.integers(10 ** 6, 2 * 10 ** 6, C)
    mat.freqs = mat.counts / mat.lengths.astype(np.float64)
    mat.ctx = gpu_ctx
    # chromosomes of the two subgenomes alternate: the lists are not runs of the matrix
    perm = rng.permutation(C)
    sg = {mat.labels[c]: ("SG1" if i < 66 else "SG2") for i, c in enumerate(perm)}
    counts = mat.counts.copy()
    mat.counts[:, perm] = counts
    mat.freqs = mat.counts / mat.lengths.astype(np.float64)
    return mat, sg


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("method", rw.METHODS)
def test_cluster_output_kmers_on_the_device(gpu_ctx, toy_matrix, method, staged, caplog):
    mat, sg = toy_matrix
    host = cluster.Cluster(mat, n_clusters=2, sg_assigned=dict(sg))
    host._ctx = None                                                       # the numpy / scipy path, as before
    sgs = sorted(set(host.d_sg.values()))
    groups = [[i for i, c in enumerate(host.chrs) if host.d_sg[c] == s] for s in sgs]
    assert [len(g) for g in groups] == [66, 66]
    ref_p = cluster.numpy_kmer_test(host.raw_data, groups, method)[2]
    # the condition on the input: no reference p-value within a relative 1e-9 of the threshold -- then no row is excused
    assert (np.abs(ref_p - MAX_PVAL) > 1e-9 * MAX_PVAL).all()
    assert (ref_p <= MAX_PVAL).sum() > 50 and (ref_p > MAX_PVAL).sum() > 50
    ref_buf, buf = io.StringIO(), io.StringIO()
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        ref = host.output_kmers(ref_buf, max_pval=MAX_PVAL, test_method=method)
    assert len([r for r in caplog.records if "on the host" in r.getMessage()]) == 1
    caplog.clear()
    dev = cluster.Cluster(mat, n_clusters=2, sg_assigned=dict(sg))
    if staged:
        dev._counts_dev = gpu_ctx.stage_rows(mat.counts)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = dev.output_kmers(buf, max_pval=MAX_PVAL, test_method=method)
    assert not [r for r in caplog.records if "on the host" in r.getMessage()]
    assert dev._counts_dev is None and not getattr(gpu_ctx, "_staged_rows", None)
    assert len(labels.keys) == int((ref_p <= MAX_PVAL).sum())
    assert (labels.keys == ref.keys).all() and (labels.sg_idx == ref.sg_idx).all() and labels.sg_names == ref.sg_names
    a = [l.split("\t") for l in buf.getvalue().splitlines()]
    b = [l.split("\t") for l in ref_buf.getvalue().splitlines()]
    assert [r[:2] for r in a] == [r[:2] for r in b]
    assert hr.tail_ok([float(r[2]) for r in a[1:]], [float(r[2]) for r in b[1:]]).all()
