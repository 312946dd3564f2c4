"""GPU: the rank-sum k-mer tests (sp_ranktest.hip: k7_ranktest, Context.kmer_ranktest) for test_method = kruskal and
mannwhitneyu, against the numpy twin of the header (tests/ranktest_ref.py) and against the host path the CLI took before
(cluster.numpy_kmer_test):

  twin        top, second and means bytes ==, stat == (NaN where NaN), p within hp_reference.tail_ok (relative 1e-10 on
              [1e-290, 0.5], absolute 1e-13 above)
  host path   the same top / second, p within tail_ok
M = 130 and 300: a full workgroup of 128 threads and a partial one; group pairs of more than 64 values take the 64-thread
shape.  The cases are those of tests/test_ranktest_host.py (tests/ranktest_cases.py) plus matrices of three and five
interleaved groups, staged rows, the entry conditions and Cluster.output_kmers on a toy genome."""
import ctypes
import io
import logging

import numpy as np
import pytest

import hp_reference as hr
import ranktest_cases as rc
import ranktest_ref as rr
from subphaser_amd import _native, cluster

pytestmark = pytest.mark.gpu


def _same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def _check(gpu_ctx, counts, lengths, groups, ref=None, stage=False, host=True):
    """both methods on one matrix; returns {method: (top, second, p, means, stat)}"""
    out = {}
    M = len(counts)
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    for m in rr.METHODS:
        got = gpu_ctx.kmer_ranktest(counts, lengths, groups, m)
        top, second, p, means, stat = got
        assert top.shape == second.shape == p.shape == stat.shape == (M,) and means.shape == (M, len(groups))
        assert top.dtype == second.dtype == np.int32 and p.dtype == stat.dtype == means.dtype == np.float64
        rt, rs, rp, rm, rst = ref[m] if ref else rr.kmer_ranktest(counts, lengths, groups, m)
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
                again = gpu_ctx.kmer_ranktest(staged, lengths, groups, m)
            finally:
                gpu_ctx.release_rows()
            for a, b in zip(got, again):
                assert a.tobytes() == b.tobytes(), m
        out[m] = got
    return out


@pytest.mark.parametrize("M", [130, 300])
@pytest.mark.parametrize("ties", [True, False])
@pytest.mark.parametrize("n1,n2", rc.SIZES)
def test_group_sizes(gpu_ctx, n1, n2, ties, M):
    counts, lengths, groups = rc.size_case(n1, n2, ties, M)
    out = _check(gpu_ctx, counts, lengths, groups, ref=rc.twin("size", n1, n2, ties, M))
    assert set(out["kruskal"][0].tolist()) == {0, 1}     # both orders of the pair are met


@pytest.mark.parametrize("ties", [True, False])
@pytest.mark.parametrize("G,M", [(3, 130), (5, 300)])
def test_interleaved_groups(gpu_ctx, G, M, ties):
    counts, lengths, groups = rc.layout_case(G, ties, M)
    assert counts.shape[1] > sum(len(g) for g in groups) and len({len(g) for g in groups}) == G
    assert any(np.any(np.diff(g) != 1) for g in groups)      # not consecutive runs
    out = _check(gpu_ctx, counts, lengths, groups, ref=rc.twin("layout", G, ties, M))
    top, second = out["mannwhitneyu"][:2]
    assert len(set(top.tolist())) == G and len(set(zip(top.tolist(), second.tolist()))) > G


def test_hand_made_rows(gpu_ctx):
    counts, lengths, groups, what = rc.hand_rows()
    out = _check(gpu_ctx, counts, lengths, groups)
    top, second, p, means, stat = out["kruskal"]
    assert (top == 0).all() and (second == 1).all()
    assert np.isnan(stat[0]) and p[0] == 1.0                               # all values identical
    top, second, p, means, stat = out["mannwhitneyu"]
    assert p[0] == 1.0 and stat[0] == 6.0
    assert p[1] == p[2] == 2.0 / 35.0 and stat[1] == stat[2] == 12.0       # the exact tail of 3 | 4, separated


def test_staged_rows_give_the_same_bytes(gpu_ctx):
    for args in ((7, 7, True, 300), (64, 64, False, 130)):
        counts, lengths, groups = rc.size_case(*args)
        _check(gpu_ctx, counts, lengths, groups, ref=rc.twin("size", *args), stage=True, host=False)
    counts, lengths, groups = rc.layout_case(5, False, 300)
    _check(gpu_ctx, counts, lengths, groups, ref=rc.twin("layout", 5, False, 300), stage=True, host=False)


def test_one_group(gpu_ctx):
    counts = np.arange(40, dtype=np.uint32).reshape(10, 4)
    for m in rr.METHODS:
        top, second, p, means, stat = gpu_ctx.kmer_ranktest(counts, np.full(4, 7, np.int64), [[2, 0, 1]], m)
        rt, rs, rp, rm, rst = rr.kmer_ranktest(counts, np.full(4, 7, np.int64), [[2, 0, 1]], m)
        assert (top == 0).all() and (second == 0).all() and (p == 1.0).all() and np.isnan(stat).all()
        assert means.tobytes() == rm.tobytes()


def test_entry_conditions(gpu_ctx):
    counts = np.ones((3, 70), np.uint32)
    lengths = np.full(70, 1000, np.int64)
    with pytest.raises(ValueError, match="sp_kmer_ranktest.*65"):
        gpu_ctx.kmer_ranktest(counts, lengths, [list(range(65)), [65, 66]], "kruskal")
    gpu_ctx.kmer_ranktest(counts, lengths, [list(range(64)), [65, 66]], "kruskal")
    with pytest.raises(ValueError, match="sp_kmer_ranktest.*method 2"):
        gpu_ctx.kmer_ranktest(counts, lengths, [[0, 1], [2, 3]], 2)
    with pytest.raises(ValueError, match="method must be one of"):
        gpu_ctx.kmer_ranktest(counts, lengths, [[0, 1], [2, 3]], "wilcoxon")
    zero = lengths.copy()
    zero[69] = 0
    with pytest.raises(ValueError, match="sp_kmer_ranktest.*chromosome 69 has length 0"):
        gpu_ctx.kmer_ranktest(counts, zero, [[0, 1], [2, 3]], "mannwhitneyu")
    with pytest.raises(ValueError, match="sp_kmer_ranktest.*out of range"):
        gpu_ctx.kmer_ranktest(counts, lengths, [[0, 1], [2, 70]], "mannwhitneyu")
    for m in rr.METHODS:
        top, second, p, means, stat = gpu_ctx.kmer_ranktest(np.zeros((0, 70), np.uint32), lengths, [[0, 1], [2, 3, 4]], m)
        assert top.shape == second.shape == p.shape == stat.shape == (0,) and means.shape == (0, 2)


def test_error_codes_and_null_pointers(gpu_ctx):
    vp = ctypes.c_void_p
    counts, lengths = np.ones((2, 70), np.uint32), np.full(70, 9, np.int64)
    goff, gch = np.array([0, 65, 67], np.int32), np.arange(67, dtype=np.int32)
    top, sec, p, means = np.empty(2, np.int32), np.empty(2, np.int32), np.empty(2), np.empty((2, 2))
    ptr = lambda a: vp(a.ctypes.data)

    def call(c=counts, l=lengths, off=goff, method=0, t=top):
        return gpu_ctx.L.sp_kmer_ranktest(gpu_ctx.h, ptr(c) if c is not None else None, 2, 70, ptr(l) if l is not None else None, 2,
                                          ptr(off), ptr(gch), method, ptr(t) if t is not None else None, ptr(sec), ptr(p),
                                          ptr(means), None)
    assert call() == _native.SP_EUNSUP
    ok = np.array([0, 3, 67], np.int32)
    assert call(off=ok) == _native.SP_OK                                   # stat may be NULL
    assert call(off=ok, method=2) == _native.SP_EINVAL and call(off=ok, method=-1) == _native.SP_EINVAL
    assert call(off=ok, c=None) == _native.SP_EINVAL and call(off=ok, l=None) == _native.SP_EINVAL
    assert call(off=ok, t=None) == _native.SP_EINVAL
    assert b"sp_kmer_ranktest" in gpu_ctx.L.sp_last_error(gpu_ctx.h)


# ---- through Cluster.output_kmers
TOY = dict(seed=7, n_sets=5, chrom_len=30000, copies=25)      # five chromosomes per subgenome: both tests reach p < 0.01
MAX_PVAL = 0.05


@pytest.fixture(scope="module")
def toy_matrix(gpu_ctx):
    import parity_cases as pc
    from subphaser_amd import jellyfish
    from toygenome import make_toy_genome
    toy = make_toy_genome(**TOY)
    files = pc.register_toy(toy, prefix="/virtual/ranktoy/")
    dumps = jellyfish.run_jellyfish_dumps(files, k=pc.K, lower_count=pc.L, ctx=gpu_ctx)
    jd = jellyfish.JellyfishDumps(dumps, toy["labels"])
    return toy, jd.filter(jd.to_matrix(), jd.lengths, toy["sgs"], min_freq=4, min_fold=1.2)


@pytest.mark.parametrize("method", rr.METHODS)
def test_cluster_output_kmers_on_the_device(gpu_ctx, toy_matrix, method, caplog):
    toy, d2 = toy_matrix
    assert d2.ctx is gpu_ctx and len(d2.keys) > 1000
    host = cluster.Cluster(d2, n_clusters=2, sg_assigned=dict(toy["sg_assigned"]))
    host._ctx = None                                                       # the numpy / scipy path, as before
    sgs = sorted(set(host.d_sg.values()))
    groups = [[i for i, c in enumerate(host.chrs) if host.d_sg[c] == sg] for sg in sgs]
    ref_p = cluster.numpy_kmer_test(host.raw_data, groups, method)[2]
    # the condition on the input: no reference p-value within a relative 1e-9 of the threshold -- then no row is excused
    assert (np.abs(ref_p - MAX_PVAL) > 1e-9 * MAX_PVAL).all()
    assert (ref_p <= MAX_PVAL).any() and (ref_p > MAX_PVAL).any()
    ref_buf, buf = io.StringIO(), io.StringIO()
    ref = host.output_kmers(ref_buf, max_pval=MAX_PVAL, test_method=method)
    dev = cluster.Cluster(d2, n_clusters=2, sg_assigned=dict(toy["sg_assigned"]))
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = dev.output_kmers(buf, max_pval=MAX_PVAL, test_method=method)
    assert not [r for r in caplog.records if "on the host" in r.getMessage()]
    assert len(labels.keys) == int((ref_p <= MAX_PVAL).sum())
    assert (labels.keys == ref.keys).all() and (labels.sg_idx == ref.sg_idx).all() and labels.sg_names == ref.sg_names
    a = [l.split("\t") for l in buf.getvalue().splitlines()]
    b = [l.split("\t") for l in ref_buf.getvalue().splitlines()]
    assert [r[:2] for r in a] == [r[:2] for r in b]
    assert hr.tail_ok([float(r[2]) for r in a[1:]], [float(r[2]) for r in b[1:]]).all()
