"""GPU: the paired k-mer test (sp_wilcoxon.hip: k7_wilcoxon, Context.kmer_wilcoxon) for test_method = wilcoxon, against the
numpy twin of the header (tests/wilcoxon_ref.py) and against the host path the CLI took before (cluster.numpy_kmer_test):

  twin        means bytes ==, top and second ==, stat == (NaN where NaN), p of the permutation branch ==, other p within
              hp_reference.tail_ok (relative 1e-10 on [1e-290, 0.5], absolute 1e-13 above), NaN where NaN
  host path   the same top / second, p within tail_ok, NaN where NaN
M = 130 and 300: with the 128-thread workgroup (n <= 32) a full workgroup and a partial one, with the 64-thread workgroup
(n > 32) two and four full ones and a partial one.  The cases are those of tests/test_wilcoxon_host.py
(tests/wilcoxon_cases.py), plus staged rows, one group alone, the entry conditions and error codes, and
Cluster.output_kmers on a toy genome."""
import ctypes
import io
import logging

import numpy as np
import pytest

import hp_reference as hr
import wilcoxon_cases as wc
import wilcoxon_ref as wr
from subphaser_amd import _native, cluster

pytestmark = pytest.mark.gpu


def _same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def _tail(p, ref):
    """tail_ok, NaN where NaN: the rows that fail"""
    nan = np.isnan(ref)
    return np.flatnonzero(~np.where(nan, np.isnan(p), hr.tail_ok(p, np.where(nan, 1.0, ref))))


def _perm_rows(counts, lengths, groups, top, second):
    """the rows whose test takes the permutation branch (by the twin's integers)"""
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    out = np.zeros(len(counts), bool)
    for r in range(len(counts)):
        if top[r] != second[r]:
            out[r] = wr.rows(X[r:r + 1, groups[top[r]]], X[r:r + 1, groups[second[r]]])[2][0] == wr.PERM
    return out


def _check(gpu_ctx, counts, lengths, groups, ref=None, stage=False, host=True):
    M = len(counts)
    got = gpu_ctx.kmer_wilcoxon(counts, lengths, groups)
    top, second, p, means, stat = got
    assert top.shape == second.shape == p.shape == stat.shape == (M,) and means.shape == (M, len(groups))
    assert top.dtype == second.dtype == np.int32 and p.dtype == stat.dtype == means.dtype == np.float64
    rt, rs, rp, rm, rst = ref if ref else wr.kmer_wilcoxon(counts, lengths, groups)
    assert means.tobytes() == rm.tobytes(), np.argwhere(means != rm)[:5]
    assert (top == rt).all() and (second == rs).all(), np.nonzero((top != rt) | (second != rs))[0][:5]
    assert _same(stat, rst), np.nonzero(~((stat == rst) | (np.isnan(stat) & np.isnan(rst))))[0][:5]
    perm = _perm_rows(counts, lengths, groups, rt, rs)
    assert p[perm].tobytes() == rp[perm].tobytes(), [(r, p[r], rp[r]) for r in np.flatnonzero(perm & (p != rp))[:5]]
    bad = _tail(p, rp)
    assert bad.size == 0, [(r, p[r], rp[r]) for r in bad[:5]]
    if host:
        X = counts.astype(np.float64) / lengths.astype(np.float64)
        ht, hs, hp, _ = cluster.numpy_kmer_test(X, groups, "wilcoxon")
        assert (top == ht).all() and (second == hs).all(), np.nonzero((top != ht) | (second != hs))[0][:5]
        bad = _tail(p, hp)
        assert bad.size == 0, [(r, p[r], hp[r]) for r in bad[:5]]
    if stage:
        staged = gpu_ctx.stage_rows(counts)
        try:
            again = gpu_ctx.kmer_wilcoxon(staged, lengths, groups)
        finally:
            gpu_ctx.release_rows()
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
    return got, perm


@pytest.mark.parametrize("M", [130, 300])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("hi", wc.RANGES)
@pytest.mark.parametrize("n", wc.SIZES)
def test_group_sizes(gpu_ctx, n, hi, G, M):
    counts, lengths, groups = wc.case(n, hi, G, M)
    assert any(np.any(np.diff(g) != 1) for g in groups) and counts.shape[1] > G * n
    (top, second, p, means, stat), perm = _check(gpu_ctx, counts, lengths, groups, ref=wc.twin(n, hi, G, M))
    assert len(set(top.tolist())) == G                       # every group is on top somewhere
    if hi == 3 and 2 < n <= wr.PERM_MAX:
        assert perm.sum() > M // 2
    if n > wr.PERM_MAX or hi == 100000:
        assert not perm.any()


@pytest.mark.parametrize("i", range(len(wc.HAND)))
def test_hand_made_rows(gpu_ctx, i):
    what, _, _, branch, p_ref, stat_ref = wc.HAND[i]
    counts, lengths, groups = wc.hand(i)
    (top, second, p, means, stat), perm = _check(gpu_ctx, counts, lengths, groups)
    assert (perm == (branch == wr.PERM)).all(), what
    assert top.tolist() in ([0, 1, 0], [0, 0, 0]) and (second == 1 - top).all(), what      # [0, 0, 0]: a == b
    if p_ref is not None:
        assert _same(p, np.full(3, p_ref)), (what, p)
    if stat_ref is not None:
        assert (stat == stat_ref).all(), (what, stat)


def test_staged_rows_give_the_same_bytes(gpu_ctx):
    for args in ((7, 3, 3, 300), (13, 40, 2, 130), (64, 100000, 2, 130)):
        counts, lengths, groups = wc.case(*args)
        _check(gpu_ctx, counts, lengths, groups, ref=wc.twin(*args), stage=True, host=False)


def test_one_group(gpu_ctx):
    counts = np.arange(40, dtype=np.uint32).reshape(10, 4)
    lengths = np.full(4, 7, np.int64)
    top, second, p, means, stat = gpu_ctx.kmer_wilcoxon(counts, lengths, [[2, 0, 1]])
    rm = wr.kmer_wilcoxon(counts, lengths, [[2, 0, 1]])[3]
    assert (top == 0).all() and (second == 0).all() and (p == 1.0).all() and np.isnan(stat).all()
    assert means.tobytes() == rm.tobytes()


def test_entry_conditions(gpu_ctx):
    counts = np.ones((3, 140), np.uint32)
    lengths = np.full(140, 1000, np.int64)
    with pytest.raises(ValueError, match="sp_kmer_wilcoxon.*65"):
        gpu_ctx.kmer_wilcoxon(counts, lengths, [list(range(65)), list(range(65, 130))])
    gpu_ctx.kmer_wilcoxon(counts, lengths, [list(range(64)), list(range(64, 128))])
    with pytest.raises(ValueError, match="sp_kmer_wilcoxon.*subgenomes of 1 chromosomes"):
        gpu_ctx.kmer_wilcoxon(counts, lengths, [[0], [1]])
    with pytest.raises(ValueError, match="sp_kmer_wilcoxon.*subgenomes of 3 and 2 chromosomes"):
        gpu_ctx.kmer_wilcoxon(counts, lengths, [[0, 1, 2], [3, 4]])
    zero = lengths.copy()
    zero[139] = 0
    with pytest.raises(ValueError, match="sp_kmer_wilcoxon.*chromosome 139 has length 0"):
        gpu_ctx.kmer_wilcoxon(counts, zero, [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="sp_kmer_wilcoxon.*out of range"):
        gpu_ctx.kmer_wilcoxon(counts, lengths, [[0, 1], [2, 140]])
    with pytest.raises(ValueError, match="lengths for"):
        gpu_ctx.kmer_wilcoxon(counts, lengths[:5], [[0, 1], [2, 3]])
    top, second, p, means, stat = gpu_ctx.kmer_wilcoxon(np.zeros((0, 140), np.uint32), lengths, [[0, 1], [2, 3]])
    assert top.shape == second.shape == p.shape == stat.shape == (0,) and means.shape == (0, 2)
    # the rank-sum entry keeps refusing the method, by index and by name
    with pytest.raises(ValueError, match="sp_kmer_ranktest.*method 2"):
        gpu_ctx.kmer_ranktest(counts, lengths, [[0, 1], [2, 3]], 2)
    with pytest.raises(ValueError, match="method must be one of"):
        gpu_ctx.kmer_ranktest(counts, lengths, [[0, 1], [2, 3]], "wilcoxon")


def test_error_codes_and_null_pointers(gpu_ctx):
    vp = ctypes.c_void_p
    counts, lengths = np.ones((2, 140), np.uint32), np.full(140, 9, np.int64)
    gch = np.arange(140, dtype=np.int32)
    top, sec, p, means = np.empty(2, np.int32), np.empty(2, np.int32), np.empty(2), np.empty((2, 2))
    ptr = lambda a: vp(a.ctypes.data)
    ok = np.array([0, 3, 6], np.int32)

    def call(c=counts, l=lengths, off=ok, ch=gch, t=top, pv=p):
        return gpu_ctx.L.sp_kmer_wilcoxon(gpu_ctx.h, ptr(c) if c is not None else None, 2, 140, ptr(l) if l is not None else None, 2,
                                          ptr(off) if off is not None else None, ptr(ch), ptr(t) if t is not None else None,
                                          ptr(sec), ptr(pv) if pv is not None else None, ptr(means), None)
    assert call() == _native.SP_OK                                         # stat may be NULL
    assert (p == 1.0).all()                                                # all d zero at n = 3
    for off, words in (([0, 65, 130], b"65"), ([0, 1, 2], b"1 chromosomes"), ([0, 3, 5], b"3 and 2")):
        assert call(off=np.array(off, np.int32)) == _native.SP_EUNSUP
        msg = gpu_ctx.L.sp_last_error(gpu_ctx.h)
        assert b"sp_kmer_wilcoxon" in msg and words in msg, msg
    assert call(off=np.array([0, 64, 128], np.int32)) == _native.SP_OK
    assert call(c=None) == _native.SP_EINVAL and call(l=None) == _native.SP_EINVAL and call(off=None) == _native.SP_EINVAL
    assert call(t=None) == _native.SP_EINVAL and call(pv=None) == _native.SP_EINVAL
    assert call(off=np.array([0, 0, 3], np.int32)) == _native.SP_EINVAL    # an empty group
    zero = lengths.copy()
    zero[7] = 0
    assert call(l=zero) == _native.SP_EINVAL
    bad = gch.copy()
    bad[4] = 140
    assert call(ch=bad) == _native.SP_EINVAL
    bad[4] = -1
    assert call(ch=bad) == _native.SP_EINVAL
    assert b"sp_kmer_wilcoxon" in gpu_ctx.L.sp_last_error(gpu_ctx.h)


# ---- through Cluster.output_kmers
TOY = dict(seed=7, n_sets=5, chrom_len=30000, copies=25)      # the toy genome of test_gpu_ranktest.py: five chromosomes per subgenome
MAX_PVAL = 0.07                                               # 2 / 2^5 = 0.0625 is the smallest p five pairs can give


@pytest.fixture(scope="module")
def toy_matrix(gpu_ctx):
    import parity_cases as pc
    from subphaser_amd import jellyfish
    from toygenome import make_toy_genome
    toy = make_toy_genome(**TOY)
    files = pc.register_toy(toy, prefix="/virtual/wxtoy/")
    dumps = jellyfish.run_jellyfish_dumps(files, k=pc.K, lower_count=pc.L, ctx=gpu_ctx)
    jd = jellyfish.JellyfishDumps(dumps, toy["labels"])
    return toy, jd.filter(jd.to_matrix(), jd.lengths, toy["sgs"], min_freq=4, min_fold=1.2)


def test_cluster_output_kmers_on_the_device(gpu_ctx, toy_matrix, caplog):
    toy, d2 = toy_matrix
    assert d2.ctx is gpu_ctx and len(d2.keys) > 1000
    host = cluster.Cluster(d2, n_clusters=2, sg_assigned=dict(toy["sg_assigned"]))
    host._ctx = None                                                       # the numpy / scipy path, as before
    sgs = sorted(set(host.d_sg.values()))
    groups = [[i for i, c in enumerate(host.chrs) if host.d_sg[c] == sg] for sg in sgs]
    assert [len(g) for g in groups] == [5, 5]
    ref_p = cluster.numpy_kmer_test(host.raw_data, groups, "wilcoxon")[2]
    # the condition on the input: no reference p-value within a relative 1e-9 of the threshold -- then no row is excused
    assert (np.abs(ref_p - MAX_PVAL) > 1e-9 * MAX_PVAL).all()
    assert (ref_p <= MAX_PVAL).any() and (ref_p > MAX_PVAL).any()
    ref_buf, buf = io.StringIO(), io.StringIO()
    ref = host.output_kmers(ref_buf, max_pval=MAX_PVAL, test_method="wilcoxon")
    dev = cluster.Cluster(d2, n_clusters=2, sg_assigned=dict(toy["sg_assigned"]))
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        labels = dev.output_kmers(buf, max_pval=MAX_PVAL, test_method="wilcoxon")
    assert not [r for r in caplog.records if "on the host" in r.getMessage()]
    assert len(labels.keys) == int((ref_p <= MAX_PVAL).sum())
    assert (labels.keys == ref.keys).all() and (labels.sg_idx == ref.sg_idx).all() and labels.sg_names == ref.sg_names
    a = [l.split("\t") for l in buf.getvalue().splitlines()]
    b = [l.split("\t") for l in ref_buf.getvalue().splitlines()]
    assert [r[:2] for r in a] == [r[:2] for r in b]
    assert hr.tail_ok([float(r[2]) for r in a[1:]], [float(r[2]) for r in b[1:]]).all()
