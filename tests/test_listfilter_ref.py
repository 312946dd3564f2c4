"""listfilter_ref (plain Python / numpy, from the written specification) against the C oracle, bit for bit, on every
hand-made input set of the list filter's device tests at its small size; decide_pairs_vec against decide_row; and what
the threshold matrix covers, classified with the exact margin.  No GPU."""
from collections import Counter

import numpy as np
import pytest

import listfilter_cases as lc
import listfilter_ref as lr
import pyoracle as po

N_MATRIX = 20000


def _same_as_oracle(lists, lengths, sgs, kw, vec=False):
    ref = lr.filter(lists, lengths, sgs, vec=vec, **kw)
    exp = po.filter_dumps(lists, sgs, list(range(len(lists))), lengths=lengths, **kw)
    n_union, keys, counts, tot, hist, freqs = ref
    assert (n_union, len(keys), len(hist)) == (exp.n_union, len(exp.keys), len(exp.hist))
    assert (keys == exp.keys).all() and (counts == exp.counts).all() and (tot == exp.tot).all()
    assert (hist == np.sort(exp.hist)).all() and (freqs == exp.freqs).all()
    assert (exp.lengths == np.asarray(lengths)).all()
    return ref


@pytest.fixture(scope="module")
def matrices():
    return {regime: lc.threshold_matrix(12, regime, N_MATRIX, seed=1) for regime in ("long", "short")}


@pytest.mark.parametrize("regime", ["long", "short"])
@pytest.mark.parametrize("argset", lc.ARGSETS_12, ids=lambda a: "%s-f%g-b%d-r%d_%s-%s" % (a[0], a[1], a[2], *a[3], a[4]))
def test_ref_equals_oracle_threshold_matrix(matrices, regime, argset):
    mat, lengths = matrices[regime]
    lists = lc.lists_of(lc.random_keys(len(mat), 17, seed=5), mat)
    memo = {}
    sgs, kw = lc.resolve_args(argset, 12, lambda sgs, **kw: lr.filter(lists, lengths, sgs, memo=memo, **kw))
    n_union, keys, counts, tot, hist, freqs = _same_as_oracle(lists, lengths, sgs, kw)
    assert n_union == N_MATRIX and 20 < len(keys) < n_union and (len(hist) < n_union) == (kw["ratio"] > 0)
    if argset[4] == "tot":        # rows that sit on the frequency bounds are kept
        assert (tot == np.uint64(kw["min_freq"])).any() and (tot == np.uint64(kw["max_freq"])).any()
    if argset[4] == "frac":
        assert kw["min_freq"] != int(kw["min_freq"]) and tot.min() > kw["min_freq"] and len(hist) > len(keys)
    num, den = argset[3]
    if num and den in (3, 5):     # include / n_multi == ratio occurs, and such a k-mer is kept
        assert lc.n_multi(sgs) == den
        on = [row for row in counts.tolist()
              if sum(lr.set_passes(row, lengths, sg, kw["min_fold"], kw["baseline"]) for sg in sgs if len(sg) > 1) == num]
        assert len(on) >= 20


@pytest.mark.parametrize("C,k,regime", [(65, 17, "long"), (130, 32, "short")])
def test_ref_equals_oracle_wide_matrix(C, k, regime):
    mat, lengths = lc.threshold_matrix(C, regime, 1500, seed=C, fill=0.05)
    lists = lc.lists_of(lc.random_keys(len(mat), k, seed=C + 1), mat)
    for argset in lc.ARGSETS_WIDE:
        memo = {}
        sgs, kw = lc.resolve_args(argset, C, lambda sgs, **kw: lr.filter(lists, lengths, sgs, memo=memo, **kw))
        ref = _same_as_oracle(lists, lengths, sgs, kw)
        assert 20 < len(ref[1]) < ref[0]
    assert lc.n_multi(lc.structures(130)["s5"]) >= 33


@pytest.mark.parametrize("C,k", [(12, 17), (12, 32), (65, 21)])
def test_ref_equals_oracle_edge_keys(C, k):
    lists, mat = lc.edge_keys(k, C, seed=k)
    keys = lists[0][0]
    assert keys[0] == 0 and int(keys[-1]) == lc.key_max(k) and len(lists[2][0]) == 0 and len(lists[C - 1][0]) == 0
    _, shift = lc.plan_ranges(sum(len(x) for x, _ in lists), C, k)
    ks = set(keys.tolist())
    for bit in (shift, shift - 1):        # neighbours across (and just inside) a range edge
        assert sum((x ^ (1 << bit)) in ks for x in ks) >= 6
    if k == 17:
        assert shift <= 31
    if k == 32:
        assert shift > 31
    ref = _same_as_oracle(lists, lc.lengths_for(C, "short"), lc.structures(C)["s5"],
                          dict(min_fold=2.0, baseline=1, min_freq=5.0, max_freq=1e9, ratio=0.4))
    assert 20 < len(ref[1]) < ref[0]


@pytest.mark.parametrize("make", [lc.all_present_case, lc.disjoint_case, lc.fifth_case], ids=lambda f: f.__name__)
@pytest.mark.parametrize("C", [4, 65])
def test_ref_equals_oracle_rows_cases(make, C):
    lists, lengths, sgs, kw = make(3000, C, 17, seed=2)
    for vec in (False, True):
        n_union, keys, counts, tot, hist, freqs = _same_as_oracle(lists, lengths, sgs, kw, vec=vec)
        if make is lc.fifth_case:
            assert len(keys) == n_union // 5 == len(hist)
        else:
            assert len(keys) == n_union == 3000


@pytest.mark.parametrize("variant", ["ratio0", "pairs"])
@pytest.mark.parametrize("C", [4, 65])
def test_ref_equals_oracle_second_pass_small(C, variant):
    lists, lengths, sgs, kw, kwc = lc.second_pass_case(C, variant, 5000, 3000, 17, seed=3)
    ref = _same_as_oracle(lists, lengths, sgs, kw, vec=True)
    assert len(ref[1]) == 5000 and (variant == "ratio0") == (ref[0] == 5000)
    ctl = _same_as_oracle(lists, lengths, sgs, kwc, vec=True)
    assert len(ctl[1]) == 3000 and (ctl[1] == ref[1][:3000]).all() and len(ctl[4]) == 5000


def test_ref_equals_oracle_skew():
    keys = lc.skew_keys(5000, 21, seed=4)
    assert len(set((keys >> np.uint64(18)).tolist())) == 1
    lists = lc.lists_of(keys, lc.pair_matrix(5000, 4, seed=4))
    ref = _same_as_oracle(lists, lc.lengths_for(4, "long"), lc.pair_sets(4), dict(lc.ROWS_KW, ratio=0.5), vec=True)
    assert 4000 < len(ref[1]) < 5000


def test_pairs_vec_equals_decide_row(matrices):
    """decide_pairs_vec against decide_row on rows of the threshold matrix (the columns of its sets A and B, whose
    units are single chromosomes), under every argument set's fold, ratio and frequency bounds"""
    n = mixed = 0
    for regime in ("long", "short"):
        mat, lengths = matrices[regime]
        sub = np.ascontiguousarray(mat[:5000, :4])
        sub = sub[sub.any(axis=1)]
        sgs = lc.pair_sets(4)
        for fold, ratio, lo, hi in ((2.0, 1.0, 1.0, 1e13), (1.5, 0.5, 100.0, 3e9), (2.0000001, 0.0, 2.5, 1e6), (1.0, 0.5, 1, 1e13)):
            for bl in (1, -1):
                h, r = lr.decide_pairs_vec(sub, lengths[:4], sgs, fold, bl, lo, hi, ratio)
                exp = [lr.decide_row(row, lengths[:4], sgs, fold, bl, lo, hi, ratio) for row in sub.tolist()]
                assert h.tolist() == [e[0] for e in exp] and r.tolist() == [e[1] for e in exp]
                assert 0 < r.sum() <= h.sum()
                mixed += 0 < h.sum() < len(sub) and r.sum() < h.sum()
        n += len(sub)
    assert n >= 5000 and mixed >= 4


def _classify(m):
    am = abs(m)
    if m == 0:
        return "zero"
    for name, lo, hi in (("tiny", 0, 1e-12), ("nano", 1e-9, 1e-6), ("mid", 1e-4, 1e-2)):
        if lo <= am < hi or (name == "mid" and am == hi):
            return name
    if 0.5e-5 <= am <= 2e-5:
        return "band"
    return "far" if am > 0.5 else None


@pytest.mark.parametrize("regime", ["long", "short"])
def test_threshold_matrix_coverage(matrices, regime):
    """Conditions on the INPUTS (exact margins, no filter involved): every class of distance from the fold threshold
    holds at least 20 (row, set) pairs on each side where the side exists, for min_fold 2 and 1.5 and baseline 1 and
    -1, in both length regimes; and at margin 0 the two regimes get different fp64 verdicts."""
    mat, lengths = matrices[regime]
    sgs = [sg for sg in lc.structures(12)["s5"] if len(sg) > 1]
    rows = mat[:8000].tolist()        # (enough of the matrix to hold every class; the whole of it holds no less)
    for fold in (2.0, 1.5):
        for bl in (1, -1):
            cnt = Counter()
            zero_verdicts = Counter()
            for row in rows:
                for sg in sgs:
                    m = lr.margin(row, lengths, sg, fold, bl)
                    if m is None:
                        cnt["allzero" if not any(row[c] for u in sg for c in u) else "lo0"] += 1
                        continue
                    cls = _classify(m)
                    if cls == "zero":
                        f = sorted((sum(row[c] for c in u) / sum(int(lengths[c]) for c in u) for u in sg), reverse=True)
                        lo = f[bl]
                        if regime == "long" and lo < 9e-5 or regime == "short" and lo > 2e-4:
                            zero_verdicts[lr.set_passes(row, lengths, sg, fold, bl)] += 1
                    if cls:
                        cnt[(cls, (m > 0) - (m < 0))] += 1
            need = [("zero", 0), "lo0", "allzero", ("far", 1)]
            need += [(c, s) for c in ("tiny", "nano", "band", "mid") for s in (1, -1)]
            for key in need:
                assert cnt[key] >= 20, (regime, fold, bl, key, cnt[key])
            # exactly on the threshold: the 1e-20 decides in the long regime (the set fails), is absorbed in the short
            # one (it passes).  With min_fold 2 the fp64 frequencies are in the exact ratio too (hi = 2 lo: lengths
            # in the ratios 1 and 2 only), so the verdict is the same for every such pair; with 1.5 the roundings of
            # the two quotients move single pairs across
            assert zero_verdicts[regime == "short"] >= 20, zero_verdicts
            if fold == 2.0:
                assert zero_verdicts[regime != "short"] == 0, zero_verdicts
