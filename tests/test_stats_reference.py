"""CPU: pin the high-precision reference (tests/hp_reference.py) and the CPU oracle it is used to judge.

The GPU statistics tests (tests/test_gpu_stats.py) compare the kernels with hp_reference at 1e-10 and with the
oracle at 1e-7; these tests establish that both yardsticks deserve it: the reference against exact rational sums,
the 30-digit golden tails and scipy, the oracle against the reference at clamp-scale margins."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import hp_reference as hr
import pyoracle as po

M = hr.MAX_INT


def _exact_tails(N, K, n):
    """{a: P[X >= a] as a Fraction} over the whole support, from math.comb."""
    lo, hi = max(0, n - (N - K)), min(K, n)
    w = {x: math.comb(K, x) * math.comb(N - K, n - x) for x in range(lo, hi + 1)}
    den = math.comb(N, n)
    out, acc = {}, 0
    for x in range(hi, lo - 1, -1):
        acc += w[x]
        out[x] = Fraction(acc, den)
    return out


@pytest.mark.parametrize("N,K,n,step", [
    (2000, 700, 900, 7),        # wide support, the mode at 315
    (1500, 1000, 1200, 3),      # lo = 700 > 0: a == lo gives d = 0
    (60, 20, 30, 1),
    (2000, 1, 1000, 1),         # K = 1: the support is {0, 1}
    (2000, 1999, 1999, 1),      # lo = 1998, hi = 1999
    (301, 150, 151, 1),
    (1200, 600, 300, 2),        # n < K: a == hi gives c = 0
])
def test_right_tail_exact_small(N, K, n, step):
    exact = _exact_tails(N, K, n)
    lo, hi = min(exact), max(exact)
    mode = ((n + 1) * (K + 1)) // (N + 2)
    picks = set(range(lo, hi + 1, step)) | {lo, lo + 1, hi - 1, hi, mode - 1, mode, mode + 1}
    picks = sorted(a for a in picks if lo <= a <= hi)
    seen = set()
    for a in picks:
        b, c, d = K - a, n - a, N - K - n + a
        assert min(b, c, d) >= 0
        seen |= {"d0"} if d == 0 else set()
        seen |= {"c0"} if c == 0 else set()
        got = hr.right_tail(a, b, c, d)
        want = exact[a]
        with mp.workdps(60):
            w = mp.mpf(want.numerator) / want.denominator
            assert abs(got - w) <= mp.mpf("1e-35") * w, (a, b, c, d, got, w)
        if a == lo:
            assert got == 1
    if lo > 0 or N - K - n == 0:
        assert "d0" in seen
    if n <= K:
        assert "c0" in seen


def test_right_tail_outside_support():
    assert hr.right_tail(0, 5, 3, 2) == 1
    with mp.workdps(50):                                   # a == hi: the single term C(3,3) C(4,0) / C(7,3)
        assert abs(hr.right_tail(3, 0, 0, 4) - mp.mpf(1) / 35) < mp.mpf("1e-45")
    assert hr.right_tail(0, 0, 0, 0) == 1


def test_right_tail_golden_mp(golden):
    for v in golden["G6_hypergeom_mp"]:
        with mp.workdps(40):
            want = mp.mpf(v["p"])
            got = hr.right_tail(*v["cells"])
            assert abs(got - want) <= mp.mpf("1e-25") * want, (v, got)


def test_right_tail_vs_scipy_moderate():
    from scipy import stats as st
    rng = np.random.RandomState(5)
    n_cmp = 0
    for _ in range(60):
        N = int(rng.randint(50, 200000))
        K = int(rng.randint(1, N))
        n = int(rng.randint(1, N))
        lo, hi = max(0, n - (N - K)), min(K, n)
        mode = ((n + 1) * (K + 1)) // (N + 2)
        sd = math.sqrt(max(n * K / N * (N - K) / N * (N - n) / max(N - 1, 1), 1.0))
        a = int(min(hi, max(lo, mode + rng.uniform(-5, 25) * sd)))
        p = hr.right_tail(a, K - a, n - a, N - K - n + a)
        sp = st.hypergeom.sf(a - 1, N, K, n)
        if float(p) < 1e-250:
            continue
        assert math.isclose(float(p), sp, rel_tol=1e-7, abs_tol=1e-300), (N, K, n, a, p, sp)
        n_cmp += 1
    assert n_cmp >= 40


def _regime(cells_unclamped):
    x21, x22 = cells_unclamped
    return (x21 > M, x22 > M)


def test_fisher_cells_vs_oracle_all_regimes():
    rng = np.random.RandomState(9)
    seen = set()
    for it in range(400):
        S = int(rng.randint(2, 6))
        kind = it % 4
        each = rng.randint(0, 5000, size=S).astype(np.int64)
        # totals: no clamp / x21 only (one large column) / x22 only (large others) / both (all large)
        big = rng.randint(M + 1, 3 * M, size=S)
        small = each + rng.randint(0, M // (2 * S), size=S)
        j = int(rng.randint(S))
        if kind == 0:
            total = small
        elif kind == 1:
            total = small.copy()
            total[j] = big[j]
        elif kind == 2:
            total = big.copy()
            total[j] = small[j]
        else:
            total = big
        total = np.maximum(total, each).astype(np.int64)
        x21 = int(total[j]) - int(each[j])
        x22 = int(total.sum()) - x21 - (int(each.sum()) - int(each[j]))
        seen.add(_regime((x21, x22)))
        assert hr.fisher_cells(each, total, j) == po.fisher_cells(each, total, j), (each, total, j)
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def _clamp_cells():
    """clamp-scale cells spread over p-decades: both clamps (K = R up to 9e5), x21 clamp only, one short of MAX_INT"""
    cells = [(450500, 450000, M, M), (200, 50, M - 5, M)]
    for R in (300, 4000, 60000, 900000):
        for z in (-6.0, -2.0, -0.5, 0.0, 0.7, 2.0, 4.0, 7.0, 12.0, 20.0, 35.0):
            n, N = R / 2 + M, R + 2.0 * M
            sd = math.sqrt(n * R / N * (N - R) / N * (N - n) / (N - 1))
            a = int(round(R * n / N + z * sd))
            if 0 < a <= R:
                cells.append((a, R - a, M, M))
    for a, b in ((40, 30), (4000, 3100), (70000, 69000)):
        cells.append((a, b, M, 120000000))        # x22 unclamped
        cells.append((a, b, 150000000, M))        # x21 unclamped
    return cells


def test_oracle_accuracy_at_clamp_scale():
    """The bound the GPU comparison kernel-vs-oracle (rtol 1e-7) rests on: the oracle's lgammal differences at
    N ~ 4.3e8 stay within 1e-8 of the mpmath tail (about 1.3e-9 measured)."""
    decades = set()
    for cell in _clamp_cells():
        ref = hr.right_tail(*cell)
        o = po.hypergeom_right_tail(*cell)
        r = float(ref)
        if r == 0.0 or ref == 1:
            assert o == r or o < 1e-300
            continue
        decades.add(int(math.floor(math.log10(r))))
        with mp.workdps(hr.DPS):
            if r < 1e-300:
                assert abs(o - r) <= 1e-300, (cell, o, ref)
                continue
            if r <= 0.5:
                assert abs(mp.mpf(o) - ref) <= 1e-8 * ref, (cell, o, ref)
            else:                                 # a complement: its error is relative to 1 - p, down to fp64's ulp
                assert abs(mp.mpf(o) - ref) <= 1e-8 * (1 - ref) + 2.3e-16, (cell, o, ref)
    assert len(decades) >= 15


def _scipy_t_rows(rng, n1, n2, n_rows):
    for _ in range(n_rows):
        xa = rng.poisson(rng.uniform(5, 500), size=n1) / float(rng.randint(10**6, 10**8))
        xb = rng.poisson(rng.uniform(5, 500), size=n2) / float(rng.randint(10**6, 10**8))
        yield xa.astype(np.float64), xb.astype(np.float64)


def test_ttest_p_vs_scipy():
    from scipy import stats as st
    rng = np.random.RandomState(3)
    for n1, n2 in ((5, 8), (2, 3), (1, 2), (64, 64), (13, 40)):
        for xa, xb in _scipy_t_rows(rng, n1, n2, 8):
            want = st.ttest_ind(xa, xb).pvalue
            got = hr.ttest_p(xa, xb)
            assert math.isclose(got, want, rel_tol=1e-12, abs_tol=1e-300), (n1, n2, got, want)
    z = np.zeros(3)
    assert math.isnan(hr.ttest_p(z, z))
    assert math.isnan(hr.ttest_p(np.ones(1), np.ones(1)))
    assert hr.ttest_p(np.full(3, 2.0), np.zeros(3)) == 0.0


def test_wheat_table_is_informative():
    """The generator of the GPU wheat-scale test must not collapse back to 0 / 1 p-values."""
    t = hr.wheat_table()
    assert t.shape == (14074, 3) and (t >= 0).all()
    tot = t.sum(axis=0)
    assert (tot >= 4e8).all() and (tot <= 8e8).all()
    p = po.enrich(t)[0]
    inf = (p > 1e-300) & (p < 1 - 1e-12)
    assert inf.mean() >= 0.5, inf.mean()
    # nearly every decade from 1 down to 1e-300 is populated, and some cells underflow
    dec = set(np.floor(np.log10(p[(p > 0) & (p < 1)])).astype(int).tolist())
    assert len(set(range(-300, 0)) - dec) <= 10
    assert (p == 0).sum() >= 100


def test_enrich_rows_vs_oracle_small():
    """enrich_rows' decisions and ratios against the oracle's on a small table (every non-fragile row)."""
    rng = np.random.RandomState(17)
    t = rng.poisson(40, size=(80, 4)).astype(np.int64)
    t[:20, 1] += rng.poisson(60, 20)
    t[20:25] = 0
    t[25:30, 2] = t[25:30, 3]                     # identical cells: a true tie, lowest index
    t[25:30, 0] = t[25:30, 1] = 0
    ref = hr.enrich_rows(t)
    with np.errstate(all="ignore"):
        op, oa, os_, orr = po.enrich(t)
    assert np.allclose(op, ref.p, rtol=1e-9, atol=1e-300)
    ok = ~ref.fragile
    assert ok.mean() > 0.9
    assert (oa[ok] == ref.argmin[ok]).all() and (os_[ok] == ref.sig[ok]).all()
    assert ((orr == ref.ratios) | (np.isnan(orr) & np.isnan(ref.ratios))).all()
    assert (ref.argmin[25:30] == 2).all()


def test_fragile_mask():
    """The mask flags a row whose p_min sits within the tolerance of max_pval, and no row with a clear decision."""
    p_fr = [0.05 * (1 + 1e-12), 0.9]
    cells = [(1, 2, 3, 4), (2, 1, 3, 4)]
    assert hr._row_fragile(p_fr, [False, False], cells, 0, 1, 0.05, True)
    assert not hr._row_fragile([0.01, 0.9], [False, False], cells, 0, 1, 0.05, True)
    assert not hr._row_fragile(p_fr, [False, False], cells, 0, 1, 0.05, False)   # the ratio decides alone
    assert hr._row_fragile([0.3, 0.3 * (1 + 1e-12)], [False, False], cells, 0, 1, 0.05, True)
    assert not hr._row_fragile([0.3, 0.3], [False, False], [cells[0], cells[0]], 0, 1, 0.05, True)
    # p_sub^2 against max_pval * p_min at the edge
    pm = 1e-3
    ps = math.sqrt(0.05 * pm)
    assert hr._row_fragile([pm, ps], [False, False], cells, 0, 1, 0.05, True)
    # both tails below TINY: kernel zeros may tie either way
    assert hr._row_fragile([1e-305, 3e-305], [False, False], cells, 0, 1, 0.05, True)
