"""GPU: the statistics kernels (sp_enrich.hip: k6_totals / k6_enrich, k7_ttest) against the high-precision
reference of tests/hp_reference.py -- relative 1e-10 on p in [1e-290, 0.5], absolute 1e-13 above, 1e-300 below --
and against the CPU oracle at 1e-7 on whole tables.  Decisions (argmin / sig) must equal the reference's on every
row a kernel within those tolerances could not turn (enrich_rows' `fragile` mask)."""
import math

import numpy as np
import pytest

import hp_reference as hr
import pyoracle as po

pytestmark = pytest.mark.gpu

M = hr.MAX_INT


def _np_ratios(t):
    """_enrich's ratios, row by row with numpy"""
    tot = t.sum(axis=0)
    out = np.empty(t.shape, np.float64)
    with np.errstate(all="ignore"):
        for w in range(t.shape[0]):
            q = np.array(t[w]) / tot
            out[w] = q / q.sum()
    return out


def _same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def _check_vs_reference(gpu_ctx, t, max_pval=0.05, min_ratio=0.5):
    """every cell against right_tail, decisions on non-fragile rows, ratios bit for bit; returns (kernel, ref)"""
    gp, ga, gs, gr = gpu_ctx.enrich(t, max_pval, min_ratio)
    ref = hr.enrich_rows(t, max_pval, min_ratio)
    ok = hr.tail_ok(gp, ref.p)
    assert ok.all(), [(w, j, ref.cells[w][j], gp[w, j], ref.p[w, j]) for w, j in zip(*np.nonzero(~ok))][:5]
    nf = ~ref.fragile
    assert (ga[nf] == ref.argmin[nf]).all(), np.nonzero((ga != ref.argmin) & nf)
    assert (gs[nf] == ref.sig[nf]).all(), np.nonzero((gs != ref.sig) & nf)
    assert _same(gr, ref.ratios)
    return (gp, ga, gs, gr), ref


# ------------------------------------------------------------------ wheat-scale window table
@pytest.fixture(scope="module")
def wheat():
    t = hr.wheat_table()
    return t, hr.enrich_rows(t)


def test_enrich_wheat_scale(gpu_ctx, wheat):
    t, ref = wheat
    gp, ga, gs, gr = gpu_ctx.enrich(t, 0.05, 0.5)
    op = po.enrich(t, 0.05, 0.5)[0]
    # the oracle on every cell
    assert np.allclose(gp, op, rtol=1e-7, atol=1e-300), np.abs(gp - op).max()
    # the reference on every cell, and the sample covers what it must: p-decades down to underflow, the complement
    # branch, the longest tails (the ballast rows, K ~ 1e9)
    ok = hr.tail_ok(gp, ref.p)
    assert ok.all(), [(w, j, ref.cells[w][j], gp[w, j], ref.p[w, j]) for w, j in zip(*np.nonzero(~ok))][:5]
    mid = (ref.p >= hr.TINY) & (ref.p <= 0.5)
    dec = set(np.floor(np.log10(ref.p[mid])).astype(int).tolist())
    assert len(set(range(-290, 0)) - dec) <= 10
    assert ((ref.p > 0.5) & (ref.p < 1 - 1e-12)).sum() >= 1000
    assert (ref.p == 0).sum() >= 100 and ((ref.p > 0) & (ref.p < 2.3e-308)).any()
    assert hr.rel_err(gp, ref.p) <= hr.TAIL_RTOL
    # decisions on every row the tolerances cannot turn; the mask stays small so this cannot go vacuous
    assert ref.fragile.mean() <= 0.005, ref.fragile.sum()
    nf = ~ref.fragile
    assert (ga[nf] == ref.argmin[nf]).all(), np.nonzero((ga != ref.argmin) & nf)
    assert (gs[nf] == ref.sig[nf]).all(), np.nonzero((gs != ref.sig) & nf)
    assert 0.1 < gs.mean() < 0.9
    assert _same(gr, ref.ratios) and _same(gr, _np_ratios(t))


def test_enrich_dev_matches_host_wheat(gpu_ctx, wheat):
    t, _ = wheat
    host = gpu_ctx.enrich(t, 0.05, 0.5)
    d = gpu_ctx.dev_alloc(t.nbytes)
    try:
        gpu_ctx.host_to_dev(d, np.ascontiguousarray(t))
        dev = gpu_ctx.enrich_dev(d, t.shape[0], t.shape[1], 0.05, 0.5)
    finally:
        gpu_ctx.dev_free(d)
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ crafted regimes
def _rows_at(rng, R_lo, R_hi, q, zs):
    """two-column rows (x, R - x) with x at R q + z sd (binomial sd), one per z"""
    out = []
    for z in zs:
        R = int(round(math.exp(rng.uniform(math.log(R_lo), math.log(R_hi)))))
        x = int(round(R * q + z * math.sqrt(R * q * (1 - q))))
        x = min(max(x, 0), R)
        out.append((x, R - x))
    return out


@pytest.mark.parametrize("regime", ["none", "x21", "x22", "both"])
def test_enrich_clamp_regimes(gpu_ctx, regime):
    """each clamp alone and both together; rows over the complement branch (within 3 sd of the mode) and the tail"""
    rng = np.random.RandomState({"none": 1, "x21": 2, "x22": 3, "both": 4}[regime])
    big, small = 3 * 10**8, 10**8
    T = {"none": (small, small), "x21": (big, small), "x22": (small, big), "both": (big, big)}[regime]
    zs = list(np.linspace(-3, 3, 25)) + list(np.linspace(3.5, 40, 30))
    # q: the share of column 0 at which a cell sits near its mode, by regime (0.5 when both clamp)
    q = {"none": 0.5, "x21": M / (M + T[1]), "x22": T[0] / (T[0] + M), "both": 0.5}[regime]
    rows = _rows_at(rng, 20, 2e5, q, zs) + [(x, y) for y, x in _rows_at(rng, 20, 2e5, 1 - q, zs[::3])]
    t = np.array(rows, np.int64)
    t = np.vstack([t, np.array(T, np.int64) - t.sum(axis=0)])
    assert (t >= 0).all()
    (gp, _, _, _), ref = _check_vs_reference(gpu_ctx, t)
    want = {"none": (False, False), "x21": (True, False), "x22": (False, True), "both": (True, True)}[regime]
    tot = t.sum(axis=0)
    hit = 0
    for w in range(t.shape[0] - 1):
        each = [int(v) for v in t[w]]
        x21 = int(tot[0]) - each[0]
        x22 = int(tot.sum()) - x21 - each[1]
        hit += (x21 > M, x22 > M) == want
    assert hit >= (t.shape[0] - 1) * 0.9
    inform = (ref.p > 1e-300) & (ref.p < 1 - 1e-12)
    assert inform[:-1, 0].sum() >= 30


def _x_for_tail(R, target):
    """the smallest x with the both-clamped cell (x, R - x, MAX, MAX) at right tail <= target (oracle bisection)"""
    lo, hi = R // 2, R
    while lo < hi:
        mid = (lo + hi) // 2
        if po.hypergeom_right_tail(mid, R - mid, M, M) <= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _ballast(t, T):
    return np.vstack([t, np.asarray(T, np.int64) - t.sum(axis=0)])


def test_enrich_far_tails_and_underflow(gpu_ctx):
    """tails at 1e-100 / 1e-200 / 1e-300, in the denormal range and below it (-> 0); p_min == 0 rows whose sig the
    ratio alone decides, both ways"""
    rows = []
    for R in (3000, 40000, 200000):
        for target in (1e-100, 1e-200, 1e-300, 1e-310, 1e-318, 1e-330):
            x = _x_for_tail(R, target)
            rows.append((x, R - x, 0))
            rows.append((x, 0, R - x))
    t = _ballast(np.array(rows, np.int64), (2 * 10**9, 5 * 10**8, 5 * 10**8))
    (gp, ga, gs, gr), ref = _check_vs_reference(gpu_ctx, t)
    p0 = ref.p[:-1, 0]
    for lo, hi in ((1e-101, 1e-99), (1e-201, 1e-199), (1e-301, 1e-299)):
        assert ((p0 > lo) & (p0 < hi)).any(), (lo, hi)
    assert ((p0 > 0) & (p0 < 2.2250738585072014e-308)).any()           # denormal
    assert (p0 == 0).any()
    z = ref.p[:-1].min(axis=1) == 0
    # p_min == 0: the sub-min test is skipped, min_ratio decides -- column 0's total is 4x the others', so a row with
    # 3/4 of its count in column 0 has a ratio below 0.5 and one with 7/8 above
    assert (ref.sig[:-1][z]).any() and (~ref.sig[:-1][z]).any()
    assert (gs[:-1][z] == ref.sig[:-1][z]).all()


def test_enrich_ratio_only_zero_p(gpu_ctx):
    rows = []
    for R in (20000, 100000):
        for frac in (0.6, 0.75, 0.8, 0.875, 0.95):
            rows.append((int(R * frac), R - int(R * frac), 0))
    t = _ballast(np.array(rows, np.int64), (2 * 10**9, 5 * 10**8, 5 * 10**8))
    (gp, ga, gs, gr), ref = _check_vs_reference(gpu_ctx, t)
    z = ref.p[:-1, 0] == 0
    assert z.sum() >= 6 and ref.sig[:-1][z].any() and (~ref.sig[:-1][z]).any()


def test_enrich_edges(gpu_ctx):
    """a <= lo (p = 1: a zero cell, a row that holds a whole column so d = 0), a == hi (b = 0, c = 0), exact p ties
    between identical columns (lowest index wins), an all-zero row, small margins (the stirlerr table and its
    short series)"""
    rng = np.random.RandomState(8)
    rows = [(0, 0, 0, 0), (0, 5, 7, 7), (40, 0, 0, 0), (9, 3, 3, 3), (30, 1, 6, 6), (2, 40, 40, 40)]
    for _ in range(60):                      # small margins: x, n - x, ... in 1..500
        a = rng.randint(0, 300, size=4)
        a[2] = a[3]
        rows.append(tuple(int(v) for v in a))
    t = np.array(rows, np.int64)
    (gp, ga, gs, gr), ref = _check_vs_reference(gpu_ctx, t)
    assert any(c[1] == 0 and c[0] > 0 for row in ref.cells for c in row)            # b = 0: a == hi
    # d = 0 needs a row holding every other column whole; c = 0 a row holding its own column whole
    (_, _, _, _), ref2 = _check_vs_reference(gpu_ctx, np.array([[0, 700, 300, 0], [50, 0, 0, 0]], np.int64))
    assert ref2.cells[0][0][3] == 0 and ref2.p[0, 0] == 1
    assert ref2.cells[1][0][2] == 0 and ref2.cells[1][0][0] == 50
    assert (gp[0] == 1).all() and ga[0] == 0 and not gs[0]       # all-zero row
    tie = [w for w in range(len(rows)) if ref.p[w, 2] == ref.p[w].min() and ref.p[w].argmin() == 2]
    assert len(tie) >= 3 and all(ga[w] == 2 and ref.argmin[w] == 2 for w in tie)   # columns 2 and 3 tie: 2 wins


def test_enrich_zero_column(gpu_ctx):
    """a column with total 0: x / 0 ratios give NaN (and inf), compared the way numpy compares them"""
    rng = np.random.RandomState(6)
    t = rng.poisson(30, size=(70, 3)).astype(np.int64)
    t[:, 1] = 0
    t[:10, 0] += 60
    (gp, ga, gs, gr), ref = _check_vs_reference(gpu_ctx, t)
    assert np.isnan(gr).all()
    assert (gs == ref.sig).all() and gs[:10].any()


@pytest.mark.parametrize("max_pval,min_ratio", [(0.01, 0.3), (1.0, 0.0)])
def test_enrich_thresholds(gpu_ctx, max_pval, min_ratio):
    rng = np.random.RandomState(int(max_pval * 100))
    t = rng.poisson(50, size=(120, 3)).astype(np.int64)
    t[:40, 0] += rng.poisson(20, 40)
    t[40:60, 2] += rng.poisson(60, 20)
    (gp, ga, gs, gr), ref = _check_vs_reference(gpu_ctx, t, max_pval, min_ratio)
    assert gs.any() and (~gs).any()


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("S", [2, 3, 7, 8, 9, 16, 17, 31, 32])
def test_enrich_shapes(gpu_ctx, S):
    """d_np_sum's 8-wide blocks and the 64-thread grid edge: W in {1, 63, 64, 65, 1000}.  Every cell against the
    oracle, decisions where the oracle's 1e-7 cannot turn them, ratios bit for bit, the first and last rows against
    the reference."""
    rng = np.random.RandomState(S)
    for W in (1, 63, 64, 65, 1000):
        t = rng.poisson(40, size=(W, S)).astype(np.int64)
        t[::7, rng.randint(S)] += 50
        gp, ga, gs, gr = gpu_ctx.enrich(t, 0.05, 0.5)
        op = po.enrich(t, 0.05, 0.5)[0]
        assert gp.shape == (W, S) and ga.shape == (W,) and gs.shape == (W,)
        assert np.allclose(gp, op, rtol=1e-7, atol=1e-300)
        tot = [int(v) for v in t.sum(axis=0)]
        for w in range(W):
            row = [int(v) for v in t[w]]
            cells = [hr.fisher_cells(row, tot, j) for j in range(S)]
            m, sg, q, fr = hr.decide_row(row, tot, op[w], cells, rtol=1e-7, atol=1e-7)
            assert fr or (ga[w] == m and gs[w] == sg), (W, w)
        assert _same(gr, _np_ratios(t))
        ref = hr.enrich_rows(t, rows=[0, W - 1])
        assert hr.tail_ok(gp[[0, W - 1]], ref.p).all()


def test_enrich_bad_widths(gpu_ctx):
    with pytest.raises(ValueError):
        gpu_ctx.enrich(np.ones((4, 1), np.int64))
    with pytest.raises(ValueError):
        gpu_ctx.enrich(np.ones((4, 33), np.int64))
    gp, ga, gs, gr = gpu_ctx.enrich(np.zeros((0, 3), np.int64))
    assert gp.shape == (0, 3) and ga.shape == (0,) and gs.shape == (0,) and gr.shape == (0, 3)


def test_enrich_totals_above_2_32(gpu_ctx):
    """k6_totals sums in 64 bits: column totals above 2^32"""
    rng = np.random.RandomState(11)
    t = rng.poisson(1000, size=(200, 3)).astype(np.int64)
    t[:3, 0] = 1_600_000_000
    t[3:6, 1] = 1_500_000_000
    assert (t.sum(axis=0)[:2] > 2**32).all()
    gp, ga, gs, gr = gpu_ctx.enrich(t, 0.05, 0.5)
    op, oa, os_, orr = po.enrich(t, 0.05, 0.5)
    assert np.allclose(gp, op, rtol=1e-7, atol=1e-300)
    assert _same(gr, orr) and _same(gr, _np_ratios(t))
    ref = hr.enrich_rows(t, rows=range(0, 200, 10))
    assert hr.tail_ok(gp[::10], ref.p).all()


# ------------------------------------------------------------------ k7_ttest
def _tt_check(gpu_ctx, counts, lengths, groups, stage=False):
    """kernel against ttest_p row by row (groups ordered by mean, ties in group order); returns kernel p, ref p"""
    top, second, pv, means = gpu_ctx.kmer_ttest(counts, lengths, groups)
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    ref = np.empty(len(counts))
    for r in range(len(counts)):
        mu = [X[r, g].sum() / len(g) for g in groups]
        order = sorted(range(len(groups)), key=lambda g: (-mu[g], g))
        assert (top[r], second[r]) == (order[0], order[1]), r
        assert (means[r] == mu).all(), r
        ref[r] = hr.ttest_p(X[r, groups[order[0]]], X[r, groups[order[1]]])
    nan = np.isnan(ref)
    assert (np.isnan(pv) == nan).all()
    ok = hr.tail_ok(pv[~nan], ref[~nan])
    assert ok.all(), [(r, pv[~nan][r], ref[~nan][r]) for r in np.nonzero(~ok)[0][:5]]
    if stage:
        staged = gpu_ctx.stage_rows(counts)
        try:
            got = gpu_ctx.kmer_ttest(staged, lengths, groups)
        finally:
            gpu_ctx.release_rows()
        for a, b in zip((top, second, pv, means), got):
            assert a.tobytes() == b.tobytes()
    return pv, ref


def _shift_rows(rng, n1, n2, shifts, noise=1000.0, base=10**6):
    """rows of n1 + n2 counts (lengths 1): group A = base + shift + noise, group B = base + noise, the noise fixed"""
    na = rng.normal(0, noise, n1)
    nb = rng.normal(0, noise, n2)
    return np.array([np.concatenate([np.round(base + s + na), np.round(base + nb)]) for s in shifts]).astype(np.uint32)


@pytest.mark.parametrize("n1,n2", [(64, 64), (1, 2), (5, 8)])
def test_ttest_p_range(gpu_ctx, n1, n2):
    """p from ~1 down to 0 (through 1e-300 and the denormals when df = 126), and x = df / (df + t^2) on both sides
    of the continued fraction's switch point (a + 1) / (a + b + 2), a = df / 2, b = 1 / 2"""
    df = n1 + n2 - 2
    x_sw = (df / 2 + 1) / (df / 2 + 2.5)
    X0 = _shift_rows(np.random.RandomState(n1), n1, n2, [0.0, 1000.0]).astype(np.float64)
    t0 = hr.ttest_t(X0[0, :n1], X0[0, n1:])[0]
    t_unit = (hr.ttest_t(X0[1, :n1], X0[1, n1:])[0] - t0) / 1000.0       # t is linear in the shift
    s_sw = (math.sqrt(df * (1 - x_sw) / x_sw) - t0) / t_unit
    s_0 = -t0 / t_unit          # t ~ 0, p ~ 1: where forming 1 - x from x = df / (df + t^2) cost the kernel 5e-12
    shifts = list(np.geomspace(1, 4e9, 400)) + list(s_sw + np.arange(-40, 41)) + list(s_0 + np.arange(-5, 6))
    counts = _shift_rows(np.random.RandomState(n1), n1, n2, shifts)
    groups = [list(range(n1)), list(range(n1, n1 + n2))]
    pv, ref = _tt_check(gpu_ctx, counts, np.ones(n1 + n2, np.int64), groups, stage=(n1 == 64))
    assert (ref > 0.99).any() and (ref < 1e-6 if df > 1 else ref < 1e-5).any()
    if df > 100:
        assert ((ref > 1e-305) & (ref < 1e-290)).any()
        assert ((ref > 0) & (ref < 2.2250738585072014e-308)).any() and (ref == 0).any()
    X = counts.astype(np.float64)
    xs = np.array([(lambda t, d: d / (d + t * t))(*hr.ttest_t(X[r, :n1], X[r, n1:])) for r in range(len(X))])
    assert ((xs < x_sw) & (xs > x_sw - 0.01)).any() and ((xs >= x_sw) & (xs < x_sw + 0.01)).any()


def test_ttest_degenerate_groups(gpu_ctx):
    """(1, 1): df = 0 -> NaN; a group of 65 chromosomes raises; 0 / 0 rows -> NaN; t = inf -> 0"""
    counts = np.array([[3, 5], [0, 0], [7, 7]], np.uint32)
    _, _, pv, _ = gpu_ctx.kmer_ttest(counts, np.ones(2, np.int64), [[0], [1]])
    assert np.isnan(pv).all()
    with pytest.raises(ValueError):
        gpu_ctx.kmer_ttest(np.ones((2, 66), np.uint32), np.ones(66, np.int64), [list(range(65)), [65]])
    c = np.zeros((3, 6), np.uint32)
    c[1] = 4
    c[2, :3] = 9
    pv, ref = _tt_check(gpu_ctx, c, np.ones(6, np.int64), [[0, 1, 2], [3, 4, 5]])
    assert np.isnan(pv[0]) and np.isnan(pv[1]) and pv[2] == 0.0


def test_ttest_extreme_counts_and_ties(gpu_ctx):
    """counts of 2^32 - 1 over lengths of 1 and 2^40; exact mean ties (group order decides top / second)"""
    rng = np.random.RandomState(21)
    C = 12
    lengths = np.array([1, 2**40, 1, 2**40, 3, 2**40 - 1, 1, 1, 2**40, 7, 1, 2**40], np.int64)
    counts = rng.randint(0, 2**32, size=(200, C), dtype=np.uint64).astype(np.uint32)
    counts[:20] = 2**32 - 1
    counts[20:40, :6] = 2**32 - 1
    groups = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    _tt_check(gpu_ctx, counts, lengths, groups)
    # ties: groups 1 and 2 hold the same values over equal lengths; group 0 above or below them
    lens = np.full(9, 1000, np.int64)
    c = rng.randint(0, 5000, size=(60, 9)).astype(np.uint32)
    c[:, 6:9] = c[:, 3:6]
    c[:30, :3] = 10000 + c[:30, :3]
    top, second, pv, means = gpu_ctx.kmer_ttest(c, lens, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    assert (means[:, 1] == means[:, 2]).all()
    assert (top[:30] == 0).all() and (second[:30] == 1).all() and (pv[:30] == pv[:30]).all()
    assert ((top[30:] == 1) & (second[30:] == 2)).any()            # the tie on top: group 1 before group 2
    _tt_check(gpu_ctx, c, lens, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])


@pytest.mark.parametrize("Mrows", [0, 1, 127, 128, 129])
def test_ttest_row_counts(gpu_ctx, Mrows):
    rng = np.random.RandomState(Mrows + 5)
    C = 13
    groups = [[0, 3, 4, 9, 12], [1, 2, 5, 6, 7, 8, 10, 11]]
    lengths = rng.randint(10**6, 10**8, size=C).astype(np.int64)
    counts = rng.poisson(30, size=(Mrows, C)).astype(np.uint32)
    counts[: Mrows // 3, groups[0]] += 20
    top, second, pv, means = gpu_ctx.kmer_ttest(counts, lengths, groups)
    assert top.shape == (Mrows,) and pv.shape == (Mrows,) and means.shape == (Mrows, 2)
    if Mrows:
        _tt_check(gpu_ctx, counts, lengths, groups, stage=True)
