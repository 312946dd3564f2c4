"""High-precision reference for the statistics kernels (Fisher right tail + enrichment call, pooled t-test).

Restated from the definitions, independent of subphaser_amd/ and oracle/:
  * fisher_cells  -- the 2 x 2 margins Stats.fisher_test forms (Stats.py:17-25), x22 quirk and both clamps;
  * right_tail    -- P[X >= a] of the hypergeometric law, to far more digits than fp64 holds;
  * enrich_rows   -- Stats._enrich + Pvalues.get_enriched (Stats.py:140-192) on the fp64 roundings of right_tail;
  * ttest_p       -- scipy.stats.ttest_ind's pooled two-sided p-value, the incomplete beta taken in mpmath.

Tolerances the GPU tests hold the kernels to are stated here once (TAIL_RTOL & co.), so the `fragile` mask of
enrich_rows and the assertions of the tests use the same intervals.
"""
import math

import mpmath as mp
import numpy as np

MAX_INT = 2147483647 // 10          # Stats.py:9
DPS = 50                            # mpmath working precision (decimal digits)

# a kernel p-value may lie this far from the reference's: relative in [TINY, 0.5], absolute above 0.5,
# absolute TINY_ATOL below TINY (fp64 loses relative precision in the denormal range)
TAIL_RTOL = 1e-10
HIGH_ATOL = 1e-13
TINY = 1e-290
TINY_ATOL = 1e-300

_FIX = 256                          # fixed-point scale of the tail sums: terms are integers of ~2^256
_STOP = 10 ** 40                    # stop once the geometric bound of the rest is below 1e-40 of the sum


def fisher_cells(each, total, j):
    """(x11, x12, x21, x22) of column j, in Python ints: the x22 quirk uses the UNclamped x21, then both clamp."""
    each = [int(v) for v in each]
    total = [int(v) for v in total]
    sum_each, sum_total = sum(each), sum(total)
    x11 = each[j]
    x12 = sum_each - x11
    x21 = total[j] - x11
    x22 = sum_total - x21 - x12
    return x11, x12, min(x21, MAX_INT), min(x22, MAX_INT)


def _lchoose(n, k):
    return mp.loggamma(n + 1) - mp.loggamma(k + 1) - mp.loggamma(n - k + 1)


def tail_bounds(a, b, c, d):
    """(lo, hi, mode) of the law right_tail sums: support [lo, hi], mode floor((n+1)(K+1)/(N+2))."""
    N, K, n = a + b + c + d, a + b, a + c
    return max(0, n - (c + d)), min(K, n), ((n + 1) * (K + 1)) // (N + 2)


def right_tail(a, b, c, d):
    """P[X >= a], X ~ Hypergeom(N = a+b+c+d, K = a+b, n = a+c), as an mpf.

    The sum starts on the side of `a` away from the mode (where the terms fall off) and runs by the exact rational
    term ratio in fixed-point integers of ~2^256; the first term comes from mpmath's loggamma.  It stops when the
    geometric bound of what is left (the ratios only shrink away from the mode) is below 1e-40 of the sum.  When
    a <= mode the left side P[X <= a-1] is summed and 1 - s returned."""
    a, b, c, d = int(a), int(b), int(c), int(d)
    N, K, n = a + b + c + d, a + b, a + c
    lo, hi, mode = tail_bounds(a, b, c, d)
    if a <= lo:
        return mp.mpf(1)
    if a > hi:
        return mp.mpf(0)
    NK = N - K
    with mp.workdps(DPS):
        if a > mode:
            x, end = a, hi
        else:
            x, end = a - 1, lo
        first = mp.exp(_lchoose(K, x) + _lchoose(NK, n - x) - _lchoose(N, n))
        term = 1 << _FIX
        s = term
        while x != end:
            if a > mode:        # t(x+1) / t(x)
                num, den = (K - x) * (n - x), (x + 1) * (NK - n + x + 1)
                x += 1
            else:               # t(x-1) / t(x)
                num, den = x * (NK - n + x), (K - x + 1) * (n - x + 1)
                x -= 1
            term = term * num // den
            if term == 0:
                break
            s += term
            # rest <= term * r / (1 - r), r = num / den the largest ratio still to come
            if den > num and term * num * _STOP < s * (den - num):
                break
        tail = first * mp.mpf(s) / mp.mpf(1 << _FIX)
        return tail if a > mode else 1 - tail


def to_f64(x):
    """Round an mpf to the nearest double (denormals and underflow to 0 included)."""
    if x == 0:
        return 0.0
    return float(mp.nstr(x, 30, strip_zeros=False, min_fixed=1, max_fixed=0))


def tail_interval(p, exact=False, rtol=TAIL_RTOL, atol=HIGH_ATOL):
    """[lo, hi] a kernel p-value may take around the reference `p` (fp64) under the tests' tolerances; an exact
    cell (a <= lo -> 1, a > hi -> 0) admits nothing else."""
    if exact:
        return p, p
    if p > 0.5:
        return p - atol, p + atol
    if p >= TINY:
        return p * (1 - rtol), p * (1 + rtol)
    return max(0.0, p - TINY_ATOL), p + TINY_ATOL


def tail_ok(got, ref):
    """got (fp64 kernel values) within the tests' tolerances of ref (fp64 roundings of the mpf reference)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    hi = ref > 0.5
    mid = (ref >= TINY) & ~hi
    ok = np.empty(ref.shape, bool)
    ok[hi] = np.abs(got[hi] - ref[hi]) <= HIGH_ATOL
    ok[mid] = np.abs(got[mid] - ref[mid]) <= TAIL_RTOL * ref[mid]
    low = ~(hi | mid)
    ok[low] = np.abs(got[low] - ref[low]) <= TINY_ATOL
    return ok & np.isfinite(got)


def rel_err(got, ref):
    """max relative error of got against ref over cells with ref in [TINY, 0.5] (0 if there are none)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = (ref >= TINY) & (ref <= 0.5)
    return float((np.abs(got[m] - ref[m]) / ref[m]).max()) if m.any() else 0.0


class Enriched:
    pass


def _decide(p, max_pval):
    """Pvalues.get_enriched on fp64 p-values: stable sort, min / sub-min, the two sig tests."""
    order = sorted(range(len(p)), key=lambda j: p[j])
    m, s2 = order[0], order[1]
    sig = True
    if p[m] > max_pval:
        sig = False
    if p[m] == 0:
        pass
    elif p[s2] / p[m] < max_pval / p[s2] * 1:
        sig = False
    return m, s2, sig


def _row_fragile(p, exact, cells, m, s2, max_pval, ratio_ok, rtol=TAIL_RTOL, atol=HIGH_ATOL):
    """Could a kernel p-value vector within tail_interval of p decide this row differently?"""
    iv = [tail_interval(p[j], exact[j], rtol, atol) for j in range(len(p))]
    lo_m, hi_m = iv[m]
    for j in range(len(p)):
        if j == m or cells[j] == cells[m]:       # identical cells give identical kernel values: a true tie
            continue
        if exact[j] and exact[m]:                # both exactly 0 or 1 in the kernel too
            continue
        if iv[j][0] <= hi_m:                     # min against sub-min (and every other candidate)
            return True
    if not ratio_ok:                             # the ratio alone says no, whatever the p-values
        return False
    above = {hi_m > max_pval, lo_m > max_pval}   # p_min against max_pval
    lo_s, hi_s = iv[s2]
    cut = set()                                  # p_sub^2 against max_pval * p_min, or the p_min == 0 branch
    if lo_m == 0:
        cut.add(False)
    if hi_m > 0:
        if lo_s * lo_s < max_pval * hi_m:
            cut.add(True)
        if hi_s * hi_s >= max_pval * lo_m:
            cut.add(False)
    return len({not (x or y) for x in above for y in cut}) > 1


def decide_row(row, total, p, cells, max_pval=0.05, min_ratio=0.5, rtol=TAIL_RTOL, atol=HIGH_ATOL):
    """_enrich + Pvalues.get_enriched for one row on given fp64 p-values: (argmin, sig, ratios, fragile).  `fragile`
    uses tail_interval(rtol, atol) around p; cells are the row's fisher_cells."""
    p = [float(v) for v in p]
    m, s2, sig = _decide(p, max_pval)
    with np.errstate(all="ignore"):
        ratios = np.array(row) / np.array(total)         # numpy, exactly as _enrich forms them
        ratios = ratios / ratios.sum()
    ratio_ok = not ratios[m] < min_ratio
    exact = []
    for c in cells:
        lo, hi, _ = tail_bounds(*c)
        exact.append(c[0] <= lo or c[0] > hi)
    fragile = _row_fragile(p, exact, cells, m, s2, max_pval, ratio_ok, rtol, atol)
    return m, sig and ratio_ok, ratios, fragile


def enrich_rows(table, max_pval=0.05, min_ratio=0.5, rows=None):
    """Stats.enrich / _enrich / Pvalues.get_enriched on the reference p-values, for `rows` of the table (all by
    default; the column totals are always the whole table's).

    Returns an object with .p_mp (lists of mpf), .p (their fp64 roundings), .argmin, .sig, .ratios, .cells and
    .fragile: the rows whose decision a kernel within the tests' tolerances could turn."""
    t = np.asarray(table, np.int64)
    S = t.shape[1]
    rows = range(t.shape[0]) if rows is None else list(rows)
    W = len(rows)
    total = list(t.sum(axis=0))                  # numpy int64 column sums, as Stats.enrich takes them
    out = Enriched()
    out.p_mp, out.cells, out.p = [], [], np.zeros((W, S), np.float64)
    out.argmin, out.sig = np.zeros(W, np.int32), np.zeros(W, bool)
    out.ratios, out.fragile = np.zeros((W, S), np.float64), np.zeros(W, bool)
    for i, w in enumerate(rows):
        row = [int(v) for v in t[w]]
        cells = [fisher_cells(row, total, j) for j in range(S)]
        pm = [right_tail(*c) for c in cells]
        p = [to_f64(v) for v in pm]
        out.p_mp.append(pm)
        out.cells.append(cells)
        out.p[i] = p
        out.argmin[i], out.sig[i], out.ratios[i], out.fragile[i] = decide_row(row, total, p, cells, max_pval, min_ratio)
    return out


def ttest_t(xa, xb):
    """scipy.stats.ttest_ind's pooled statistic, formed in fp64 (a group of one adds no variance)."""
    xa, xb = np.asarray(xa, np.float64), np.asarray(xb, np.float64)
    n1, n2 = xa.size, xb.size
    m1, m2 = xa.mean(), xb.mean()
    with np.errstate(all="ignore"):
        v1 = np.var(xa, ddof=1) if n1 > 1 else 0.0
        v2 = np.var(xb, ddof=1) if n2 > 1 else 0.0
        df = float(n1 + n2) - 2.0
        if not df > 0:
            return np.float64("nan"), df
        svar = ((n1 - 1) * v1 + (n2 - 1) * v2) / df
        denom = np.sqrt(svar * (1.0 / n1 + 1.0 / n2))
        return np.float64(m1 - m2) / denom, df


def ttest_p_mp(xa, xb):
    """Two-sided p-value as an mpf: I_x(df/2, 1/2), x = df / (df + t^2) with the fp64 t; NaN for 0/0 and df = 0,
    0 for |t| = inf."""
    t, df = ttest_t(xa, xb)
    if not df > 0 or math.isnan(t):
        return mp.mpf("nan")
    if math.isinf(t):
        return mp.mpf(0)
    with mp.workdps(DPS):
        tt = mp.mpf(float(t)) ** 2
        x = df / (df + tt)
        return mp.betainc(df / 2, mp.mpf(1) / 2, 0, x, regularized=True)


def ttest_p(xa, xb):
    """ttest_p_mp rounded to fp64."""
    v = ttest_p_mp(xa, xb)
    return float("nan") if mp.isnan(v) else to_f64(v)


def wheat_table(seed=2024, W=14074, S=3):
    """A seeded synthetic window table at the scale of the wheat run: W x S int64, column totals of 4e8-8e8, so
    x21 and x22 (Stats.py:24-25) are clamped on nearly every cell.

    Three ballast rows at the end carry what the totals need beyond the other rows.  Every other row has a sum R
    (log-uniform in [20, 2e5]) and puts x11 of one cell at mode + z * sd of that cell's own law: three rows in four
    take z in [-8, 8] and a second cell near its mode too (p-values between 1e-15 and 1 - 1e-15), the fourth takes
    z in [8, 60] (p-values over every decade from 1e-15 down to underflow).  The totals follow the wheat run's scale;
    the row sums are not calibrated against a `bench.py --dump-outputs` table, whose p-values are almost all 0 or 1."""
    rng = np.random.RandomState(seed)
    T = np.sort(rng.uniform(4e8, 8e8, size=S)).astype(np.int64)
    M = MAX_INT
    t = np.zeros((W, S), np.int64)

    def place(R, z):
        a = R / 2.0
        for _ in range(4):                      # both clamps: K = R, n = a + MAX_INT, N = R + 2 MAX_INT
            K, n, N = R, a + M, R + 2.0 * M
            mode = (n + 1) * (K + 1) / (N + 2)
            sd = math.sqrt(n * K / N * (N - K) / N * (N - n) / (N - 1))
            a = mode + z * sd
        return int(min(max(round(a), 0), R))

    for w in range(W - 3):
        R = int(round(math.exp(rng.uniform(math.log(20), math.log(2e5)))))
        j, k, l = rng.permutation(S)[:3] if S >= 3 else (0, 1, 1)
        if rng.random_sample() < 0.75:
            t[w, j] = place(R, rng.uniform(-8, 8))
            left = R - t[w, j]
            t[w, k] = min(left, place(R, rng.uniform(-8, 8)))
            t[w, l] += left - t[w, k]
        else:
            t[w, j] = place(R, rng.uniform(8, 60))
            rest = R - t[w, j]
            t[w, k] = rng.randint(0, rest + 1)
            t[w, l] += rest - t[w, k]
    B = T - t.sum(axis=0)
    t[W - 3] = B // 2
    t[W - 2] = B // 3
    t[W - 1] = B - B // 2 - B // 3
    return t
