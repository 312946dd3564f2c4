"""GPU: the k-mer t-test for subgenomes of more than 64 chromosomes (sp_enrich.hip: k7_ttest_wide_means / k7_ttest_wide_test,
Context.kmer_ttest_wide) against a reference written here from the reference's own lines (Cluster.py:181-183) and
tests/hp_reference.py:

  means[r][g]   np.sum(X[r, g]) / n            -- np.mean of the group's list, numpy's pairwise sum: bit-equal
  key[r][g]     sum(list(X[r, g])) / n         -- Python's left-to-right sum; top / second = sorted by (-key, g): equal
  p[r]          hr.ttest_p(top group, second group) in mpmath: NaN exactly where it is NaN, hr.tail_ok elsewhere
                (relative 1e-10 on [1e-290, 0.5], absolute 1e-13 above, 1e-300 below)."""
import math

import numpy as np
import pytest

import hp_reference as hr

pytestmark = pytest.mark.gpu


def _reference(counts, lengths, groups):
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    M, G = len(counts), len(groups)
    means, top, second, p = np.empty((M, G)), np.empty(M, np.int32), np.empty(M, np.int32), np.empty(M)
    for r in range(M):
        xs = [X[r, g] for g in groups]                                  # fancy index: contiguous, in list order
        means[r] = [np.sum(x) / len(x) for x in xs]
        key = [sum(list(x)) / len(x) for x in xs]
        order = sorted(range(G), key=lambda g: (-key[g], g))
        top[r], second[r] = order[0], order[1 if G > 1 else 0]
        p[r] = hr.ttest_p(xs[top[r]], xs[second[r]])
    return top, second, p, means


def _check(gpu_ctx, counts, lengths, groups, stage=False):
    top, second, pv, means = gpu_ctx.kmer_ttest_wide(counts, lengths, groups)
    M = len(counts)
    assert top.shape == (M,) and second.shape == (M,) and pv.shape == (M,) and means.shape == (M, len(groups))
    rt, rs, rp, rm = _reference(counts, lengths, groups)
    assert means.tobytes() == rm.tobytes(), np.argwhere(means != rm)[:5]
    assert (top == rt).all() and (second == rs).all(), np.nonzero((top != rt) | (second != rs))[0][:5]
    nan = np.isnan(rp)
    assert (np.isnan(pv) == nan).all(), np.nonzero(np.isnan(pv) != nan)[0][:5]
    ok = hr.tail_ok(pv[~nan], rp[~nan])
    assert ok.all(), [(r, pv[~nan][r], rp[~nan][r]) for r in np.nonzero(~ok)[0][:5]]
    if stage:
        staged = gpu_ctx.stage_rows(counts)
        try:
            got = gpu_ctx.kmer_ttest_wide(staged, lengths, groups)
        finally:
            gpu_ctx.release_rows()
        for a, b in zip((top, second, pv, means), got):
            assert a.tobytes() == b.tobytes()
    return pv, rp, top, second, means


def _poisson_case(seed, M, sizes, C=None, lift=0):
    """Poisson counts, a third of the rows lifted in one group, lengths in 1e6..1e8; groups = consecutive runs"""
    rng = np.random.RandomState(seed)
    C = C or sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    groups = [list(range(off[i], off[i + 1])) for i in range(len(sizes))]
    lengths = rng.randint(10**6, 10**8, size=C).astype(np.int64)
    counts = rng.poisson(30, size=(M, C)).astype(np.uint32)
    counts[: M // 3, groups[lift][0]:groups[lift][-1] + 1] += 20
    return counts, lengths, groups


@pytest.mark.parametrize("n1,n2", [(65, 1), (65, 65), (127, 7), (128, 8), (129, 257), (136, 264), (255, 256), (1000, 1025),
                                   (8192, 3)])
def test_wide_group_sizes(gpu_ctx, n1, n2):
    """leaf of up to 128 values, its 8-wide blocks and tail, the first splits, several levels of the tree; chunks of the
    column list that end inside a block"""
    counts, lengths, groups = _poisson_case(n1 * 3 + n2, 130, (n1, n2))
    pv, rp, _, _, _ = _check(gpu_ctx, counts, lengths, groups)
    assert np.isfinite(rp).all()


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 257])
def test_wide_tile_edges(gpu_ctx, M):
    counts, lengths, groups = _poisson_case(M + 11, M, (129, 257))
    top, second, pv, means = gpu_ctx.kmer_ttest_wide(counts, lengths, groups)
    assert top.shape == (M,) and second.shape == (M,) and pv.shape == (M,) and means.shape == (M, 2)
    assert top.dtype == np.int32 and pv.dtype == np.float64
    if M:
        _check(gpu_ctx, counts, lengths, groups)


@pytest.mark.parametrize("G", [3, 5])
def test_wide_layout(gpu_ctx, G):
    """interleaved groups (chromosome i in group i % G), one list shuffled (the list order is the summation order),
    40 chromosomes in no group"""
    rng = np.random.RandomState(G)
    C, M = 700, 130
    lengths = rng.randint(10**6, 10**8, size=C).astype(np.int64)
    counts = rng.poisson(30, size=(M, C)).astype(np.uint32)
    free = set(rng.choice(C, 40, replace=False).tolist())
    used = [i for i in range(C) if i not in free]
    groups = [[c for i, c in enumerate(used) if i % G == g] for g in range(G)]
    rng.shuffle(groups[1])
    for r in range(M):
        counts[r, groups[r % G]] *= 3        # every group is top somewhere
    counts[:, sorted(free)] = 2**31          # would show in every mean if it were read
    _, _, top, _, _ = _check(gpu_ctx, counts, lengths, groups)
    assert len(set(top.tolist())) == G


def test_wide_staged_rows(gpu_ctx):
    counts, lengths, groups = _poisson_case(5, 200, (150, 90, 70), lift=1)
    _check(gpu_ctx, counts, lengths, groups, stage=True)


def test_wide_extreme_counts_and_lengths(gpu_ctx):
    """counts of 2^32 - 1 over lengths of 1 and 2^40 mixed, groups of 200"""
    rng = np.random.RandomState(21)
    n, C = 200, 600
    pattern = np.array([1, 2**40, 1, 2**40, 3, 2**40 - 1, 1, 1, 2**40, 7, 1, 2**40], np.int64)
    lengths = np.tile(pattern, C // len(pattern))
    counts = rng.randint(0, 2**32, size=(130, C), dtype=np.uint64).astype(np.uint32)
    counts[:20] = 2**32 - 1
    counts[20:40, :C // 2] = 2**32 - 1
    groups = [list(range(g * n, (g + 1) * n)) for g in range(3)]
    _check(gpu_ctx, counts, lengths, groups)


def test_wide_ties_zero_rows_and_constant_groups(gpu_ctx):
    """two groups with identical columns (the earlier one wins top or second); all-zero rows -> NaN; a constant group
    against a shifted constant group -> p = 0"""
    rng = np.random.RandomState(22)
    n = 200
    lens = np.full(3 * n, 1024, np.int64)
    c = rng.randint(0, 5000, size=(60, 3 * n)).astype(np.uint32)
    c[:, 2 * n:] = c[:, n:2 * n]
    c[:30, :n] += 10000
    c[30:, :n] //= 4
    c[56:58] = 0
    c[58:, :n], c[58:, n:] = 8192, 4096
    groups = [list(range(g * n, (g + 1) * n)) for g in range(3)]
    pv, rp, top, second, means = _check(gpu_ctx, c, lens, groups)
    assert (means[:, 1] == means[:, 2]).all()
    assert (top[:30] == 0).all() and (second[:30] == 1).all()
    assert (top[30:56] == 1).all() and (second[30:56] == 2).all()       # the tie on top: group 1 before group 2
    assert np.isnan(pv[56:58]).all()
    assert (pv[58:] == 0.0).all() and (top[58:] == 0).all() and (second[58:] == 1).all()


def _shift_rows(rng, n1, n2, shifts, noise=1000.0, base=10**6):
    """rows of n1 + n2 counts (lengths 1): group A = base + shift + noise, group B = base + noise, the noise fixed"""
    na = rng.normal(0, noise, n1)
    nb = rng.normal(0, noise, n2)
    return np.array([np.concatenate([np.round(base + s + na), np.round(base + nb)]) for s in shifts]).astype(np.uint32)


def test_wide_p_range_at_df_16382(gpu_ctx):
    """p from 1 down to 0 at df = 16382, through 1e-300 and the denormals, and x = df / (df + t^2) on both sides of the
    continued fraction's switch point: the range where exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a log(x) + b log(y))
    with a = 8191 keeps only 1e-11 and the prefactor of sp_tt_pvalue is needed"""
    n1 = n2 = 8192
    df = n1 + n2 - 2
    x_sw = (df / 2 + 1) / (df / 2 + 2.5)
    X0 = _shift_rows(np.random.RandomState(n1), n1, n2, [0.0, 1000.0]).astype(np.float64)
    t0 = hr.ttest_t(X0[0, :n1], X0[0, n1:])[0]
    t_unit = (hr.ttest_t(X0[1, :n1], X0[1, n1:])[0] - t0) / 1000.0       # t is linear in the shift
    s_sw = (math.sqrt(df * (1 - x_sw) / x_sw) - t0) / t_unit
    s_0 = -t0 / t_unit
    shifts = (list(np.geomspace(1, 4e9, 400)) + list(s_sw + np.arange(-40, 41)) + list(s_0 + np.arange(-5, 6))
              + list(s_0 + np.linspace(0.0, 42.0, 281) / t_unit))
    counts = _shift_rows(np.random.RandomState(n1), n1, n2, shifts)
    groups = [list(range(n1)), list(range(n1, n1 + n2))]
    pv, ref, _, _, _ = _check(gpu_ctx, counts, np.ones(n1 + n2, np.int64), groups)
    assert (ref > 0.99).any() and (ref < 1e-6).any()
    assert ((ref > 1e-305) & (ref < 1e-290)).any()
    assert ((ref > 0) & (ref < 2.2250738585072014e-308)).any() and (ref == 0).any()
    X = counts.astype(np.float64)
    ts = np.array([hr.ttest_t(X[r, :n1], X[r, n1:])[0] for r in range(len(X))])
    xs = df / (df + ts * ts)
    assert ((xs < x_sw) & (xs > x_sw - 0.01)).any() and ((xs >= x_sw) & (xs < x_sw + 0.01)).any()
    lin = np.abs(ts[-281:])
    assert lin.min() < 0.2 and lin.max() > 41.5 and np.diff(np.sort(lin)).max() < 0.3


def test_wide_group_cap(gpu_ctx):
    """65536 chromosomes per group are taken, 65537 are not"""
    n = 65537
    with pytest.raises(ValueError, match="65537"):
        gpu_ctx.kmer_ttest_wide(np.ones((2, n + 1), np.uint32), np.ones(n + 1, np.int64), [list(range(n)), [n]])
