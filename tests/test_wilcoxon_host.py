"""The paired k-mer test on the host: subphaser_amd/csrc/sp_wilcoxon.h built with the host C++ compiler
(tests/wilcoxon_host_check.cpp, -ffp-contract=off as the library is built) against the numpy twin (tests/wilcoxon_ref.py),
the twin against the array form the CLI used before (cluster._wilcoxon_rows) and against scipy row by row.

  header vs twin   m, W2, T, the branch and the statistic with ==; p of the permutation branch with ==; p of the exact and
                   the asymptotic branch within hp_reference.tail_ok (relative 1e-10 on [1e-290, 0.5], absolute 1e-13
                   above; in fact the exact branch is a table look-up and only erfc differs); NaN where NaN
  exact tables     every entry == float(exact fraction) for n = 1 .. 50, the fractions from generating-function products
                   over Python integers; total == 2^n
  twin vs host     permutation rows ==, exact and asymptotic rows within tail_ok, NaN where NaN
  twin vs scipy    scipy.stats.wilcoxon row by row on a subset: statistic ==, p as above"""
import struct

import numpy as np
import pytest
from scipy import stats as st

import host_check
import hp_reference as hr
import wilcoxon_cases as wc
import wilcoxon_ref as wr
from subphaser_amd import cluster

M = 60
ALL_CASES = [(n, hi, G, M) for n in wc.SIZES for hi in wc.RANGES for G in (2, 3)]


def _hand_pairs():
    out = []
    for i in range(len(wc.HAND)):
        counts, lengths, groups = wc.hand(i)
        X = counts.astype(np.float64)
        out.append((X[:, groups[0]], X[:, groups[1]]))
    return out


@pytest.fixture(scope="module")
def blocks():
    out = _hand_pairs()
    for args in ALL_CASES:
        out += wc.pairs(*args)
    return out


@pytest.fixture(scope="module")
def host_run(tmp_path_factory, blocks):
    tmp = tmp_path_factory.mktemp("wilcoxon_host")
    blob = [struct.pack("=q", len(blocks))]
    for a, b in blocks:
        x = np.ascontiguousarray(np.concatenate([a, b], axis=1), np.float64)
        blob += [struct.pack("=qq", a.shape[1], len(x)), x.tobytes()]
    src, dst = tmp / "cases.bin", tmp / "out.bin"
    src.write_bytes(b"".join(blob))
    r = host_check.run(tmp, "wilcoxon_host_check", [src, dst], flags=["-ffp-contract=off"], libs=["-lm"])
    assert r.returncode == 0, r.stdout[-2000:]
    return dst.read_bytes()


def _same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def _p_agrees(p, ref, br):
    """== on the permutation rows, NaN where NaN, tail_ok elsewhere; returns the rows that fail"""
    nan = np.isnan(ref)
    perm = br == wr.PERM
    ok = np.where(nan, np.isnan(p), np.where(perm, p == ref, hr.tail_ok(p, np.where(nan, 1.0, ref))))
    return np.flatnonzero(~ok)


def test_header_against_the_twin(host_run, blocks):
    at = 0
    seen = {wr.EXACT: 0, wr.PERM: 0, wr.ASYM: 0}
    n_nan = 0
    for a, b in blocks:
        R, n = a.shape
        rec = np.frombuffer(host_run, np.dtype([("i", "<i8", 4), ("d", "<f8", 2)]), R, at)
        at += R * 48
        stat, p, br, (m, W2, T) = wr.rows(a, b)
        for k, ref in enumerate((m, W2, T, br)):
            assert (rec["i"][:, k] == ref).all(), (n, "m W2 T branch".split()[k])
        assert rec["d"][:, 0].tobytes() == stat.tobytes(), n
        bad = _p_agrees(rec["d"][:, 1], p, br)
        assert bad.size == 0, (n, rec["d"][bad, 1][:4], p[bad][:4], br[bad][:4])
        assert (p[~np.isnan(p)] >= 0).all() and (p[~np.isnan(p)] <= 1).all()
        for k in seen:
            seen[k] += int((br == k).sum())
        n_nan += int(np.isnan(p).sum())
    assert min(seen.values()) > 300 and n_nan >= 3, (seen, n_nan)


def test_exact_tables_against_fractions(host_run, blocks):
    at = sum(len(a) for a, _ in blocks) * 48
    for n in range(1, wr.EXACT_MAX + 1):
        D = n * (n + 1) // 2
        total = struct.unpack_from("<Q", host_run, at)[0]
        tab = np.frombuffer(host_run, "<f8", D + 1, at + 8)
        at += 8 + 8 * (D + 1)
        assert total == 2 ** n == sum(wr.exact_counts(n))
        ref = wr.exact_table_fractions(n)
        assert len(ref) == D + 1 and ref[0] * 2 ** n == 1 and ref[D] * 2 ** n == 1
        assert tab.tolist() == [float(f) for f in ref], n
        assert all(f.denominator <= 2 ** n for f in ref)          # dyadic: float(f) is exact
    assert at == len(host_run)
    c = wr.exact_counts(4)
    assert c == (1, 1, 1, 2, 2, 2, 2, 2, 1, 1, 1) and c == c[::-1]


@pytest.mark.parametrize("n,hi,G,m", ALL_CASES)
def test_twin_against_the_host_path(n, hi, G, m):
    for a, b in wc.pairs(n, hi, G, m):
        stat, p, br, _ = wr.rows(a, b)
        ref = cluster._wilcoxon_rows(a, b)
        bad = _p_agrees(p, ref, br)
        assert bad.size == 0, (p[bad][:4], ref[bad][:4], br[bad][:4])
        if hi == 100000:
            assert (br == (wr.EXACT if n <= wr.EXACT_MAX else wr.ASYM)).all()
        if hi == 3 and n <= wr.PERM_MAX and n > 2:
            assert (br == wr.PERM).any()


@pytest.mark.parametrize("n,hi,G,m", ALL_CASES)
def test_twin_picks_the_groups_of_the_host_path(n, hi, G, m):
    counts, lengths, groups = wc.case(n, hi, G, m)
    top, second, p, means, stat = wc.twin(n, hi, G, m)
    ht, hs, hp, hm = cluster.numpy_kmer_test(counts.astype(np.float64) / lengths.astype(np.float64), groups, "wilcoxon")
    assert (top == ht).all() and (second == hs).all()
    assert len(set(top.tolist())) == G                       # every group is on top somewhere
    nan = np.isnan(hp)
    assert (np.isnan(p) == nan).all() and hr.tail_ok(p[~nan], hp[~nan]).all()


def _scipy_row(a, b):
    r = st.wilcoxon(a, b)
    return r.statistic, r.pvalue


@pytest.mark.parametrize("n", wc.SIZES)
def test_twin_against_scipy_row_by_row(n):
    for hi in wc.RANGES:
        for a, b in wc.pairs(n, hi, 2, M):
            k = 8 if n != wr.PERM_MAX else 2         # scipy's own permutation test takes 0.3 s a row at 13 pairs
            a, b = a[:k], b[:k]
            stat, p, br, _ = wr.rows(a, b)
            ref = np.array([_scipy_row(x, y) for x, y in zip(a, b)])
            assert _same(stat, ref[:, 0]), (n, hi)
            bad = _p_agrees(p, ref[:, 1], br)
            assert bad.size == 0, (n, hi, p[bad][:4], ref[bad, 1][:4], br[bad][:4])


def test_hand_made_rows():
    for (what, _, _, branch, p_ref, stat_ref), (a, b) in zip(wc.HAND, _hand_pairs()):
        stat, p, br, (m, W2, T) = wr.rows(a, b)
        assert (br == branch).all(), what
        assert p[0] == p[1] == p[2] or np.isnan(p).all(), what      # roles swapped, pairs reversed: the same test
        assert stat[0] == stat[1] == stat[2], what
        if p_ref is not None:
            assert _same(p, np.full(3, p_ref)), (what, p)
        if stat_ref is not None:
            assert (stat == stat_ref).all(), (what, stat)
        ref = cluster._wilcoxon_rows(a, b)
        assert _p_agrees(p, ref, br).size == 0, (what, p, ref)
        sp = np.array([_scipy_row(x, y) for x, y in zip(a, b)])
        assert _same(stat, sp[:, 0]) and _p_agrees(p, sp[:, 1], br).size == 0, (what, p, sp)
    what = [h[0] for h in wc.HAND]
    # every |d| equal at n = 13: all 13 ranks are 7, W2 = 8 x 14; the tie group {2, -2, 2}: T = 3 x (9 - 1)
    a, b = _hand_pairs()[what.index("n = 13, every |d| equal and nonzero")]
    assert [int(v[0]) for v in wr.rows(a, b)[3]] == [13, 112, 13 * 168]
    a, b = _hand_pairs()[what.index("a tie group that straddles the sign")]
    assert [int(v[0]) for v in wr.rows(a, b)[3]] == [7, 2 * (3 + 3 + 1 + 6 + 7), 24]


def test_one_group_has_no_test():
    counts = np.arange(12, dtype=np.uint32).reshape(3, 4)
    top, second, p, means, stat = wr.kmer_wilcoxon(counts, np.full(4, 7), [[2, 0, 1]])
    assert (top == 0).all() and (second == 0).all() and (p == 1.0).all() and np.isnan(stat).all()
    assert means.shape == (3, 1)
