"""The rank-sum k-mer tests on the host: subphaser_amd/csrc/sp_ranktest.h built with the host C++ compiler
(tests/ranktest_host_check.cpp, -ffp-contract=off as the library is built) against the numpy twin (tests/ranktest_ref.py),
and the twin against scipy row by row.

  header vs twin   S1, S2, T and both statistics with ==, NaN where NaN; p within hp_reference.tail_ok (relative 1e-10 on
                   [1e-290, 0.5], absolute 1e-13 above): erfc is the C library's on one side and scipy's on the other
  sf tables        every entry == float(exact fraction) for all n1 <= 8, n2 <= 64, the fractions from the textbook
                   recurrence over Python integers; total == C(n1 + n2, n1)
  np_sum           == np.sum for every length 1 .. 128
  twin vs scipy    stat == scipy.stats.kruskal / mannwhitneyu (...).statistic, p within tail_ok of cluster._scipy_rows,
                   for the sizes of ranktest_cases.SIZES with and without ties, and the hand-made rows"""
import math
import struct

import numpy as np
import pytest
from scipy import stats as st

import host_check
import hp_reference as hr
import ranktest_cases as rc
import ranktest_ref as rr
from subphaser_amd import cluster

M = 40


def _pooled(kind_args):
    """[(n1, n2, a [R, n1], b [R, n2])]: the rows of a case split by the (top, second) pair the twin chose"""
    counts, lengths, groups = rc.size_case(*kind_args)
    top, second = rc.twin("size", *kind_args)["kruskal"][:2]
    X = counts.astype(np.float64) / lengths.astype(np.float64)
    out = []
    for ga, gb in ((0, 1), (1, 0)):
        sel = np.flatnonzero((top == ga) & (second == gb))
        if sel.size:
            out.append((len(groups[ga]), len(groups[gb]), X[np.ix_(sel, groups[ga])], X[np.ix_(sel, groups[gb])]))
    return out


def _hand():
    counts, lengths, groups, what = rc.hand_rows()
    X = counts.astype(np.float64)
    return [(3, 4, X[:, groups[0]], X[:, groups[1]]), (4, 3, X[:, groups[1]], X[:, groups[0]])]


ALL_CASES = [(n1, n2, ties, M) for n1, n2 in rc.SIZES for ties in (True, False)]


@pytest.fixture(scope="module")
def blocks():
    out = list(_hand())
    for args in ALL_CASES:
        out += _pooled(args)
    return out


@pytest.fixture(scope="module")
def host_run(tmp_path_factory, blocks):
    tmp = tmp_path_factory.mktemp("ranktest_host")
    rng = np.random.RandomState(128)
    blob = [struct.pack("=q", len(blocks))]
    for n1, n2, a, b in blocks:
        x = np.ascontiguousarray(np.concatenate([a, b], axis=1), np.float64)
        blob += [struct.pack("=qqq", n1, n2, len(x)), x.tobytes()]
    vecs = [np.ascontiguousarray(10.0 ** rng.uniform(-9, 3, size=n)) for n in range(1, 129)]
    blob.append(struct.pack("=q", len(vecs)))
    for v in vecs:
        blob += [struct.pack("=q", len(v)), v.tobytes()]
    src, dst = tmp / "cases.bin", tmp / "out.bin"
    src.write_bytes(b"".join(blob))
    r = host_check.run(tmp, "ranktest_host_check", [src, dst], flags=["-ffp-contract=off"], libs=["-lm"])
    assert r.returncode == 0, r.stdout[-2000:]
    return dst.read_bytes(), vecs


def _same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def test_header_against_the_twin(host_run, blocks):
    raw, _ = host_run
    at = 0
    n_exact = n_asym = 0
    for n1, n2, a, b in blocks:
        R = len(a)
        rec = np.frombuffer(raw, np.dtype([("i", "<i8", 3), ("d", "<f8", 4)]), R, at)
        at += R * 56
        S1, S2, T = rr.rank_ints(np.concatenate([a, b], axis=1), n1)
        assert (rec["i"][:, 0] == S1).all() and (rec["i"][:, 1] == S2).all() and (rec["i"][:, 2] == T).all(), (n1, n2)
        assert (S1 + S2 == (n1 + n2) * (n1 + n2 + 1)).all()          # doubled ranks 1 .. N
        for m, cols in (("kruskal", (0, 1)), ("mannwhitneyu", (2, 3))):
            stat, p = rr.rows(a, b, m)
            assert _same(rec["d"][:, cols[0]], stat), (m, n1, n2)
            ok = hr.tail_ok(rec["d"][:, cols[1]], p)
            assert ok.all(), (m, n1, n2, rec["d"][~ok, cols[1]][:4], p[~ok][:4])
        exact = (T == 0) & (min(n1, n2) <= rr.EXACT_MAX)
        n_exact += int(exact.sum())
        n_asym += int((~exact).sum())
    assert n_exact > 100 and n_asym > 100


def test_np_sum_is_numpys(host_run, blocks):
    raw, vecs = host_run
    at = sum(len(a) for _, _, a, _ in blocks) * 56
    got = np.frombuffer(raw, "<f8", len(vecs), at)
    assert got.tobytes() == np.array([np.sum(v) for v in vecs]).tobytes()


def test_exact_tables_against_fractions(host_run, blocks):
    raw, vecs = host_run
    at = sum(len(a) for _, _, a, _ in blocks) * 56 + len(vecs) * 8
    for n1 in range(1, rr.EXACT_MAX + 1):
        for n2 in range(1, rr.MAXG + 1):
            total = struct.unpack_from("<Q", raw, at)[0]
            sf = np.frombuffer(raw, "<f8", n1 * n2 + 1, at + 8)
            at += 8 + 8 * (n1 * n2 + 1)
            assert total == math.comb(n1 + n2, n1) == sum(rr.exact_counts(n1, n2))
            ref = rr.exact_sf_fractions(n1, n2)
            assert len(ref) == n1 * n2 + 1 and ref[0] == 1
            assert sf.tolist() == [float(f) for f in ref], (n1, n2)
    assert at == len(raw)
    # the null is symmetric in the two sizes and around n1 n2 / 2
    c = rr.exact_counts(3, 5)
    assert c == rr.exact_counts(5, 3) and c == c[::-1] and c[:4] == (1, 1, 2, 3)


def _scipy_stat(name, a, b):
    out = np.empty(len(a))
    for i in range(len(a)):
        try:
            out[i] = getattr(st, name)(a[i], b[i])[0]
        except ValueError as e:          # kruskal: "All numbers are identical"
            assert "identical" in str(e)
            out[i] = np.nan
    return out


@pytest.mark.parametrize("n1,n2,ties,m", ALL_CASES)
def test_twin_against_scipy(n1, n2, ties, m):
    for ga, gb, a, b in _pooled((n1, n2, ties, m)):
        T = rr.rank_ints(np.concatenate([a, b], axis=1), ga)[2]
        assert ties or (T == 0).all()
        for method in rr.METHODS:
            stat, p = rr.rows(a, b, method)
            ref = _scipy_stat(method, a, b)
            if method == "kruskal":
                assert (np.isnan(ref) == (T == (ga + gb) ** 3 - (ga + gb))).all()
            assert _same(stat, ref), (method, stat[stat != ref][:4], ref[stat != ref][:4])
            pref = cluster._scipy_rows(method, a, b)
            ok = hr.tail_ok(p, pref)
            assert ok.all(), (method, p[~ok][:4], pref[~ok][:4])


def test_twin_against_scipy_on_hand_made_rows():
    what = rc.hand_rows()[3]
    for n1, n2, a, b in _hand():
        T = rr.rank_ints(np.concatenate([a, b], axis=1), n1)[2]
        assert T.tolist() == [7 * 48, 0, 0, 6, 6, 24, 12, 6 * 35]
        for method in rr.METHODS:
            stat, p = rr.rows(a, b, method)
            assert _same(stat, _scipy_stat(method, a, b)), method
            ok = hr.tail_ok(p, cluster._scipy_rows(method, a, b))
            assert ok.all(), (method, [w for w, o in zip(what, ok) if not o])
        # all identical: p = 1 under both, no H; separated 3 | 4: the exact two-sided tail 2 / C(7, 3)
        sk, pk = rr.rows(a, b, "kruskal")
        su, pu = rr.rows(a, b, "mannwhitneyu")
        assert np.isnan(sk[0]) and pk[0] == 1.0 and pu[0] == 1.0 and su[0] == 6.0
        assert pu[1] == pu[2] == 2.0 / 35.0 and su[1] == (12.0 if n1 == 3 else 0.0)


def test_one_group_has_no_test():
    counts = np.arange(12, dtype=np.uint32).reshape(3, 4)
    for m in rr.METHODS:
        top, second, p, means, stat = rr.kmer_ranktest(counts, np.full(4, 7), [[2, 0, 1]], m)
        assert (top == 0).all() and (second == 0).all() and (p == 1.0).all() and np.isnan(stat).all()
        assert means.shape == (3, 1)
