"""The clustering arithmetic of subphaser_amd/csrc/sp_hclust.h, checked on the host.

tests/hclust_host_check.cpp is compiled against the header with the host C++ compiler (-ffp-contract=off, as the library
is built) and compared with the numpy twin (tests/hclust_ref.py) with `==`: the distance matrix and the merges of the
nearest-neighbour chain.  The cases are P = 2, 3, 64, 65, 257 points in D = 1, 21, 130 dimensions, once with random fp64
coordinates and once with small-integer coordinates and duplicated points (ties in distance, chains that stop on the tie
rule, zero heights), and one case whose points are all equal.

The twin is held against scipy: heatmap.to_linkage(twin merges) `==` linkage(squareform(twin dist), "complete") and
heatmap.leaves `==` leaves_list on every case -- scipy's nn_chain follows the same procedure before it sorts and relabels,
so on the SAME distances nothing is left to rounding.  The twin's distances against pdist: both sum the same D
non-negative terms and can differ only by contraction or vector order in scipy's build; each of the D - 1 additions, the
D squares and the root contributes at most one rounding of relative size 2^-53 to the root of the sum on either side, so
the relative difference is below (D + 2) 2^-52 (derived, not measured)."""
import os
import struct

import numpy as np
import pytest

import hclust_ref as hc
import host_check
from subphaser_amd import heatmap as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, P, D, kind)
CASES = [("%s-%dx%d" % (kind, P, D), P, D, kind)
         for kind in ("random", "tied") for P in (2, 3, 64, 65, 257) for D in (1, 21, 130)] + [("equal-70x5", 70, 5, "equal")]
_cache = {}


def case(name):
    """(points, twin merges, twin dist) -- computed once, shared, never changed"""
    if name not in _cache:
        _, P, D, kind = next(c for c in CASES if c[0] == name)
        seed = 100 * P + D
        if kind == "random":
            pts = hc.random_points(seed, P, D)
        elif kind == "tied":
            pts = hc.tied_points(seed, P, D)
        else:
            pts = np.full((P, D), 1.25)
        m, d = hc.hclust(pts)
        for a in (pts, m, d):
            a.setflags(write=False)
        _cache[name] = (pts, m, d)
    return _cache[name]


NAMES = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hclust_host")
    blob = [struct.pack("=q", len(NAMES))]
    for name in NAMES:
        pts = case(name)[0]
        blob += [struct.pack("=qq", *pts.shape), np.ascontiguousarray(pts).tobytes()]
    data, res = tmp / "cases.bin", tmp / "result.bin"
    data.write_bytes(b"".join(blob))
    r = host_check.run(tmp, "hclust_host_check", [data, res], flags=["-ffp-contract=off"], libs=["-lm"])
    assert r.returncode == 0, r.stdout[-2000:]
    raw = res.read_bytes()
    got, at = {}, 0
    for name in NAMES:
        P = case(name)[0].shape[0]
        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a
        got[name] = (take(np.float64, P * P).reshape(P, P), take(np.float64, (P - 1) * 4).reshape(P - 1, 4),
                     int(take(np.int64, 1)[0]), int(take(np.int64, 1)[0]))
    assert at == len(raw)
    return got


@pytest.mark.parametrize("name", NAMES)
def test_header_is_the_twin(host_run, name):
    pts, m, d = case(name)
    P = len(pts)
    dist, merges, status, scans = host_run[name]
    assert (dist == d).all(), np.argwhere(dist != d)[:5]
    assert (dist == dist.T).all() and (np.diag(dist) == 0).all() and not np.signbit(dist).any()
    assert status == 0 and P - 1 <= scans <= 3 * (P - 1)
    assert (merges == m).all(), np.argwhere(merges != m)[:5]
    assert (merges[:, 0] < merges[:, 1]).all() and merges[-1, 3] == P


@pytest.mark.parametrize("name", NAMES)
def test_twin_is_scipy_on_the_same_distances(name):
    from scipy.cluster.hierarchy import leaves_list, linkage
    from scipy.spatial.distance import squareform
    pts, m, d = case(name)
    Z = hm.to_linkage(m, len(pts))
    ref = linkage(squareform(d), "complete")
    assert (Z == ref).all(), np.argwhere(Z != ref)[:5]
    assert (hm.leaves(Z) == leaves_list(ref)).all()


@pytest.mark.parametrize("name", NAMES)
def test_twin_distances_against_pdist(name):
    from scipy.spatial.distance import pdist, squareform
    pts, _, d = case(name)
    ref = squareform(pdist(pts))
    tol = (pts.shape[1] + 2) * 2.0 ** -52
    assert (np.abs(d - ref) <= tol * ref).all()


def test_the_tied_cases_hold_ties_and_zero_heights():
    pts, m, d = case("tied-257x21")
    off = d[np.triu_indices(257, 1)]
    assert (off == 0).any() and len(np.unique(off)) < off.size // 10
    assert (m[:, 2] == 0).any()
    _, m, d = case("equal-70x5")
    assert (d == 0).all() and (m[:, 2] == 0).all()
    # every chain of all-equal points stops on the tie rule at once: slot 0 and its lowest live neighbour merge
    assert m[:, 0].tolist() == list(range(69)) and m[:, 1].tolist() == list(range(1, 70))


def _Z(rows):
    return np.array(rows, np.float64)


def test_reorder_on_hand_made_trees():
    # ((0, 1), 2): leaf 2 is lighter than the pair, so it moves in front; inside the pair 1 is lighter than 0
    Z = _Z([[0, 1, 1.0, 2], [2, 3, 2.0, 3]])
    assert hm.leaves(Z).tolist() == [2, 0, 1]
    assert hm.reorder(Z, [5.0, 1.0, 2.0]).tolist() == [2, 1, 0]
    assert hm.reorder(Z, [1.0, 2.0, 9.0]).tolist() == [0, 1, 2]
    # ((0, 1), (2, 3)) under 4: sums 3 and 7 keep the pairs, 0.5 puts leaf 4 first
    Z = _Z([[0, 1, 1.0, 2], [2, 3, 1.5, 2], [5, 6, 2.0, 4], [4, 7, 3.0, 5]])
    assert hm.leaves(Z).tolist() == [4, 0, 1, 2, 3]
    assert hm.reorder(Z, [2.0, 1.0, 3.0, 4.0, 0.5]).tolist() == [4, 1, 0, 2, 3]
    assert hm.reorder(Z, [2.0, 1.0, 3.0, 4.0, 20.0]).tolist() == [1, 0, 2, 3, 4]
    # ties: equal leaves and equal sums keep the left child first
    Z = _Z([[0, 1, 1.0, 2], [2, 3, 1.0, 2], [4, 5, 2.0, 4]])
    assert hm.reorder(Z, [1.0, 1.0, 1.0, 1.0]).tolist() == [0, 1, 2, 3]
    assert hm.reorder(Z, [3.0, 1.0, 2.0, 2.0]).tolist() == [1, 0, 2, 3]
    assert hm.reorder(Z, [3.0, 1.5, 2.0, 2.0]).tolist() == [2, 3, 1, 0]


def test_ten_thousand_leaves_in_a_chain_need_no_recursion():
    from scipy.cluster.hierarchy import leaves_list
    n = 10000
    Z = np.empty((n - 1, 4))
    Z[0] = (0, 1, 1.0, 2)
    for i in range(1, n - 1):
        Z[i] = (i + 1, n + i - 1, i + 1.0, i + 2)
    assert (hm.leaves(Z) == leaves_list(Z)).all()
    order = hm.reorder(Z, np.arange(n, dtype=np.float64)[::-1])
    assert sorted(order.tolist()) == list(range(n))
    xs, ys = hm.dendrogram_segments(Z, hm.leaves(Z))
    assert xs.shape == ys.shape == (n - 1, 4) and ys.max() == n - 1.0 and (xs >= 0).all() and (xs <= n - 1).all()


def test_dendrogram_segments_of_three_leaves():
    Z = _Z([[0, 1, 1.0, 2], [2, 3, 2.0, 3]])
    xs, ys = hm.dendrogram_segments(Z, [2, 0, 1])
    assert xs.tolist() == [[1, 1, 2, 2], [0, 0, 1.5, 1.5]] and ys.tolist() == [[0, 1, 1, 0], [0, 2, 2, 1]]


def test_to_linkage_sorts_stably_and_relabels():
    # the chain found the higher merge first; equal heights keep the chain's order
    m = _Z([[2, 3, 5.0, 2], [0, 1, 1.0, 2], [4, 5, 1.0, 2], [1, 3, 9.0, 4], [3, 5, 9.5, 6]])
    Z = hm.to_linkage(m, 6)
    assert Z.tolist() == [[0, 1, 1.0, 2], [4, 5, 1.0, 2], [2, 3, 5.0, 2], [6, 8, 9.0, 4], [7, 9, 9.5, 6]]


def test_sample_rows():
    a = hm.sample_rows(1000, 100, 7)
    assert a.dtype == np.int64 and len(a) == 100 and (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < 1000
    assert (a == hm.sample_rows(1000, 100, 7)).all() and (a != hm.sample_rows(1000, 100, 8)).any()
    assert (a == np.sort(np.random.RandomState(7).choice(1000, 100, replace=False))).all()
    assert hm.sample_rows(100, 100, 7).tolist() == list(range(100)) and hm.sample_rows(5, 100, 7).tolist() == list(range(5))


def test_library_exports_the_entry():
    from subphaser_amd import _native
    lib = _native.load()
    assert hasattr(lib, "sp_hclust_complete") and "sp_hclust_complete" in _native.SYMBOLS
    assert _native.HCLUST_MAX_POINTS == hc.MAX_POINTS == 16384
    header = open(os.path.join(ROOT, "subphaser_amd", "csrc", "sp_hclust.h")).read()
    assert "#define SP_HC_MAXP 16384" in header
