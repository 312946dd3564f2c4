"""The arithmetic of subphaser_amd/csrc/sp_ltrtree.h, checked on the host, and the host side of the tree (ltrtree.py).

tests/ltrtree_host_check.cpp is compiled against the header with the host C++ compiler and its drivers are compared with
the Python twin (tests/ltrtree_ref.py) with `==`: sketches (N runs, an element shorter than k, fewer than / exactly / more
than s distinct k-mers, tandem repeats, a reverse-complemented copy), pairs (identical, disjoint, one or both empty,
unequal lengths, denom cut at s before either list ends) and the join records for N = 2, 3, 4, 5, 33, 64, 65 on random,
all-equal, zero and far-from-a-tree matrices.

The guard.  No matrix inside the input contract (entries in [0, 2^31)) was found that drives a derived distance to 2^40: on
random, sparse 0 / 2^31 - 1 and hill-climbed matrices (N = 6 .. 257) no derived |D| ever exceeded the largest input entry.
The drivers therefore take the limit as an argument, and the guard is checked twice: on the far-from-a-tree matrices with the
limit lowered to a value their run reaches in its second half (ltrtree_ref.guard_limit), where a limit above the run's largest value changes nothing,
and at the real 2^40 on a matrix with entries of 2^41 -- outside the contract, which the header's driver does not check (the
library entry does).

The planted families of the end-to-end GPU test are checked here on the twin alone: for the committed seeds every family is
one clade, members of a family share at least 17 of 256 hashes, members of different families at most 1.

The twin against something independent: no phylogenetics package is installed, so neighbour joining's defining property is
used.  Distances read off a random tree with even integer edge lengths are additive, every halving is exact, and the
records must give back exactly the tree's splits and edge lengths (N = 4, 5, 9, 33)."""
import math
import struct

import numpy as np
import pytest

import host_check
import ltrtree_cases as cases
import ltrtree_ref as lt
from subphaser_amd import ltrtree

CODES = {"A": 0, "C": 1, "G": 2, "T": 3}


def _guard_matrix(N):
    D = np.full((N, N), 1 << 41, np.int64)
    np.fill_diagonal(D, 0)
    D[0, 1] = D[1, 0] = 0
    return D


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """every case through the compiled header: {(kind, name): result}"""
    tmp = tmp_path_factory.mktemp("ltrtree_host")
    blob, plan = [], []
    for name, seq, k, s, _ in cases.sketch_cases():
        blob += [struct.pack("=qqqq", 1, k, s, len(seq)), bytes(CODES.get(ch, 4) for ch in seq)]
        plan.append(("sketch", name, s))
    for name, a, b, s, _ in cases.pair_cases():
        blob += [struct.pack("=qqqq", 2, s, len(a), len(b)), np.array(a + b, np.uint64).tobytes()]
        plan.append(("pair", name, s))
    mats = cases.nj_matrices() + [(t[0], t[2]) for t in cases.tree_cases()] + [("guard-%d" % N, _guard_matrix(N)) for N in (3, 33)]
    mats = [(name, D, lt.DMAX) for name, D in mats]
    for name, D in cases.nj_matrices((33, 65)):
        if name.startswith("negative"):
            limit, _, top = lt.guard_limit(D)
            mats += [("lowered-" + name, D, limit), ("above-" + name, D, top + 1)]
    for name, D, limit in mats:
        blob += [struct.pack("=qqq", 3, D.shape[0], limit), np.ascontiguousarray(D, np.int64).tobytes()]
        plan.append(("nj", name, D.shape[0]))
    sk, ln = cases.hand_sketches(33, 16, 1)
    blob += [struct.pack("=qqq", 4, 16, 33), sk.tobytes(), ln.tobytes()]
    plan.append(("pairs", "hand", 33))
    blob.append(struct.pack("=q", 0))
    data, res = tmp / "cases.bin", tmp / "result.bin"
    data.write_bytes(b"".join(blob))
    r = host_check.run(tmp, "ltrtree_host_check", [data, res])
    assert r.returncode == 0, r.stdout[-2000:]
    raw, at, out = res.read_bytes(), 0, {}

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a
    for kind, name, n in plan:
        if kind == "sketch":
            out[kind, name] = (take(np.uint64, n).tolist(), int(take(np.int64, 1)[0]))
        elif kind == "pair":
            out[kind, name] = tuple(take(np.int64, 2).tolist())
        elif kind == "nj":
            out[kind, name] = (int(take(np.int64, 1)[0]), take(np.int64, (n - 1) * 5).reshape(n - 1, 5))
        else:
            out[kind, name] = (take(np.int32, n * n).reshape(n, n), take(np.int32, n * n).reshape(n, n))
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", [c[0] for c in cases.sketch_cases()])
def test_sketch(host, name):
    _, seq, k, s, want = next(c for c in cases.sketch_cases() if c[0] == name)
    assert host["sketch", name] == want
    n_distinct = len(lt.hashes(seq, k))
    assert want[1] == min(s, n_distinct) and want[0][want[1]:] == [lt.NONE] * (s - want[1])
    assert {"short": n_distinct == 0, "all-n": n_distinct == 0, "one-kmer": n_distinct == 1, "fewer": 0 < n_distinct < s, "exactly": n_distinct == s,
            "more": n_distinct > s, "tandem": n_distinct == 37 and len(seq) - k + 1 > 10 * n_distinct}.get(name, True)


def test_revcomp_has_the_same_sketch(host):
    assert host["sketch", "forward"] == host["sketch", "revcomp"] and host["sketch", "forward"][1] == 64


@pytest.mark.parametrize("name", [c[0] for c in cases.pair_cases()])
def test_pair(host, name):
    _, a, b, s, want = next(c for c in cases.pair_cases() if c[0] == name)
    assert host["pair", name] == want
    assert {"identical": want == (64, 64), "disjoint": want == (0, 64), "both-empty": want == (0, 0), "one-empty": want == (0, 30),
            "cut-at-s": want == (14, 64) and a[-1] > sorted(set(a) | set(b))[63] < b[-1]}.get(name, True)


def test_pairs_matrix(host):
    sk, ln = cases.hand_sketches(33, 16, 1)
    shared, denom = lt.pairs(sk, ln, 16)
    assert (host["pairs", "hand"][0] == shared).all() and (host["pairs", "hand"][1] == denom).all()
    assert (np.diag(shared) == ln).all() and (np.diag(denom) == ln).all() and (shared == shared.T).all()


@pytest.mark.parametrize("name", [m[0] for m in cases.nj_matrices()])
def test_nj_records(host, name):
    D = next(m[1] for m in cases.nj_matrices() if m[0] == name)
    want = cases.nj_expected(name, D)
    status, got = host["nj", name]
    assert status == 0 and (got == want).all()
    if D.shape[0] <= 33:      # the vectorised twin against the scan written from the definition
        assert [tuple(r) for r in want.tolist()] == lt.nj(D.tolist())
    if name.startswith("tied"):      # all Q equal: the lowest i, then the lowest j
        assert want[0, 0] == 0 and want[0, 1] == 1
    if name in ("negative-33", "negative-64", "negative-65"):
        assert (want[:, 2] < 0).any()


@pytest.mark.parametrize("N", [3, 33])
def test_guard(host, N):
    status, _ = host["nj", "guard-%d" % N]
    assert status == 1
    with pytest.raises(lt.Guard):
        lt.nj(_guard_matrix(N).tolist())
    with pytest.raises(lt.Guard):
        lt.nj_numpy(_guard_matrix(N))


@pytest.mark.parametrize("name", [t[0] for t in cases.tree_cases()])
def test_additive_distances_give_the_tree_back(host, name):
    _, edges, D = next(t for t in cases.tree_cases() if t[0] == name)
    N = D.shape[0]
    status, got = host["nj", name]
    want = lt.nj_numpy(D)
    assert status == 0 and (got == want).all() and [tuple(r) for r in want.tolist()] == lt.nj(D.tolist())
    assert ltrtree.splits(ltrtree.unrooted_edges(want), N) == {k: float(v) for k, v in ltrtree.splits(edges, N).items()}


@pytest.mark.parametrize("N", [33, 65])
def test_guard_at_a_lowered_limit(host, N):
    name = "negative-%d" % N
    D = next(m[1] for m in cases.nj_matrices((N,)) if m[0] == name)
    limit, join, top = lt.guard_limit(D)
    assert 0 < limit <= top < 1 << 31 and join < N - 3      # joins are left when it fires
    assert host["nj", "lowered-" + name][0] == 1
    with pytest.raises(lt.Guard):
        lt.nj_numpy(D, dmax=limit)
    with pytest.raises(lt.Guard):
        lt.nj(D.tolist(), dmax=limit)
    status, got = host["nj", "above-" + name]      # a limit that is not reached changes nothing
    assert status == 0 and (got == cases.nj_expected(name, D)).all() and (lt.nj_numpy(D, dmax=top + 1) == got).all()


@pytest.mark.parametrize("seed", cases.PLANTED_SEEDS)
def test_planted_families_are_clades_of_the_twin(seed):
    chrom, el, fams, sk, ln, shared, denom, D, want = cases.planted_twin(seed)
    assert cases.families_are_clades(want, fams)
    n = len(fams)
    same = [shared[i, j] for i in range(n) for j in range(i + 1, n) if fams[i] == fams[j]]
    diff = [shared[i, j] for i in range(n) for j in range(i + 1, n) if fams[i] != fams[j]]
    print("seed %d: within a family >= %d shared hashes, between families <= %d" % (seed, min(same), max(diff)))
    assert min(same) >= 17 and max(diff) <= 1


# ---- host functions
def test_mash_units():
    k, s = 13, 1024
    got = ltrtree.mash_units([[1024, 512, 1, 0, 0]], [[1024, 1024, 1024, 1024, 0]], k, s)
    want = [0] + [int(math.floor(-math.log(2 * j / (1 + j)) / k * (1 << 30) + 0.5)) for j in (0.5, 1 / 1024, 0.5 / 1024, 0.5 / 1024)]
    assert got.dtype == np.int64 and got.tolist() == [want] and want[3] > want[2] > want[1] > 0
    for kk, ss in ((9, 4096), (9, 16), (31, 4096)):      # the largest distance of every corner is below 2^31
        assert 0 < int(ltrtree.mash_units(0, ss, kk, ss)) < 1 << 31
    assert int(ltrtree.mash_units(0, 4096, 9, 4096)) == max(int(ltrtree.mash_units(0, d, 9, 4096)) for d in (1, 16, 4095, 4096))
    with pytest.raises(ValueError):
        ltrtree.mash_units(5, 4, k, s)
    D = ltrtree.distance_matrix([[0, 3], [3, 0]], [[0, 16], [16, 16]], 13, 16)
    assert D.tolist() == [[0, int(ltrtree.mash_units(3, 16, 13, 16))]] * 1 + [[int(ltrtree.mash_units(3, 16, 13, 16)), 0]]


def test_branch_lengths_rooting_and_newick():
    # ((0:2,1:4):6,(2:8,3:10)) as an unrooted tree: inner edge 6
    edges = [(4, 0, 2), (4, 1, 4), (5, 2, 8), (5, 3, 10), (4, 5, 6)]
    D = np.zeros((4, 4), np.int64)
    for a, b, d in ((0, 1, 6), (0, 2, 16), (0, 3, 18), (1, 2, 18), (1, 3, 20), (2, 3, 18)):
        D[a, b] = D[b, a] = d
    rec = lt.nj_numpy(D)
    assert rec.tolist() == [[0, 1, 6, 40, 44], [0, 2, 14, 30, 32], [0, 3, 10, 0, 0]]
    assert ltrtree.branch_lengths(rec) == [(2.0, 4.0), (6.0, 8.0), (10.0, 0.0)]
    assert ltrtree.splits(ltrtree.unrooted_edges(rec), 4) == ltrtree.splits(edges, 4) == {
        frozenset({1}): 4.0, frozenset({1, 2, 3}): 2.0, frozenset({2, 3}): 6.0, frozenset({2}): 8.0, frozenset({3}): 10.0}
    # longest path 1 .. 3 = 20: the midpoint lies 10 from leaf 3, at the inner node next to it
    text = ltrtree.tree_text(rec, ["a", "b c", "c", "d:1"])
    assert text == "((a:%s,'b c':%s):%s,c:%s,'d:1':%s);" % tuple("{:.6g}".format(x / 2 ** 30) for x in (2, 4, 6, 8, 10))
    # a midpoint inside an edge: one long leaf edge
    rec2 = np.array([[0, 1, 10, 0, 0]], np.int64)
    assert ltrtree.tree_text(rec2, ["x", "y"]) == "(x:{0},y:{0});".format("{:.6g}".format(5 / 2 ** 30))
    # negative lengths are written as 0
    rec3 = np.array([[0, 1, 2, 0, 40], [0, 2, 4, 0, 0]], np.int64)      # l_0 = 1 + (0 - 40) / 2 = -19, l_1 = 21
    assert ltrtree.branch_lengths(rec3)[0] == (-19.0, 21.0)
    assert ":-" not in ltrtree.tree_text(rec3, ["p", "q", "r"]) and "p:0" in ltrtree.tree_text(rec3, ["p", "q", "r"])
    assert ltrtree.choose(5, 10, 0) == [0, 1, 2, 3, 4]
    pick = ltrtree.choose(100, 10, 7)
    assert pick == sorted(set(pick)) and len(pick) == 10 and pick == ltrtree.choose(100, 10, 7) != ltrtree.choose(100, 10, 8)
