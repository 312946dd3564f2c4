"""The k-means bootstrap replicate of subphaser_amd/csrc/sp_kboot.h, checked on the host.

tests/kboot_host_check.cpp is compiled against the header with the host C++ compiler (-ffp-contract=off, as the library
is built) and fed Gram matrices from the numpy twin (tests/kboot_ref.py).  On every replicate the twin calls decided
(smallest relative decision margin >= 1e-9; at most 1 % of a case may be undecided) the program must give the twin's
labels and iteration count; its uniform draws must be the twin's to the bit.

The twin itself is held against scikit-learn statistically: on a separable and a noisy toy matrix (C = 12, K = 3,
R = 400 replicates of 400 columns, the same columns for both) the support columns a (twin) and b (scikit-learn loop),
in percentage points, must satisfy |a - b| <= 5 sqrt((a (100 - a) + b (100 - b)) / R) + 1: five standard deviations of
the difference of two binomial shares plus one point for the truncation to integers."""
import struct

import numpy as np
import pytest

import host_check
import kboot_ref as kr

# (C, K, n columns, replicates): the shapes of the GPU test, and K = 1
SHAPES = [(2, 2, 50, 30), (3, 3, 50, 30), (5, 1, 40, 10), (12, 3, 400, 40), (21, 3, 1000, 40), (33, 4, 100, 20),
          (64, 7, 300, 20), (128, 32, 200, 6)]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kboot_host")
    cases, blob = [], []
    for i, (C, K, n, R) in enumerate(SHAPES):
        z = kr.blobs(100 + i, C, K, 500, noise=0.8)
        cols = np.random.RandomState(i).randint(0, z.shape[1], size=(R, n))
        G = kr.gram(z, cols)
        seed = 0x9E3779B97F4A7C15 * (i + 1) % 2**64
        labels, iters, gaps = kr.solve_all(G, K, seed)
        cases.append((C, K, labels, iters, gaps))
        for r in range(R):
            blob += [struct.pack("=qqQQ", C, K, seed, r), np.ascontiguousarray(G[r]).tobytes()]
    n_cases = sum(s[3] for s in SHAPES)
    draws = [(s, r, i) for s in (0, 1, 2**64 - 1, 0xDEADBEEF) for r in (0, 1, 999, 2**40) for i in (0, 1, 7, 2**33)]
    data = tmp / "cases.bin"
    data.write_bytes(struct.pack("=q", n_cases) + b"".join(blob) + struct.pack("=q", len(draws))
                     + b"".join(struct.pack("=QQQ", *d) for d in draws))
    r = host_check.run(tmp, "kboot_host_check", [data], flags=["-ffp-contract=off"], libs=["-lm"])
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines(), cases, draws


def test_draws_and_trial_counts(host_run):
    lines, _, draws = host_run
    got = [float.fromhex(l.split()[1]) for l in lines if l.startswith("U ")]
    assert got == [kr.u(*d) for d in draws]
    assert all(0.0 <= v < 1.0 for v in got) and len(set(got)) == len(got)
    t = {int(l.split()[1]): int(l.split()[2]) for l in lines if l.startswith("T ")}
    assert t == {K: kr.trials(K) for K in range(1, 65)}


def test_labels_and_iterations_on_decided_replicates(host_run):
    lines, cases, _ = host_run
    rows = [list(map(int, l.split()[1:])) for l in lines if l.startswith("R ")]
    at = 0
    for C, K, labels, iters, gaps in cases:
        R = len(iters)
        got = np.array(rows[at:at + R])
        at += R
        ok = kr.decided(gaps)
        print("C = %3d K = %2d: %d of %d decided, smallest gap %.1e, iterations %d..%d" % (
            C, K, int(ok.sum()), R, float(gaps.min()), int(iters.min()), int(iters.max())))
        assert got.shape == (R, C + 1)
        assert (got[ok, 0] == iters[ok]).all(), (C, K, np.nonzero(got[:, 0] != iters)[0][:5])
        assert (got[ok, 1:] == labels[ok]).all(), (C, K, np.nonzero((got[:, 1:] != labels).any(axis=1))[0][:5])
        assert (got[:, 1:] >= 0).all() and (got[:, 1:] < K).all()
    assert at == len(rows)
    # the set reaches what it is meant to: more than one Lloyd iteration somewhere, K = 1 in one
    assert max(int(c[3].max()) for c in cases) > 1 and all((c[3] == 1).all() for c in cases if c[1] == 1)


@pytest.mark.parametrize("noise", [0.5, 3.0], ids=["separable", "noisy"])
def test_twin_support_against_sklearn(noise):
    from sklearn.cluster import KMeans
    from subphaser_amd.cluster import relabel_by_chromosome_order
    C, K, R = 12, 3, 400
    z = kr.blobs(7, C, K, 3000, noise)
    chrs = ["chr%02d" % i for i in range(C)]
    base = relabel_by_chromosome_order(chrs, np.arange(C) % K)
    cols = kr.bootstrap_cols(11, z.shape[1], R)
    labels, _, gaps = kr.solve_all(kr.gram(z, cols), K, seed=11)
    kr.decided(gaps)
    a = np.array(kr.support(chrs, base, labels), float)
    b = np.array(kr.support(chrs, base, [KMeans(n_clusters=K, random_state=r).fit(z[:, cols[r]]).labels_
                                         for r in range(R)]), float)
    bound = 5 * np.sqrt((a * (100 - a) + b * (100 - b)) / R) + 1
    print("twin   ", a.astype(int).tolist())
    print("sklearn", b.astype(int).tolist())
    print("bound  ", np.round(bound, 1).tolist())
    assert (np.abs(a - b) <= bound).all()
    if noise > 1:
        # (the first chromosome in name order is cluster 0 of every renumbered replicate: its support is 100 by construction)
        assert a[1:].max() < 100 and b[1:].max() < 100, "the noisy matrix is meant to leave the support below 100"
