"""The k-mer PCA arithmetic of subphaser_amd/csrc/sp_kpca.h, checked on the host.

tests/kpca_host_check.cpp is compiled against the header with the host C++ compiler (-ffp-contract=off, as the library is
built) and compared with the numpy twin (tests/kpca_ref.py) with `==`: row statistics, the Gram matrix in chunk order,
the bad-row count, the sign rows and their values.  The inputs hold counts of 0 and 2^32 - 1, lengths above 2^32,
constant rows and duplicated rows.

The twin's recipe (eigh of the Gram matrix, scores U sqrt(w), signs from the largest-|v| k-mer, percentages w / trace,
then the reference's per-component normalisation) is held against scikit-learn's PCA(svd_solver="full") on matrices
with planted subgenome structure.  The two differ by rounding only, amplified by the eigen-gap; measured here
(profiles/kpca_notes.md, 3 components): normalised scores within 3.1e-12 (C = 12; 1.8e-12 at C = 21), percentages within
5.7e-14.  TOL is 100 x the larger figure; the third component, which carries no planted structure and whose eigenvalue
has a close neighbour, sets it.

Derivable check: every good row adds z . z = C up to rounding, so trace(G) = C (M - n_bad) within 4 C M 2^-52 C."""
import struct

import numpy as np
import pytest

import host_check
import kpca_ref as kp

TOL = 3.1e-10         # 100 x the measured twin-vs-sklearn difference (never looser than 1e-6)

# (seed, M, C, n_comp, extreme, bad rows, dup)
CASES = [
    (1, 1, 2, 1, False, (), None),
    (2, kp.ROWS - 1, 3, 2, False, (), None),
    (3, kp.ROWS, 21, 3, True, (5,), (7, 900)),
    (4, kp.ROWS + 1, 33, 32, True, (0, kp.ROWS), None),
    (5, 3 * kp.ROWS + 7, 12, 2, True, (3, kp.ROWS + 500, 3 * kp.ROWS + 6), (10, 3 * kp.ROWS + 5)),
    (6, 300, 65, 4, False, (), (0, 299)),
]


def _inputs():
    out = []
    for seed, M, C, n_comp, extreme, bad, dup in CASES:
        counts, lengths = kp.random_case(seed, M, C, extreme, bad, dup)
        U = np.random.default_rng(seed).normal(size=(C, n_comp))
        out.append((counts, lengths, U))
    return out


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kpca_host")
    inputs = _inputs()
    blob = [struct.pack("=q", len(inputs))]
    for counts, lengths, U in inputs:
        blob += [struct.pack("=qqq", counts.shape[0], counts.shape[1], U.shape[1]), lengths.tobytes(),
                 np.ascontiguousarray(counts).tobytes(), np.ascontiguousarray(U).tobytes()]
    data, res = tmp / "cases.bin", tmp / "result.bin"
    data.write_bytes(b"".join(blob))
    r = host_check.run(tmp, "kpca_host_check", [data, res], flags=["-ffp-contract=off"], libs=["-lm"])
    assert r.returncode == 0, r.stdout[-2000:]
    raw = res.read_bytes()
    got, at = [], 0
    for counts, lengths, U in inputs:
        (M, C), n = counts.shape, U.shape[1]
        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a
        got.append((take(np.float64, 2 * M).reshape(M, 2), take(np.float64, C * C).reshape(C, C), int(take(np.int64, 1)[0]),
                    take(np.int64, n), take(np.float64, n)))
    assert at == len(raw)
    return inputs, got


def test_header_stats_and_gram_are_the_twin(host_run):
    inputs, got = host_run
    for (counts, lengths, _), (stats, G, n_bad, _, _), case in zip(inputs, got, CASES):
        tG, tbad, tstats = kp.gram(counts, lengths)
        assert (stats == tstats).all(), (case, np.argwhere(stats != tstats)[:5])
        assert n_bad == tbad == len(case[5]), case
        assert (G == tG).all() and (G == G.T).all(), (case, np.argwhere(G != tG)[:5])
        assert np.isfinite(G).all()


def test_header_sign_rows_are_the_twin(host_run):
    inputs, got = host_run
    for (counts, lengths, U), (_, _, _, rows, vals), case in zip(inputs, got, CASES):
        trows, tvals = kp.signs(counts, lengths, U)
        assert (rows == trows).all() and (vals == tvals).all(), case
        dup = case[6]
        if dup is not None:
            assert not (rows == dup[1]).any()        # of two equal rows the lower index wins


def test_inputs_reach_the_extremes():
    counts, lengths = kp.random_case(*CASES[4][:3], True, CASES[4][5], CASES[4][6])
    assert counts.max() == 2 ** 32 - 1 and counts.min() == 0 and lengths.max() > 2 ** 32 and lengths.min() == 1
    stats, bad = kp.rowstats(counts, lengths)
    assert bad.sum() == 3 and (stats[bad] == 0).all()
    assert (counts[10] == counts[3 * kp.ROWS + 5]).all()


def test_all_rows_bad():
    counts = np.zeros((5, 4), np.uint32)
    lengths = np.arange(1, 5, dtype=np.int64)
    G, n_bad, _ = kp.gram(counts, lengths)
    assert n_bad == 5 and (G == 0).all()
    rows, vals = kp.signs(counts, lengths, np.ones((4, 2)))
    assert (rows == -1).all() and (vals == 0).all()


PLANTED = {"C12": (11, 12, 3000), "C21": (12, 21, 4000)}
_planted_cache = {}


def planted_case(name):
    """(counts, lengths, group, freqs M x C) -- computed once, shared, never changed"""
    if name not in _planted_cache:
        seed, C, M = PLANTED[name]
        counts, lengths, group = kp.planted(seed, C, M)
        for a in (counts, lengths, group):
            a.setflags(write=False)
        _planted_cache[name] = (counts, lengths, group, counts / lengths.astype(np.float64))
    return _planted_cache[name]


def sklearn_pca(freqs, n):
    """the reference's Cluster.pca arithmetic (Cluster.py:24-26, 49-52) with the full solver"""
    from sklearn.decomposition import PCA
    x = freqs.T
    z = (x - x.mean(axis=0)) / x.std(axis=0)
    p = PCA(n_components=n, svd_solver="full")
    s = p.fit_transform(z)
    return (s - s.mean(axis=0)) / s.std(axis=0), p.explained_variance_ratio_ * 100


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_twin_recipe_against_sklearn_full(name):
    counts, lengths, group, freqs = planted_case(name)
    n = 3
    G, n_bad, _ = kp.gram(counts, lengths)
    assert n_bad == 0
    scores, percent, U = kp.pca(G, lambda U: kp.signs(counts, lengths, U)[1], n)
    ref_scores, ref_percent = sklearn_pca(freqs, n)
    ds, dp = np.abs(scores - ref_scores).max(), np.abs(percent - ref_percent).max()
    v, _ = kp.projections(counts, lengths, U)
    top2 = -np.sort(-np.abs(v), axis=0)[:2]
    w = np.linalg.eigvalsh(G)[::-1]
    print("%s: scores differ by %.2e, percentages by %.2e; eigenvalues %s; largest |v| per component %s, runner-up %s" % (
        name, ds, dp, np.round(w[:4], 1).tolist(), top2[0].round(4).tolist(), top2[1].round(4).tolist()))
    assert ds <= TOL and dp <= TOL
    # the structure is there: the first two components separate the three groups
    cent = np.array([scores[group == g, :2].mean(axis=0) for g in range(3)])
    spread = max(scores[group == g, :2].std(axis=0).max() for g in range(3))
    assert min(np.linalg.norm(cent[a] - cent[b]) for a in range(3) for b in range(a)) > 5 * spread


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_trace_is_the_number_of_good_rows(name):
    counts, lengths, _, _ = planted_case(name)
    counts = counts.copy()
    counts[17] = 0
    G, n_bad, _ = kp.gram(counts, lengths)
    M, C = counts.shape
    assert n_bad == 1
    assert abs(np.trace(G) - C * (M - n_bad)) <= 4 * C * M * 2.0 ** -52 * C


def test_library_exports_the_pca_entries():
    from subphaser_amd import _native
    lib = _native.load()
    assert hasattr(lib, "sp_kmer_pca_gram") and hasattr(lib, "sp_kmer_pca_signs")
    assert {"sp_kmer_pca_gram", "sp_kmer_pca_signs"} <= set(_native.SYMBOLS)
    assert _native.KPCA_MAX_CHROM == kp.MAX_CHROM == 1024 and _native.KPCA_MAX_COMP == kp.MAX_COMP == 32
