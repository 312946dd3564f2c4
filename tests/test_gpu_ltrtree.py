"""GPU: the LTR tree's three entries (sp_ltrtree.hip; Context.ltr_sketch, ltr_sketch_pairs, nj_tree) against the Python twin
(tests/ltrtree_ref.py) with `==`, the planted end-to-end case, the errors and the command line under -ltr_tree.

Sketches: s = 16, 64, 1024 with k = 9, 13, 31; element lengths 1, k - 1, k, around one chunk and several chunks with the
chunk set to 50 and 333 starts, the same bytes at every chunk size and at the default; every start residue modulo 32; an
element at either end of a chromosome; all-N and N-run elements; 2500 elements in one call.
Pairs: the hand-made host cases and n = 1, 2, 33, 257 (ragged tiles at every tile size: s = 16 gives 16 x 16 tiles,
s = 1024 gives 8 x 8, s = 4096 gives 2 x 2).
Neighbour joining: N = 2, 3, 4, 5, 33, 64, 65, 257, 1000 on random, all-equal, zero and far-from-a-tree matrices and the
additive trees, all five columns; both drivers (the looping workgroup and the two launches per join) at every N up to 257,
and the default choice on either side of its crossover (SP_LT_NJ_LOOP_MAX = 128), which sp_prof_report proves.

The guard: no matrix inside the input contract is known to reach 2^40 (test_ltrtree_host.py), so sp_nj_set_guard lowers the
limit to a value the far-from-a-tree matrices reach in the second half of their joins: SP_ESTATE under both drivers, the
2 (N - 2) launches still enqueued and the ones behind the guard no-ops, and the next call on the same context the twin's.

Not here: SP_ENOMEM -- provoking it means exhausting the memory of a device that other people's work shares, which is not done
on purpose; and SP_CU_LIMIT cases -- no kernel of the unit caps its grid (one workgroup per element, per pair tile, per matrix
row; test_grids_are_the_problem_sizes reads them back)."""
import os
import random

import numpy as np
import pytest

import ltrtree_cases as cases
import ltrtree_ref as lt
from subphaser_amd import ltrtree

pytestmark = pytest.mark.gpu

CHUNKS = (50, 333)


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.ltr_sketch_set_chunk(0)
    gpu_ctx.nj_set_mode(0)
    gpu_ctx.nj_set_guard(0)


def load(ctx, seqs):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)


# ---------------------------------------------------------------------------------------------- sketches
def element_world(k):
    """two chromosomes and the elements (chrom, start, end) of the sketch test at k"""
    rng = random.Random(40 + k)
    c0 = lt.rand_seq(rng, 2600)
    c0 = c0[:900] + "N" * 5 + c0[905:1000] + "N" * 64 + c0[1064:1400] + "N" * 400 + c0[1800:]
    c1 = lt.rand_seq(rng, 1500)
    c1 = c1[:700] + c1[100:400] * 2 + c1[1300:]          # repeated k-mers
    el = [(0, 0, 1), (0, 10, 10 + k - 1), (0, 10, 10 + k), (0, 10, 11 + k)]
    for c in CHUNKS:
        el += [(1, 3, 3 + c + k - 2), (1, 3, 3 + c + k - 1), (1, 3, 3 + c + k), (1, 7, 7 + 3 * c + k + 5)]
    el += [(0, r, r + 150 + r) for r in range(32)]       # every residue of the start, crossing the first N runs from r >= ...
    el += [(0, 0, 300), (0, len(c0) - 300, len(c0)), (1, 0, len(c1)), (0, 0, len(c0))]
    el += [(0, 1420, 1780), (0, 1000, 1064), (0, 850, 1500), (0, 1390, 1810)]      # all N (twice), N runs inside
    return [c0, c1], el


_sk = {}


def sketch_twin(k, s):
    if (k, s) not in _sk:
        seqs, el = element_world(k)
        _sk[k, s] = (seqs, el) + lt.sketches([seqs[c][a:b] for c, a, b in el], k, s)
    return _sk[k, s]


@pytest.mark.parametrize("k,s", [(9, 16), (13, 64), (31, 1024), (13, 1024)])
def test_sketch_is_the_twin_at_every_chunk_size(ctx, k, s):
    seqs, el, want_sk, want_ln = sketch_twin(k, s)
    load(ctx, seqs)
    chrom, start, end = (np.array(x) for x in zip(*el))
    first = None
    for chunk in (0,) + CHUNKS:
        ctx.ltr_sketch_set_chunk(chunk)
        sk, ln = ctx.ltr_sketch(chrom, start, end, k, s)
        assert sk.dtype == np.uint64 and sk.shape == (len(el), s) and ln.dtype == np.int32
        bad = [i for i in range(len(el)) if ln[i] != want_ln[i] or (sk[i] != want_sk[i]).any()]
        assert not bad, (chunk, [(el[i], int(ln[i]), int(want_ln[i])) for i in bad[:5]])
        first = first or (sk.tobytes(), ln.tobytes())
        assert (sk.tobytes(), ln.tobytes()) == first
    by = dict(zip(el, want_ln.tolist()))
    assert by[0, 0, 1] == 0 and by[0, 10, 10 + k - 1] == 0 and by[0, 10, 10 + k] == 1 and by[0, 1420, 1780] == 0 and by[0, 1000, 1064] == 0
    assert by[0, 0, len(seqs[0])] == min(s, len(lt.hashes(seqs[0], k))) and 0 < by[0, 850, 1500] <= s


def test_2500_elements_in_one_call(ctx):
    rng = random.Random(9)
    seqs = [lt.rand_seq(rng, 5000), lt.rand_seq(rng, 3000)]
    el = []
    for _ in range(2500):
        c = rng.randrange(2)
        a = rng.randrange(0, len(seqs[c]) - 90)
        el.append((c, a, a + rng.randrange(1, 90)))
    load(ctx, seqs)
    want_sk, want_ln = lt.sketches([seqs[c][a:b] for c, a, b in el], 13, 16)
    chrom, start, end = (np.array(x) for x in zip(*el))
    sk, ln = ctx.ltr_sketch(chrom, start, end, 13, 16)
    assert (ln == want_ln).all() and (sk == want_sk).all()
    e_sk, e_ln = ctx.ltr_sketch(chrom[:0], start[:0], end[:0], 13, 16)      # n = 0 is fine
    assert e_sk.shape == (0, 16) and e_ln.shape == (0,)


# ---------------------------------------------------------------------------------------------- pairs
def test_pair_cases(ctx):
    for s in (64, 16):
        group = [c for c in cases.pair_cases() if c[3] == s]
        sk, ln = np.full((2 * len(group), s), lt.NONE, np.uint64), np.zeros(2 * len(group), np.int32)
        for q, (_, a, b, _, _) in enumerate(group):
            for row, x in ((2 * q, a), (2 * q + 1, b)):
                sk[row, :len(x)], ln[row] = np.array(x, np.uint64), len(x)
        shared, denom = ctx.ltr_sketch_pairs(sk, ln)
        for q, (name, _, _, _, want) in enumerate(group):
            assert (int(shared[2 * q, 2 * q + 1]), int(denom[2 * q, 2 * q + 1])) == want, name
            assert (int(shared[2 * q + 1, 2 * q]), int(denom[2 * q + 1, 2 * q])) == want, name


@pytest.mark.parametrize("n,s", [(1, 16), (2, 16), (33, 16), (257, 16), (33, 1024), (5, 4096), (18, 100)])
def test_pairs_are_the_twin(ctx, n, s):
    sk, ln = cases.hand_sketches(n, s, 100 * n + s)
    want_sh, want_dn = lt.pairs(sk, ln, s)
    shared, denom = ctx.ltr_sketch_pairs(sk, ln)
    assert shared.dtype == denom.dtype == np.int32 and shared.shape == denom.shape == (n, n)
    assert (shared == want_sh).all() and (denom == want_dn).all()
    assert (np.diag(shared) == ln).all() and (np.diag(denom) == ln).all() and (shared == shared.T).all() and (denom == denom.T).all()


# ---------------------------------------------------------------------------------------------- neighbour joining
def _nj_check(ctx, name, D, modes):
    want = cases.nj_expected(name, D)
    for mode in modes:
        ctx.nj_set_mode(mode)
        got = ctx.nj_tree(D)
        assert got.dtype == np.int64 and got.shape == want.shape
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (name, mode, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
    return want


@pytest.mark.parametrize("name", [m[0] for m in cases.nj_matrices()])
def test_nj_is_the_twin_under_both_drivers(ctx, name):
    D = next(m[1] for m in cases.nj_matrices() if m[0] == name)
    _nj_check(ctx, name, D, (0, 1, 2))


@pytest.mark.parametrize("name", [m[0] for m in cases.nj_matrices((257,))])
def test_nj_257(ctx, name):
    D = next(m[1] for m in cases.nj_matrices((257,)) if m[0] == name)
    _nj_check(ctx, name, D, (1, 2))


def test_nj_1000_and_the_default_choice(ctx):
    ctx.prof_enable(True)
    try:
        for N, kernel, other in ((65, "nj_loop", "nj_join"), (257, "nj_join", "nj_loop"), (1000, "nj_join", "nj_loop")):
            ctx.prof_reset()
            name = "random-%d" % N
            _nj_check(ctx, name, lt.random_matrix(N, N), (0,))
            rep = ctx.prof_report()
            assert kernel in rep and other not in rep, sorted(rep)
            if kernel == "nj_join":
                assert rep["nj_join"]["calls"] == N - 2 == rep["nj_rowmin"]["calls"] and rep["nj_rowmin"]["grid"] == N
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("name", [t[0] for t in cases.tree_cases()])
def test_additive_trees(ctx, name):
    _, edges, D = next(t for t in cases.tree_cases() if t[0] == name)
    want = _nj_check(ctx, name, D, (1, 2))
    N = D.shape[0]
    assert ltrtree.splits(ltrtree.unrooted_edges(want), N) == {k: float(v) for k, v in ltrtree.splits(edges, N).items()}


@pytest.mark.parametrize("N", [33, 65, 257])
def test_guard_at_a_lowered_limit(ctx, N):
    name = "negative-%d" % N
    D = next(m[1] for m in cases.nj_matrices((N,)) if m[0] == name)
    want = cases.nj_expected(name, D)
    limit, join, top = lt.guard_limit(D)
    assert join < N - 3
    ctx.prof_enable(True)
    try:
        for mode in (1, 2):
            ctx.nj_set_mode(mode)
            ctx.nj_set_guard(limit)
            ctx.prof_reset()
            with pytest.raises(ValueError, match="a derived distance reached %d in magnitude" % limit):
                ctx.nj_tree(D)
            rep = ctx.prof_report()
            if mode == 2:      # every launch was enqueued; the ones behind the guard returned at once
                assert rep["nj_rowmin"]["calls"] == rep["nj_join"]["calls"] == N - 2 and rep["nj_last"]["calls"] == 1
            else:
                assert rep["nj_loop"]["calls"] == 1 and "nj_join" not in rep
            ctx.nj_set_guard(top + 1)      # a limit that is not reached changes nothing
            assert (ctx.nj_tree(D) == want).all()
            ctx.nj_set_guard(0)
            assert (ctx.nj_tree(D) == want).all()
    finally:
        ctx.prof_enable(False)
    for bad in (-1, (1 << 40) + 1):
        with pytest.raises(ValueError, match="sp_nj_set_guard"):
            ctx.nj_set_guard(bad)


def test_grids_are_the_problem_sizes(ctx):
    """no kernel of the unit caps its grid: one workgroup per element, per tile of the pair triangle's square, per row"""
    rng = random.Random(3)
    seq = lt.rand_seq(rng, 4000)
    load(ctx, [seq])
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        n = 700
        start = np.arange(n) * 5
        sk, ln = ctx.ltr_sketch(np.zeros(n, np.int32), start, start + 60, 13, 16)
        ctx.ltr_sketch_pairs(sk, ln)
        rep = ctx.prof_report()
        assert rep["lt_sketch"]["grid"] == n and rep["lt_pairs"]["grid"] == ((n + 15) // 16) ** 2
    finally:
        ctx.prof_enable(False)


# ---------------------------------------------------------------------------------------------- errors
def test_errors(ctx):
    rng = random.Random(2)
    seqs = [lt.rand_seq(rng, 70000), lt.rand_seq(rng, 100)]
    load(ctx, seqs)
    one = lambda c, a, b, k=13, s=16: ctx.ltr_sketch(np.array([c], np.int32), np.array([a]), np.array([b]), k, s)

    def good():
        sk, ln = one(1, 0, 100)
        assert ln.tolist() == [16] and (sk[0] == lt.sketches([seqs[1]], 13, 16)[0][0]).all()
    good()
    for args, text in (((1, 0, 100, 12), "k = 12"), ((1, 0, 100, 7), "k = 7"), ((1, 0, 100, 33), "k = 33"), ((1, 0, 100, 13, 15), "s = 15"),
                       ((1, 0, 100, 13, 4097), "s = 4097"), ((2, 0, 10), "chromosome 2 out of range"), ((-1, 0, 10), "out of range"),
                       ((1, 0, 101), "outside chromosome 1"), ((1, -1, 50), "outside chromosome 1"), ((1, 50, 50), "is empty"), ((1, 60, 50), "is empty"),
                       ((0, 0, 65537), "65537 bases")):
        with pytest.raises(ValueError, match=text):
            one(*args)
        good()
    assert one(0, 0, 65536)[1].tolist() == [16]      # the longest element that is taken
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="sp_ltr_sketch_set_chunk"):
            ctx.ltr_sketch_set_chunk(bad)
    with pytest.raises(ValueError, match="sp_nj_set_mode"):
        ctx.nj_set_mode(3)
    good()
    # pairs
    sk, ln = cases.hand_sketches(4, 16, 1)
    for bad_ln, text in ((np.array([17, 0, 0, 0], np.int32), "len = 17"), (np.array([0, -1, 0, 0], np.int32), "len = -1")):
        with pytest.raises(ValueError, match=text):
            ctx.ltr_sketch_pairs(sk, bad_ln)
    with pytest.raises(ValueError, match="s = 15"):
        ctx.ltr_sketch_pairs(sk[:, :15], np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="bytes"):      # more than 32 MiB of sketches
        ctx.ltr_sketch_pairs(np.zeros((1025, 4096), np.uint64), np.zeros(1025, np.int32))
    assert (ctx.ltr_sketch_pairs(sk, ln)[0] == lt.pairs(sk, ln, 16)[0]).all()
    # neighbour joining
    D = lt.random_matrix(1, 5)
    want = lt.nj_numpy(D)
    for change, text in ((lambda M: M.__setitem__((1, 2), M[1, 2] + 1), r"D\(1, 2\)"), (lambda M: M.__setitem__((3, 3), 1), r"D\(3, 3\)"),
                         (lambda M: (M.__setitem__((0, 4), 1 << 31), M.__setitem__((4, 0), 1 << 31)), "outside"),
                         (lambda M: (M.__setitem__((0, 4), -1), M.__setitem__((4, 0), -1)), "outside")):
        M = D.copy()
        change(M)
        with pytest.raises(ValueError, match=text):
            ctx.nj_tree(M)
        assert (ctx.nj_tree(D) == want).all()
    with pytest.raises(ValueError, match="1 slots"):
        ctx.nj_tree(np.zeros((1, 1), np.int64))
    with pytest.raises(ValueError, match="4097 slots"):
        ctx.nj_tree(np.zeros((4097, 4097), np.int64))
    assert (ctx.nj_tree(D) == want).all()
    # no genome
    ctx.genome_reset(1)
    with pytest.raises(ValueError, match="no packed sequence|no genome"):
        one(0, 0, 10)
    ctx.genome_add(0, seqs[1])
    assert one(0, 0, 100)[1].tolist() == [16]


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("seed", cases.PLANTED_SEEDS)
def test_planted_families(ctx, seed):
    """the twin alone meets the clade condition for these seeds: test_ltrtree_host.py checks that on the CPU"""
    chrom, el, fams, sk, ln, shared, denom, D, want = cases.planted_twin(seed)
    assert cases.families_are_clades(want, fams)
    load(ctx, [chrom])
    start, end = (np.array(x) for x in zip(*el))
    records, _ = ltrtree.build(ctx, np.zeros(len(el), np.int32), start, end, 13, 256)
    g_sk, g_ln = ctx.ltr_sketch(np.zeros(len(el), np.int32), start, end, 13, 256)
    assert (g_sk == sk).all() and (g_ln == ln).all()
    g_sh, g_dn = ctx.ltr_sketch_pairs(g_sk, g_ln)
    assert (g_sh == shared).all() and (g_dn == denom).all()
    assert (records == want).all() and cases.families_are_clades(records, fams)
    text = ltrtree.tree_text(records, ["e%d" % i for i in range(len(el))])
    assert text.count(",") == len(el) - 1 and text.endswith(";")


# ---------------------------------------------------------------------------------------------- the command line
def test_cli_denovo_with_the_tree(gpu_ctx, toy, tmp_path, caplog):
    import ltr_cases
    from test_gpu_ltrdetect import _cli
    labels = toy["labels"]
    seqs, _, elements = ltr_cases.plant_elements({lab: str(toy["seqs"][lab]) for lab in labels}, labels)
    base, log = _cli(gpu_ctx, toy, seqs, tmp_path / "tree", caplog, ["-ltr_denovo", "-ltr_tree", "-ltr_tree_sketch", "256"])
    for ext in (".ltr.tree.nwk", ".ltr.tree.map", ".ltr.tree.png"):
        assert os.path.exists(base + ext), (ext, log[-12:])
    rows = open(base + ".ltr.tree.map").read().splitlines()
    assert rows[0] == "label\tClade\tSubgenome" and len(rows) >= 5 and all(r.split("\t")[1] == "unknown" for r in rows[1:])
    listed = {r.split("\t")[0] for r in open(base + ".ltr.insert.data").read().splitlines()[1:]}
    assert {r.split("\t")[0] for r in rows[1:]} == listed
    nwk = open(base + ".ltr.tree.nwk").read()
    assert nwk.count(",") == len(rows) - 2 and nwk.endswith(";\n")
    assert any(m.startswith("LTR tree of %d elements (k = 13, 256 hashes)" % (len(rows) - 1)) for m in log)
    note = [m for m in log if m.startswith("Of modules 3-4")]
    assert len(note) == 1 and "the LTR trees" not in note[0] and "TEsorter classification and the circos figure" in note[0]
