"""GPU: what the five device k-mer tests share -- the narrow and the wide t-test (sp_enrich.hip), kruskal and mannwhitneyu
(sp_ranktest.hip) and wilcoxon (sp_wilcoxon.hip) all stage the rows, lay out one workspace (Context b_tt), order the
groups by mean and return means / top / second the same way (csrc/sp_kmertest.h).  Looked at across the entries:

  agreement   means, top and second of the five ways are ==, byte for byte (groups of fewer than 8 chromosomes: numpy's
              sum and the wide kernel's left-to-right order key coincide); p-values are each test's own
  64 threads  kruskal at N = 66 and wilcoxon at 2n = 66 run on their 64-thread launch; the same three arrays as k7_ttest
  workspace   one context through calls that grow the workspace, use a corner of it, and add their own arrays behind
              the common ones: every result equals the same call on a fresh context
  staging     staged rows (stage_rows) and host rows give the same bytes, every way
  codes       the return codes of the two t-test entries through raw ctypes; a length of 0 is no error for them
  lengths     a lengths vector of the wrong size is a ValueError from all four wrappers"""
import ctypes

import numpy as np
import pytest

from subphaser_amd import _native

pytestmark = pytest.mark.gpu

WAYS = {
    "ttest_ind": lambda ctx, c, l, g: ctx.kmer_ttest(c, l, g),
    "ttest_wide": lambda ctx, c, l, g: ctx.kmer_ttest_wide(c, l, g),
    "kruskal": lambda ctx, c, l, g: ctx.kmer_ranktest(c, l, g, "kruskal"),
    "mannwhitneyu": lambda ctx, c, l, g: ctx.kmer_ranktest(c, l, g, "mannwhitneyu"),
    "wilcoxon": lambda ctx, c, l, g: ctx.kmer_wilcoxon(c, l, g),
}


def _case(M, sizes, seed, interleave=True):
    """Poisson-like counts with some all-zero rows, distinct lengths; group g of sizes[g] chromosomes, interleaved"""
    rng = np.random.default_rng(seed)
    C = sum(sizes)
    counts = rng.poisson(rng.uniform(2, 40, size=(M, 1)) * rng.uniform(0.5, 2, size=(M, C))).astype(np.uint32)
    lengths = (1000 + 37 * np.arange(C)).astype(np.int64)
    order = rng.permutation(C) if interleave else np.arange(C)
    at = np.concatenate([[0], np.cumsum(sizes)])
    groups = [order[at[g]:at[g + 1]].tolist() for g in range(len(sizes))]
    for g, chroms in enumerate(groups):                   # every group is the top one on some rows
        counts[np.ix_(np.arange(g, M, len(groups)), chroms)] *= 5
    counts[::11] = 0
    return counts, lengths, groups


def _bytes(res):
    return [a.tobytes() for a in res]


@pytest.fixture(scope="module")
def small():
    return _case(129, (3, 3), 1)


@pytest.fixture(scope="module")
def small_results(gpu_ctx, small):
    return {w: f(gpu_ctx, *small) for w, f in WAYS.items()}


def test_the_five_ways_agree_on_means_top_second(small, small_results):
    counts, lengths, groups = small
    top, second, p, means = small_results["ttest_ind"][:4]
    assert means.shape == (129, 2) and set(top.tolist()) == {0, 1} and (counts.sum(axis=1) == 0).sum() >= 10
    for w, got in small_results.items():
        assert len(got) == (4 if w.startswith("ttest") else 5), w
        assert got[0].tobytes() == top.tobytes() and got[1].tobytes() == second.tobytes(), w
        assert got[3].tobytes() == means.tobytes(), w


def test_the_64_thread_launches_agree_with_the_narrow_ttest(gpu_ctx):
    counts, lengths, groups = _case(65, (33, 33), 2)
    top, second, p, means = gpu_ctx.kmer_ttest(counts, lengths, groups)
    assert set(top.tolist()) == {0, 1}
    for w in ("kruskal", "wilcoxon"):
        got = WAYS[w](gpu_ctx, counts, lengths, groups)
        assert got[0].tobytes() == top.tobytes() and got[1].tobytes() == second.tobytes(), w
        assert got[3].tobytes() == means.tobytes(), w


def test_one_workspace_through_growing_and_shrinking_calls():
    calls = [("wilcoxon", _case(300, (4, 4, 4), 3)), ("ttest_ind", _case(1, (3, 3), 4)),
             ("mannwhitneyu", _case(300, (8, 9), 5)), ("ttest_wide", _case(65, (65, 1), 6))]
    shared = _native.Context(0)
    try:
        got = [_bytes(WAYS[w](shared, *case)) for w, case in calls]
    finally:
        shared.close()
    for (w, case), g in zip(calls, got):
        fresh = _native.Context(0)
        try:
            assert _bytes(WAYS[w](fresh, *case)) == g, w
        finally:
            fresh.close()


@pytest.mark.parametrize("way", list(WAYS))
def test_staged_and_host_rows_give_the_same_bytes(gpu_ctx, small, small_results, way):
    counts, lengths, groups = small
    staged = gpu_ctx.stage_rows(counts)
    try:
        again = WAYS[way](gpu_ctx, staged, lengths, groups)
    finally:
        gpu_ctx.release_rows()
    assert _bytes(again) == _bytes(small_results[way])


@pytest.mark.parametrize("entry,limit", [("sp_kmer_ttest", 64), ("sp_kmer_ttest_wide", 65536)])
def test_ttest_error_codes_and_null_pointers(gpu_ctx, entry, limit):
    vp = ctypes.c_void_p
    C = 65540
    counts, lengths = np.ones((2, C), np.uint32), np.full(C, 9, np.int64)
    gch = np.arange(C, dtype=np.int32)
    ok = np.array([0, 3, 67], np.int32)
    top, sec, p, means = np.empty(2, np.int32), np.empty(2, np.int32), np.empty(2), np.empty((2, 2))
    ptr = lambda a: vp(a.ctypes.data) if a is not None else None
    fn = getattr(gpu_ctx.L, entry)

    def call(c=counts, l=lengths, off=ok, ch=gch, t=top, M=2):
        return fn(gpu_ctx.h, ptr(c), M, C, ptr(l), 2, ptr(off), ptr(ch), ptr(t), ptr(sec), ptr(p), ptr(means))
    assert call() == _native.SP_OK
    assert call(c=None) == _native.SP_EINVAL and call(l=None) == _native.SP_EINVAL
    assert call(off=None) == _native.SP_EINVAL and call(t=None) == _native.SP_EINVAL
    assert entry.encode() in gpu_ctx.L.sp_last_error(gpu_ctx.h)
    for bad in (C, -1):
        ch = gch.copy()
        ch[66] = bad
        assert call(ch=ch) == _native.SP_EINVAL
        assert b"out of range" in gpu_ctx.L.sp_last_error(gpu_ctx.h)
    assert call(off=np.array([0, 65, 67], np.int32)) == (_native.SP_EUNSUP if limit == 64 else _native.SP_OK)
    assert call(off=np.array([0, 65537, 65539], np.int32)) == _native.SP_EUNSUP
    assert b"65537" in gpu_ctx.L.sp_last_error(gpu_ctx.h)
    assert call(M=0) == _native.SP_OK and call(M=0, c=None, t=None) == _native.SP_OK
    zero = lengths.copy()
    zero[1] = 0
    assert call(l=zero) == _native.SP_OK                  # the t-tests divide by it; they do not reject it


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("delta", [1, -1])
def test_a_lengths_vector_of_the_wrong_size_is_refused(gpu_ctx, small, way, delta):
    counts, lengths, groups = small
    wrong = np.full(len(lengths) + delta, 1000, np.int64)
    with pytest.raises(ValueError, match="lengths for 6 chromosomes"):
        WAYS[way](gpu_ctx, counts, wrong, groups)
