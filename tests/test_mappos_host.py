"""The positional reference (tests/mappos_ref.py) against the CPU oracle, before a GPU is involved: two independent
routes to the same tables.  The oracle computes the chunk of a start, and the chunk of a slot, from closed forms (the
kernels' own); the reference walks the chunks.  Equal, never close -- and the oracle's chunk inversion is pinned on the
way, at window and chunk sizes that are no multiples of the bin."""
import ctypes

import numpy as np
import pytest

import pyoracle as po
import mappos_cases as mc
import mappos_ref as ref
from oracle_ctx import OracleContext, OracleDistContext


def _oracle(k, S, cls=OracleContext):
    seqs, _ = mc.genome(k)
    o = cls(nthreads=1)
    o.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        o.genome_add(i, s)
    o.k = k
    o.labels_set(*mc.labels(k, S), S)
    return o


def test_reference_on_a_hand_made_sequence():
    """the reference against counts made by hand: ACGTACGTAC, k = 3, keys ACG (= CGT reversed) and TAC (= GTA)"""
    from subphaser_amd import kmer as km
    keys = np.array([km.encode("ACG"), km.encode("GTA")], np.uint64)       # both canonical, in key order
    lab = np.array([0, 1], np.uint8)
    la, ix = ref.hits(b"ACGTACGTAC", 3, keys, lab)         # ACG CGT GTA TAC ACG CGT GTA TAC
    assert la.tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    la, _ = ref.hits(b"acgtNCGTAC", 3, keys, lab)          # acg cgt  -   -   -  CGT GTA TAC
    assert la.tolist() == [0, 0, -1, -1, -1, 0, 1, 1]
    la, _ = ref.hits(b"ACGTACGTAC", 3, keys, lab)
    # chunks of 4 with 2 bases of overlap: [0,4) [2,8) [6,10): starts 0 1 | 2 3 4 5 | 6 7; bin 3 -> rows 0 0 | 1 2 2 2 | 4 4
    assert ref.chunks(10, 3, 4) == [(0, 4), (2, 8), (6, 10)]
    assert ref.bins(la, 10, 3, 2, 3, 4).tolist() == [[2, 0], [0, 1], [2, 1], [0, 0], [0, 2], [0, 0], [0, 0], [0, 0]]
    assert ref.n_rows(10, 3, 3, 4) == 8 == po.n_slots(10, 3, 4, 3)
    # windows of 4 over bins of 3: bin starts 0 0 0 3 3 3 6 6 -> rows 0 0 0 0 0 0 1 1
    assert ref.windows(la, 2, 3, 4, 4).tolist() == [[4, 2], [0, 2], [0, 0], [0, 0]]
    cnt, inside = ref.ranges(la, 3, 2, [0, 2, 4, 9], [3, 6, 4, 10])       # starts {0}, {2, 3}, {}, {}
    assert cnt.tolist() == [[1, 0], [0, 2], [0, 0], [0, 0]] and inside.tolist() == [True, False, True, True] + [False] * 4


@pytest.mark.parametrize("k,S", mc.BIN_KS)
def test_bins_reference_is_the_oracle(k, S):
    seqs, _ = mc.genome(k)
    keys, lab = mc.labels(k, S)
    for bin_size, W in mc.bin_geoms(S):
        tabs, n_exp, seen_exp = mc.bins_expected(k, S, bin_size, W)
        hit_all = np.zeros(keys.size, np.uint8)
        for s, t, n in zip(seqs, tabs, n_exp):
            got, hit, n_got = po.map_bins(s, k, keys, lab, S, bin_size, W, nthreads=1)
            hit_all |= hit
            assert t.shape[0] == po.n_slots(s.size, bin_size, W, k) == got.shape[0], (bin_size, W, s.size)
            assert (got == t).all(), (bin_size, W, s.size, np.argwhere(got != t)[:5])
            assert n_got == n
        assert int(hit_all.sum()) == seen_exp
        idx = np.unique(np.concatenate([ix[ix >= 0] for _, ix in mc.hits(k, S)]))
        assert (np.flatnonzero(hit_all) == idx).all()


@pytest.mark.parametrize("k,S", mc.WINDOW_KS)
def test_windows_reference_is_the_oracle(k, S):
    o = _oracle(k, S)
    for bin_size, W, window in mc.WINDOW_GEOMS:
        mc._check_chunk_edges(k, S, W)
        exp, woff = mc.windows_expected(k, S, bin_size, window)
        o.map_bins_all(bin_size, W)
        got, goff = o.stack_windows(bin_size, W, window, mc.lengths(k))
        assert (goff == woff).all() and got.shape == exp.shape, (bin_size, W, window)
        assert (got == exp).all(), (bin_size, W, window, np.argwhere(got != exp)[:5])


def test_windows_do_not_depend_on_the_chunks():
    """one (bin, window), every chunk size of the list: the same table, from the oracle's slots and its chunk inversion"""
    k, S = 15, 3
    bin_size, window = mc.CHUNK_FREE
    o = _oracle(k, S)
    exp, _ = mc.windows_expected(k, S, bin_size, window)
    for W in mc.CHUNK_LIST:
        mc._check_chunk_edges(k, S, W)
        o.map_bins_all(bin_size, W)
        got, _ = o.stack_windows(bin_size, W, window, mc.lengths(k))
        assert (got == exp).all(), (W, np.argwhere(got != exp)[:5])


@pytest.mark.parametrize("multiple", [True, False])
@pytest.mark.parametrize("k,S", mc.WINDOW_KS)
def test_windows_dev_reference_is_the_oracle(k, S, multiple):
    """OracleDistContext.stack_windows_dev with a seg_start (a multiple of the bin / not one): accumulated into the
    caller's table, so a second call doubles it"""
    o = _oracle(k, S, OracleDistContext)
    for bin_size, W, window in mc.WINDOW_GEOMS:
        seg = tuple(mc.seg_starts(bin_size, multiple))
        assert all(g % bin_size == 0 for g in seg) == (multiple or bin_size == 1)
        exp, woff = mc.windows_expected(k, S, bin_size, window, seg)
        o.map_bins_all(bin_size, W)
        tab = np.zeros(exp.shape, np.int64)
        for rep in (1, 2):
            o.stack_windows_dev(bin_size, W, window, woff[:-1], seg, tab.ctypes.data_as(ctypes.c_void_p).value)
            assert (tab == rep * exp).all(), (bin_size, W, window, rep, np.argwhere(tab != rep * exp)[:5])


@pytest.mark.parametrize("k,S", mc.RANGE_KS)
def test_features_and_intervals_reference_is_the_oracle(k, S):
    cat, off, cat77, off77 = mc.feature_buffers(k)
    exp, n, seen = mc.features_expected(k, S)
    o = _oracle(k, S)
    got = o.map_features_cat(cat, off)
    assert (got == exp).all() and o.labels_hit() == seen
    assert (o.map_features_cat(cat77, off77) == exp).all()
    chrom, st, en, _ = mc.features(k)
    exp_iv, seen_iv = mc.ranges_expected(k, S, "features")
    assert (exp_iv == exp).all() and seen_iv == seen          # the same sub-sequences, cut from the genome
    o = _oracle(k, S)
    assert (o.map_intervals(chrom, st, en) == exp).all() and o.labels_hit() == seen
    chrom, st, en = mc.intervals(k)
    exp, seen = mc.ranges_expected(k, S, "intervals")
    o = _oracle(k, S)
    assert (o.map_intervals(chrom, st, en) == exp).all() and o.labels_hit() == seen
