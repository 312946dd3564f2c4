"""The hash families of the map stage (csrc/sp_maphash.h) on the device: at k <= 15 the pair filter's word and bits and the
compact table's bucket come from 24-bit multiplies, at k > 15 from the functions the filter has always had.  Whatever the
hashes are, the filter must have no false negatives and the table must stay exact, so every case maps a small chromosome
-- random bases, runs of N, copies of a "repeat" planted at all four residues of the position modulo 4 -- with EVERY k-mer of
the chromosome labelled (a single filter false negative or misplaced table key loses a hit) and again with a random 30 % of
them, and compares bin counts, n_mapped and the labelled k-mers seen with the oracle.  Equal, never close.  S = 2 and 3 use
the compact quad buckets, S = 5 the direct pair table."""
import functools

import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu

_B = np.frombuffer(b"ACGT", dtype=np.uint8)
N_BASES = 6000             # 94 units of 64 starts, the last one partly filled
BINS = ((1, 0), (7, 100))


@functools.lru_cache(maxsize=None)
def _chrom(k):
    rng = np.random.RandomState(4200 + k)
    s = _B[rng.randint(0, 4, size=N_BASES)]
    rep = _B[rng.randint(0, 4, size=90)]
    p = 300
    for i in range(12):                      # copies at every residue mod 4, three times over, at changing places of a unit
        p = (p + 63) // 64 * 64 + 17 * (i // 4) + i % 4
        s[p:p + rep.size] = rep
        p += rep.size + 2 * k
    for start, ln in ((0, 3), (1000, 1), (1003, 2), (2500, 70), (2700 + k, 1), (4001, 5), (N_BASES - 2, 2)):
        s[start:start + ln] = ord("N")       # single N, short runs, a run longer than a unit, N at both ends
    s[5000:5000 + rep.size] = rep            # one more copy, cut by an N inside it
    s[5040] = ord("N")
    return s


@functools.lru_cache(maxsize=None)
def _all_keys(k):
    keys, _ = po.count(_chrom(k), k, 1)
    assert keys.size > (500 if k > 5 else 400)
    return keys


@functools.lru_cache(maxsize=None)
def _labelled(k, S, share):
    """(keys, labels): every k-mer of the chromosome (share = 100) or a random `share` per cent of them"""
    keys = _all_keys(k)
    rng = np.random.RandomState(100 * k + 10 * S + share)
    if share < 100:
        keys = keys[rng.random_sample(keys.size) < share / 100.0]
    return keys, rng.randint(0, S, size=keys.size).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _expected(k, S, share):
    keys, lab = _labelled(k, S, share)
    out = []
    hit_all = np.zeros(keys.size, np.uint8)
    for bin_size, chunk in BINS:
        exp, hit, n = po.map_bins(_chrom(k), k, keys, lab, S, bin_size, chunk)
        hit_all |= hit
        out.append((exp, n))
    if share == 100:       # every valid start maps, and every labelled k-mer is seen
        assert out[0][1] > N_BASES - 40 * k and hit_all.all()
    return out, int(hit_all.sum())


def _check(ctx, k, S, engine):
    ctx.genome_reset(1)
    ctx.genome_add(0, _chrom(k))
    ctx.count(k, 1, engine)
    if k <= 15:
        assert (ctx.dump(0)[0] == _all_keys(k)).all()      # the labelled set IS the dumped set
    for share in (100, 30):
        keys, lab = _labelled(k, S, share)
        exp, exp_hit = _expected(k, S, share)
        ctx.labels_set(keys, lab, S)
        for (bin_size, chunk), (e, n_exp) in zip(BINS, exp):
            got, n = ctx.map_bins(0, bin_size, chunk)
            assert got.shape == e.shape, (share, bin_size)
            assert (got == e).all(), (share, bin_size, np.argwhere(got != e)[:5])
            assert n == n_exp, (share, bin_size)
        assert ctx.labels_hit() == exp_hit, share


@pytest.mark.parametrize("S", (2, 3, 5))
@pytest.mark.parametrize("k", range(5, 16))
def test_every_labelled_kmer_is_found(gpu_ctx, k, S):
    _check(gpu_ctx, k, S, 0)


@pytest.mark.parametrize("k,S", [(16, 2), (21, 3)])
def test_the_wide_family_still_answers(gpu_ctx, k, S):
    _check(gpu_ctx, k, S, 1)
