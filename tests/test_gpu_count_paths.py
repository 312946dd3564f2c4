"""Engine 2 (the dense count chain) where its kernels change path: the wave-uniform fast paths of c2_part1 / c2_part2 next to
their masked slow paths, pad records and short tiles in c2_part2, and the two-counters-per-word write-out of c2_count16 at its
thresholds.  Everything is compared with the oracle's dump (k-mers and counts, bit for bit) and `lengths()`.

A part1 tile is 512 threads x 32 starts = 16384 starts; a thread owns one unit of 32 starts, a wave 64 units.  A single N at
base p spoils the starts p-k+1 .. p, so with p % 32 >= k - 1 exactly one lane of one wave leaves the fast path."""
import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu

TILE = 512 * 32
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _acgt(rng, n, letters=4):
    return ACGT[rng.randint(0, letters, size=n)].copy()


def _with_n(seq, *pos):
    s = seq.copy()
    for p in pos:
        s[p] = ord("N")
    return s


def _count_both(ctx, seqs, k, lower, engine=2):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)
    ctx.count(k, lower, engine)
    out = []
    for i, s in enumerate(seqs):
        gk, gc = ctx.dump(i)
        ok, oc = po.count(s, k, lower, nthreads=4)
        assert gk.shape == ok.shape, (k, lower, i, gk.shape, ok.shape)
        assert (gk == ok).all() and (gc == oc).all(), (k, lower, i)
        out.append((gk, gc))
    assert ctx.lengths().tolist() == [int(c.astype(np.int64).sum()) for _, c in out]
    return out


@pytest.mark.parametrize("batch", ["1", "0"])
@pytest.mark.parametrize("k", [12, 14, 15])
def test_part1_fast_and_slow_path_seams(gpu_ctx, monkeypatch, k, batch):
    """Three-tile all-ACGT chromosomes of 512 x 32 x 3 + {0, 1, 31, 32, 33} bases (the last unit full, one start, 31, 32 + a
    new unit); one N that takes exactly one lane out of one wave: the first and the last lane of a wave, the last unit of the
    chromosome, k-1 bases before a unit boundary, the first base; a chromosome shorter than one tile (every part2 sub-region a
    short tile) and an empty one next to the long ones.  Batched and per-chromosome launches."""
    monkeypatch.setenv("SP_C2_BATCH", batch)
    rng = np.random.RandomState(1000 + k)
    seqs = [_acgt(rng, 3 * TILE + extra) for extra in (0, 1, 31, 32, 33)]
    base = _acgt(rng, 3 * TILE + 33)
    off = 20                                         # >= k - 1 for k <= 15: the spoiled starts stay inside the unit
    wave = TILE + 5 * 2048                           # a wave of the second tile
    seqs += [_with_n(base, wave + 0 * 32 + off),     # first lane of a wave
             _with_n(base, wave + 63 * 32 + off),    # last lane of a wave
             _with_n(base, 3 * TILE + off),          # the last unit (one start of its own is left behind it)
             _with_n(base, len(base) - 1),           # the last base
             _with_n(base, wave + 7 * 32 + 32 - (k - 1)),   # k-1 bases before a unit boundary
             _with_n(base, wave + 7 * 32 + 3),       # spoils starts of two units: two lanes
             _with_n(base, 0),
             np.frombuffer(b"", np.uint8), _acgt(rng, 5000), _acgt(rng, k), _acgt(rng, k - 1)]
    _count_both(gpu_ctx, seqs, k, 1)
    _count_both(gpu_ctx, seqs[5:9] + seqs[-4:], k, 3)


def test_part1_several_tiles_per_block(gpu_ctx):
    """36 Mb of plain ACGT: more part1 tiles than the launch has blocks (eight per CU), so blocks loop over tiles with the next
    tile's words prefetched across the fast path; one N at the first lane of a wave in the middle, one in the last tile."""
    rng = np.random.RandomState(1515)
    n = 2200 * TILE + 17
    big = _with_n(_acgt(rng, n), 1100 * TILE + 3 * 2048 + 20, 2199 * TILE + 63 * 32 + 31)
    _count_both(gpu_ctx, [big, np.frombuffer(b"", np.uint8), _acgt(rng, 70_001)], 15, 3)


@pytest.mark.parametrize("k", [9, 14, 15])
def test_part2_pads_and_short_tiles(gpu_ctx, k):
    """Random sequence: the runs a part1 tile writes have every length modulo 4, so the level-1 regions part2 reads are full of
    pad records (full tiles: the unconditional path with its branch-free pads) and end in short tiles; 1 % of other letters keep
    part1's slow path busy next to them; the small chromosomes are one short tile per sub-region."""
    rng = np.random.RandomState(2000 + k)
    a = _acgt(rng, 1_300_003)
    b = _acgt(rng, 400_001)
    m = rng.random_sample(len(b)) < 0.01
    b[m] = ord("N")
    seqs = [a, b, _acgt(rng, 3000), _acgt(rng, 64), _acgt(rng, 6 * 24 * 256 + 1)]
    _count_both(gpu_ctx, seqs, k, 1)
    _count_both(gpu_ctx, seqs, k, 2)


def _repeat(kmer, copies):
    """`copies` occurrences of one k-mer and of nothing else (an N behind every copy)"""
    return np.tile(np.concatenate([kmer, np.frombuffer(b"N", np.uint8)]), copies)


@pytest.mark.parametrize("k", [9, 14, 15])
def test_count16_write_out_thresholds(gpu_ctx, k):
    """Counters exactly at lower-1, lower, 254, 255, 256, 65535 and past 65535 (the wrap + recount path) in the two halves of ONE
    counter word: the k-mers A..A + tag + A and A..A + tag + C are their own representatives (a leading A against a revcomp that
    starts with T or G; for odd k the base that holds bit k is an A) and differ in the lowest slot bit only.  Every `lower` the
    write-out distinguishes: 1, 2, 3 (the bench's), 255 / 256 (the byte saturation) and 40000 (above 0x8000: the per-slot path)."""
    rng = np.random.RandomState(3000 + k)
    tags = [b"CGT", b"GTC", b"TCG", b"CCT", b"GGA", b"TTC", b"CTG", b"GAC"]
    lowers = (1, 2, 3, 255, 256, 40000) if k != 9 else (3, 255)      # (k = 9 runs the saturated bucket below as well)
    pairs = [(254, 255), (255, 256), (256, 254), (1, 2), (2, 3), (39999, 40000), (65535, 253), (65535, 65536), (70000, 65535)]
    # (a pair per (tag, base in front of the tag): 8 x 2 >= 9 distinct prefixes)
    parts = [_acgt(rng, 50_000)]
    for i, (c0, c1) in enumerate(pairs):
        head = b"A" * (k - 5) + (b"A" if i < 8 else b"C") + tags[i % 8]
        for last, copies in ((b"A", c0), (b"C", c1)):
            parts.append(_repeat(np.frombuffer(head + last, np.uint8), copies))
    seq = np.concatenate(parts)
    small = np.concatenate([_acgt(rng, 20_000), _repeat(np.frombuffer(b"A" * (k - 4) + b"GCTA", np.uint8), 254),
                            _repeat(np.frombuffer(b"A" * (k - 4) + b"GCTC", np.uint8), 255)])
    for lower in lowers:
        out = _count_both(gpu_ctx, [seq, small], k, lower)
        if lower == 1 and k == 15:     # the construction holds (at smaller k the random flank may add a copy or two)
            assert {253, 254, 255, 256, 65535, 65536, 70000, 39999, 40000} <= set(out[0][1].tolist())
    if k == 9:
        # thousands of saturated slots in one bucket: 3^9 k-mers over {A, C, G} share 8 Mb, about 400 copies each, in four fine
        # buckets of 2 M records (16-bit counters that could wrap but do not)
        sat = _acgt(rng, 8_000_000, letters=3)
        for lower in (3, 255):
            out = _count_both(gpu_ctx, [sat, _acgt(rng, 5000)], k, lower)
        assert int((out[0][1] >= 255).sum()) > 4000
