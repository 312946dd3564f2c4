"""The inputs of the positional map tests (test_mappos_host.py, test_gpu_mappos.py): one small genome, a hand-made label
set, the bin / window geometries, one feature list and one interval list, and what tests/mappos_ref.py says about each.
Everything is cached per k (the genome holds a chromosome of k - 1 and one of k bases) and computed once.

Every case checks its own preconditions on the reference (the `assert`s below): where one fails, change the seed or
the layout, not the assertion."""
import functools

import numpy as np

import mappos_ref as ref
from test_gpu_map_runs import _keys_by_position

_B = np.frombuffer(b"ACGT", dtype=np.uint8)
SEG_LEN = 160
UNIT = 64
MAP_RANGE = 32768            # starts per workgroup pass of the bins walk (MAP_BLOCK x SP_UNIT, csrc/sp_mapslots.h)
MAP_LDS_ENTRIES = 1024       # its LDS histogram (csrc/sp_mapslots.h)


def lengths(k):
    """three ranges of MAP_RANGE starts (the last partial) | whole units, and unit offsets behind it | no k-mer | one | odd"""
    return [70_001, 4096, k - 1, k, 12_345]


# ------------------------------------------------------------------------------------------------------- (k, S)
BIN_KS = [(15, 3), (15, 5), (15, 9), (17, 3), (17, 5), (17, 9)]          # MAP_KERNELS of test_gpu_cu_limit.py
RANGE_KS = [(15, 3), (15, 9), (17, 3), (17, 9), (15, 5), (17, 5)]        # FEATURE_KERNELS of it, and the S = 5 tables
WINDOW_KS = [(15, 3), (17, 3)]
# the kernels of feature and interval mode at S = 5 (direct pair table, pair-keyed hash table): the dispatch of
# map_feat_launch / map_mask_launch names them like the S = 3 tables'
RANGE_KERNELS_S5 = {(15, 5): ["k5_map_feat", "k5_map_mask"], (17, 5): ["k5_map_feat_sparse", "k5_map_mask_sparse"]}


# ----------------------------------------------------------------------------------------------------- the genome
@functools.lru_cache(maxsize=None)
def genome(k):
    """(chromosomes as uint8 arrays, the three segments).  A random background densely planted with copies of the
    segments (whole, cut short, at every residue of the unit), runs of N, a lower-case stretch, and a copy at the
    first and the last base of every chromosome that can hold one."""
    rng = np.random.RandomState(4200 + k)
    segs = [_B[rng.randint(0, 4, size=SEG_LEN)] for _ in range(3)]
    out = []
    for ci, L in enumerate(lengths(k)):
        s = _B[rng.randint(0, 4, size=L)]
        p = 0
        while p + SEG_LEN < L:                         # copies of 40 .. 160 bases, gaps of 17 .. 140: about half the starts hit
            seg = segs[rng.randint(3)]
            ln = SEG_LEN if rng.rand() < 0.7 else int(rng.randint(40, SEG_LEN))
            o = int(rng.randint(0, SEG_LEN - ln + 1))
            s[p:p + ln] = seg[o:o + ln]
            p += ln + int(rng.randint(17, 141))
        if L > 66_000:
            # copies across starts 30 000 (a chunk boundary of the list), 32 768 and 65 536 (the walk's ranges), 5000 k
            for q in (5000, 10_000, 30_000, 32_768, 60_000, 65_536):
                s[q - 80:q + 80] = segs[q % 3]
            s[1000:1050] = ord("N")                    # a run of N, single ones inside and at the edge of copies
            s[[5003, 29_950, 32_790, 40_000, 40_001]] = ord("N")
            s[20_000:20_400] |= 0x20                   # a lower-case stretch: maps like upper case
        if L >= SEG_LEN:
            s[:SEG_LEN] = segs[ci % 3]
            s[L - SEG_LEN:] = segs[(ci + 1) % 3]
            if L == 12_345:
                s[6000:6003] = ord("n")
                s[7000:7100] |= 0x20
        else:                                          # k - 1 and k bases: the head of a segment
            s[:] = segs[0][:L]
        out.append(s)
    return out, segs


@functools.lru_cache(maxsize=None)
def labels(k, S):
    """every k-mer of the three segments; label = (3 x segment + quarter of the segment the k-mer starts in) mod S, so
    that every column of up to nine has hits"""
    _, segs = genome(k)
    n = SEG_LEN - k + 1
    keys = np.concatenate([_keys_by_position(g, k) for g in segs])
    lab = np.concatenate([(3 * i + np.arange(n) // 40) % S for i in range(3)]).astype(np.uint8)
    keys, first = np.unique(keys, return_index=True)
    return keys, lab[first]


@functools.lru_cache(maxsize=None)
def hits(k, S):
    """per chromosome (label, key index) of every start; the case's preconditions on them"""
    seqs, _ = genome(k)
    keys, lab = labels(k, S)
    out = [ref.hits(s, k, keys, lab) for s in seqs]
    n_starts = sum(h[0].size for h in out)
    n_hit = sum(int((h[0] >= 0).sum()) for h in out)
    assert 0.4 * n_starts < n_hit < 0.6 * n_starts, (n_hit, n_starts)
    for (la, _), L in zip(out, lengths(k)):
        assert la.size == max(0, L - k + 1)
        if L >= k:                 # the first and the last start: the first and last slot, window and unit that can have a hit
            assert la[0] >= 0 and la[-1] >= 0
    la = out[0][0]
    for edge in (MAP_RANGE, 2 * MAP_RANGE):
        assert la[edge - 1] >= 0 and la[edge] >= 0
    assert (out[0][0][20_000:20_400 - k] >= 0).any() and (out[0][0][1000 - k + 1:1050] < 0).all()      # lower case maps, N does not
    assert set(np.concatenate([h[0] for h in out]).tolist()) == set(range(-1, min(S, 9)))       # every column is used
    return out


# ---------------------------------------------------------------------------------------------------------- bins
def lds_edge(S):
    """the two bin sizes either side of map_params_of's LDS rule at chunk 0: MAP_RANGE / bin + 3 entries times S against
    MAP_LDS_ENTRIES.  (the largest bin whose table does not fit, the smallest whose table does)"""
    fits = [b for b in range(1, MAP_RANGE) if (MAP_RANGE // b + 3) * S <= MAP_LDS_ENTRIES]
    return fits[0] - 1, fits[0]


# as the constants stand: the values the walk was reviewed with; a change of MAP_BLOCK or MAP_LDS_ENTRIES moves them
assert [lds_edge(S) for S in (3, 5, 9)] == [(96, 97), (162, 163), (295, 296)]

BIN_GEOMS = [(10_000, 10_000_000), (1, 0), (37, 5000), (100, 2000), (1000, 40), (100_000, 0), (100_000, 30_000)]


def bin_geoms(S):
    return BIN_GEOMS + [(b, 0) for b in lds_edge(S)]


# (the last one is not the issue's: every chunk's first start j W - (k - 1) is a multiple of the bin at k = 15 and 17, so
# every chunk boundary leaves a slot that no start maps to between the two chunks' slots, and two windows out of three
# begin inside a bin)
WINDOW_GEOMS = [(37, 5000, 1000), (64, 0, 64), (100, 1000, 50), (1000, 40, 100_000), (10_000, 10_000_000, 15_000), (163, 0, 1),
                (2, 1000, 3)]
CHUNK_LIST = [0, 40, 1000, 5000, 30_000, 10_000_000]      # the window table of a (bin, window) is the same under each
CHUNK_FREE = (100, 250)


def _check_chunk_edges(k, S, W):
    """a geometry whose chunk boundary lies inside a chromosome has hits at j W - k (the last start of chunk j - 1) and
    at j W - (k - 1) (the first of chunk j) for some j.  (10 Mb chunks: no boundary inside this genome, nothing to check.)"""
    assert W == 0 or W >= k
    la = hits(k, S)[0][0]
    if W and W < la.size:
        j = np.arange(1, (la.size + k - 1) // W + 1)
        j = j[j * W - (k - 1) < la.size]
        assert ((la[j * W - k] >= 0) & (la[j * W - (k - 1)] >= 0)).any(), W


@functools.lru_cache(maxsize=None)
def bins_expected(k, S, bin_size, W):
    """per chromosome the [rows, S] table and n_mapped; the distinct keys hit (bins mode counts every hit)"""
    _check_chunk_edges(k, S, W)
    tabs = [ref.bins(la, L, k, S, bin_size, W) for (la, _), L in zip(hits(k, S), lengths(k))]
    for t, (la, _) in zip(tabs, hits(k, S)):
        assert int(t.sum()) == int((la >= 0).sum())
    return tabs, [int(t.sum()) for t in tabs], labels_hit_all(k, S)


def labels_hit_all(k, S):
    return int(np.unique(np.concatenate([ix[ix >= 0] for _, ix in hits(k, S)])).size)


# -------------------------------------------------------------------------------------------------------- windows
def window_offsets(k, window, seg=None):
    """row offsets of the chromosomes: ceil((seg + L) / window) + 1 rows each"""
    seg = seg or [0] * 5
    return np.concatenate(([0], np.cumsum([ref.window_rows(g + L, window) for g, L in zip(seg, lengths(k))]))).astype(np.int64)


def seg_starts(bin_size, multiple):
    """where base 0 of each local chromosome lies in the chromosome it is a piece of"""
    m = [3, 0, 1, 7, 12]
    return [x * bin_size + (0 if multiple else (1 + 5 * i) % bin_size if bin_size > 1 else 0) for i, x in enumerate(m)]


@functools.lru_cache(maxsize=None)
def windows_expected(k, S, bin_size, window, seg=None):
    """(the [rows, S] table over all chromosomes, its row offsets); seg: tuple of seg_start or None"""
    woff = window_offsets(k, window, seg)
    seg = seg or (0,) * 5
    tab = np.concatenate([ref.windows(la, S, bin_size, window, int(woff[i + 1] - woff[i]), seg[i])
                          for i, (la, _) in enumerate(hits(k, S))])
    for i, (la, _) in enumerate(hits(k, S)):      # first and last window row that can have a hit
        if la.size:
            assert tab[woff[i] + seg[i] // window].any()
            assert tab[woff[i] + (seg[i] + (la.size - 1) // bin_size * bin_size) // window].any()
    return tab, woff


# ------------------------------------------------------------------------------------------------------- features
@functools.lru_cache(maxsize=None)
def features(k):
    """(chrom, start, end) of the features as sub-sequences of the genome, back to back in one buffer: empty ones first,
    last, in the middle and two in a row; k - 1, k, k + 1 bases; boundaries at unit offsets 0 (position 64 and 192), 1 and
    63; one of more than three units; a lower-case base before and an N behind a boundary; 712 + 3 k bases in all"""
    L0 = lengths(k)[0]
    f = [(0, 10, 10),                    # empty, first
         (0, 0, 64),                     # ends at position 64: unit offset 0
         (0, 64, 129),                   # ends at 129: unit offset 1     (these three follow one another in the genome too:
         (0, 129, 191),                  # ends at 191: unit offset 63     the k-mers across their boundaries are labelled)
         (0, 9950, 9951),                # one base, ends at 192
         (1, 5, 5), (4, 7, 7),           # two empty ones in a row
         (0, 5, 4 + k), (0, 4 + k, 4 + 2 * k), (0, 4 + 2 * k, 5 + 3 * k),      # (contiguous as well)
         (0, 32_700, 32_950),            # longer than three units
         (3, 0, 0),                      # empty, in the middle
         (0, 20_300, 20_400),            # its last base is lower case
         (0, 5003, 5103),                # its first base is N
         (0, L0 - 70, L0),
         (2, 0, 0)]                      # empty, last
    chrom, st, en = (np.array(x) for x in zip(*f))
    off = np.concatenate(([0], np.cumsum(en - st))).astype(np.int64)
    assert off[-1] == 712 + 3 * k and off[-1] % UNIT != 0
    assert [int(off[i]) % UNIT for i in (2, 3, 4, 5)] == [0, 1, 63, 0]
    return chrom.astype(np.int32), st.astype(np.int64), en.astype(np.int64), off


def cut(k, chrom, st, en):
    seqs, _ = genome(k)
    parts = [seqs[c][a:b] for c, a, b in zip(chrom, st, en)]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


@functools.lru_cache(maxsize=None)
def feature_buffers(k):
    """(cat, off) and the same features inside a longer buffer at off[0] = 77: 77 bases of a segment in front (they would
    hit if the entry did not rebase), 50 behind"""
    chrom, st, en, off = features(k)
    cat = cut(k, chrom, st, en)
    assert cat.size == off[-1]
    _, segs = genome(k)
    return cat, off, np.concatenate([segs[0][:77], cat, segs[1][:50]]), off + 77


@functools.lru_cache(maxsize=None)
def features_expected(k, S):
    """([n, S] counts, n_mapped, labels_hit) of the feature list through the reference, on the buffer itself"""
    cat, off, _, _ = feature_buffers(k)
    keys, lab = labels(k, S)
    la, ix = ref.hits(cat, k, keys, lab)
    cnt, inside = ref.ranges(la, k, S, off[:-1], off[1:])
    n, seen = ref.totals(la, ix, inside)
    ln = np.diff(off)
    assert cnt[ln == k].sum() == 1 and cnt[ln == k + 1].sum() == 2 and not cnt[ln < k].any()
    assert cnt[1].any() and cnt[-2].any() and n == cnt.sum()          # the first and the last feature that can have a hit
    assert n < (la >= 0).sum()                                          # k-mers across a boundary hit and are not counted
    return cnt, n, int(seen.size)


# ------------------------------------------------------------------------------------------------------ intervals
@functools.lru_cache(maxsize=None)
def intervals(k):
    """intervals on all five chromosomes: start & 63 in {0, 1, 63}; (end - k + 1) & 63 in {0, 1, 63}; 0, k - 1, k, k + 1
    bases; one of 10 000 bases (more than 64 units: a lane of the wave takes a second one); duplicated, nested and
    overlapping ones; ends on the last base of the 4096- and the 12 345-base chromosome; the k - 1 and k chromosomes"""
    e = k - 1                        # end = b + k - 1 for a range of starts [a, b)
    L = lengths(k)
    iv = [(0, 128, 256 + e), (0, 129, 257 + e), (0, 191, 319 + e), (0, 129, 257 + e),      # (the second one twice)
          (0, 0, 64 + e),                                                                  # exactly one whole unit
          (0, 3, 3), (0, 3, 3 + k - 1), (0, 3, 3 + k), (0, 3, 3 + k + 1),
          (0, 30_000, 40_000), (0, 32_700, 32_900), (0, 32_800, 33_000), (0, 0, L[0]),
          (1, 0, 4096), (1, 4032, 4096), (1, 3969, 4032 + e), (1, 63, 64 + e), (1, 4096 - k, 4096), (1, 4096, 4096),
          (2, 0, k - 1), (2, 0, 0), (2, 1, k - 1),
          (3, 0, k), (3, 0, k - 1), (3, 1, k),
          (4, 0, L[4]), (4, L[4] - k, L[4]), (4, L[4] - 100, L[4]), (4, 64, 128 + e), (4, 63, 200), (4, 6000 - k, 6003 + k)]
    chrom, st, en = (np.array(x) for x in zip(*iv))
    assert {int(a) & 63 for a in st} >= {0, 1, 63} and {int(b - k + 1) & 63 for b in en} >= {0, 1, 63}
    assert {int(b - a) for a, b in zip(st, en)} >= {0, k - 1, k, k + 1} and (en - st).max() > 8192
    assert all(0 <= a <= b <= L[c] for c, a, b in iv)
    return chrom.astype(np.int32), st.astype(np.int64), en.astype(np.int64)


@functools.lru_cache(maxsize=None)
def ranges_expected(k, S, which):
    """([n, S] counts, labels_hit) of an interval list -- `which`: "intervals", or "features" for the feature list read as
    intervals of the genome -- through the reference, chromosome by chromosome"""
    chrom, st, en = intervals(k) if which == "intervals" else features(k)[:3]
    cnt = np.zeros((chrom.size, S), np.int64)
    seen = []
    for c, (la, ix) in enumerate(hits(k, S)):
        sel = np.flatnonzero(chrom == c)
        cnt[sel], inside = ref.ranges(la, k, S, st[sel], en[sel])
        seen.append(ref.totals(la, ix, inside)[1])
    if which == "intervals":
        assert cnt[chrom == 3].sum(axis=1).tolist() == [1, 0, 0] and not cnt[chrom == 2].any()
        assert cnt[(chrom == 1) & (en == 4096) & (en > st)].all(axis=0).any() and cnt[4].any()
    return cnt, int(np.unique(np.concatenate(seen)).size)
