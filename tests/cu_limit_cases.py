"""Seeded inputs and oracle results of tests/test_gpu_cu_limit.py, built once per limit and shared, never changed.

A context made under SP_CU_LIMIT=n caps its grids at n x {1/2 .. 64} workgroups.  The genome of limit n is three
chromosomes sized from the two caps that need the most sequence, those of the map walk (16 n ranges of 32 768 starts)
and of the pack kernel (64 n workgroups of 8192 bases):

    limit 1:   655 365    450 001    370 007 bases    21 + 14 + 12 = 47 ranges >= 2 * 16 + 1
    limit 3: 1 638 405  1 000 003    700 001 bases    51 + 31 + 22 = 104 ranges >= 2 * 48 + 1

so the one k5_map launch of map_bins_all gives some workgroup three ranges, and the launches that work on one
chromosome at a time (k5_map_lab, k5_map_sparse, k5_map_mask, k0_pack, the count chains) find more than a full grid in
chromosome 0.  No length is a multiple of 64 or of 32 768; chromosome 0 ends five bases after a range boundary.  The
content is test_gpu_parity's _rand_seq (lower case, IUPAC codes and other invalid bytes) with planted repeat families as
in its medium-scale test, so that the filter keeps rows and the map has hits: two libraries of 8 x limit families of
600 bases, a copy every 3000 bases -- 14 000 / 40 000 list entries, which the join cuts into 32 / 64 key ranges for its
16 x limit workgroups."""
import numpy as np

import pyoracle as po
from test_gpu_parity import _rand_seq

LIMITS = (1, 3)
LENGTHS = {1: (32768 * 20 + 5, 450_001, 370_007), 3: (32768 * 50 + 5, 1_000_003, 700_001)}
LOWER = 3
FILTER_ARGS = (2.0, 1, 10, 1e9, 1.0)       # min_fold, baseline, min_freq, max_freq, ratio
MAP_SHAPES = ((10000, 10_000_000), (333, 50_000), (64, 0))      # (bin_size, chunk_size)
# one chromosome for the pack stage: 129 / 385 workgroups' worth of mask words (256 words of 32 bases each) and an odd tail
PACK_LENGTH = {1: 32 * 256 * 129 + 1037, 3: 32 * 256 * 385 + 1037}

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (tuple, list)):
        for y in x:
            _freeze(y)
    return x


def genome(limit):
    def make():
        rng = np.random.RandomState(4200 + limit)
        fams = [[_rand_seq(rng, 600, 0, 0) for _ in range(8 * limit)] for _ in range(2)]
        seqs = []
        for c, n in enumerate(LENGTHS[limit]):
            s = _rand_seq(rng, n, 0.0005, 0.1)
            lib = fams[c % 2]
            for _ in range(n // 3000):
                r = lib[rng.randint(0, len(lib))].copy()
                mut = rng.rand(r.size) < 0.02
                r[mut] = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, int(mut.sum()))]
                p = rng.randint(0, s.size - 700)
                s[p:p + r.size] = r
            seqs.append(s)
        return _freeze(seqs)
    return _once(("genome", limit), make)


def pack_seq(limit):
    return _once(("pack", limit), lambda: _freeze(_rand_seq(np.random.RandomState(77 + limit), PACK_LENGTH[limit])))


def unpacked(s):
    """what genome_unpack returns for `s`, as test_pack_roundtrip works it out"""
    up = s & 0xDF
    ok = (up == 65) | (up == 67) | (up == 71) | (up == 84)
    return np.where(ok, up, ord("N")).astype(np.uint8)


def counts(limit, k):
    """po.count of every chromosome: [(keys, counts)]"""
    return _once(("count", limit, k), lambda: _freeze([po.count(s, k, LOWER, nthreads=4) for s in genome(limit)]))


def oracle(limit, k):
    """a fresh OracleContext holding the genome, counted at k (its results below are cached, the context is not)"""
    from oracle_ctx import OracleContext
    o = OracleContext(nthreads=4)
    seqs = genome(limit)
    o.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        o.genome_add(i, s)
    o.k, o.lower, o.dumps = k, LOWER, counts(limit, k)       # (what o.count(k, LOWER) would compute again)
    return o


def filter_csr():
    from subphaser_amd.config import sets_to_csr
    return sets_to_csr([[[0], [1], [2]]], [0, 1, 2])


def run_filter(ctx, csr=None, args=FILTER_ARGS):
    """((n_union, n_rows, n_hist), keys, counts, freqs, tot, sorted hist) of one filter pass"""
    nu, nr, nh = ctx.filter(*(csr or filter_csr()), *args)
    keys, cnt, freqs, tot = ctx.filter_fetch(nr)
    return (nu, nr, nh), keys, cnt, freqs, tot, np.sort(ctx.filter_hist(nh))


def filtered(limit, k):
    return _once(("filter", limit, k), lambda: _freeze(run_filter(oracle(limit, k))))


def labels(limit, k, S):
    """the filter's rows, labelled by the chromosome that holds most copies; every 40th counted k-mer of each chromosome
    (thousands: the *_seen counters of labels_hit run 4 or 8 workgroups per compute unit over them) and the k-mers of
    3000 random bases, which the genome hardly holds and labels_hit must not count, labelled round robin"""
    def make():
        f = filtered(limit, k)
        absent = po.count(_rand_seq(np.random.RandomState(limit + k), 3000, 0, 0), k, 1)[0]
        keys = np.unique(np.concatenate([f[1]] + [kk[::40] for kk, _ in counts(limit, k)] + [absent]))
        sg = (np.arange(keys.size) % S).astype(np.uint8)
        sg[np.searchsorted(keys, f[1])] = (np.argmax(f[2], axis=1) % S).astype(np.uint8)
        return _freeze((keys, sg))
    return _once(("labels", limit, k, S), make)


def run_map(ctx, n_chrom):
    """map_bins per chromosome and map_bins_all at every shape, then labels_hit"""
    out = []
    for bs, ch in MAP_SHAPES:
        for i in range(n_chrom):
            b, n = ctx.map_bins(i, bs, ch)
            out.append((np.array(b), int(n)))
        allb, nm = ctx.map_bins_all(bs, ch)
        out.append(([np.array(b) for b in allb], np.array(nm)))
    out.append(int(ctx.labels_hit()))
    return out


def mapped(limit, k, S):
    def make():
        o = oracle(limit, k)
        o.labels_set(*labels(limit, k, S), S)
        return _freeze(run_map(o, 3))
    return _once(("map", limit, k, S), make)


def features(limit, k):
    """(chrom, start, length) of 800 features per limit cut from all three chromosomes: 1 .. 10 000 bases (most below
    2000), the first 60 around and below k, every eighth overlapping its predecessor"""
    def make():
        rng = np.random.RandomState(900 + limit + k)
        n = 800 * (2 if limit == 3 else 1)
        ln = np.where(rng.rand(n) < 0.1, rng.randint(2000, 10001, size=n), rng.randint(1, 2000, size=n))
        ln[:60] = rng.randint(1, k + 3, size=60)
        ch = rng.randint(0, 3, size=n).astype(np.int32)
        lens = np.array(LENGTHS[limit])
        st = (rng.rand(n) * (lens[ch] - ln)).astype(np.int64)
        for f in range(8, n, 8):
            ch[f] = ch[f - 1]
            st[f] = min(st[f - 1] + ln[f - 1] // 2, lens[ch[f]] - ln[f])
        return _freeze((ch, st, ln.astype(np.int64)))
    return _once(("features", limit, k), make)


def feature_cat(limit, k):
    ch, st, ln = features(limit, k)
    seqs = genome(limit)
    cat = np.concatenate([seqs[c][s:s + l] for c, s, l in zip(ch.tolist(), st.tolist(), ln.tolist())])
    return cat, np.concatenate(([0], np.cumsum(ln))).astype(np.int64)


def run_features(ctx, limit, k, S):
    """map_features_cat and map_intervals of the same features, each on freshly set labels, with their labels_hit"""
    ch, st, ln = features(limit, k)
    cat, off = feature_cat(limit, k)
    ctx.labels_set(*labels(limit, k, S), S)
    a = np.array(ctx.map_features_cat(cat, off))
    ha = int(ctx.labels_hit())
    ctx.labels_set(*labels(limit, k, S), S)
    b = np.array(ctx.map_intervals(ch, st, st + ln))
    return a, ha, b, int(ctx.labels_hit())


def featured(limit, k, S):
    return _once(("feat", limit, k, S), lambda: _freeze(run_features(oracle(limit, k), limit, k, S)))


def run_windows(ctx, limit, k, S):
    lens = LENGTHS[limit]
    ctx.labels_set(*labels(limit, k, S), S)
    ctx.map_bins_all(10000, 10_000_000)
    win, woff = ctx.stack_windows(10000, 10_000_000, 50_000, lens)
    win, woff = np.array(win), np.array(woff)
    e = ctx.stack_enrich(10000, 10_000_000, 50_000, lens)
    return win, woff, [np.array(x) for x in e]


def windowed(limit, k, S):
    return _once(("win", limit, k, S), lambda: _freeze(run_windows(oracle(limit, k), limit, k, S)))


def wide_genome(limit):
    """130 short chromosomes of test_gpu_wide_join's generator (one of them `long_factor` times the rest)"""
    from test_gpu_wide_join import make_genome
    return _once(("wide", limit), lambda: _freeze(make_genome(130, seed=130 + limit, long_factor=40 * limit)))


def blocks_pair(limit):
    """a homoeologous pair built from blocks_cases' pieces as its planted() is, 140 003 bases per limit: B is A with 5 %
    substitutions, a fifth of it inverted in place and 5000 unrelated bases inserted"""
    import blocks_cases as bc

    def make():
        rng = np.random.RandomState(50 + limit)
        n = 140_003 * limit
        a = bc.rand_seq(rng, n)
        b = bc.mutate(rng, a, 0.05)
        i0, i1 = n // 5, 2 * n // 5
        b = bc._put(b, i0, bc.revcomp(b[i0:i1]))
        at = 3 * n // 4
        return a, b[:at] + bc.rand_seq(rng, 5000) + b[at:]
    return _once(("blocks", limit), make)
