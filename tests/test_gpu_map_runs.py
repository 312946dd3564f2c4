"""The runs rule of the two-phase map walks (csrc/sp_map.h, MAP_RUNS): a lane whose last probed quads of starts passed the
pair filter on both pairs enqueues the next quads unprobed, and the exact table decides them.  Results must not move: every
case maps a hand-built chromosome -- a random background with copies of three "repeat" segments planted where the rule can go
wrong -- through the library as shipped (rule on), through the same library with SP_MAP_RUNS=0 (every quad probed) and through
the oracle, and compares bin counts, n_mapped and the number of labelled k-mers seen.  Equal, never close.  The k > 15 twin
of the walk probes every quad whatever the switch says (profiles/map_runs_notes.md, section 5): its cases pin that walk on
the same shapes."""
import functools

import numpy as np
import pytest

import pyoracle as po
from subphaser_amd import kmer as km

pytestmark = pytest.mark.gpu

_B = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}
SEG_LEN = 160
N_BASES = 150_016          # 2344 units of 64 starts: five 512-unit ranges, the last one partly filled


def _revcomp(a):
    return np.array([_COMP[int(c)] for c in a[::-1]], np.uint8)


def _keys_by_position(seq, k):
    """canonical key of the k-mer at every start of an ACGT-only sequence"""
    code = np.searchsorted(_B, seq).astype(np.uint64)
    n = seq.size - k + 1
    key = np.zeros(n, np.uint64)
    for i in range(k):
        key = (key << np.uint64(2)) | code[i:i + n]
    return km.canonical(key, k)


@functools.lru_cache(maxsize=None)
def _case(k):
    """(chromosome, the three segments, positions worth cutting intervals at).  Positions are absolute starts in the
    chromosome: a unit is 64 starts from a multiple of 64, a round of the walk 32 starts, a quad 4 starts."""
    rng = np.random.RandomState(1000 + k)
    s = _B[rng.randint(0, 4, size=N_BASES)]
    A, Bs, Cs = (_B[rng.randint(0, 4, size=SEG_LEN)] for _ in range(3))
    cur = [4096]

    def slot(residue, room):
        """next free position == residue (mod 64), `room` bases reserved behind it (+ a gap longer than k)"""
        p = (cur[0] + 63) // 64 * 64 + residue
        cur[0] = p + room + 40
        return p

    cuts = []
    # whole copies starting at every residue mod 4 of the position (and at different places of a unit)
    for r in range(4):
        for base in (0, 20, 41):
            p = slot(base + r, SEG_LEN)
            s[p:p + SEG_LEN] = A
            cuts.append(p)
    # short copies lying across a unit boundary and across a round boundary: the lane state resets / carries
    for edge in (64, 32):
        for back in range(k + 3, k + 24, 3):
            ln = k + 24
            p = slot(0, 128) + edge - back
            s[p:p + ln] = Bs[11:11 + ln]
    # copies cut down to every length from k to k + 16 bases, at every residue: runs of 1, 2, 3 ... quads, and whatever the
    # walk predicts next lies just past the end
    for ln in range(k, k + 17):
        for r in range(4):
            p = slot(8 + r, ln)
            s[p:p + ln] = A[30:30 + ln]
    # one substituted base in the middle of a copy: the run breaks for k starts and resumes
    for r in range(4):
        p = slot(12 + r, SEG_LEN)
        s[p:p + SEG_LEN] = Cs
        q = p + 77 + r
        s[q] = _B[(int(np.searchsorted(_B, s[q])) + 1 + r % 3) % 4]
        cuts.append(p)
    # an N at each of the four offsets of a quad, in copies at each residue: invalid pairs inside a would-be predicted quad
    # (the first pair's (k-1)-mer only, the second's only, both)
    n_at = []
    for r in range(4):
        for o in range(4):
            p = slot(r, SEG_LEN)
            s[p:p + SEG_LEN] = A
            n_at.append((p + 80) // 4 * 4 + o)
    # a reverse-complemented copy; two different segments back to back (the label changes inside a run: the k-mers over
    # the joint are labelled too)
    for r in (1, 2):
        p = slot(30 + r, SEG_LEN)
        s[p:p + SEG_LEN] = _revcomp(Bs)
        p = slot(5 + r, 2 * SEG_LEN)
        s[p:p + SEG_LEN] = A
        s[p + SEG_LEN:p + 2 * SEG_LEN] = Cs
        cuts.append(p + SEG_LEN - 40)
    assert cur[0] < N_BASES - 4096
    # copies at the chromosome's first and last bases
    s[:SEG_LEN] = A
    s[N_BASES - SEG_LEN:] = Bs
    s[n_at] = ord("N")
    return s, (A, Bs, Cs), cuts


@functools.lru_cache(maxsize=None)
def _labels(k, S):
    """label set = every k-mer of the three segments and of the joint A + C; label = the segment's index mod S"""
    _, (A, Bs, Cs), _ = _case(k)
    keys = np.concatenate([_keys_by_position(A, k), _keys_by_position(Bs, k), _keys_by_position(Cs, k),
                           _keys_by_position(np.concatenate([A[-(k - 1):], Cs[:k - 1]]), k)])
    lab = np.concatenate([np.full(SEG_LEN - k + 1, i % S, np.uint8) for i in range(3)] + [np.full(k - 1, 2 % S, np.uint8)])
    keys, first = np.unique(keys, return_index=True)
    return keys, lab[first]


BINS = ((1000, 10_000_000), (64, 0), (37, 5000))


@functools.lru_cache(maxsize=None)
def _expected(k, S):
    s, _, _ = _case(k)
    keys, lab = _labels(k, S)
    out = []
    hit_all = np.zeros(keys.size, np.uint8)
    for bin_size, chunk in BINS:
        exp, hit, n = po.map_bins(s, k, keys, lab, S, bin_size, chunk, nthreads=2)
        hit_all |= hit
        out.append((exp, n))
    assert out[0][1] > 40 * (SEG_LEN - k)          # the copies are found at all
    return out, int(hit_all.sum())


def _load(ctx, k):
    s, _, _ = _case(k)
    ctx.genome_reset(1)
    ctx.genome_add(0, s)
    ctx.count(k, 1, 1)          # (fixes k; the label set below is hand-made)


PARAMS = [(15, 2), (15, 3), (15, 5), (14, 2), (14, 5), (17, 3), (17, 5)]


@pytest.mark.parametrize("k,S", PARAMS)
def test_bins_with_runs(gpu_ctx, monkeypatch, k, S):
    """S <= 3: compact quad buckets (k = 17: the k > 15 twin's), S = 5: the direct pair table (k = 17: the pair-keyed hash
    table); rule on (default) and off, both equal to the oracle."""
    keys, lab = _labels(k, S)
    exp, exp_hit = _expected(k, S)
    _load(gpu_ctx, k)
    for runs in ("1", "0"):
        monkeypatch.setenv("SP_MAP_RUNS", runs)
        gpu_ctx.labels_set(keys, lab, S)
        for (bin_size, chunk), (e, n_exp) in zip(BINS, exp):
            got, n = gpu_ctx.map_bins(0, bin_size, chunk)
            assert got.shape == e.shape, (runs, bin_size)
            assert (got == e).all(), (runs, bin_size, np.argwhere(got != e)[:5])
            assert n == n_exp, (runs, bin_size)
        assert gpu_ctx.labels_hit() == exp_hit, runs


@pytest.mark.parametrize("k,S", [(15, 2), (15, 5), (17, 3)])
def test_intervals_cut_runs(gpu_ctx, monkeypatch, k, S):
    """interval mode (sp_map_intervals) on the same walk: intervals that begin and end in the middle of a copy"""
    from oracle_ctx import OracleContext
    s, _, cuts = _case(k)
    keys, lab = _labels(k, S)
    st, en = [], []
    for p in cuts:
        st += [p - 50, p + 81, p + 83, p + 60, p + 2]
        en += [p + 81, p + 200, p + 83 + k + 5, p + 60 + k, p + 2 + 3 * k]
    st += [0, N_BASES - 100, 0]
    en += [70, N_BASES, N_BASES]
    st, en = np.array(st, np.int64), np.array(en, np.int64)
    octx = OracleContext(nthreads=1)
    octx.genome_reset(1)
    octx.genome_add(0, s)
    octx.k = k
    octx.labels_set(keys, lab, S)
    exp = octx.map_intervals(np.zeros(st.size, np.int32), st, en)
    assert int(exp.sum()) > 0
    _load(gpu_ctx, k)
    for runs in ("1", "0"):
        monkeypatch.setenv("SP_MAP_RUNS", runs)
        gpu_ctx.labels_set(keys, lab, S)
        got = gpu_ctx.map_intervals(np.zeros(st.size, np.int32), st, en)
        assert got.shape == exp.shape and (got == exp).all(), (runs, np.argwhere(got != exp)[:5])
        assert gpu_ctx.labels_hit() == octx.labels_hit(), runs
