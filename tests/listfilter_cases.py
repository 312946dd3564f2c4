"""Hand-made inputs of the list filter tests (test_listfilter_ref.py on the CPU, test_gpu_listfilter_view.py on the
device): per-chromosome (key, count) lists and lengths that no counted sequence produces.  Every construction is
deterministic; what the inputs cover is asserted in test_listfilter_ref.py with listfilter_ref.margin.

Chromosomes come in blocks of 12 (block b owns chromosomes 12b .. 12b + 11) with the lengths
    L, L, L+1, L, L+1000, L-3, L+997, L, L, L, 2L, 2L-1          (L = L0 + 2b)
and the generator's sets
    A [[0], [1]]              equal lengths: counts (2m + d, m) sit d / 2m from fold 2
    B [[2], [3]]              lengths L+1 and L: small count ratios sit 1e-9 (long) / 2.5e-4 (short) from the threshold
    C [[4, 5], [6, 7]]        two-chromosome units of equal summed length: unit sums above 2^32
    D [[8], [9], [10]]        three units (baseline 1 and -1 differ), one of twice the length
chromosome 11 of a block is in no generator set.  Two regimes: "long" (L0 = 1 000 000 007: with counts below ~9e4 the
1e-20 of the fold test changes the fp64 quotient, an exact ratio of 2 fails `>= 2`) and "short" (L0 = 4001: the 1e-20
is absorbed, the same ratio passes)."""
import math
import random
from fractions import Fraction

import numpy as np

U32 = 2 ** 32 - 1
L0 = {"long": 1_000_000_007, "short": 4001}
FOLDS = {2.0: (2, 1), 1.5: (3, 2)}
CLASSES = ("zero", "tiny", "nano", "band", "mid", "far", "lo0", "allzero", "small")


# ------------------------------------------------------------------ the join's plan (csrc/sp_listplan.h)
def plan_ranges(total, C, k):
    """-> (rb, shift): 2^rb key ranges, range of a key = key >> shift."""
    bits = min(2 * k, 64)
    per = 32 * C if C > 64 else 1024 * 2 // 3
    rb = 0
    while rb < bits and rb < 23 and (1 << rb) * per < total:
        rb += 1
    if bits - rb > 63:
        rb = bits - 63
    return rb, bits - rb


def row_cap(total, n_cu):
    cap = total // 16
    if cap < (1 << 20):
        cap = min(total, 1 << 20)
    return cap + n_cu * 16 * 256


def key_max(k):
    """the largest key a list may hold (2^64 - 1 is the staging sentinel, never a canonical k-mer)"""
    return 4 ** k - 1 if k < 32 else 2 ** 64 - 2


# ------------------------------------------------------------------ lengths and set structures
def lengths_for(C, regime):
    out = []
    for c in range(C):
        L = L0[regime] + 2 * (c // 12)
        out.append([L, L, L + 1, L, L + 1000, L - 3, L + 997, L, L, L, 2 * L, 2 * L - 1][c % 12])
    return np.array(out, np.int64)


def gen_sets(C):
    """the generator's sets: four per whole block of 12"""
    sgs = []
    for b in range(C // 12):
        o = 12 * b
        sgs += [[[o], [o + 1]], [[o + 2], [o + 3]], [[o + 4, o + 5], [o + 6, o + 7]], [[o + 8], [o + 9], [o + 10]]]
    return sgs


def structures(C):
    """name -> sets the filter is run with.  s3 / s5: 3 / 5 non-singleton sets per block next to a singleton set and
    chromosomes in no set (C = 12: include / n_multi reaches 1/3 and 0.6 exactly); b2: units for baseline 2 (generic
    decisions); many: 33 sets of two two-chromosome units that reuse chromosomes 0 and 1 -- 132 walk descriptors, more
    than the fast walk holds (C = 12 only)."""
    s3, s5, b2 = [], [], []
    for b in range(C // 12):
        o = 12 * b
        s3 += [[[o], [o + 1]], [[o + 2]], [[o + 4, o + 5], [o + 6, o + 7]], [[o + 8], [o + 9], [o + 10]]]
        s5 += [[[o], [o + 1]], [[o + 2], [o + 3]], [[o + 4, o + 5], [o + 6, o + 7]], [[o + 8], [o + 9], [o + 10]],
               [[o + 11]], [[o, o + 2], [o + 1, o + 3]]]
        b2 += [[[o], [o + 1], [o + 2], [o + 3]], [[o + 4], [o + 5], [o + 6], [o + 7]],
               [[o + 8], [o + 9], [o + 10], [o + 11]]]
    out = {"s3": s3, "s5": s5, "b2": b2}
    if C == 12:
        pairs = [(a, b) for a in range(2, 12) for b in range(2, 12) if a != b][:33]
        out["many"] = [[[0, a], [1, b]] for a, b in pairs]
    return out


# ------------------------------------------------------------------ rows near the threshold
def _logint(rng, lo, hi):
    """an integer in [lo, hi], log-uniform"""
    if hi <= lo:
        return lo
    return min(hi, max(lo, int(round(math.exp(rng.uniform(math.log(lo), math.log(hi)))))))


def _target(rng, cls, side, LA, LB, capA, capB, pq, regime):
    """unit sums (A of the top unit, B of the baseline unit) of the class, or None when the lengths do not allow it.
    margin = (A LB q - B LA p) / (B LA p) for min_fold = p / q."""
    p, q = pq
    a, b = LB * q, LA * p
    g = math.gcd(a, b)
    a, b = a // g, b // g               # A a - B b = (numerator of the margin) / g
    if cls == "allzero":
        return 0, 0
    if cls == "lo0":
        return _logint(rng, 1, capA), 0
    if cls == "zero":                   # A = t b, B = t a
        if regime == "long":            # lo = B / LB below 9e-5
            t_lo, t_hi = 1, min(capA // b, (8 * LB // 100000) // a)
        else:                           # lo above 2e-4
            t_lo, t_hi = -(-3 * LB // (10000 * a)) + 1, min(capA // b, capB // a)
        if t_hi < t_lo:
            return None
        t = _logint(rng, t_lo, t_hi)
        return t * b, t * a
    if cls == "tiny":                   # A a - B b = +-1: |margin| = g / (B LA p)
        s = 1 if side > 0 else -1
        A0 = (s * pow(a, -1, b)) % b if b > 1 else 0
        t_hi = (min(capA, capB * b // a) - A0) // b
        if t_hi < 0:
            return None
        for _ in range(8):
            A = A0 + b * rng.randint(max(0, t_hi // 2), t_hi)
            B = (A * a - s) // b
            if 1 <= B <= capB and A >= 1 and B * LA * p > 1.01e12 * g:
                return A, B
        return None
    if cls == "small":                  # the dense test's rows: ratios of small integers
        m = _logint(rng, 1, 1 << 20)
        return p * m + rng.choice((-1, 0, 1)), q * m
    lo, hi = {"nano": (3e-9, 0.8e-6), "band": (0.55e-5, 1.9e-5), "mid": (1.2e-4, 0.8e-2), "far": (0.6, 5.0)}[cls]
    mu = math.exp(rng.uniform(math.log(lo), math.log(hi))) * (1 if side > 0 else -1)
    A = _logint(rng, min(capA, int(30 / abs(mu)) + 1), capA)
    B = int(round(Fraction(A * a, b) / (1 + Fraction(mu))))
    if not 1 <= B <= capB:
        return None
    return A, B


def _split(rng, S, n):
    """S as n counts of at most 2^32 - 1"""
    parts = [S // n + (1 if i < S % n else 0) for i in range(n)]
    if n > 1 and parts[1] > 0:
        t = rng.randint(0, min(parts[1] - 1, U32 - parts[0]))
        parts[0] += t
        parts[1] -= t
    assert sum(parts) == S and max(parts) <= U32
    return parts


def _fill_set(rng, row, lengths, sg, cls, side, pq, baseline, regime):
    """counts of one generator set so that its top and baseline units sit in class `cls`"""
    nu = len(sg)
    ulen = [sum(int(lengths[c]) for c in u) for u in sg]
    cap = [len(u) * U32 for u in sg]
    h, l = rng.sample(range(nu), 2)
    ab = _target(rng, cls, side, ulen[h], ulen[l], cap[h], cap[l], pq, regime)
    if ab is None:
        ab = _target(rng, "small", side, ulen[h], ulen[l], cap[h], cap[l], pq, regime)
    A, B = ab
    sums = [0] * nu
    sums[h], sums[l] = A, B
    for o in range(nu):
        if o in (h, l) or A == 0:
            continue
        if baseline == 1:               # the third unit below the baseline unit
            sums[o] = min(cap[o], int(Fraction(B * ulen[o], ulen[l]) * Fraction(rng.randint(0, 9), 10)))
        else:                           # between the baseline (smallest) and the top unit
            lo_o, hi_o = -(-B * ulen[o] // ulen[l]), A * ulen[o] // ulen[h]
            sums[o] = min(cap[o], (lo_o + hi_o) // 2 if hi_o >= lo_o else hi_o)
    for u, s in zip(sg, sums):
        for c, v in zip(u, _split(rng, s, len(u))):
            row[c] = v


def threshold_matrix(C, regime, n_rows, seed, fill=0.25):
    """n_rows x C uint32 count rows (none all zero), every row aimed at one (generator set, min_fold, baseline, class,
    side) in turn; the other sets of the row are empty, small random counts or aimed rows of their own."""
    rng = random.Random(seed)
    lengths = lengths_for(C, regime)
    gs = gen_sets(C)
    combos = [(cls, side, fold, bl) for cls in CLASSES for side in (1, -1) for fold in sorted(FOLDS) for bl in (1, -1)]
    mat = np.zeros((n_rows, C), np.uint32)
    for i in range(n_rows):
        cls, side, fold, bl = combos[i % len(combos)]
        row = [0] * C
        s_main = (i // len(combos)) % len(gs)
        for s, sg in enumerate(gs):
            if s == s_main:
                _fill_set(rng, row, lengths, sg, cls, side, FOLDS[fold], bl, regime)
                continue
            x = rng.random()
            if x < fill * 0.4:
                _fill_set(rng, row, lengths, sg, rng.choice(CLASSES), rng.choice((1, -1)),
                          FOLDS[rng.choice(sorted(FOLDS))], rng.choice((1, -1)), regime)
            elif x < fill:
                for u in sg:
                    for c in u:
                        if rng.random() < 0.5:
                            row[c] = rng.randint(1, 50)
        for c in range(C):
            if c % 12 == 11 or c >= 12 * (C // 12):
                if rng.random() < fill:
                    row[c] = rng.randint(1, 50)
        if not any(row):
            row[C - 1] = rng.randint(1, 50)
        mat[i] = row
    return mat, lengths


def random_keys(n, k, seed):
    """n distinct keys, ascending, below key_max(k)"""
    rng = random.Random(seed)
    top = key_max(k)
    keys = set()
    while len(keys) < n:
        keys.add(rng.randint(0, top))
    return np.array(sorted(keys), np.uint64)


def lists_of(keys, mat):
    """keys (ascending, one per row of mat) -> per-chromosome (keys, counts) lists of the non-zero counts"""
    out = []
    for col in np.ascontiguousarray(mat.T):
        nz = np.flatnonzero(col)
        out.append((np.ascontiguousarray(keys[nz]), np.ascontiguousarray(col[nz])))
    return out


# ------------------------------------------------------------------ keys and ranges
def edge_keys(k, C, seed, n_fill=3000):
    """Lists whose keys sit on every possible range edge: 0, the largest legal key, pairs that differ in one bit only
    (every bit: whatever `shift` the plan picks, neighbours across a range edge are among them), all ones below every
    bit; chromosome 0 holds every key, chromosomes 2 and C - 1 hold none, the rest a random third."""
    rng = random.Random(seed)
    bits = min(2 * k, 64)
    top = key_max(k)
    keys = {0, top, top - 1, 1}
    for s in range(bits):
        for base in (0, rng.randint(0, top), rng.randint(0, top)):
            for x in (base, base ^ (1 << s), (base | (1 << s)) - 1, base | ((1 << s) - 1)):
                if 0 <= x <= top:
                    keys.add(x)
    while len(keys) < n_fill:
        keys.add(rng.randint(0, top))
    keys = np.array(sorted(keys), np.uint64)
    mat = np.zeros((len(keys), C), np.uint32)
    for i in range(len(keys)):
        mat[i, 0] = rng.randint(1, 40)
        for c in range(1, C):
            if c not in (2, C - 1) and rng.random() < 1 / 3:
                mat[i, c] = rng.randint(1, 40)
    return lists_of(keys, mat), mat


def skew_keys(n, k, seed):
    """n ascending keys that share their top 24 bits (of 2k): all of them fall into one range"""
    bits = min(2 * k, 64)
    free = bits - 24
    assert (1 << free) >= n
    rng = random.Random(seed)
    prefix = rng.randint(1, (1 << 24) - 2) << free
    low = np.array(sorted(rng.sample(range(1 << free), n)), np.uint64)
    return low + np.uint64(prefix)


def pair_sets(C):
    """[[0], [1]], [[2], [3]], ...: the structure decide_pairs_vec takes (an odd last chromosome is in no set)"""
    return [[[2 * i], [2 * i + 1]] for i in range(C // 2)]


def pair_matrix(n, C, seed, keep=0.9, present=None):
    """n rows for pair_sets(C): row i holds counts in the chromosomes of pair i % (C // 2) only -- (5, 1) or (1, 6), a
    fold of 5 or 6, in `keep` of the rows, (3, 2) in the rest (with equal lengths: fold 1.5)."""
    rng = np.random.RandomState(seed)
    mat = np.zeros((n, C), np.uint32)
    pair = np.arange(n) % (C // 2)
    kept = rng.rand(n) < keep
    flip = rng.rand(n) < 0.5
    a = np.where(kept, np.where(flip, 1, 5), 3).astype(np.uint32)
    b = np.where(kept, np.where(flip, 6, 1), 2).astype(np.uint32)
    mat[np.arange(n), 2 * pair] = a
    mat[np.arange(n), 2 * pair + 1] = b
    return mat


def spaced_keys(n, k, seed):
    """n ascending keys spread evenly over the key space (every range of the plan holds the same share)"""
    top = key_max(k)
    stride = top // n
    rng = np.random.RandomState(seed)
    jitter = rng.randint(0, min(stride, 1 << 30), size=n).astype(np.uint64)
    return np.arange(n, dtype=np.uint64) * np.uint64(stride) + jitter


def disjoint_lists(keys, C, counts):
    """one entry per key: key i goes to chromosome i % C with counts[i]"""
    out = []
    idx = np.arange(len(keys))
    for c in range(C):
        sel = idx[c::C]
        out.append((np.ascontiguousarray(keys[sel]), np.ascontiguousarray(counts[sel].astype(np.uint32))))
    return out


# ------------------------------------------------------------------ filter arguments of the threshold matrix
OPEN = (1.0, 1e13)
# (structure, min_fold, baseline, ratio as (numerator, "n_multi" or denominator), frequency bounds)
# bounds: "open"; "tot": min_freq / max_freq are the tot of the fold-passing k-mers at 1/4 and 3/4 of their sorted
# list (rows with tot == min_freq and tot == max_freq exist and are kept); "frac": min_freq = that tot + 0.5
ARGSETS_12 = (
    ("s3", 2.0, 1, (1, 1), "open"),
    ("s3", 1.5, -1, (1, 3), "tot"),
    ("s5", 2.0000001, 1, (3, 5), "frac"),          # 0.6
    ("s5", 1.0, -1, (1, 2), "tot"),
    ("s5", 2.0, -1, (0, 1), "tot"),
    ("s5", 1.5, 1, (1, 1), "open"),
    ("b2", 2.0, 2, (1, 3), "open"),
    ("many", 2.0, 1, (3, 33), "open"),
)
ARGSETS_WIDE = (                                   # ratio = numerator / n_multi: the rows touch a few sets each
    ("s3", 2.0, 1, (1, "n_multi"), "open"),
    ("s5", 1.5, -1, (2, "n_multi"), "tot"),
    ("s5", 2.0000001, 1, (0, 1), "frac"),
    ("s5", 1.0, -1, (1, "n_multi"), "tot"),
    ("b2", 2.0, 2, (1, "n_multi"), "open"),
)


def n_multi(sgs):
    return sum(len(sg) > 1 for sg in sgs)


def resolve_args(argset, C, filt):
    """-> sgs, keyword arguments of listfilter_ref.filter.  filt(sgs, **kw) runs the reference (bounds "tot" / "frac"
    take their values from its fold-passing totals with the bounds open)."""
    name, fold, bl, (num, den), bounds = argset
    sgs = structures(C)[name]
    ratio = num / (n_multi(sgs) if den == "n_multi" else den)
    kw = dict(min_fold=fold, baseline=bl, min_freq=OPEN[0], max_freq=OPEN[1], ratio=ratio)
    if bounds != "open":
        hist = filt(sgs, **kw)[4]
        assert len(hist) >= 8
        lo, hi = float(hist[len(hist) // 4]), float(hist[3 * len(hist) // 4])
        kw.update(min_freq=lo + 0.5 if bounds == "frac" else lo, max_freq=OPEN[1] if bounds == "frac" else hi)
    return sgs, kw


# ------------------------------------------------------------------ every entry a row, stranded chunks, second pass
ROWS_KW = dict(min_fold=2.0, baseline=1, min_freq=1.0, max_freq=1e13, ratio=0.0)


def all_present_case(n, C, k, seed):
    """every key in all C lists; with ROWS_KW the rows are the union matrix itself"""
    rng = np.random.RandomState(seed)
    keys = spaced_keys(n, k, seed)
    mat = rng.randint(1, 1000, size=(n, C)).astype(np.uint32)
    return lists_of(keys, mat), lengths_for(C, "short"), pair_sets(C), dict(ROWS_KW)


def disjoint_case(n, C, k, seed):
    """one entry per key; with ROWS_KW every entry is a row"""
    rng = np.random.RandomState(seed)
    keys = spaced_keys(n, k, seed)
    return (disjoint_lists(keys, C, rng.randint(1, 1000, size=n)), lengths_for(C, "short"), pair_sets(C), dict(ROWS_KW))


def fifth_case(n, C, k, seed):
    """one entry per key, every fifth key in chromosome 0 or 1 -- the only set of two units, which such a key passes
    (the other unit is empty) -- and the rest in chromosomes that no set of two units names: with ratio 1 a range
    keeps a fifth of its entries, about half a chunk of the row staging, and strands the other half."""
    rng = np.random.RandomState(seed)
    keys = spaced_keys(n, k, seed)
    i = np.arange(n)
    chrom = np.where(i % 5 == 0, (i // 5) % 2, 2 + i % (C - 2))
    counts = rng.randint(1, 1000, size=n).astype(np.uint32)
    lists = []
    for c in range(C):
        sel = np.flatnonzero(chrom == c)
        lists.append((np.ascontiguousarray(keys[sel]), np.ascontiguousarray(counts[sel])))
    sgs = [[[0], [1]]] + [[[c]] for c in range(2, min(C, 6))]
    return lists, lengths_for(C, "short"), sgs, dict(ROWS_KW, ratio=1.0)


def second_pass_case(C, variant, rows_kept, rows_control, k, seed):
    """-> lists, lengths, sgs, kw, kw_control: kw keeps exactly rows_kept rows, kw_control (a max_freq) the first
    rows_control of them in key order.  variant "ratio0": disjoint lists, every key a row; "pairs": every key in the two
    chromosomes of one set of pair_sets(C), about 90 % of them with a fold of 5 or 6, the rest 1.5 (decide_pairs_vec)."""
    lengths = lengths_for(C, "long")
    sgs = pair_sets(C)
    if variant == "ratio0":
        keys = spaced_keys(rows_kept, k, seed)
        counts = np.where(np.arange(rows_kept) < rows_control, 1, 2)
        kw = dict(ROWS_KW)
        return disjoint_lists(keys, C, counts), lengths, sgs, kw, dict(kw, max_freq=1.0)
    mat = pair_matrix(int(rows_kept / 0.9 * 1.02) + 64, C, seed)
    cum = np.cumsum(mat.max(axis=1) >= 5)
    n = int(np.searchsorted(cum, rows_kept)) + 1
    mat, cum = mat[:n], cum[:n]
    mat[cum > rows_control] *= np.uint32(2)        # past the control's rows: tot 10 / 12 / 14 instead of 5 / 6 / 7
    keys = spaced_keys(n, k, seed)
    kw = dict(ROWS_KW, ratio=1 / len(sgs))
    return lists_of(keys, mat), lengths, sgs, kw, dict(kw, max_freq=7.0)
