"""The Python twin of subphaser_amd/csrc/sp_ltrdetect.h, written from the definition in its head: words, partners, seeds,
the gapless X-drop extension and the HSP list of one chromosome.  Integers only; compared with `==`.

numpy finds the valid starts and groups equal words (a stable sort: ascending position inside a group); every rule is a
plain Python loop over those groups."""
import numpy as np

LMIN, LMAX, SCAN, FANOUT, MAXDIST, MAXLEN, INVALID = 12, 20, 32, 8, 32767, 8192, 4
MATCH, MISMATCH = 2, -2
BODY = (1 << 24) - 32768 - 32
DEFAULTS = dict(L=20, X=20, dmin=1000, dmax=15000, maxlen=7000)

_CODE = np.full(256, INVALID, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def encode(seq):
    """codes 0..3, INVALID for everything that is not A, C, G, T in either case"""
    if isinstance(seq, str):
        seq = seq.encode()
    return _CODE[np.frombuffer(bytes(seq), np.uint8)]


def word_groups(codes, L):
    """[ascending positions] of every word that has two or more valid starts, and the number of valid starts"""
    n = len(codes) - L + 1
    if n < 1:
        return [], 0
    bad = np.concatenate(([0], np.cumsum(codes >= INVALID)))
    valid = np.flatnonzero(bad[L:L + n] == bad[:n])
    w = np.zeros(n, np.uint64)
    for j in range(L):
        w = (w << np.uint64(2)) | (codes[j:j + n] & 3).astype(np.uint64)
    w = w[valid]
    order = np.argsort(w, kind="stable")
    ws, pos = w[order], valid[order]
    cut = np.flatnonzero(ws[1:] != ws[:-1]) + 1
    return [g.tolist() for g in np.split(pos, cut) if len(g) > 1], len(valid)


def partners(group, i, dmin, dmax):
    """of start group[i] among the ascending starts of its word"""
    out = []
    for q in group[i + 1:i + 1 + SCAN]:
        if q - group[i] > dmax:
            break
        if q - group[i] >= dmin:
            out.append(q)
            if len(out) == FANOUT:
                break
    return out


def is_seed(codes, p, q):
    return p == 0 or codes[p - 1] >= INVALID or codes[q - 1] >= INVALID or codes[p - 1] != codes[q - 1]


def seeds(codes, L, dmin, dmax):
    out = []
    for group in word_groups(codes, L)[0]:
        for i in range(len(group)):
            out += [(group[i], q) for q in partners(group, i, dmin, dmax) if is_seed(codes, group[i], q)]
    return sorted(out)


def extend(codes, p, q, L, X, maxlen):
    """the HSP (p0, n, d) of the seed (p, q)"""
    n_bases, d = len(codes), q - p
    cap = min(d, maxlen)
    e, s, best, r = L, 0, 0, L
    while e < cap and q + e < n_bases and codes[p + e] < INVALID and codes[q + e] < INVALID:
        s += MATCH if codes[p + e] == codes[q + e] else MISMATCH
        e += 1
        if s > best:
            best, r = s, e
        elif s < best - X:
            break
    e, s, best, l = 0, 0, 0, 0
    while p - e - 1 >= 0 and r + e < cap and codes[p - e - 1] < INVALID and codes[q - e - 1] < INVALID:
        s += MATCH if codes[p - e - 1] == codes[q - e - 1] else MISMATCH
        e += 1
        if s > best:
            best, l = s, e
        elif s < best - X:
            break
    return p - l, r + l, d


def hsps(seq, L=20, X=20, dmin=1000, dmax=15000, maxlen=7000):
    """(n_seeds, the distinct HSPs (p0, n, d) ascending) of one chromosome"""
    codes = encode(seq).tolist()
    sd = seeds(np.asarray(codes, np.uint8), L, dmin, dmax)
    return len(sd), sorted({extend(codes, p, q, L, X, maxlen) for p, q in sd})


def trace(seq, L=20, X=20, dmin=1000, dmax=15000, maxlen=7000):
    """every intermediate of one chromosome, for the host check of the header: (valid starts, sum of their words modulo 2^64,
    partner pairs, [(p, q, p0, n, d)] of the seeds ascending)"""
    arr = encode(seq)
    codes = arr.tolist()
    n = len(codes) - L + 1
    n_valid = wsum = 0
    for p in range(max(n, 0)):
        if all(c < INVALID for c in codes[p:p + L]):
            w = 0
            for c in codes[p:p + L]:
                w = (w << 2) | c
            n_valid, wsum = n_valid + 1, (wsum + w) & (2 ** 64 - 1)
    groups, nv = word_groups(arr, L)
    assert nv == n_valid
    n_pairs = sum(len(partners(g, i, dmin, dmax)) for g in groups for i in range(len(g)))
    return n_valid, wsum, n_pairs, [(p, q) + extend(codes, p, q, L, X, maxlen) for p, q in seeds(arr, L, dmin, dmax)]
