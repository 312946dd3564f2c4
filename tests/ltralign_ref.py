"""Plain numpy twin of the LTR-pair alignment (subphaser_amd/csrc/sp_ltralign.h), written from its definition.

A global, banded alignment with linear gap costs, all integers, no traceback:

  sequences  a (la bases), b (lb bases); a base is a code 0..3 or 4 (invalid: anything but ACGTacgt)
  band       cells (i, j), 0 <= i <= la, 0 <= j <= lb, with d = j - i in [min(0, lb - la) - w, max(0, lb - la) + w]
  column     both valid and equal +2 (match), both valid and different -2 (mismatch), one invalid 0 (skip), a gap -3
  cell       the maximum over its diagonal, up (consumes a[i - 1]) and left (consumes b[j - 1]) predecessors inside the
             band, ties in that order; it carries (score, match, mismatch, gap, skip, edge) of the predecessor it chose
             plus its own column
  edge       1 once the chosen path stands on the lowest or highest diagonal of the band while w > 0
  result     the state at (la, lb); an LTR above MAXLEN, or a band above MAXBAND, is not aligned and only flagged

`align` walks the anti-diagonals with numpy (the cells of one are independent of each other), `align_rows` walks the same
cells one by one in plain Python; `full_dp` is the textbook full-matrix loop with the same tie order, for the tests that
hold them against each other."""
import numpy as np

MAXLEN, MAXBAND = 8192, 1024
MATCH, MISMATCH, GAP = 2, -2, -3
F_EDGE, F_BAND, F_LEN = 1, 2, 4
INVALID = 4
NEG = -(1 << 40)

_CODE = np.full(256, INVALID, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def encode(seq):
    """codes 0..3 of ACGT / acgt, 4 for everything else"""
    return _CODE[np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)]


def band_bounds(la, lb, w):
    return min(0, lb - la) - w, max(0, lb - la) + w


def check(la, lb, w):
    """0, or the flag of a pair that is not aligned"""
    if la > MAXLEN or lb > MAXLEN:
        return F_LEN
    dlo, dhi = band_bounds(la, lb, w)
    return F_BAND if dhi - dlo + 1 > MAXBAND else 0


def align(a, b, w):
    """(score, match, mismatch, gap, skip, flags) of code arrays a, b under band w"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    la, lb = len(a), len(b)
    assert la >= 1 and lb >= 1 and w >= 0
    flag = check(la, lb, w)
    if flag:
        return (0, 0, 0, 0, 0, flag)
    dlo, dhi = band_bounds(la, lb, w)
    width = dhi - dlo + 1

    # an anti-diagonal: a row per diagonal of the band and one of padding either side; three of them take turns
    two_back, one_back, cur = (np.zeros((width + 2, 6), np.int64) for _ in range(3))
    two_back[:, 0] = one_back[:, 0] = NEG
    one_back[0 - dlo + 1] = 0           # the origin
    for s in range(1, la + lb + 1):
        cur[:, 0] = NEG
        lo, hi = max(dlo, -s, s - 2 * la), min(dhi, s, 2 * lb - s)
        lo += (lo - s) % 2
        if lo <= hi:
            d = np.arange(lo, hi + 1, 2)
            i, j, r = (s - d) // 2, (s + d) // 2, d - dlo + 1
            x, y = a[i - 1], b[j - 1]            # (wraps where i or j is 0: no diagonal predecessor there)
            skip = (x >= INVALID) | (y >= INVALID)
            same = ~skip & (x == y)
            diff = ~skip & (x != y)
            col = np.zeros((len(d), 6), np.int64)
            col[:, 0] = MATCH * same + MISMATCH * diff
            col[:, 1], col[:, 2], col[:, 4] = same, diff, skip
            gap = np.array([GAP, 0, 0, 1, 0, 0], np.int64)
            cd, cu, cl = two_back[r] + col, one_back[r + 1] + gap, one_back[r - 1] + gap
            for c, src in ((cd, two_back[r]), (cu, one_back[r + 1]), (cl, one_back[r - 1])):
                c[src[:, 0] == NEG, 0] = NEG
            take_d = (cd[:, 0] >= cu[:, 0]) & (cd[:, 0] >= cl[:, 0])
            take_u = ~take_d & (cu[:, 0] >= cl[:, 0])
            new = np.where(take_d[:, None], cd, np.where(take_u[:, None], cu, cl))
            assert (new[:, 0] > NEG).all()
            if w > 0:
                new[:, 5] |= (d == dlo) | (d == dhi)
            cur[r] = new
        two_back, one_back, cur = one_back, cur, two_back
    end = one_back[lb - la - dlo + 1]
    return (int(end[0]), int(end[1]), int(end[2]), int(end[3]), int(end[4]), F_EDGE if end[5] else 0)


def full_dp(a, b):
    """(score, match, mismatch, gap, skip) of the unbanded alignment: the full matrix, row by row, same tie order"""
    la, lb = len(a), len(b)
    prev = [(GAP * j, 0, 0, j, 0) for j in range(lb + 1)]
    for i in range(1, la + 1):
        row = [(GAP * i, 0, 0, i, 0)]
        for j in range(1, lb + 1):
            x, y = int(a[i - 1]), int(b[j - 1])
            dg, up, lf = prev[j - 1], prev[j], row[j - 1]
            if x >= INVALID or y >= INVALID:
                cd = (dg[0], dg[1], dg[2], dg[3], dg[4] + 1)
            elif x == y:
                cd = (dg[0] + MATCH, dg[1] + 1, dg[2], dg[3], dg[4])
            else:
                cd = (dg[0] + MISMATCH, dg[1], dg[2] + 1, dg[3], dg[4])
            cu = (up[0] + GAP, up[1], up[2], up[3] + 1, up[4])
            cl = (lf[0] + GAP, lf[1], lf[2], lf[3] + 1, lf[4])
            if cd[0] >= cu[0] and cd[0] >= cl[0]:
                row.append(cd)
            elif cu[0] >= cl[0]:
                row.append(cu)
            else:
                row.append(cl)
        prev = row
    return prev[lb]


def align_rows(a, b, w):
    """`align` once more, cell by cell and row by row in plain Python: the same answers, quicker for pairs of a few bases"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    la, lb = len(a), len(b)
    assert la >= 1 and lb >= 1 and w >= 0
    flag = check(la, lb, w)
    if flag:
        return (0, 0, 0, 0, 0, flag)
    dlo, dhi = band_bounds(la, lb, w)
    prev = None
    for i in range(la + 1):
        row = [None] * (lb + 1)
        for j in range(max(0, i + dlo), min(lb, i + dhi) + 1):
            if i == 0 and j == 0:
                row[0] = (0, 0, 0, 0, 0, 0)
                continue
            best = None
            if i > 0 and j > 0 and prev[j - 1] is not None:
                p = prev[j - 1]
                x, y = a[i - 1], b[j - 1]
                if x >= INVALID or y >= INVALID:
                    best = (p[0], p[1], p[2], p[3], p[4] + 1, p[5])
                elif x == y:
                    best = (p[0] + MATCH, p[1] + 1, p[2], p[3], p[4], p[5])
                else:
                    best = (p[0] + MISMATCH, p[1], p[2] + 1, p[3], p[4], p[5])
            for p in (prev[j] if i > 0 else None, row[j - 1] if j > 0 else None):      # up, then left
                if p is not None and (best is None or p[0] + GAP > best[0]):
                    best = (p[0] + GAP, p[1], p[2], p[3] + 1, p[4], p[5])
            if w > 0 and j - i in (dlo, dhi):
                best = best[:5] + (1,)
            row[j] = best
        prev = row
    end = prev[lb]
    return end[:5] + (F_EDGE if end[5] else 0,)


def align_intervals(seqs, chrom, a_start, a_len, b_start, b_len, band):
    """what Context.ltr_align returns for 0-based intervals on the sequences `seqs` (strings, by chromosome index)"""
    codes = {}
    out = np.zeros((len(chrom), 6), np.int32)
    for n, (c, s0, l0, s1, l1) in enumerate(zip(chrom, a_start, a_len, b_start, b_len)):
        c = int(c)
        if c not in codes:
            codes[c] = encode(seqs[c])
        a, b = codes[c][s0:s0 + l0], codes[c][s1:s1 + l1]
        out[n] = align_rows(a, b, band) if l0 * l1 <= 400 else align(a, b, band)
    return out
