"""Plain Python twin of subphaser_amd/csrc/sp_domalign.h, written from the definition in its head comment (not from its
code): the item, the back-pointer order of the three cells, the trace, the outputs; and of sp_dom_peptide / sp_aln_pairs.

Two versions of one item (the residues of a window against one profile):
  align_plain   a triple loop over tuples (score, -start): Python's tuple order IS the pair order; the back-pointer of a
                cell is the first argument, in the definition's order, that equals the maximum.  Slow; small cases.
  align         the same cells a row at a time in numpy on the packed word (domains_ref.frames_hits' arithmetic), the
                codes by comparing the maximum with its arguments in the same order.
Both return (hit, col, path): hit = [score, i_start, i_end, k_start, k_end], col = M frame indices or -1, path = the cells
from the start to the hit as (state, i, k), state in "MID".  tests/test_domalign_host.py compares the two with `==`."""
import numpy as np

import domains_ref as dr

MAXWIN = 8192
LETTERS = dr.AA + "X*"
GAP = 255
MM, MI, MD, IM, II, DM, DD = range(7)


def window_residues(seq, f, i0, i1):
    """the residue codes i0 .. i1 (inclusive) of frame f of the interval's sequence"""
    return dr.translate(seq, f)[i0:i1 + 1]


def peptide(codes):
    return "".join(LETTERS[c] for c in codes)


def trace(codes, M, i0, i_end, k_end):
    """codes[(state, i, k)] -> predecessor state or None (the entry); returns (col, path)"""
    col, path = [-1] * M, []
    state, i, k = "M", i_end, k_end
    while True:
        path.append((state, i, k))
        if state == "M":
            col[k - 1] = i
            prev = codes[("M", i, k)]
            if prev is None:
                break
            state, i, k = prev, i - 1, k - 1
        elif state == "I":
            state, i = codes[("I", i, k)], i - 1
        else:
            state, k = codes[("D", i, k)], k - 1
        assert i >= i0 and k >= 1
    return col, path[::-1]


def align_plain(res, i0, prof):
    M, e, t, entry = prof["M"], prof["emis"].tolist(), prof["trans"].tolist(), int(prof["entry"])

    def first_max(terms):
        """(value, name) of the first term that equals the maximum over the existing ones; (None, first name) when none exists"""
        real = [v for v, _ in terms if v is not None]
        if not real:
            return None, terms[0][1]
        top = max(real)
        for v, name in terms:
            if v == top:
                return v, name

    def add(v, x):
        return None if v is None else (v[0] + x, v[1])
    pm, pi, pd, codes, hit = {}, {}, {}, {}, None
    for r, x in enumerate(res):
        i = i0 + r
        cm, ci, cd = {}, {}, {}
        for k in range(1, M + 1):
            tp = t[k - 2] if k >= 2 else None
            terms = [((entry, -(i * 2048 + (k - 1))), None)]
            if k >= 2:
                terms += [(add(pm.get(k - 1), tp[MM]), "M"), (add(pi.get(k - 1), tp[IM]), "I"), (add(pd.get(k - 1), tp[DM]), "D")]
            v, codes[("M", i, k)] = first_max(terms)
            cm[k] = add(v, e[k - 1][x])
            if k <= M - 1:
                ci[k], codes[("I", i, k)] = first_max([(add(pm.get(k), t[k - 1][MI]), "M"), (add(pi.get(k), t[k - 1][II]), "I")])
            if k >= 2:
                cd[k], codes[("D", i, k)] = first_max([(add(cm.get(k - 1), tp[MD]), "M"), (add(cd.get(k - 1), tp[DD]), "D")])
            key = (cm[k][0], cm[k][1], -i, -k)
            if hit is None or key > hit:
                hit = key
        pm, pi, pd = cm, {k: v for k, v in ci.items() if v is not None}, {k: v for k, v in cd.items() if v is not None}
    score, start, i_end, k_end = hit[0], -hit[1], -hit[2], -hit[3]
    col, path = trace(codes, M, i0, i_end, k_end)
    return [score, start >> 11, i_end, (start & 2047) + 1, k_end], col, path


_SH = 26
_MASK = (1 << _SH) - 1
_NONE = -(1 << 62)
_LOW = -(1 << 61)


def _norm(a):
    a[a < _LOW] = _NONE
    return a


def align(res, i0, prof):
    M, n = prof["M"], len(res)
    assert 1 <= n <= MAXWIN and n + M < 1 << 14
    T, E = prof["trans"].astype(np.int64) << _SH, prof["emis"].astype(np.int64) << _SH
    entry = int(prof["entry"]) << _SH
    S = np.concatenate(([0], np.cumsum(T[:, DD])))
    ks = np.arange(M, dtype=np.int64)
    pM = np.full(M + 1, _NONE, np.int64)
    pI, pD = pM.copy(), pM.copy()
    plane = np.zeros((n, M), np.uint8)      # bits 0-1 M (0 entry, 1 M, 2 I, 3 D), bit 2 I (0 M, 1 I), bit 3 D (0 M, 1 D)
    best = (_NONE, 0, 0)
    for r, x in enumerate(res):
        i = i0 + r
        cM, cI, cD = np.full(M + 1, _NONE, np.int64), np.full(M + 1, _NONE, np.int64), np.full(M + 1, _NONE, np.int64)
        b0 = entry + (_MASK - (i * 2048 + ks))
        top = b0.copy()
        if M >= 2:
            b1, b2, b3 = _norm(pM[1:M] + T[:M - 1, MM]), _norm(pI[1:M] + T[:M - 1, IM]), _norm(pD[1:M] + T[:M - 1, DM])
            top[1:] = np.maximum(np.maximum(np.maximum(b0[1:], b1), b2), b3)
            plane[r, 1:] = np.where(top[1:] == b0[1:], 0, np.where(top[1:] == b1, 1, np.where(top[1:] == b2, 2, 3)))
            a, b = _norm(pM[1:M] + T[:M - 1, MI]), _norm(pI[1:M] + T[:M - 1, II])
            cI[1:M] = np.maximum(a, b)
            plane[r, :M - 1] |= np.where(cI[1:M] == a, 0, 4).astype(np.uint8)
        cM[1:] = top + E[:, x]
        if M >= 2:
            first = cM[1:M] + T[:M - 1, MD]
            cD[2:] = np.maximum.accumulate(first - S[1:M]) + S[1:M]
            plane[r, 1:] |= np.where(cD[2:] == first, 0, 8).astype(np.uint8)
        k = int(np.argmax(cM[1:])) + 1
        if int(cM[k]) > best[0]:
            best = (int(cM[k]), i, k)
        pM, pI, pD = cM, cI, cD
    w, i_end, k_end = best
    score, start = w >> _SH, _MASK - (w & _MASK)
    codes = _Codes(plane, i0)
    col, path = trace(codes, M, i0, i_end, k_end)
    return [score, start >> 11, i_end, (start & 2047) + 1, k_end], col, path


class _Codes:
    def __init__(self, plane, i0):
        self.plane, self.i0 = plane, i0

    def __getitem__(self, key):
        state, i, k = key
        b = int(self.plane[i - self.i0, k - 1])
        if state == "M":
            return (None, "M", "I", "D")[b & 3]
        return ("M", "I")[(b >> 2) & 1] if state == "I" else ("M", "D")[(b >> 3) & 1]


def path_score(path, res, i0, prof):
    """the entry, emissions and transitions of a path, re-added from the tables"""
    e, t = prof["emis"], prof["trans"]
    total = int(prof["entry"])
    for q, (state, i, k) in enumerate(path):
        if state == "M":
            total += int(e[k - 1][res[i - i0]])
        if q:
            ps, pi, pk = path[q - 1]
            total += int(t[pk - 1][{"MM": MM, "MI": MI, "MD": MD, "IM": IM, "II": II, "DM": DM, "DD": DD}[ps + state]])
            assert (i - pi, k - pk) == {"M": (1, 1), "I": (1, 0), "D": (0, 1)}[state]
    return total


def align_items(seqs, items, profs, engine=align):
    """the outputs of Context.dom_align for items (sequence index, frame, i0, i1, profile index): (hit int32 [n, 5], col
    int32 flat, coff int64 [n + 1])"""
    hits, cols, coff = [], [], [0]
    for s, f, i0, i1, p in items:
        hit, col, _ = engine(window_residues(seqs[s], f, i0, i1), i0, profs[p])
        hits.append(hit)
        cols += col
        coff.append(len(cols))
    return np.array(hits, np.int32).reshape(len(items), 5), np.array(cols, np.int32), np.array(coff, np.int64)


def aln_pairs(rows):
    """(same, both) int32 [N, N] of uint8 rows [N, C]: a residue is a byte below 20"""
    rows = np.asarray(rows, np.uint8)
    N = rows.shape[0]
    ok = rows < 20
    same, both = np.zeros((N, N), np.int32), np.zeros((N, N), np.int32)
    for a in range(N):
        pair = ok & ok[a]
        both[a] = pair.sum(axis=1)
        same[a] = (pair & (rows == rows[a])).sum(axis=1)
    return same, both
