"""Plain Python twin of subphaser_amd/csrc/sp_domains.h, written from the definition in its head comment (not from its
code): frames, the standard genetic code, the pair order, the recurrence, the hit and its tie order.

Two versions of the search of one frame against one profile:
  frame_hit_plain   a triple loop over tuples (score, -start): Python's tuple order IS the pair order.  Slow; tiny cases.
  frames_hits       the same cells a row at a time in numpy on the packed word score * 2^26 + (2^26 - 1 - start), many
                    (frame, profile) jobs side by side; the D chain of a row is a running maximum over prefix sums of the
                    d->d transitions.  frame_hit is one job.  tests/test_domains_host.py compares the two with `==`.
A profile is a dict: M, emis int32 [M, 22], trans int32 [M, 7], entry int.  element() memoises on (sequence, profile id)."""
import math

import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY"
X, STOP = 20, 21
X_COL = X
SCALE = 256
NEG = -(1 << 20)
STOPCOST = 2048
MAXM, MAXLEN, MAXP = 2048, 65536, 4096
INT32_MIN = -(1 << 31)
MM, MI, MD, IM, II, DM, DD = range(7)
# the standard genetic code in the textbook's order of the bases, T C A G
_TCAG = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODON = {a + b + c: _TCAG[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
CODONS_OF = {a: [c for c, r in CODON.items() if r == a] for a in AA + "*"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
BACKGROUND = {a: len(CODONS_OF[a]) / 61.0 for a in AA}


def revcomp(s):
    return "".join(COMP.get(c, "N") for c in reversed(s.upper()))


def translate(seq, f):
    """residue indices of frame f (0..2 forward, 3..5 reverse complement)"""
    s = seq.upper() if f < 3 else revcomp(seq)
    o = f % 3
    out = []
    for j in range((len(s) - o) // 3 if len(s) >= o else 0):
        r = CODON.get(s[o + 3 * j:o + 3 * j + 3])
        out.append(X if r is None else STOP if r == "*" else AA.index(r))
    return out


def entry_score(M):
    return int(math.floor(math.log2(2.0 / (M * (M + 1))) * SCALE + 0.5))


# ------------------------------------------------------------------------------------------------ the triple loop
def frame_hit_plain(res, prof):
    """(score, start, i, k) of the best M cell, or None"""
    M, e, t, entry = prof["M"], prof["emis"].tolist(), prof["trans"].tolist(), int(prof["entry"])
    none = None

    def add(v, x):
        return none if v is none else (v[0] + x, v[1])

    def best(*vs):
        vs = [v for v in vs if v is not none]
        return max(vs) if vs else none
    pm, pi, pd = {}, {}, {}
    hit = None
    for i, x in enumerate(res):
        cm, ci, cd = {}, {}, {}
        for k in range(1, M + 1):
            tp = t[k - 2] if k >= 2 else None
            terms = [(entry, -(i * 2048 + (k - 1)))]
            if i >= 1 and k >= 2:
                terms += [add(pm.get(k - 1), tp[MM]), add(pi.get(k - 1), tp[IM]), add(pd.get(k - 1), tp[DM])]
            cm[k] = add(best(*terms), e[k - 1][x])
            if i >= 1 and k <= M - 1:
                ci[k] = best(add(pm.get(k), t[k - 1][MI]), add(pi.get(k), t[k - 1][II]))
            if k >= 2:
                cd[k] = best(add(cm.get(k - 1), tp[MD]), add(cd.get(k - 1), tp[DD]))
            key = (cm[k][0], cm[k][1], -i, -k)
            if hit is None or key > hit:
                hit = key
        pm, pi, pd = cm, {k: v for k, v in ci.items() if v is not none}, {k: v for k, v in cd.items() if v is not none}
    return None if hit is None else (hit[0], -hit[1], -hit[2], -hit[3])


# ------------------------------------------------------------------------------------------------ a row at a time
_SH = 26
_MASK = (1 << _SH) - 1
_NONE = -(1 << 62)
_LOW = -(1 << 61)


def frames_hits(jobs):
    """[(score, start, i, k) or None] of the jobs [(residues, profile)]: every job's DP advances one row per step, the
    jobs side by side in [J, Mmax + 1] arrays; nodes behind a job's M and rows behind its last residue are masked"""
    J = len(jobs)
    if J == 0:
        return []
    Ms = np.array([p["M"] for _, p in jobs], np.int64)
    Mx, R = int(Ms.max()), max(len(r) for r, _ in jobs)
    assert R + Mx < 1 << 14      # |word| <= (rows + nodes) * 2^21 * 2^26 < 2^61: the sentinel stays apart from every real word
    T, E = np.zeros((J, Mx, 7), np.int64), np.zeros((J, Mx, 22), np.int64)
    X, n = np.full((J, max(R, 1)), X_COL, np.int64), np.array([len(r) for r, _ in jobs], np.int64)
    for j, (r, p) in enumerate(jobs):
        assert np.abs(p["trans"]).max(initial=0) <= 1 << 20 and np.abs(p["emis"]).max(initial=0) <= 1 << 20
        T[j, :p["M"]], E[j, :p["M"]] = p["trans"], p["emis"]
        X[j, :len(r)] = r
    T, E = T << _SH, E << _SH
    entry = np.array([int(p["entry"]) for _, p in jobs], np.int64) << _SH
    S = np.concatenate((np.zeros((J, 1), np.int64), np.cumsum(T[:, :, DD], axis=1)), axis=1)      # S[j]: the d->d transitions of nodes 1 .. j
    ks = np.arange(Mx, dtype=np.int64)
    beyond = np.arange(Mx + 1)[None, :] > Ms[:, None]              # nodes a job does not have
    no_ins = np.arange(Mx + 1)[None, :] >= Ms[:, None]             # I[.][M] does not exist
    rows_j = np.arange(J)
    pM = np.full((J, Mx + 1), _NONE, np.int64)
    pI, pD = pM.copy(), pM.copy()
    best_w, best_i, best_k = np.full(J, _NONE, np.int64), np.zeros(J, np.int64), np.zeros(J, np.int64)
    for i in range(R):
        cM = np.full((J, Mx + 1), _NONE, np.int64)
        cI, cD = cM.copy(), cM.copy()
        cand = entry[:, None] + (_MASK - (i * 2048 + ks))[None, :]
        if Mx >= 2:
            prev = np.maximum(np.maximum(pM[:, 1:Mx] + T[:, :Mx - 1, MM], pI[:, 1:Mx] + T[:, :Mx - 1, IM]), pD[:, 1:Mx] + T[:, :Mx - 1, DM])
            cand[:, 1:] = np.maximum(cand[:, 1:], prev)
            cI[:, 1:Mx] = np.maximum(pM[:, 1:Mx] + T[:, :Mx - 1, MI], pI[:, 1:Mx] + T[:, :Mx - 1, II])
        cM[:, 1:] = cand + E[rows_j, :, X[:, i]]
        cM[beyond] = _NONE
        if Mx >= 2:
            run = np.maximum.accumulate(cM[:, 1:Mx] + T[:, :Mx - 1, MD] - S[:, 1:Mx], axis=1)      # over j = 1 .. k - 1
            cD[:, 2:] = run + S[:, 1:Mx]
        cI[no_ins] = _NONE
        cD[beyond] = _NONE
        for a in (cI, cD):
            a[a < _LOW] = _NONE
        k = np.argmax(cM[:, 1:], axis=1) + 1
        w = cM[rows_j, k]
        take = (i < n) & (w > best_w)
        best_w[take], best_i[take], best_k[take] = w[take], i, k[take]
        pM, pI, pD = cM, cI, cD
    return [None if n[j] == 0 else (int(best_w[j]) >> _SH, _MASK - (int(best_w[j]) & _MASK), int(best_i[j]), int(best_k[j])) for j in range(J)]


def frame_hit(res, prof):
    """(score, start, i, k) of the best M cell, or None"""
    return frames_hits([(res, prof)])[0]


def _best_frame(hits):
    """the six numbers from the hits of the six frames: the best, the lower frame on a tie"""
    best = None
    for f, h in enumerate(hits):
        if h is None:
            continue
        cand = (h[0], -h[1], -h[2], -h[3], -f)
        if best is None or cand > best:
            best = cand
    if best is None:
        return [INT32_MIN, 0, 0, 0, 0, 0]
    s, st, i, k, f = best[0], -best[1], -best[2], -best[3], -best[4]
    return [s, f, st >> 11, i, (st & 2047) + 1, k]


def element(seq, prof, engine=frame_hit, memo=None):
    """the six numbers of an (element, profile): score, frame, i_start, i_end, k_start, k_end"""
    key = (seq, id(prof))
    if memo is not None and key in memo:
        return memo[key]
    out = _best_frame([engine(translate(seq, f), prof) for f in range(6)])
    if memo is not None:
        memo[key] = out
    return out


def search(seqs, profs, memo=None, batch=384):
    """int32 [n, P, 6] of inner sequences (strings) against profiles; the frames of the (sequence, profile) pairs not in
    `memo` are run `batch` at a time, the longest first"""
    memo = {} if memo is None else memo
    todo = sorted({(s, id(p)): (s, p) for s in seqs for p in profs if (s, id(p)) not in memo}.values(), key=lambda sp: -len(sp[0]))
    trans = {}
    for q in range(0, len(todo), max(1, batch // 6)):
        part = todo[q:q + max(1, batch // 6)]
        for s, _ in part:
            if s not in trans:
                trans[s] = [translate(s, f) for f in range(6)]
        hits = frames_hits([(trans[s][f], p) for s, p in part for f in range(6)])
        for j, (s, p) in enumerate(part):
            memo[(s, id(p))] = _best_frame(hits[6 * j:6 * j + 6])
    return np.array([[memo[(s, id(p))] for p in profs] for s in seqs], np.int32).reshape(len(seqs), len(profs), 6)


# ------------------------------------------------------------------------------------------------ profiles
def tables(profs):
    """(moff, emis, trans, entry) of a list of profiles, as Context.dom_search takes them"""
    moff = np.concatenate(([0], np.cumsum([p["M"] for p in profs]))).astype(np.int32)
    return (moff, np.concatenate([p["emis"] for p in profs]).astype(np.int32).reshape(-1, 22),
            np.concatenate([p["trans"] for p in profs]).astype(np.int32).reshape(-1, 7), np.array([p["entry"] for p in profs], np.int32))


def make_profile(M, emis, trans, entry=None, name="p"):
    emis, trans = np.asarray(emis, np.int32).reshape(M, 22), np.asarray(trans, np.int32).reshape(M, 7)
    return {"M": M, "emis": emis, "trans": trans, "entry": entry_score(M) if entry is None else int(entry), "name": name}


def trans_score(p):
    return NEG if p <= 0 else int(math.floor(math.log2(p) * SCALE + 0.5))


def emis_score(p, a):
    return NEG if p <= 0 else int(math.floor((math.log2(p) - math.log2(BACKGROUND[a])) * SCALE + 0.5))


def consensus_profile(rng, consensus, p_cons=0.8, p_indel=0.01, p_ext=0.4, name="p"):
    """A profile whose node k emits consensus[k] with p_cons and the others by the background, with HMMER-like gap
    transitions.  Returns the profile; its probabilities are in profile["probs"] (for an .hmm text)."""
    M = len(consensus)
    emis, trans, probs = np.zeros((M, 22), np.int64), np.zeros((M, 7), np.int64), []
    for k, c in enumerate(consensus):
        rest = 1.0 - BACKGROUND[c]
        pe = {a: p_cons if a == c else (1.0 - p_cons) * BACKGROUND[a] / rest for a in AA}
        last = k == M - 1
        pt = [1.0 - 2 * p_indel, p_indel, p_indel, 1.0 - p_ext, p_ext, 1.0 - p_ext, p_ext]
        if last:
            pt = [1.0 - p_indel, p_indel, 0.0, 1.0 - p_ext, p_ext, 1.0, 0.0]
        probs.append((pe, pt))
        emis[k, :20] = [emis_score(pe[a], a) for a in AA]
        emis[k, STOP] = -STOPCOST
        trans[k] = [trans_score(p) for p in pt]
    prof = make_profile(M, emis, trans, name=name)
    prof["probs"] = probs
    return prof


def random_profile(rng, M, star=0.0, name="p"):
    """integer tables straight from a random generator: emissions -1500..1500, transitions -2500..0, `*` with
    probability `star`"""
    emis = np.array([[rng.randint(-1500, 1500) for _ in range(20)] + [0, -STOPCOST] for _ in range(M)], np.int64)
    trans = np.array([[NEG if rng.random() < star else -rng.randint(0, 2500) for _ in range(7)] for _ in range(M)], np.int64)
    return make_profile(M, emis, trans, name=name)


def rand_dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rand_protein(rng, n):
    """residues drawn by the background (no stop)"""
    pool = [CODON[c] for c in CODON if CODON[c] != "*"]
    return "".join(rng.choice(pool) for _ in range(n))


def back_translate(rng, protein):
    return "".join(rng.choice(CODONS_OF[a]) for a in protein)


def hmm_text(profs, compo=True, version="HMMER3/f [3.1b2 | February 2015]", annot=True):
    """a HMMER3 ASCII file of profiles that carry "probs" (consensus_profile)"""
    def val(p):
        return "*" if p <= 0 else "%.5f" % (-math.log(p))
    out = []
    for prof in profs:
        M = prof["M"]
        out += [version, "NAME  %s" % prof["name"], "ACC   PF00000.1", "LENG  %d" % M, "ALPH  amino", "RF    no", "CS    no",
                "STATS LOCAL MSV      -9.9000  0.70000", "HMM          " + "        ".join(AA),
                "            m->m     m->i     m->d     i->m     i->i     d->m     d->d"]
        bg = "  ".join(val(BACKGROUND[a]) for a in AA)
        if compo:
            out.append("  COMPO   " + bg)
        out += ["          " + bg, "          " + "  ".join(val(p) for p in (0.99, 0.005, 0.005, 0.6, 0.4, 1.0, 0.0))]
        for k, (pe, pt) in enumerate(prof["probs"], 1):
            out.append("%7d   %s%s" % (k, "  ".join(val(pe[a]) for a in AA), "  %d x - - -" % k if annot else ""))
            out.append("          " + bg)
            out.append("          " + "  ".join(val(p) for p in pt))
        out.append("//")
    return "\n".join(out) + "\n"
