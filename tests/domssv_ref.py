"""Plain Python twin of the ungapped prefilter of subphaser_amd/csrc/sp_domains.h, written from the definition in its head
comment (not from its code):

    S[i][k] = e[k][x_i] + max( entry, S[i-1][k-1] + tMM[k-1] )        (the second term only when i >= 1 and k >= 2)
    ssv     = max over all cells;  a frame without residues has none (INT32_MIN)

  ssv_frame_plain   a double loop over Python integers.  Slow; small cases.
  ssv_frame         the same cells a row at a time in numpy (int64).  tests/test_domssv_host.py compares the two with `==`,
                    and both with the maximum over every ungapped segment summed directly (ssv_brute).
  ssv_frames        many frames against one profile, a NODE at a time in numpy, the frames side by side.
  ssv               int32 [n, P, 6] of inner sequences against profiles, as Context.dom_ssv returns it (by ssv_frames).
  search            the filtered search: domains_ref's hit of every frame, the frames with ssv < T dropped, then
                    domains_ref's best-frame rule -- what sp_dom_search_pre computes.  Returns (int32 [n, P, 6], items with
                    residues, items that passed).
A profile is domains_ref's dict."""
import numpy as np

import domains_ref as dr

INT32_MIN = dr.INT32_MIN


def ssv_frame_plain(res, prof):
    M, e, t, entry = prof["M"], prof["emis"].tolist(), prof["trans"].tolist(), int(prof["entry"])
    best, prev = None, {}
    for i, x in enumerate(res):
        cur = {}
        for k in range(1, M + 1):
            into = entry
            if i >= 1 and k >= 2:
                into = max(into, prev[k - 1] + t[k - 2][dr.MM])
            cur[k] = e[k - 1][x] + into
            if best is None or cur[k] > best:
                best = cur[k]
        prev = cur
    return INT32_MIN if best is None else best


def ssv_frame(res, prof):
    M, entry = prof["M"], int(prof["entry"])
    if len(res) == 0:
        return INT32_MIN
    E = prof["emis"].astype(np.int64)
    tmm = prof["trans"][:M - 1, dr.MM].astype(np.int64)      # tMM of nodes 1 .. M - 1: what enters nodes 2 .. M
    S = E[:, res[0]] + entry
    best = int(S.max())
    for x in res[1:]:
        into = np.full(M, entry, np.int64)
        if M >= 2:
            into[1:] = np.maximum(into[1:], S[:-1] + tmm)
        S = E[:, x] + into
        best = max(best, int(S.max()))
    return best


def ssv_brute(res, prof):
    """the maximum over every ungapped segment: start cell (i, k), length L; entry + the emissions + the transitions between"""
    M, e, t, entry = prof["M"], prof["emis"].tolist(), prof["trans"].tolist(), int(prof["entry"])
    best = None
    for i in range(len(res)):
        for k in range(1, M + 1):
            for L in range(1, min(len(res) - i, M - k + 1) + 1):
                s = entry + sum(e[k - 1 + q][res[i + q]] for q in range(L)) + sum(t[k - 1 + q][dr.MM] for q in range(L - 1))
                if best is None or s > best:
                    best = s
    return INT32_MIN if best is None else best


def ssv_frames(frames, prof, cells=1 << 22):
    """[ssv] of many frames (lists of residues) against one profile: the same cells a NODE at a time, the frames side by
    side in [J, R] arrays (residues behind a frame's last one are masked), at most `cells` array entries a batch"""
    M, entry = prof["M"], int(prof["entry"])
    E, tmm = prof["emis"].astype(np.int64), prof["trans"][:, dr.MM].astype(np.int64)
    out = [INT32_MIN] * len(frames)
    order = sorted((j for j in range(len(frames)) if len(frames[j])), key=lambda j: -len(frames[j]))
    low = -(1 << 40)
    while order:
        R = len(frames[order[0]])
        part, order = order[:max(1, cells // R)], order[max(1, cells // R):]
        X = np.zeros((len(part), R), np.int64)
        live = np.zeros((len(part), R), bool)
        for a, j in enumerate(part):
            X[a, :len(frames[j])] = frames[j]
            live[a, :len(frames[j])] = True
        best = np.full(len(part), low, np.int64)
        S = None
        for k in range(1, M + 1):
            into = np.full(X.shape, entry, np.int64)
            if k >= 2:
                into[:, 1:] = np.maximum(into[:, 1:], S[:, :-1] + tmm[k - 2])      # S[i-1][k-1]: the residue in front, the node in front
            S = np.where(live, E[k - 1][X] + into, low)
            best = np.maximum(best, S.max(axis=1))
        for a, j in enumerate(part):
            out[j] = int(best[a])
    return out


def ssv(seqs, profs, memo=None):
    """int32 [n, P, 6]; memo: {(sequence, profile id): the six scores}"""
    memo = {} if memo is None else memo
    trans = {}
    for p in profs:
        todo = sorted({s for s in seqs if (s, id(p)) not in memo})
        for s in todo:
            if s not in trans:
                trans[s] = [dr.translate(s, f) for f in range(6)]
        got = ssv_frames([trans[s][f] for s in todo for f in range(6)], p)
        for q, s in enumerate(todo):
            memo[(s, id(p))] = got[6 * q:6 * q + 6]
    return np.array([[memo[(s, id(p))] for p in profs] for s in seqs], np.int64).reshape(len(seqs), len(profs), 6).astype(np.int32)


def search(seqs, profs, T, hit_memo=None, ssv_memo=None):
    """(int32 [n, P, 6], items with residues, items that passed) of the search behind the prefilter at threshold T.  Only
    the frames that pass are searched (the others have no hit whatever theirs would be).
    hit_memo: {(sequence, profile id, frame): the frame's hit (domains_ref.frames_hits)}"""
    hit_memo = {} if hit_memo is None else hit_memo
    scores = ssv(seqs, profs, ssv_memo)
    todo = {}
    for a, s in enumerate(seqs):
        for b, p in enumerate(profs):
            for f in range(6):
                if scores[a, b, f] != INT32_MIN and scores[a, b, f] >= T and (s, id(p), f) not in hit_memo:
                    todo[(s, id(p), f)] = (s, p, f)
    todo = sorted(todo.values(), key=lambda spf: -len(spf[0]))
    for q in range(0, len(todo), 384):
        part = todo[q:q + 384]
        hits = dr.frames_hits([(dr.translate(s, f), p) for s, p, f in part])
        for (s, p, f), h in zip(part, hits):
            hit_memo[(s, id(p), f)] = h
    out = np.empty((len(seqs), len(profs), 6), np.int64)
    items = passed = 0
    for a, s in enumerate(seqs):
        for b, p in enumerate(profs):
            hits = [None] * 6
            for f in range(6):
                if scores[a, b, f] == INT32_MIN:      # no residue: no item
                    continue
                items += 1
                if scores[a, b, f] >= T:
                    passed += 1
                    hits[f] = hit_memo[(s, id(p), f)]
            out[a, b] = dr._best_frame(hits)
    return out.astype(np.int32), items, passed
