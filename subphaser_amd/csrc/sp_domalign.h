// sp_domalign.h -- the arithmetic of the profile alignment of the LTR stage's domain trees (-ltr_domtree), compiled for
// the host and for the device.  It adds a traceback to the search of sp_domains.h and changes nothing in it.
//
// The reference aligns the domain peptides of its LTR-RTs with mafft.  No alignment program exists here, so the alignment
// of this build is DEFINED by the arithmetic below -- the Viterbi path of sp_domains.h's local search, residues placed on
// the match nodes of ONE profile -- and is never compared with mafft.  tests/domalign_ref.py is the plain Python twin,
// written from this definition and compared with `==`.
//
// Item: (interval of the genome, frame f, residue window [i0, i1] of that frame, profile p).  The recurrences, the pair
//   order, the packed word and the hit order are exactly those of sp_domains.h, run over the rows i0 .. i1 only (a row
//   before i0 does not exist: its terms are dropped as those of row -1 are there) and over all nodes of p.  The indices i
//   in `start` and in the outputs stay indices of the FRAME, not of the window.  1 <= i1 - i0 + 1 <= SP_DA_MAXWIN.
// Back-pointers.  The argument that attains a maximum is the FIRST one, in the order sp_dm_match / sp_dm_insert /
//   sp_dm_delete evaluate them, that equals the result (sp_dm_max keeps its left argument on a tie, so this is what the
//   search already "chooses"):
//     M: entry (0), M (1), I (2), D (3)      I: M (0), I (1)      D: M (0), D (1)
//   The entry term can never tie with a predecessor as a whole word: its start is the cell itself, and a predecessor's
//   path started in an earlier row or at a lower node, so the two words differ in their start bits.  Tied predecessors
//   are equal words and so share their start: the traced path always begins at the start the hit's word carries.
//   One byte per cell holds the three codes: bits 0-1 (M), bit 2 (I), bit 3 (D).  A cell whose predecessors all do not
//   exist has code 0 in I and D; the trace never reaches such a cell (a path runs over existing cells only).
// Trace.  From the hit (the best M cell, sp_domains.h's order) back: an M cell (i, k) puts i into col[k]; code 0 ends the
//   path, codes 1..3 go to M, I, D of (i - 1, k - 1).  An I cell (i, k) goes to M or I of (i - 1, k); a D cell (i, k) to M
//   or D of (i, k - 1).
// Outputs per item:
//   hit  = score, i_start, i_end, k_start, k_end, formed as sp_dm_result forms them (there is always a hit: the window has
//          a residue and the profile a node).
//   col  [M_p]: for node k (entry k - 1) the frame index of the residue in that node's match state; -1 for a node the path
//          deletes and for the nodes outside k_start .. k_end.
//   LIMIT of the alignment: inserted residues (I states) appear in no column.  Two rows are compared on match columns
//   only, as hmmalign's --trim / --outformat with match columns only would be.
// Limits: a window of at most SP_DA_MAXWIN = 8192 residues and M <= SP_DM_MAXM = 2048, so the back-pointer plane of an
//   item (one byte per cell, rows of SP_DA_PITCH(M) bytes) is at most 16 MiB.
#pragma once
#include "sp_domains.h"

#define SP_DA_MAXWIN 8192
#define SP_DA_PITCH(M) (((M) + 3) & ~3)      // bytes of a plane row: whole 32-bit words

// the codes of the three cells (arguments as sp_dm_match / sp_dm_insert / sp_dm_delete take them)
SP_DM_HD inline int sp_da_bp_match(int64_t m, int64_t i, int64_t d, int tmm, int tim, int tdm, int entry, int64_t start) {
    const int64_t b0 = sp_dm_pack(entry, start), b1 = sp_dm_add(m, tmm), b2 = sp_dm_add(i, tim), b3 = sp_dm_add(d, tdm);
    const int64_t b = sp_dm_max(sp_dm_max(sp_dm_max(b0, b1), b2), b3);
    return b == b0 ? 0 : b == b1 ? 1 : b == b2 ? 2 : 3;
}
SP_DM_HD inline int sp_da_bp_insert(int64_t m, int64_t i, int tmi, int tii) {
    return sp_dm_insert(m, i, tmi, tii) == sp_dm_add(m, tmi) ? 0 : 1;
}
SP_DM_HD inline int sp_da_bp_delete(int64_t m, int64_t d, int tmd, int tdd) {
    return sp_dm_delete(m, d, tmd, tdd) == sp_dm_add(m, tmd) ? 0 : 1;
}
SP_DM_HD inline uint8_t sp_da_byte(int cm, int ci, int cd) { return (uint8_t)(cm | (ci << 2) | (cd << 3)); }

// the five numbers of an item from its hit
SP_DM_HD inline void sp_da_result(const sp_dm_hit &h, int32_t *out) {
    const int64_t st = sp_dm_start(h.w);
    out[0] = (int32_t)sp_dm_score(h.w);
    out[1] = (int32_t)(st >> 11);
    out[2] = h.i;
    out[3] = (int32_t)(st & 2047) + 1;
    out[4] = h.k;
}

// Walks the plane back from the M cell (i_end, k_end) and fills col (M entries, all -1 before the call).  plane: row
// i - i0 at plane + (i - i0) * SP_DA_PITCH(M), node k at byte k - 1.  A path has fewer than nwin + M steps and never
// leaves the window or the profile; the loop is bounded by both all the same.  Returns the steps taken.
SP_DM_HD inline int sp_da_trace(const uint8_t *plane, int M, int32_t i0, int32_t nwin, int32_t i_end, int32_t k_end, int32_t *col) {
    const int64_t pitch = SP_DA_PITCH(M);
    int32_t i = i_end, k = k_end;
    int state = 0, steps = 0;      // 0 M, 1 I, 2 D
    while (i >= i0 && i < i0 + nwin && k >= 1 && k <= M && steps < nwin + M) {
        const int b = plane[(int64_t)(i - i0) * pitch + (k - 1)];
        steps++;
        if (state == 0) {
            col[k - 1] = i;
            const int c = b & 3;
            if (c == 0) break;
            state = c - 1;
            i--;
            k--;
        } else if (state == 1) {
            state = (b >> 2) & 1 ? 1 : 0;
            i--;
        } else {
            state = (b >> 3) & 1 ? 2 : 0;
            k--;
        }
    }
    return steps;
}

// ---- host drivers: a full plane, filled row by row, node by node, then traced
// res: the nwin residues of the window (res[0] is row i0 of the frame); row: 6 (M + 1) words of scratch; plane:
// nwin * SP_DA_PITCH(M) bytes; hit: 5 numbers; col: M numbers
static inline void sp_da_host_item(const uint8_t *res, int32_t i0, int32_t nwin, int M, const int32_t *emis, const int32_t *trans, int32_t entry,
                                   int64_t *row, uint8_t *plane, int32_t *hit, int32_t *col) {
    int64_t *pM = row, *pI = row + (M + 1), *pD = row + 2 * (M + 1), *cM = row + 3 * (M + 1), *cI = row + 4 * (M + 1), *cD = row + 5 * (M + 1);
    for (int q = 0; q < 6 * (M + 1); q++) row[q] = SP_DM_NONE;
    const int64_t pitch = SP_DA_PITCH(M);
    sp_dm_hit best = sp_dm_nohit();
    for (int32_t r = 0; r < nwin; r++) {
        const int32_t i = i0 + r;
        const int x = res[r];
        cM[0] = cI[0] = cD[0] = SP_DM_NONE;
        for (int k = 1; k <= M; k++) {
            const int32_t *tp = trans + 7 * (k >= 2 ? k - 2 : 0), *tk = trans + 7 * (k - 1);
            const int64_t start = (int64_t)i * 2048 + (k - 1);
            cM[k] = sp_dm_match(pM[k - 1], pI[k - 1], pD[k - 1], tp[SP_DM_MM], tp[SP_DM_IM], tp[SP_DM_DM], entry, start,
                                emis[(int64_t)(k - 1) * SP_DM_COLS + x]);
            const int bm = sp_da_bp_match(pM[k - 1], pI[k - 1], pD[k - 1], tp[SP_DM_MM], tp[SP_DM_IM], tp[SP_DM_DM], entry, start);
            int bi = 0, bd = 0;
            cI[k] = SP_DM_NONE;
            if (k <= M - 1) {
                cI[k] = sp_dm_insert(pM[k], pI[k], tk[SP_DM_MI], tk[SP_DM_II]);
                bi = sp_da_bp_insert(pM[k], pI[k], tk[SP_DM_MI], tk[SP_DM_II]);
            }
            cD[k] = SP_DM_NONE;
            if (k >= 2) {
                cD[k] = sp_dm_delete(cM[k - 1], cD[k - 1], tp[SP_DM_MD], tp[SP_DM_DD]);
                bd = sp_da_bp_delete(cM[k - 1], cD[k - 1], tp[SP_DM_MD], tp[SP_DM_DD]);
            }
            plane[(int64_t)r * pitch + (k - 1)] = sp_da_byte(bm, bi, bd);
            const sp_dm_hit h = sp_dm_hit{cM[k], i, k};
            if (sp_dm_better(h, best)) best = h;
        }
        int64_t *t;
        t = pM, pM = cM, cM = t;
        t = pI, pI = cI, cI = t;
        t = pD, pD = cD, cD = t;
    }
    sp_da_result(best, hit);
    for (int k = 0; k < M; k++) col[k] = -1;
    sp_da_trace(plane, M, i0, nwin, best.i, best.k, col);
}

// ---- the pair comparison of aligned rows (sp_aln_pairs): a residue is a byte 0..19, anything else is "no residue"
#define SP_DA_NRES 20
#define SP_DA_GAP 255
#define SP_DA_MAXN 4096
#define SP_DA_MAXC 8192
// the comparison itself runs eight bytes at a time: sp_swar_lt20_bytes, sp_swar_eq_bytes (sp_swar.h)
