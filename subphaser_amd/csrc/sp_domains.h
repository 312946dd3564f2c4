// sp_domains.h -- the arithmetic of the protein-domain search of the LTR stage, compiled for the host and for the device.
//
// The reference classifies its LTR-RTs with TEsorter: hmmscan of the six-frame translation of every element against
// REXdb's profile HMMs.  Neither HMMER nor a profile database exists here, so the search of this build is DEFINED by the
// integer arithmetic below -- a local Viterbi alignment of one translated frame to one profile, one hit per (frame,
// profile) -- and is never compared with hmmscan.  tests/domains_ref.py is the plain Python twin, written from this
// definition and compared with `==`.  The step from a HMMER3 text file to the integer tables is host arithmetic, done
// once, in float64 (subphaser_amd/domains.py: read_hmm); nothing below ever sees a float.
//
// Tables of a profile of M nodes (1 <= M <= SP_DM_MAXM), scores in units of 1 / SP_DM_SCALE bit:
//   emis   M x 22: the match emission of node k (row k - 1) for residue x.  Columns 0..19 are A C D E F G H I K L M N P Q
//          R S T V W Y; column 20 (SP_DM_X) is a codon with an invalid base, 0 by read_hmm; column 21 (SP_DM_STOP) a stop
//          codon, -SP_DM_STOPCOST by read_hmm.  Insert emissions score 0 (as in HMMER's local profiles) and have no table.
//          read_hmm's background is the codon composition of translated random DNA (codons of the residue over 61), a
//          PROVISIONAL constant of the definition and not HMMER's Swiss-Prot composition.
//   trans  M x 7: of node k (row k - 1), in HMMER's order m->m, m->i, m->d, i->m, i->i, d->m, d->d; a `*` of the file is
//          SP_DM_NEG = -2^20, a finite number: such a step is very expensive, not impossible.
//   entry  one number: floor(log2(2 / (M (M + 1))) * 256 + 0.5), HMMER's uniform local entry.  Leaving a match state costs 0.
//   No length model, no flanking loops, no multi-hit loop.
//   The C entry takes  -2^20 <= trans, entry <= 0  and  -2^20 <= emis <= 2^15  (SP_DM_EMAX).
// Frames of an inner sequence of n bases (0 <= n <= SP_DM_MAXLEN): 0..2 start at offsets 0, 1, 2 of the forward strand,
//   3..5 at offsets 0, 1, 2 of the reverse complement.  Frame f has floor((n - f mod 3) / 3) residues (none when n is
//   below f mod 3), translated by the standard genetic code; a codon with an invalid base is SP_DM_X.
// A cell value is a pair (score, start); start = i_start * 2048 + (k_start - 1), i the 0-based residue index in the frame,
//   k the 1-based node.  Pairs are ordered by higher score, then by smaller start; adding a number adds to the score only,
//   which keeps the order of two pairs, so every max below is over a total order that + distributes over: no result
//   depends on the evaluation order, and the chain of D along a row is a legal (max, +) scan.
//     M[i][k] = e[k][x_i] + max( (entry, start (i, k)),  M[i-1][k-1] + tMM[k-1],  I[i-1][k-1] + tIM[k-1],  D[i-1][k-1] + tDM[k-1] )
//     I[i][k] = max( M[i-1][k] + tMI[k],    I[i-1][k] + tII[k] )          1 <= k <= M - 1
//     D[i][k] = max( M[i][k-1] + tMD[k-1],  D[i][k-1] + tDD[k-1] )        2 <= k <= M
//   Terms that refer to row -1, node 0, I[.][M] or D[.][1] do not exist.
// Hit of a (frame, profile): the best M cell -- higher score, then smaller start, then smaller i, then smaller k.  Hit of an
//   (element, profile): the best over the six frames, the lower frame on a tie; a frame without residues has none.
//   out = score, frame, i_start, i_end, k_start, k_end (i 0-based, k 1-based, both inclusive); an element without residues
//   in any frame: score = INT32_MIN and zeros.
// Ranges.  M <= 2048 = 2^11 and at most 21845 < 2^15 residues, so start < 2^15 * 2^11 = 2^26.  A step of a path consumes a
//   residue (M, I) or a node (D), and a path never goes back in either, so it has fewer than 2^15 + 2^11 steps; a step adds
//   one transition or the entry and at most one emission, each of magnitude <= 2^20, so |score| < (2^15 + 2^11) * 2^21
//   = 2^36 + 2^32 < 2^37: a score fits in 38 signed bits, and a pair in one 64-bit word  w = score * 2^26 + (2^26 - 1 - start), whose order as a signed integer IS the order
//   of the pairs.  INT64_MIN is no such word (|w| < 2^63 - 2^26) and stands for "does not exist" (SP_DM_NONE).
//   The hit's score fits int32: the best cell is at least a one-cell path, entry + e >= -2^21, and at most 21845 emissions of
//   at most 2^15 each with transitions and entry <= 0: below 2^15 * 2^15 = 2^30.
//
// The ungapped prefilter (SSV).  The score of one frame against one profile is the recurrence above restricted to the
//   match states -- the best ungapped segment, a score only: no start, no end, no tie rule:
//     S[i][k] = e[k][x_i] + max( entry, S[i-1][k-1] + tMM[k-1] )        (the second term only when i >= 1 and k >= 2)
//     ssv     = max over all cells S[i][k];  a frame without residues has none (INT32_MIN)
//   Tables, columns and entry are those of M[i][k]; tMM[k-1] is trans[7 (k - 2) + SP_DM_MM].  A cell depends on its
//   diagonal i - k alone, and the maximum is one of integers: no result depends on the order the cells are visited in.
//   Range.  S >= entry + e >= -2^21.  S is at most 21845 emissions of at most 2^15 each (transitions and entry <= 0), so
//   S < 21845 * 2^15 < 2^30.  A predecessor that does not exist is SP_DM_SSV_NONE = -2^30: NONE + tMM >= -2^30 - 2^20 does
//   not wrap and lies below every entry (>= -2^20), so the max takes the entry.  int32 throughout, no saturation.
//   Bound.  S[i][k] <= score(M[i][k]) by induction over the cells: both take the entry, M[i][k] takes the maximum over a
//   superset of S's terms, and S[i-1][k-1] <= score(M[i-1][k-1]) is the hypothesis.  Hence ssv <= the score of the frame's
//   Viterbi hit.  A search that keeps only the frames with ssv >= T is a HEURISTIC: a domain whose best ungapped segment
//   scores below T is lost, however well its gapped alignment scores.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SP_DM_HD __host__ __device__
#else
#define SP_DM_HD
#endif

#define SP_DM_SCALE 256
#define SP_DM_NEG (-(1 << 20))
#define SP_DM_EMAX (1 << 15)
#define SP_DM_STOPCOST 2048          // 8 bits
#define SP_DM_MAXM 2048
#define SP_DM_MAXLEN 65536
#define SP_DM_MAXP 4096
#define SP_DM_COLS 22
#define SP_DM_X 20
#define SP_DM_STOP 21
#define SP_DM_STARTBITS 26
#define SP_DM_STARTMASK ((1LL << SP_DM_STARTBITS) - 1LL)
#define SP_DM_NONE INT64_MIN
#define SP_DM_INVALID 4              // a base code that is no A, C, G, T
// transitions, HMMER's order
#define SP_DM_MM 0
#define SP_DM_MI 1
#define SP_DM_MD 2
#define SP_DM_IM 3
#define SP_DM_II 4
#define SP_DM_DM 5
#define SP_DM_DD 6

// residue of the codon (c0, c1, c2), base codes A = 0, C = 1, G = 2, T = 3, anything else invalid
SP_DM_HD inline int sp_dm_codon(unsigned c0, unsigned c1, unsigned c2) {
    // index 16 c0 + 4 c1 + c2 -> "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF" as columns
    const uint8_t code[64] = {8, 11, 8, 11, 16, 16, 16, 16, 14, 15, 14, 15, 7, 7, 10, 7, 13, 6, 13, 6, 12, 12, 12, 12, 14, 14, 14, 14, 9, 9, 9, 9,
                              3, 2, 3, 2, 0, 0, 0, 0, 5, 5, 5, 5, 17, 17, 17, 17, 21, 19, 21, 19, 15, 15, 15, 15, 21, 1, 18, 1, 9, 4, 9, 4};
    if (c0 > 3u || c1 > 3u || c2 > 3u) return SP_DM_X;
    return code[16u * c0 + 4u * c1 + c2];
}
// residues of frame f of n bases
SP_DM_HD inline int32_t sp_dm_nres(int64_t n, int f) {
    const int o = f % 3;
    return n < o ? 0 : (int32_t)((n - o) / 3);
}
// where base t (0..2) of residue j of frame f lies in the interval of n bases, and whether it is complemented
SP_DM_HD inline int64_t sp_dm_pos(int64_t n, int f, int64_t j, int t) {
    const int64_t p = f % 3 + 3 * j + t;
    return f < 3 ? p : n - 1 - p;
}
SP_DM_HD inline unsigned sp_dm_strand(int f, unsigned c) { return (f < 3 || c > 3u) ? c : 3u - c; }

// the pair (score, start) as one word, and the word plus a number
SP_DM_HD inline int64_t sp_dm_pack(int64_t score, int64_t start) { return score * (1LL << SP_DM_STARTBITS) + (SP_DM_STARTMASK - start); }
SP_DM_HD inline int64_t sp_dm_add(int64_t w, int64_t t) { return w == SP_DM_NONE ? w : w + t * (1LL << SP_DM_STARTBITS); }
SP_DM_HD inline int64_t sp_dm_max(int64_t a, int64_t b) { return a > b ? a : b; }
SP_DM_HD inline int64_t sp_dm_score(int64_t w) { return (w - (w & SP_DM_STARTMASK)) / (1LL << SP_DM_STARTBITS); }
SP_DM_HD inline int64_t sp_dm_start(int64_t w) { return SP_DM_STARTMASK - (w & SP_DM_STARTMASK); }

// the three updates of a cell; the arguments are the words of the predecessors (SP_DM_NONE: does not exist)
SP_DM_HD inline int64_t sp_dm_match(int64_t m, int64_t i, int64_t d, int tmm, int tim, int tdm, int entry, int64_t start, int e) {
    int64_t b = sp_dm_pack(entry, start);
    b = sp_dm_max(b, sp_dm_add(m, tmm));
    b = sp_dm_max(b, sp_dm_add(i, tim));
    b = sp_dm_max(b, sp_dm_add(d, tdm));
    return sp_dm_add(b, e);
}
SP_DM_HD inline int64_t sp_dm_insert(int64_t m, int64_t i, int tmi, int tii) { return sp_dm_max(sp_dm_add(m, tmi), sp_dm_add(i, tii)); }
SP_DM_HD inline int64_t sp_dm_delete(int64_t m, int64_t d, int tmd, int tdd) { return sp_dm_max(sp_dm_add(m, tmd), sp_dm_add(d, tdd)); }

// the cell of the ungapped prefilter: prev = S[i-1][k-1] or SP_DM_SSV_NONE, tmm = tMM[k-1] (anything in range where prev is NONE)
#define SP_DM_SSV_NONE (-(1 << 30))
SP_DM_HD inline int32_t sp_dm_ssv_cell(int32_t prev, int tmm, int entry, int e) {
    const int32_t through = prev + tmm;
    return e + (through > entry ? through : entry);
}

// a hit: the word of the best M cell and where it ends; k = 0: no hit
struct sp_dm_hit {
    int64_t w;
    int32_t i, k;
};
SP_DM_HD inline sp_dm_hit sp_dm_nohit() { return sp_dm_hit{SP_DM_NONE, 0, 0}; }
// is a better than b?  (a hit beats no hit; equal hits: false)
SP_DM_HD inline bool sp_dm_better(const sp_dm_hit &a, const sp_dm_hit &b) {
    if (a.k == 0) return false;
    if (b.k == 0) return true;
    return a.w > b.w || (a.w == b.w && (a.i < b.i || (a.i == b.i && a.k < b.k)));
}
// the six numbers of an (element, profile) from the hits of its frames
SP_DM_HD inline void sp_dm_result(const sp_dm_hit *frames, int32_t *out) {
    int bf = 0;
    sp_dm_hit b = sp_dm_nohit();
    for (int f = 0; f < 6; f++)
        if (sp_dm_better(frames[f], b)) {
            b = frames[f];
            bf = f;
        }
    if (b.k == 0) {
        out[0] = INT32_MIN;
        for (int q = 1; q < 6; q++) out[q] = 0;
        return;
    }
    const int64_t st = sp_dm_start(b.w);
    out[0] = (int32_t)sp_dm_score(b.w);
    out[1] = bf;
    out[2] = (int32_t)(st >> 11);
    out[3] = b.i;
    out[4] = (int32_t)(st & 2047) + 1;
    out[5] = b.k;
}
// are the tables of one profile in the range the proof above needs?
SP_DM_HD inline bool sp_dm_tables_ok(int M, const int32_t *emis, const int32_t *trans, int32_t entry) {
    if (entry > 0 || entry < SP_DM_NEG) return false;
    for (int64_t q = 0; q < (int64_t)M * SP_DM_COLS; q++)
        if (emis[q] > SP_DM_EMAX || emis[q] < SP_DM_NEG) return false;
    for (int64_t q = 0; q < (int64_t)M * 7; q++)
        if (trans[q] > 0 || trans[q] < SP_DM_NEG) return false;
    return true;
}

// ---- host drivers: the pieces above, looped row by row, node by node
// codes: the n bases of the interval (0..3 or SP_DM_INVALID); res: room for sp_dm_nres(n, f) residues
static inline void sp_dm_host_translate(const uint8_t *codes, int64_t n, int f, uint8_t *res) {
    const int32_t nr = sp_dm_nres(n, f);
    for (int32_t j = 0; j < nr; j++) {
        unsigned c[3];
        for (int t = 0; t < 3; t++) c[t] = sp_dm_strand(f, codes[sp_dm_pos(n, f, j, t)]);
        res[j] = (uint8_t)sp_dm_codon(c[0], c[1], c[2]);
    }
}
// one frame against one profile; row: 6 (M + 1) words of scratch
static inline sp_dm_hit sp_dm_host_frame(const uint8_t *res, int32_t nres, int M, const int32_t *emis, const int32_t *trans, int32_t entry,
                                         int64_t *row) {
    int64_t *pM = row, *pI = row + (M + 1), *pD = row + 2 * (M + 1), *cM = row + 3 * (M + 1), *cI = row + 4 * (M + 1), *cD = row + 5 * (M + 1);
    for (int q = 0; q < 6 * (M + 1); q++) row[q] = SP_DM_NONE;
    sp_dm_hit best = sp_dm_nohit();
    for (int32_t i = 0; i < nres; i++) {
        const int x = res[i];
        cM[0] = cI[0] = cD[0] = SP_DM_NONE;
        for (int k = 1; k <= M; k++) {
            const int32_t *tp = trans + 7 * (k >= 2 ? k - 2 : 0), *tk = trans + 7 * (k - 1);      // of node k - 1 (unused at k = 1), of node k
            cM[k] = sp_dm_match(pM[k - 1], pI[k - 1], pD[k - 1], tp[SP_DM_MM], tp[SP_DM_IM], tp[SP_DM_DM], entry, (int64_t)i * 2048 + (k - 1),
                                emis[(int64_t)(k - 1) * SP_DM_COLS + x]);
            cI[k] = k <= M - 1 ? sp_dm_insert(pM[k], pI[k], tk[SP_DM_MI], tk[SP_DM_II]) : SP_DM_NONE;
            cD[k] = k >= 2 ? sp_dm_delete(cM[k - 1], cD[k - 1], tp[SP_DM_MD], tp[SP_DM_DD]) : SP_DM_NONE;
            const sp_dm_hit h = sp_dm_hit{cM[k], i, k};
            if (sp_dm_better(h, best)) best = h;
        }
        int64_t *t;
        t = pM, pM = cM, cM = t;
        t = pI, pI = cI, cI = t;
        t = pD, pD = cD, cD = t;
    }
    return best;
}
// the ungapped prefilter of one frame against one profile; row: M + 1 int32 of scratch.  Row i overwrites row i - 1 in
// place, from node M down, so that row[k - 1] still holds S[i-1][k-1] when node k reads it
static inline int32_t sp_dm_host_ssv_frame(const uint8_t *res, int32_t nres, int M, const int32_t *emis, const int32_t *trans, int32_t entry,
                                           int32_t *row) {
    for (int k = 0; k <= M; k++) row[k] = SP_DM_SSV_NONE;
    int32_t best = INT32_MIN;
    for (int32_t i = 0; i < nres; i++) {
        const int x = res[i];
        for (int k = M; k >= 1; k--) {
            const int32_t s = sp_dm_ssv_cell(row[k - 1], k >= 2 ? trans[7 * (k - 2) + SP_DM_MM] : 0, entry, emis[(int64_t)(k - 1) * SP_DM_COLS + x]);
            row[k] = s;
            if (s > best) best = s;
        }
    }
    return best;
}
// one element against one profile: res and row are scratch (n / 3 + 1 bytes, 6 (M + 1) words)
static inline void sp_dm_host_element(const uint8_t *codes, int64_t n, int M, const int32_t *emis, const int32_t *trans, int32_t entry, uint8_t *res,
                                      int64_t *row, int32_t *out) {
    sp_dm_hit frames[6];
    for (int f = 0; f < 6; f++) {
        sp_dm_host_translate(codes, n, f, res);
        frames[f] = sp_dm_host_frame(res, sp_dm_nres(n, f), M, emis, trans, entry, row);
    }
    sp_dm_result(frames, out);
}
