// sp_ltralign.h -- the arithmetic of the LTR-pair alignment, compiled for the host and for the device.
//
// The reference takes the similarity of an element's two LTRs from whichever detector wrote the record (LTR.py:680-686):
// ltr_finder rounds it to 0.1 %, ltrharvest reports that of its own X-drop extension.  Here every pair is aligned the same
// way, on the resident genome: a GLOBAL, BANDED alignment with linear gap costs, all integers, no traceback -- the column
// counts travel with the score.  tests/ltralign_ref.py is the plain Python twin, written from the definition and
// compared with `==`.
//
//   sequences  a (left LTR, la bases), b (right LTR, lb bases), 1 <= la, lb <= SP_LA_MAXLEN; a base is a code 0..3 or
//              SP_LA_INVALID (whatever the genome's validity mask marks: N, IUPAC, ...)
//   band       cells (i, j), 0 <= i <= la, 0 <= j <= lb, whose diagonal d = j - i lies in [dlo, dhi]:
//              dlo = min(0, lb - la) - w, dhi = max(0, lb - la) + w, w >= 0 -- both corners are inside for every w.
//              Its width dhi - dlo + 1 = |lb - la| + 2 w + 1 is at most SP_LA_MAXBAND, or the pair is not aligned.
//   column     both bases valid and equal +2 (match), valid and different -2 (mismatch), one invalid 0 (skip), a gap on
//              either side -3 (gap): ltrharvest's default scores
//   cell       the best of its diagonal, up (consumes a[i - 1]) and left (consumes b[j - 1]) predecessors plus its own
//              column; equal scores go to the diagonal, then up, then left.  A predecessor outside the band or the
//              matrix is the sentinel SP_LA_NEG: it cannot win (every cell but the origin has a predecessor inside, whose
//              score is above -3 * 2 * SP_LA_MAXLEN) and cannot overflow (it is never stored, so nothing accumulates on it).
//   edge       set once the chosen path stands on diagonal dlo or dhi while w > 0: the result may be band-limited
//   result     the cell (la, lb)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SP_LA_HD __host__ __device__
#else
#define SP_LA_HD
#endif

#define SP_LA_MAXLEN 8192              // the reference's detectors allow LTRs of up to 7000 (LTR.py:39-41)
// diagonals of a band.  A workgroup is one wave and owns one pair: 2 * SP_LA_MAXLEN bytes of bases + 12 bytes per
// diagonal = 28 KiB of the CU's 160 KiB -- five workgroups per CU.  At -ltr_band 64 it admits LTRs that differ by 895 bases.
#define SP_LA_MAXBAND 1024
#define SP_LA_INVALID 4
#define SP_LA_NEG (-(1 << 30))

#define SP_LA_MATCH 2
#define SP_LA_MISMATCH (-2)
#define SP_LA_GAP (-3)

#define SP_LA_F_EDGE 1                 // flag bits of the result
#define SP_LA_F_BAND 2                 // band wider than SP_LA_MAXBAND: not aligned, counts zero
#define SP_LA_F_LEN 4                  // an LTR longer than SP_LA_MAXLEN: not aligned, counts zero

// A cell: the score, and the four column counts and the edge bit in one word -- 15 bits each (a path has at most
// 2 * SP_LA_MAXLEN = 2^14 columns), the edge at bit 60 -- so that a column is one addition.
#define SP_LA_C_MATCH (1ULL << 0)
#define SP_LA_C_MISMATCH (1ULL << 15)
#define SP_LA_C_GAP (1ULL << 30)
#define SP_LA_C_SKIP (1ULL << 45)
#define SP_LA_C_EDGE (1ULL << 60)
struct sp_la_cell {
    int32_t score;
    uint64_t cnt;
};

SP_LA_HD inline int64_t sp_la_dlo(int64_t la, int64_t lb, int64_t w) { return (lb < la ? lb - la : 0) - w; }
SP_LA_HD inline int64_t sp_la_dhi(int64_t la, int64_t lb, int64_t w) { return (lb > la ? lb - la : 0) + w; }

// 0 when the pair is aligned, else the flag it gets (the length goes first).  la, lb >= 1 and w >= 0 are the caller's.
SP_LA_HD inline int sp_la_check(int64_t la, int64_t lb, int64_t w) {
    if (la > SP_LA_MAXLEN || lb > SP_LA_MAXLEN) return SP_LA_F_LEN;
    if (sp_la_dhi(la, lb, w) - sp_la_dlo(la, lb, w) + 1 > SP_LA_MAXBAND) return SP_LA_F_BAND;
    return 0;
}

// the diagonal column of bases x, y: its score, and its count word through *cnt
SP_LA_HD inline int sp_la_column(unsigned x, unsigned y, uint64_t *cnt) {
    if (x >= SP_LA_INVALID || y >= SP_LA_INVALID) {
        *cnt = SP_LA_C_SKIP;
        return 0;
    }
    *cnt = x == y ? SP_LA_C_MATCH : SP_LA_C_MISMATCH;
    return x == y ? SP_LA_MATCH : SP_LA_MISMATCH;
}

SP_LA_HD inline sp_la_cell sp_la_none() { return sp_la_cell{SP_LA_NEG, 0}; }

// The cell on diagonal d from its three predecessors (sp_la_none() for one outside the band or the matrix) and the bases
// x = a[i - 1], y = b[j - 1] of its diagonal column (anything when there is no diagonal predecessor).
SP_LA_HD inline sp_la_cell sp_la_update(sp_la_cell diag, sp_la_cell up, sp_la_cell left, unsigned x, unsigned y, int64_t d,
                                        int64_t dlo, int64_t dhi, int64_t w) {
    uint64_t col;
    const int sub = sp_la_column(x, y, &col);
    const int32_t sd = diag.score == SP_LA_NEG ? SP_LA_NEG : diag.score + sub;
    const int32_t su = up.score == SP_LA_NEG ? SP_LA_NEG : up.score + SP_LA_GAP;
    const int32_t sl = left.score == SP_LA_NEG ? SP_LA_NEG : left.score + SP_LA_GAP;
    sp_la_cell r;
    if (sd >= su && sd >= sl) {
        r.score = sd;
        r.cnt = diag.cnt + col;
    } else if (su >= sl) {
        r.score = su;
        r.cnt = up.cnt + SP_LA_C_GAP;
    } else {
        r.score = sl;
        r.cnt = left.cnt + SP_LA_C_GAP;
    }
    if (w > 0 && (d == dlo || d == dhi)) r.cnt |= SP_LA_C_EDGE;
    return r;
}

// the six outputs of a pair from its last cell
SP_LA_HD inline void sp_la_result(sp_la_cell c, int32_t out[6]) {
    out[0] = c.score;
    out[1] = (int32_t)(c.cnt & 0x7fff);
    out[2] = (int32_t)((c.cnt >> 15) & 0x7fff);
    out[3] = (int32_t)((c.cnt >> 30) & 0x7fff);
    out[4] = (int32_t)((c.cnt >> 45) & 0x7fff);
    out[5] = (c.cnt & SP_LA_C_EDGE) ? SP_LA_F_EDGE : 0;
}
