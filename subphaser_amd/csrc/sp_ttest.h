// sp_ttest.h -- the two pieces of the wide k-mer t-test (k7_ttest_wide*, sp_enrich.hip) that must be right to the bit:
// numpy's pairwise float64 sum as a streaming accumulator, and the two-sided Student p-value at large df.
//
// Everything here is plain fp64 arithmetic, __host__ __device__, so that tests/test_ttest_host.py checks it with the
// host compiler against numpy and mpmath.  Build with -ffp-contract=off: a fused multiply-add changes the sums.
//
// (a) np.sum of a contiguous 1-D float64 vector (numpy's pairwise_sum):
//       P(a, n):  n < 8     ((0.0 + a0) + a1) + ...
//                 n <= 128  r[j] = a[j], j = 0..7;  r[j] += a[i + j] for i = 8, 16, ... below n - n % 8;
//                           ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 tail in order
//                 n > 128   h = n / 2 - (n / 2) % 8;  P(a, h) + P(a + h, n - h)
//     and, because the reduction hands its inner loop at most one buffer (np.getbufsize() = 8192 values) at a time,
//       np.sum(a, n) = (((0.0 + P(a, 8192)) + P(a + 8192, 8192)) + ...) + P(rest)          for n > 8192
//     (P alone is np.sum up to 8192 values; beyond, it differs from numpy 2.2 in the last bits for most vectors).
//     Every split point is a multiple of 8, so the stream is a run of aligned blocks of 8 plus one tail of n % 8 values;
//     which blocks open and close a leaf, and how many "pop the left sum, add" merges follow a leaf, depends on n alone.
//     sp_tt_program writes that out once per vector length (one byte per block of 8); the accumulator then takes the
//     blocks in order.  The eight lane sums are only ever indexed by constants (registers on the device); the stack of
//     pending left sums is reached through a caller-supplied accessor, so that a kernel can keep it in LDS laid out
//     [depth][lane] where the (wave-uniform) depth costs nothing.
// (b) sp_tt_pvalue(df, t) = I_x(df / 2, 1 / 2), x = df / (df + t^2): what 2 * stdtr(df, -|t|) is.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_TT_HD __host__ __device__ __forceinline__
#define SP_TT_HDN __host__ __device__
#else
#define SP_TT_HD static inline
#define SP_TT_HDN static
#endif

#define SP_TT_WIDE_MAX 65536   // chromosomes per group: sp_tt_pvalue is inside the tests' tolerance up to df = 2 * 65536 - 2
#define SP_TT_DEPTH 12         // pending left sums: at most 11 for n <= 65536 (sp_tt_program reports the depth it needs)
#define SP_TT_LEAF 128         // numpy's PW_BLOCKSIZE
#define SP_TT_NPBUF 8192       // numpy's default ufunc buffer, in values

// program byte of one block of 8
#define SP_TT_FIRST 1u         // opens a leaf: r[j] = v[j]
#define SP_TT_LAST 2u          // closes a leaf: the eight lane sums are combined
#define SP_TT_FINAL 4u         // ... of the last leaf: the tail and the remaining merges follow (sp_tt_finish)
#define SP_TT_MERGE_SHIFT 3    // merges after a leaf that is not the last

// host: the program of a vector of n values, n / 8 bytes into prog (may be NULL: only the depth is wanted); returns the
// deepest the stack of pending sums gets
static inline int sp_tt_program_rec(int64_t n, int64_t block0, uint8_t *prog, int *sp, int *deepest, int is_last) {
    if (n <= SP_TT_LEAF) {
        const int64_t nb = n / 8;
        if (prog && nb) {
            for (int64_t b = 0; b < nb; b++) prog[block0 + b] = 0;
            prog[block0] |= SP_TT_FIRST;
            prog[block0 + nb - 1] |= SP_TT_LAST | (is_last ? SP_TT_FINAL : 0u);
        }
        if (!is_last) {              // pushed; the last leaf stays in the accumulator
            *sp += 1;
            if (*sp > *deepest) *deepest = *sp;
        }
        return 0;
    }
    int64_t h = n / 2;
    h -= h % 8;
    sp_tt_program_rec(h, block0, prog, sp, deepest, 0);
    sp_tt_program_rec(n - h, block0 + h / 8, prog, sp, deepest, is_last);
    if (!is_last) {                  // left + right, after the right part's last leaf (which is a whole number of blocks)
        if (prog) prog[block0 + n / 8 - 1] += 1u << SP_TT_MERGE_SHIFT;
        *sp -= 1;
    }
    return 0;
}
static inline int sp_tt_program(int64_t n, uint8_t *prog) {
    int sp = 0, deepest = 0;
    for (int64_t at = 0; at < n || at == 0; at += SP_TT_NPBUF) {
        const int64_t len = n - at < SP_TT_NPBUF ? n - at : SP_TT_NPBUF;
        const int is_last = at + len >= n;
        sp_tt_program_rec(len, at / 8, prog, &sp, &deepest, is_last);
        if (at > 0 && !is_last) {    // total + P(piece): the total of the pieces before lies under this piece's sum
            if (prog) prog[(at + len) / 8 - 1] += 1u << SP_TT_MERGE_SHIFT;
            sp -= 1;
        }
    }
    return deepest;
}

struct sp_tt_acc {
    double r[8];     // lane sums of the open leaf
    double res;      // sum of the leaf just closed, then of everything merged into it
    int sp;          // pending left sums
};
SP_TT_HD void sp_tt_begin(sp_tt_acc &a) {
    for (int j = 0; j < 8; j++) a.r[j] = 0.0;
    a.res = 0.0;     // n < 8 has no block: the tail adds onto 0.0 like numpy's short loop
    a.sp = 0;
}
// the next 8 values with their program byte; Stack: double &at(int depth)
template <class Stack>
SP_TT_HD void sp_tt_block(sp_tt_acc &a, const double (&v)[8], unsigned flags, Stack &st) {
    if (flags & SP_TT_FIRST) {
        for (int j = 0; j < 8; j++) a.r[j] = v[j];
    } else {
        for (int j = 0; j < 8; j++) a.r[j] += v[j];
    }
    if (flags & SP_TT_LAST) {
        a.res = ((a.r[0] + a.r[1]) + (a.r[2] + a.r[3])) + ((a.r[4] + a.r[5]) + (a.r[6] + a.r[7]));
        if (!(flags & SP_TT_FINAL)) {
            for (unsigned m = flags >> SP_TT_MERGE_SHIFT; m; m--) a.res = st.at(--a.sp) + a.res;
            st.at(a.sp++) = a.res;
            a.res = 0.0;             // a last piece of fewer than 8 values has no block: its tail starts from 0.0
        }
    }
}
// one of the n % 8 values after the last block
SP_TT_HD void sp_tt_tail(sp_tt_acc &a, double v) { a.res += v; }
template <class Stack>
SP_TT_HD double sp_tt_finish(sp_tt_acc &a, Stack &st) {
    while (a.sp > 0) a.res = st.at(--a.sp) + a.res;
    return a.res;
}

// ---------------------------------------------------------------------------------------------------------------------
// log B(a, 1/2) = lgamma(a) + lgamma(1/2) - lgamma(a + 1/2).  From a = 64 on the two lgamma values (~a log a) would
// leave only their difference's absolute error, ~1e-16 * a log a: the asymptotic series of lgamma(a + 1/2) - lgamma(a)
// = log(a) / 2 - 1 / (8 a) + 1 / (192 a^3) - 1 / (640 a^5) + 17 / (14336 a^7) - ... is exact to fp64 there.
SP_TT_HD double sp_tt_lbeta_half(double a) {
    if (a < 64.0) return lgamma(a) + lgamma(0.5) - lgamma(a + 0.5);
    const double ia = 1.0 / a, ia2 = ia * ia;
    const double d = 0.5 * log(a) - ia * (1.0 / 8.0 - ia2 * (1.0 / 192.0 - ia2 * (1.0 / 640.0 - ia2 * (17.0 / 14336.0))));
    return 0.5723649429247000870717137 /* log(pi) / 2 */ - d;
}
// continued fraction of the incomplete beta (modified Lentz), the iteration of d_betacf in sp_enrich.hip
SP_TT_HDN double sp_tt_betacf(double a, double b, double x) {
    const double tiny = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 500; m++) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 3e-16) break;
    }
    return h;
}
// two-sided p-value of Student's t with df degrees of freedom, t finite.  x^a is taken as exp(-a log1p(t^2 / df)): for
// a in the thousands a * log(x) with x = df / (df + t^2) rounded next to 1 loses as many digits as a has.
SP_TT_HDN double sp_tt_pvalue(double df, double t) {
    const double a = 0.5 * df, b = 0.5, tt = t * t;
    const double x = df / (df + tt), y = tt / (df + tt);
    if (!(x > 0.0)) return 0.0;
    if (!(y > 0.0)) return 1.0;      // t = 0; an x that merely rounds to 1 still has its y (p = 1 - 6e-9 at t = 1e-8)
    const double bt = exp(-a * log1p(tt / df) + 0.5 * log(y) - sp_tt_lbeta_half(a));
    if (x < (a + 1.0) / (a + b + 2.0)) return bt * sp_tt_betacf(a, b, x) / a;
    return 1.0 - bt * sp_tt_betacf(b, a, y) / b;
}
