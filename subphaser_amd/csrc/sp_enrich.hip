// sp_enrich.hip -- K6: per-window Fisher right tail + enrichment decision.
//
// Replaces Stats.fisher_test / enrich / _enrich / Pvalues.get_enriched
// (reference: subphaser/Stats.py:14-31, 140-192).  One thread per window.
//
// The hypergeometric point mass is evaluated with Loader's saddle-point
// formulation (stirlerr / bd0), which stays accurate to ~1e-14 relative for
// margins of 2e8 where a difference of lgamma() values loses 6-7 digits; the
// tail is then summed by the exact term recurrence.  All arithmetic is fp64.
#include "sp_device.h"
#include "sp_internal.h"
#include "sp_kmertest.h"
#include "sp_ttest.h"

#define SP_MAX_INT_CLAMP (2147483647LL / 10)  // Stats.py:9
#define SP_ENRICH_MAXS 32

__device__ static const double c_sfe[16] = {
    0.0,                           /* 0: unused */
    0.08106146679532726,           /* 1 */
    0.04134069595540929,           /* 2 */
    0.02767792568499834,           /* 3 */
    0.02079067210376509,           /* 4 */
    0.01664469118982119,           /* 5 */
    0.01387612882307075,           /* 6 */
    0.01189670994589177,           /* 7 */
    0.010411265261972096,          /* 8 */
    0.009255462182712733,          /* 9 */
    0.008330563433362871,          /* 10 */
    0.007573675487951841,          /* 11 */
    0.006942840107209530,          /* 12 */
    0.006408994188004207,          /* 13 */
    0.005951370112758848,          /* 14 */
    0.005554733551962801           /* 15 */
};

__device__ __forceinline__ double d_stirlerr(double n) {
    const double S0 = 0.083333333333333333333, S1 = 0.00277777777777777777778,
                 S2 = 0.00079365079365079365079365, S3 = 0.000595238095238095238095238,
                 S4 = 0.0008417508417508417508417508;
    if (n <= 15.0) return c_sfe[(int)n];
    double nn = n * n;
    if (n > 500) return (S0 - S1 / nn) / n;
    if (n > 80) return (S0 - (S1 - S2 / nn) / nn) / n;
    if (n > 35) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
    return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

__device__ __forceinline__ double d_bd0(double x, double np) {
    if (fabs(x - np) < 0.1 * (x + np)) {
        double v = (x - np) / (x + np);
        double s = (x - np) * v;
        if (fabs(s) < 2.2250738585072014e-308) return s;
        double ej = 2 * x * v;
        v = v * v;
        for (int j = 1; j < 1000; j++) {
            ej *= v;
            double s1 = s + ej / ((j << 1) + 1);
            if (s1 == s) return s1;
            s = s1;
        }
    }
    return x * log(x / np) + np - x;
}

// log of the binomial point mass, Loader's dbinom_raw
__device__ __forceinline__ double d_ldbinom(double x, double n, double p, double q) {
    const double NEG_INF = -INFINITY;
    if (p == 0) return x == 0 ? 0.0 : NEG_INF;
    if (q == 0) return x == n ? 0.0 : NEG_INF;
    if (x == 0) {
        if (n == 0) return 0.0;
        return (p < 0.1) ? -d_bd0(n, n * q) - n * p : n * log(q);
    }
    if (x == n) return (q < 0.1) ? -d_bd0(n, n * p) - n * q : n * log(p);
    if (x < 0 || x > n) return NEG_INF;
    double lc = d_stirlerr(n) - d_stirlerr(x) - d_stirlerr(n - x) - d_bd0(x, n * p) - d_bd0(n - x, n * q);
    double lf = 1.837877066409345483560659472811 + log(x) + log1p(-x / n);
    return lc - 0.5 * lf;
}

// P[X = x], x white drawn when n are drawn from r white + b black
__device__ __forceinline__ double d_dhyper(double x, double r, double b, double n) {
    if (n < x || r < x || n - x > b) return 0.0;
    if (n == 0) return x == 0 ? 1.0 : 0.0;
    double p = n / (r + b), q = (r + b - n) / (r + b);
    double l = d_ldbinom(x, r, p, q) + d_ldbinom(n - x, b, p, q) - d_ldbinom(n, r + b, p, q);
    return exp(l);
}

// P[X >= a], X ~ Hypergeom(N = a+b+c+d, K = a+b, n = a+c): what
// fisher.pvalue(a,b,c,d).right_tail returns (Stats.py:26)
__device__ double d_right_tail(long long a, long long b, long long c, long long d) {
    const double K = (double)(a + b), NK = (double)(c + d), n = (double)(a + c);
    const double N = K + NK;
    long long lo = (a + c) - (c + d);
    if (lo < 0) lo = 0;
    const long long hi = (a + b) < (a + c) ? (a + b) : (a + c);
    if (a <= lo) return 1.0;
    if (a > hi) return 0.0;
    const double mode = floor((n + 1.0) * (K + 1.0) / (N + 2.0));
    if ((double)a > mode) {
        double x = (double)a;
        double term = d_dhyper(x, K, NK, n);
        double s = term;
        while (x < (double)hi && term > 0.0) {
            term *= (K - x) * (n - x) / ((x + 1.0) * (NK - n + x + 1.0));
            x += 1.0;
            s += term;
            if (term < s * 1e-18) break;
        }
        return s;
    }
    double x = (double)a - 1.0;
    double term = d_dhyper(x, K, NK, n);
    double s = term;
    while (x > (double)lo && term > 0.0) {
        term *= x * (NK - n + x) / ((K - x + 1.0) * (n - x + 1.0));
        x -= 1.0;
        s += term;
        if (term < s * 1e-18) break;
    }
    return 1.0 - s;
}

// numpy's float64 add.reduce order for a short contiguous vector
__device__ __forceinline__ double d_np_sum(const double *a, int n) {
    if (n < 8) {
        double r = 0.;
        for (int i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}

__global__ void __launch_bounds__(64)
k6_enrich(const long long *__restrict__ counts, const long long *__restrict__ total /* S column sums, then their sum */,
          long long W, int S, double max_pval, double min_ratio, double *__restrict__ pvals,
          int *__restrict__ argmin, unsigned char *__restrict__ sig, double *__restrict__ ratios) {
    long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    const long long sum_total = total[S];
    const long long *row = counts + w * S;
    double *p = pvals + w * S;
    double *q = ratios + w * S;
    long long sum_each = 0;
    for (int j = 0; j < S; j++) sum_each += row[j];
    for (int j = 0; j < S; j++) {
        // fisher_test margins incl. the x22 quirk and clamps (Stats.py:20-25)
        long long x11 = row[j];
        long long x12 = sum_each - x11;
        long long x21 = total[j] - x11;
        long long x22 = sum_total - x21 - x12;
        if (x21 > SP_MAX_INT_CLAMP) x21 = SP_MAX_INT_CLAMP;
        if (x22 > SP_MAX_INT_CLAMP) x22 = SP_MAX_INT_CLAMP;
        p[j] = d_right_tail(x11, x12, x21, x22);
    }
    // Pvalues.get_enriched (Stats.py:181-192): stable sort by p, first two
    int m = 0;
    for (int j = 1; j < S; j++)
        if (p[j] < p[m]) m = j;
    int s2 = -1;
    for (int j = 0; j < S; j++) {
        if (j == m) continue;
        if (s2 < 0 || p[j] < p[s2]) s2 = j;
    }
    bool sg = true;
    if (p[m] > max_pval) sg = false;
    if (p[m] == 0) {
    } else if (p[s2] / p[m] < max_pval / p[s2] * 1.0)
        sg = false;
    // _enrich (Stats.py:157-162)
    for (int j = 0; j < S; j++) q[j] = (double)row[j] / (double)total[j];
    double qs = d_np_sum(q, S);
    for (int j = 0; j < S; j++) q[j] = q[j] / qs;
    if (q[m] < min_ratio) sg = false;
    argmin[w] = m;
    sig[w] = sg ? 1 : 0;
}

// ----------------------------------------------------------------- f-1: subgenome-specific k-mer test
// Cluster.output_kmers / _output_kmers (Cluster.py:151-194) for test_method = ttest_ind: per differential
// k-mer, the chromosome frequencies count/length are grouped by subgenome, the groups are ordered by mean
// (descending, ties in subgenome order) and scipy.stats.ttest_ind(top, second) -- pooled variance, two-sided --
// gives the p-value: 2 * stdtr(df, -|t|) = I_x(df/2, 1/2) with x = df / (df + t^2) (regularised incomplete beta,
// continued fraction in fp64).  One thread per k-mer.  Validation, staging, the workspace, the copies back and the
// top / second update are the shared ones of sp_kmertest.h.
#define SP_TT_MAXG 64
__device__ double d_betacf(double a, double b, double x) {
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
        // a few eps: 1e-16 lies below the spacing of doubles around 1 (1.1e-16 / 2.2e-16) and only ever fired on
        // del == 1.0 exactly -- otherwise every thread ran all 500 iterations.  p-values agree with scipy's
        // stdtr to a relative 1e-9 (tests/test_gpu_parity.py::test_kmer_ttest_device_vs_scipy), not bit for bit.
        if (fabs(del - 1.0) < 3e-16) break;
    }
    return h;
}
// I_x(a, b) with y = 1 - x formed by the caller without cancellation: for a small t, x = df / (df + t^2) rounds
// next to 1 and 1 - x would keep only a few digits of t^2 / (df + t^2) (p near 1 was 5e-12 off at df = 126)
__device__ double d_betainc(double a, double b, double x, double y) {
    if (!(x > 0.0)) return 0.0;
    if (!(x < 1.0)) return 1.0;
    const double bt = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(y));
    if (x < (a + 1.0) / (a + b + 2.0)) return bt * d_betacf(a, b, x) / a;
    return 1.0 - bt * d_betacf(b, a, y) / b;
}

__global__ void __launch_bounds__(128)
k7_ttest(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G,
         const int *__restrict__ goff, const int *__restrict__ gchrom, int *__restrict__ top, int *__restrict__ second,
         double *__restrict__ pvals, double *__restrict__ means) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const uint32_t *row = counts + r * C;
    sp_kt_best best;
    for (int g = 0; g < G; g++) {            // means in numpy's summation order; descending, ties in group order
        double v[SP_TT_MAXG];
        const int n = goff[g + 1] - goff[g];
        for (int i = 0; i < n; i++) v[i] = (double)row[gchrom[goff[g] + i]] / chrom_len[gchrom[goff[g] + i]];
        const double mean = d_np_sum(v, n) / (double)n;
        means[r * G + g] = mean;
        best = sp_kt_top2(g, mean, best);
    }
    const int t1 = best.t1, t2 = best.t2 < 0 ? best.t1 : best.t2;
    top[r] = t1;
    second[r] = t2;
    double var[2], mu[2];
    int nn[2];
    for (int s = 0; s < 2; s++) {
        const int g = s ? t2 : t1;
        double v[SP_TT_MAXG];
        const int n = goff[g + 1] - goff[g];
        for (int i = 0; i < n; i++) v[i] = (double)row[gchrom[goff[g] + i]] / chrom_len[gchrom[goff[g] + i]];
        const double mean = d_np_sum(v, n) / (double)n;
        for (int i = 0; i < n; i++) { const double d = v[i] - mean; v[i] = d * d; }
        var[s] = n > 1 ? d_np_sum(v, n) / (double)(n - 1) : 0.0;
        mu[s] = mean;
        nn[s] = n;
    }
    const double df = (double)(nn[0] + nn[1]) - 2.0;
    double p;
    if (!(df > 0.0)) {
        p = sp_kt_nan();
    } else {
        const double svar = ((nn[0] - 1) * var[0] + (nn[1] - 1) * var[1]) / df;
        const double denom = sqrt(svar * (1.0 / nn[0] + 1.0 / nn[1]));
        const double t = (mu[0] - mu[1]) / denom;
        if (t != t) p = t;                               // 0 / 0: NaN, kept by the caller like the reference does
        else if (isinf(t)) p = 0.0;
        else p = d_betainc(0.5 * df, 0.5, df / (df + t * t), t * t / (df + t * t));
    }
    pvals[r] = p;
}

extern "C" int sp_kmer_ttest(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                             const int32_t *group_off, const int32_t *group_chrom, int32_t *top, int32_t *second,
                             double *pvals, double *means) {
    sp_kt_call k{ctx, "sp_kmer_ttest", counts, M, C, lengths, n_groups, group_off, group_chrom, top, second, pvals, means, nullptr};
    int rc = sp_kt_check_groups(k, SP_TT_MAXG, SP_EUNSUP);
    if (rc || M == 0) return rc;
    rc = sp_kt_begin(k, false, [](sp_carve &) {});
    if (rc) return rc;
    SP_LAUNCH(ctx, "k7_ttest", k7_ttest, dim3((unsigned)((M + 127) / 128)), dim3(128), 0, k.rows, (long long)M, C,
              (const double *)k.d.len, n_groups, (const int *)k.d.goff, (const int *)k.d.gch, k.d.top, k.d.sec, k.d.p, k.d.means);
    return sp_kt_finish(k);
}

// ----------------------------------------------------------------- f-1, subgenomes of more than SP_TT_MAXG chromosomes
// The same test for groups of up to SP_TT_WIDE_MAX chromosomes (scaffold-level assemblies: every scaffold is assigned to
// a subgenome).  No array sized by the group: a thread still owns a row and adds its values in list order, but the
// values stream through the accumulator of sp_ttest.h (numpy's pairwise sum, bit for bit, from a per-group program
// built on the host) and the counts reach the thread through an LDS transpose, so that global reads run along the rows:
//   a workgroup = one wave = SP_TW_ROWS rows; per chunk of SP_TW_COLS entries of a group's column list, lane l loads
//   column entry l of every row (one row segment per load instruction), stores it at [row][l] with an odd pitch, and
//   after the barrier reads [its row][0 .. SP_TW_COLS) -- conflict-free both ways.  The column lengths of the chunk sit
//   beside the tile and are read as broadcasts.  Control flow depends on the group sizes only: uniform across lanes.
// k7_ttest_wide_means (pass 1): means[r][g] = np.mean of the list (pairwise); top / second by the reference's own order
//   key -sum(x) / len(x), the Python sum added strictly left to right (Cluster.py:183) -- the two differ in the last bits.
// k7_ttest_wide_test (pass 2): sweeps every group again with (v - mean)^2 and keeps the variances of top and second (G is
//   2..8 in practice and every column belongs to one group: one more read of the matrix, no divergence), then t and p as
//   k7_ttest forms them, the p-value from sp_tt_pvalue (accurate at df in the thousands, where d_betainc is not).
#define SP_TW_ROWS 64
#define SP_TW_COLS 64
#define SP_TW_PITCH (SP_TW_COLS + 1)
struct sp_tw_lds {
    uint32_t tile[SP_TW_ROWS * SP_TW_PITCH];
    double len[SP_TW_COLS];
    uint32_t prog[SP_TW_COLS / 8];              // the chunk's program bytes
    double stack[SP_TT_DEPTH * SP_TW_ROWS];     // [depth][lane]
};
struct sp_tw_stack {
    double *base;                               // &stack[lane]
    __device__ __forceinline__ double &at(int d) { return base[d * SP_TW_ROWS]; }
};
// one group of one row tile: returns P(f(v)) over the group's list, f(v) = v (SQ = false; *key gets the left-to-right sum)
// or (v - mean)^2 (SQ = true)
template <bool SQ>
__device__ __forceinline__ double
tw_group(sp_tw_lds &L, const uint32_t *__restrict__ counts, long long r0, long long M, int C, const double *__restrict__ chrom_len,
         const int *__restrict__ gch /* the group's list */, int n, const uint8_t *__restrict__ prog /* the group's program */,
         double mean, double *key) {
    const int lane = threadIdx.x;
    sp_tt_acc acc;
    sp_tw_stack st{L.stack + lane};
    sp_tt_begin(acc);
    double seq = 0.0;
    const int nfull = n - n % 8;
    for (int c0 = 0; c0 < n; c0 += SP_TW_COLS) {
        const int valid = n - c0 < SP_TW_COLS ? n - c0 : SP_TW_COLS;
        __syncthreads();                        // the chunk before has been consumed
        int col = 0;
        if (lane < valid) {
            col = gch[c0 + lane];
            L.len[lane] = chrom_len[col];
        }
        if (lane < SP_TW_COLS / 8 && c0 + lane * 8 + 8 <= nfull) L.prog[lane] = prog[(c0 >> 3) + lane];
        // every address is in bounds whatever the lane: rows past the last repeat it, lanes past the chunk read column
        // 0 (nobody consumes either), so the loads carry no branch and sixteen of them are in flight per lane
        const uint32_t *src = counts + col;
#pragma unroll 1
        for (int rb = 0; rb < SP_TW_ROWS; rb += 16) {
            uint32_t c[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const long long row = r0 + rb + j < M ? r0 + rb + j : M - 1;
                c[j] = src[row * C];
            }
#pragma unroll
            for (int j = 0; j < 16; j++) L.tile[(rb + j) * SP_TW_PITCH + lane] = c[j];
        }
        __syncthreads();
        const uint32_t *mine = L.tile + lane * SP_TW_PITCH;
        const int full_here = (nfull - c0 < valid ? nfull - c0 : valid);      // values of this chunk that lie in whole blocks
        for (int i = 0; i < full_here; i += 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                v[j] = (double)mine[i + j] / L.len[i + j];
                if (SQ) { const double d = v[j] - mean; v[j] = d * d; }
                else seq += v[j];
            }
            sp_tt_block(acc, v, (unsigned)__builtin_amdgcn_readfirstlane((int)L.prog[i >> 3]), st);
        }
        for (int i = full_here > 0 ? full_here : 0; i < valid; i++) {        // the n % 8 tail, in the last chunk only
            double v = (double)mine[i] / L.len[i];
            if (SQ) { const double d = v - mean; v = d * d; }
            else seq += v;
            sp_tt_tail(acc, v);
        }
    }
    if (!SQ) *key = seq;
    return sp_tt_finish(acc, st);
}

__global__ void __launch_bounds__(SP_TW_ROWS)
k7_ttest_wide_means(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G,
                    const int *__restrict__ goff, const int *__restrict__ gchrom, const int *__restrict__ poff,
                    const uint8_t *__restrict__ prog, int *__restrict__ top, int *__restrict__ second,
                    double *__restrict__ means) {
    __shared__ sp_tw_lds L;
    const long long r0 = (long long)blockIdx.x * SP_TW_ROWS, r = r0 + threadIdx.x;
    sp_kt_best best;
    for (int g = 0; g < G; g++) {
        const int n = goff[g + 1] - goff[g];
        double seq;
        const double mean = tw_group<false>(L, counts, r0, M, C, chrom_len, gchrom + goff[g], n, prog + poff[g], 0.0, &seq) / (double)n;
        const double key = seq / (double)n;
        if (r < M) means[r * G + g] = mean;
        best = sp_kt_top2(g, key, best);
    }
    if (r < M) {
        top[r] = best.t1;
        second[r] = best.t2 < 0 ? best.t1 : best.t2;
    }
}

__global__ void __launch_bounds__(SP_TW_ROWS)
k7_ttest_wide_test(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G,
                   const int *__restrict__ goff, const int *__restrict__ gchrom, const int *__restrict__ poff,
                   const uint8_t *__restrict__ prog, const int *__restrict__ top, const int *__restrict__ second,
                   const double *__restrict__ means, double *__restrict__ pvals) {
    __shared__ sp_tw_lds L;
    const long long r0 = (long long)blockIdx.x * SP_TW_ROWS, r = r0 + threadIdx.x;
    const long long rc = r < M ? r : M - 1;     // lanes past the last row go through the motions on it and store nothing
    const int t1 = top[rc], t2 = second[rc];
    double var1 = 0, var2 = 0, mu1 = 0, mu2 = 0;
    int n1 = 1, n2 = 1;
    for (int g = 0; g < G; g++) {
        const int n = goff[g + 1] - goff[g];
        const double mean = means[rc * G + g];
        const double ss = tw_group<true>(L, counts, r0, M, C, chrom_len, gchrom + goff[g], n, prog + poff[g], mean, nullptr);
        const double var = n > 1 ? ss / (double)(n - 1) : 0.0;
        if (g == t1) { var1 = var; mu1 = mean; n1 = n; }
        if (g == t2) { var2 = var; mu2 = mean; n2 = n; }
    }
    const double df = (double)(n1 + n2) - 2.0;
    double p;
    if (!(df > 0.0)) {
        p = sp_kt_nan();
    } else {
        const double svar = ((n1 - 1) * var1 + (n2 - 1) * var2) / df;
        const double denom = sqrt(svar * (1.0 / n1 + 1.0 / n2));
        const double t = (mu1 - mu2) / denom;
        if (t != t) p = t;
        else if (isinf(t)) p = 0.0;
        else p = sp_tt_pvalue(df, t);
    }
    if (r < M) pvals[r] = p;
}

// pass 1 for the other units (sp_internal.h): the summation program of every group, one byte per block of 8 values
// (sp_ttest.h), and the launch of k7_ttest_wide_means on it
int sp_tw_means_plan(sp_ctx *ctx, const char *who, int n_groups, const int32_t *group_off, sp_tw_plan &plan) {
    plan.poff.assign((size_t)n_groups + 1, 0);
    for (int g = 0; g < n_groups; g++) plan.poff[(size_t)g + 1] = plan.poff[(size_t)g] + (group_off[g + 1] - group_off[g]) / 8;
    plan.prog.assign((size_t)plan.poff[(size_t)n_groups] + 1, 0);
    for (int g = 0; g < n_groups; g++) {
        const int depth = sp_tt_program(group_off[g + 1] - group_off[g], plan.prog.data() + plan.poff[(size_t)g]);
        if (depth > SP_TT_DEPTH) return sp_fail(ctx, SP_EUNSUP, "%s: summation stack of %d (%d supported)", who, depth, SP_TT_DEPTH);
    }
    return SP_OK;
}
int sp_tw_means_launch(sp_ctx *ctx, const sp_tw_plan &plan, int *d_poff, uint8_t *d_prog, const uint32_t *rows, int64_t M, int C,
                       const double *d_len, int n_groups, const int *d_goff, const int *d_gch, int *d_top, int *d_sec,
                       double *d_means) {
    SP_HIP(ctx, hipMemcpyAsync(d_poff, plan.poff.data(), plan.poff.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_prog, plan.prog.data(), plan.prog.size(), hipMemcpyHostToDevice, ctx->stream));
    SP_LAUNCH(ctx, "k7_ttest_wide_means", k7_ttest_wide_means, dim3((unsigned)((M + SP_TW_ROWS - 1) / SP_TW_ROWS)), dim3(SP_TW_ROWS),
              0, rows, (long long)M, C, d_len, n_groups, d_goff, d_gch, (const int *)d_poff, (const uint8_t *)d_prog, d_top,
              d_sec, d_means);
    return SP_OK;
}

extern "C" int sp_kmer_ttest_wide(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                                  const int32_t *group_off, const int32_t *group_chrom, int32_t *top, int32_t *second,
                                  double *pvals, double *means) {
    sp_kt_call k{ctx, "sp_kmer_ttest_wide", counts, M, C, lengths, n_groups, group_off, group_chrom, top, second, pvals, means, nullptr};
    int rc = sp_kt_check_groups(k, SP_TT_WIDE_MAX, SP_EUNSUP);
    if (rc || M == 0) return rc;
    sp_tw_plan plan;
    rc = sp_tw_means_plan(ctx, k.who, n_groups, group_off, plan);
    if (rc) return rc;
    int *d_poff;
    uint8_t *d_prog;
    rc = sp_kt_begin(k, false, [&](sp_carve &cv) {
        d_poff = cv.take<int>(plan.poff.size());
        d_prog = cv.take<uint8_t>(plan.prog.size());
    });
    if (rc) return rc;
    rc = sp_tw_means_launch(ctx, plan, d_poff, d_prog, k.rows, M, C, k.d.len, n_groups, k.d.goff, k.d.gch, k.d.top, k.d.sec, k.d.means);
    if (rc) return rc;
    SP_LAUNCH(ctx, "k7_ttest_wide_test", k7_ttest_wide_test, dim3((unsigned)((M + SP_TW_ROWS - 1) / SP_TW_ROWS)), dim3(SP_TW_ROWS), 0,
              k.rows, (long long)M, C, (const double *)k.d.len, n_groups, (const int *)k.d.goff, (const int *)k.d.gch,
              (const int *)d_poff, (const uint8_t *)d_prog, (const int *)k.d.top, (const int *)k.d.sec, (const double *)k.d.means, k.d.p);
    return sp_kt_finish(k);
}

// column sums of the window table (Stats.py:142) + their sum, on the device
__global__ void __launch_bounds__(256)
k6_totals(const long long *__restrict__ counts, long long W, int S, long long *__restrict__ total /* S + 1 */) {
    __shared__ unsigned long long acc[SP_ENRICH_MAXS + 1];
    if (threadIdx.x <= S) acc[threadIdx.x] = 0;
    __syncthreads();
    for (int j = 0; j < S; j++) {
        unsigned long long s = 0;
        for (long long w = threadIdx.x; w < W; w += blockDim.x) s += (unsigned long long)counts[w * S + j];
        if (s) atomicAdd(&acc[j], s);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int j = 0; j < S; j++) {
            total[j] = (long long)acc[j];
            t += acc[j];
        }
        total[S] = (long long)t;
    }
}

extern "C" int sp_enrich_dev(sp_ctx *ctx, const void *d_counts, int64_t W, int S, double max_pval, double min_ratio,
                             double *pvals, int32_t *argmin, uint8_t *sig, double *ratios) {
    if (!ctx || W < 0 || (W > 0 && (!d_counts || !pvals || !argmin || !sig || !ratios)))
        return sp_fail(ctx, SP_EINVAL, "sp_enrich: bad arguments");
    if (S < 2) return sp_fail(ctx, SP_ESTATE, "sp_enrich: at least 2 subgenome columns required (Stats.py:172)");
    if (S > SP_ENRICH_MAXS) return sp_fail(ctx, SP_EUNSUP, "sp_enrich: S=%d > %d", S, SP_ENRICH_MAXS);
    if (W == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nWS = (size_t)W * S;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // one growth-only buffer: totals | p | ratios | argmin | sig   (no per-call hipMalloc)
    int rc = sp_buf_ensure(ctx, ctx->b_enr, (int64_t)(al((size_t)(S + 1) * 8) + 2 * al(nWS * 8) + al((size_t)W * 4) + al((size_t)W)));
    if (rc) return rc;
    char *q = (char *)ctx->b_enr.p;
    long long *d_total = (long long *)q; q += al((size_t)(S + 1) * 8);
    double *d_p = (double *)q; q += al(nWS * 8);
    double *d_q = (double *)q; q += al(nWS * 8);
    int *d_arg = (int *)q; q += al((size_t)W * 4);
    unsigned char *d_sig = (unsigned char *)q;
    SP_LAUNCH(ctx, "k6_totals", k6_totals, dim3(1), dim3(256), 0, (const long long *)d_counts, (long long)W, S, d_total);
    SP_LAUNCH(ctx, "k6_enrich", k6_enrich, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, (const long long *)d_counts,
              (const long long *)d_total, (long long)W, S, max_pval, min_ratio, d_p, d_arg, d_sig, d_q);
    SP_HIP(ctx, hipMemcpyAsync(pvals, d_p, nWS * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(ratios, d_q, nWS * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(argmin, d_arg, (size_t)W * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(sig, d_sig, (size_t)W, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

extern "C" int sp_enrich(sp_ctx *ctx, const int64_t *counts, int64_t W, int S, double max_pval,
                         double min_ratio, double *pvals, int32_t *argmin, uint8_t *sig, double *ratios) {
    if (!ctx || W < 0 || (W > 0 && (!counts || !pvals || !argmin || !sig || !ratios)))
        return sp_fail(ctx, SP_EINVAL, "sp_enrich: bad arguments");
    if (W == 0 || S < 2 || S > SP_ENRICH_MAXS) return sp_enrich_dev(ctx, counts, W, S, max_pval, min_ratio, pvals, argmin, sig, ratios);
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nWS = (size_t)W * S;
    int rc = sp_buf_ensure(ctx, ctx->b_wtab, (int64_t)nWS * 8 + 64);
    if (rc) return rc;
    SP_HIP(ctx, hipMemcpyAsync(ctx->b_wtab.p, counts, nWS * 8, hipMemcpyHostToDevice, ctx->stream));
    return sp_enrich_dev(ctx, ctx->b_wtab.p, W, S, max_pval, min_ratio, pvals, argmin, sig, ratios);
}
