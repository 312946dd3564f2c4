// sp_kpca.h -- the arithmetic of the k-mer PCA (Cluster.pca, the reference's Cluster.py:48-75) that runs over the M
// differential k-mers: row statistics, the C x C Gram matrix of the Z-scores and the projections that decide the
// component signs.  Everything after that is C x C work on the host (subphaser_amd/cluster.py).
//
// __host__ __device__ and free of runtime calls, so that tests/test_kpca_host.py builds it with the host compiler and
// checks it against the numpy twin (tests/kpca_ref.py).  Build with -ffp-contract=off: the orders below are the
// definition, and a fused multiply-add changes the sums.  Division and square root are the correctly rounded ones.
//
// Input: counts, M x C uint32 (row = k-mer, column = chromosome), and the C chromosome lengths, converted to double once.
// Row statistics of one k-mer
//   x_c  = (double)count_c / (double)lengths_c
//   mean = (x_0 + x_1 + ... + x_{C-1}) / C            the sum strictly left to right
//   var  = ((x_0 - mean)^2 + ... ) / C                left to right; the population variance, as np.std
//   sd   = sqrt(var)
//   bad  = sd == 0, or mean or sd not finite          (a k-mer with the same frequency everywhere: 0 / 0 in the Z-score)
//   z_c  = (x_c - mean) / sd                          a division, not a multiplication by a reciprocal
// Gram matrix.  The rows are cut into chunks of SP_KP_ROWS consecutive rows.  For b <= a
//   G[a][b] = sum over chunks, left to right, of (sum over the chunk's good rows, left to right, of z_a * z_b)
// every sum started at +0, the product rounded, then added; G[b][a] = G[a][b].  Bad rows contribute nothing.
// Projection on component j of U (C x n_comp, row-major): v_j(row) = U[0][j] z_0 + U[1][j] z_1 + ..., left to right.
// Sign row of component j: the good row with the largest |v_j|, the lowest row index on ties (a maximum with that tie
// rule does not depend on the order of the comparisons); row -1, value 0 when no row is good.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_KP_HD __host__ __device__ __forceinline__
#else
#define SP_KP_HD static inline
#endif

#define SP_KP_ROWS 1024      // rows per chunk of the Gram sum: part of the bit definition, not a tuning knob
#define SP_KP_MAXC 1024      // chromosomes: the limit of filter views and bound tables
#define SP_KP_MAXCOMP 32     // components per sign call

SP_KP_HD double sp_kp_x(uint32_t count, double len) { return (double)count / len; }
SP_KP_HD double sp_kp_mean(double sum, int C) { return sum / (double)C; }
SP_KP_HD double sp_kp_dev2(double x, double mean) {
    const double d = x - mean;
    return d * d;
}
SP_KP_HD double sp_kp_sd(double ss, int C) { return sqrt(ss / (double)C); }
SP_KP_HD bool sp_kp_bad(double mean, double sd) { return !(sd > 0.0) || !isfinite(sd) || !isfinite(mean); }
SP_KP_HD double sp_kp_z(uint32_t count, double len, double mean, double sd) { return (sp_kp_x(count, len) - mean) / sd; }
SP_KP_HD int64_t sp_kp_chunks(int64_t M) { return (M + SP_KP_ROWS - 1) / SP_KP_ROWS; }
// the symmetric half, row a holding columns 0 .. a
SP_KP_HD int64_t sp_kp_tri(int a, int b) { return (int64_t)a * (a + 1) / 2 + b; }
// is candidate (abs_a, row_a) a better sign row than (abs_b, row_b)?  abs < 0 marks "no row"
SP_KP_HD bool sp_kp_better(double abs_a, int64_t row_a, double abs_b, int64_t row_b) {
    return abs_a > abs_b || (abs_a == abs_b && row_a < row_b);
}

// ---- host drivers: the pieces above, looped in the stated orders
// mean and sd of one row; returns whether the row is bad
static inline bool sp_kp_row_stats(const uint32_t *row, const double *len, int C, double *mean, double *sd) {
    double s = 0.0;
    for (int c = 0; c < C; c++) s += sp_kp_x(row[c], len[c]);
    const double m = sp_kp_mean(s, C);
    double ss = 0.0;
    for (int c = 0; c < C; c++) ss += sp_kp_dev2(sp_kp_x(row[c], len[c]), m);
    *mean = m;
    *sd = sp_kp_sd(ss, C);
    return sp_kp_bad(*mean, *sd);
}
// stats: M x 2 (mean, sd); gram: C x C; part: C x C scratch; returns the number of bad rows
static inline int64_t sp_kp_host_gram(const uint32_t *counts, int64_t M, int C, const double *len, double *stats, double *gram,
                                      double *part, double *z) {
    int64_t n_bad = 0;
    for (int64_t i = 0; i < (int64_t)C * C; i++) gram[i] = 0.0;
    for (int64_t r0 = 0; r0 < M; r0 += SP_KP_ROWS) {
        const int64_t r1 = r0 + SP_KP_ROWS < M ? r0 + SP_KP_ROWS : M;
        for (int64_t i = 0; i < (int64_t)C * C; i++) part[i] = 0.0;
        for (int64_t r = r0; r < r1; r++) {
            const uint32_t *row = counts + r * C;
            double mean, sd;
            const bool bad = sp_kp_row_stats(row, len, C, &mean, &sd);
            stats[2 * r] = mean;
            stats[2 * r + 1] = sd;
            if (bad) {
                n_bad++;
                continue;
            }
            for (int c = 0; c < C; c++) z[c] = sp_kp_z(row[c], len[c], mean, sd);
            for (int a = 0; a < C; a++)
                for (int b = 0; b <= a; b++) part[(int64_t)a * C + b] += z[a] * z[b];
        }
        for (int a = 0; a < C; a++)
            for (int b = 0; b <= a; b++) gram[(int64_t)a * C + b] += part[(int64_t)a * C + b];
    }
    for (int a = 0; a < C; a++)
        for (int b = 0; b < a; b++) gram[(int64_t)b * C + a] = gram[(int64_t)a * C + b];
    return n_bad;
}
// U: C x n_comp; rows / vals: n_comp; v: n_comp scratch
static inline void sp_kp_host_signs(const uint32_t *counts, int64_t M, int C, const double *len, const double *U, int n_comp,
                                    int64_t *rows, double *vals, double *v) {
    double best[SP_KP_MAXCOMP];
    for (int j = 0; j < n_comp; j++) {
        best[j] = -1.0;
        rows[j] = -1;
        vals[j] = 0.0;
    }
    for (int64_t r = 0; r < M; r++) {
        const uint32_t *row = counts + r * C;
        double mean, sd;
        if (sp_kp_row_stats(row, len, C, &mean, &sd)) continue;
        for (int j = 0; j < n_comp; j++) v[j] = 0.0;
        for (int c = 0; c < C; c++) {
            const double z = sp_kp_z(row[c], len[c], mean, sd);
            for (int j = 0; j < n_comp; j++) v[j] += U[(int64_t)c * n_comp + j] * z;
        }
        for (int j = 0; j < n_comp; j++)
            if (sp_kp_better(fabs(v[j]), r, best[j], rows[j] < 0 ? INT64_MAX : rows[j])) {
                best[j] = fabs(v[j]);
                rows[j] = r;
                vals[j] = v[j];
            }
    }
}
