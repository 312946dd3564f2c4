// sp_rankwide.h -- the arithmetic of the rank-sum k-mer tests for subgenomes of up to SP_RW_MAXG chromosomes
// (k7_ranktest_wide, sp_rankwide.hip): the definitions of sp_ranktest.h at sizes where the three integers of a pooled
// sample no longer fit in 32 bits and N^2 comparisons per row no longer pay.
//
// __host__ __device__, so that tests/test_rankwide_host.py builds it with the host compiler and checks it against the
// numpy twin (tests/rankwide_ref.py).  Build with -ffp-contract=off, as sp_ranktest.h.
//
// x[0 .. n1) are the values of the top group, x[n1 .. N) those of the second, N = n1 + n2, 1 <= n1, n2 <= SP_RW_MAXG.
// Ranks  r2[i] = 2 #{j: x[j] < x[i]} + e_i + 1, e_i = #{j: x[j] == x[i]}; S1, S2 = the sums of r2 over the two groups
//        (at most N (N + 1) = 6.7e7), T = sum_i (e_i^2 - 1) (at most N^3 - N = 5.5e11): int64_t, every value below 2^53,
//        so the conversions to double are exact.  Here each group's values are SORTED and an element is ranked by its
//        lower and upper bounds in both sorted segments: lt = lb1 + lb2, eq = (ub1 - lb1) + (ub2 - lb2).  The three
//        results are integers: any correct ranking gives the same bits (sp_rw_ranks is the host form the tests run;
//        the kernel sorts in LDS with a bitonic network and searches with sp_rw_lower / sp_rw_upper).
// Statistics: sp_rw_kruskal and sp_rw_mwu are sp_rt_kruskal and sp_rt_mwu operation for operation on the 64-bit
//        integers -- at sizes both headers accept, the statistic and p are the same bits.
// Exact Mann-Whitney null: scipy 1.15 takes it whenever a row has no ties and min(n1, n2) <= 8, whatever the larger
//        size; sp_rw_exact_table builds the table of a size pair on the host.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_RW_HD __host__ __device__ __forceinline__
#else
#define SP_RW_HD static inline
#endif

#define SP_RW_MAXG 4096                                 // chromosomes per group: a pooled row is at most 64 KiB of doubles
#define SP_RW_KRUSKAL 0
#define SP_RW_MWU 1
#define SP_RW_EXACT_MAX 8                               // exact Mann-Whitney null: the smaller group has at most this many
#define SP_RW_SF_MAX (SP_RW_EXACT_MAX * SP_RW_MAXG + 1) // entries of the largest table: u = 0 .. n1 n2
#define SP_RW_SF_SLOTS (SP_RW_EXACT_MAX * SP_RW_MAXG)   // size pairs that can have one

// slot of a size pair in the offset table handed to the kernel (the null distribution is symmetric in n1, n2)
SP_RW_HD int sp_rw_sf_slot(int n1, int n2) {
    const int lo = n1 < n2 ? n1 : n2, hi = n1 < n2 ? n2 : n1;
    return (lo - 1) * SP_RW_MAXG + (hi - 1);
}
SP_RW_HD bool sp_rw_exact_sizes(int n1, int n2) { return n1 <= SP_RW_EXACT_MAX || n2 <= SP_RW_EXACT_MAX; }
// the smallest power of two >= n (n >= 1): the length a segment is padded to with +inf
SP_RW_HD int sp_rw_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// #{j < P: v[j] < x} and #{j < P: v[j] <= x} in an ascending segment of P values, P a power of two: log2(P) + 1 probes,
// the same number for every x.  V: double at(int i)
template <class V>
SP_RW_HD int sp_rw_lower(const V &v, int P, double x) {
    int pos = 0;
    for (int step = P >> 1; step > 0; step >>= 1)
        if (v.at(pos + step - 1) < x) pos += step;
    return pos + (v.at(pos) < x ? 1 : 0);
}
template <class V>
SP_RW_HD int sp_rw_upper(const V &v, int P, double x) {
    int pos = 0;
    for (int step = P >> 1; step > 0; step >>= 1)
        if (v.at(pos + step - 1) <= x) pos += step;
    return pos + (v.at(pos) <= x ? 1 : 0);
}
// what one element contributes: lt and eq from its bounds in the two sorted segments (a: P1 values, b: P2 values)
template <class V>
SP_RW_HD void sp_rw_rank_one(const V &a, int P1, const V &b, int P2, double x, int *lt, int *eq) {
    const int lb1 = sp_rw_lower(a, P1, x), ub1 = sp_rw_upper(a, P1, x);
    const int lb2 = sp_rw_lower(b, P2, x), ub2 = sp_rw_upper(b, P2, x);
    *lt = lb1 + lb2;
    *eq = (ub1 - lb1) + (ub2 - lb2);
}

SP_RW_HD double sp_rw_clip01(double p) { return p < 0.0 ? 0.0 : p > 1.0 ? 1.0 : p; }

SP_RW_HD double sp_rw_kruskal(int n1, int n2, int64_t S1, int64_t S2, int64_t T, double *stat) {
    const double N = (double)(n1 + n2);
    const double R1 = (double)S1 / 2.0, R2 = (double)S2 / 2.0;
    const double ties = 1.0 - (double)T / (N * N * N - N);
    if (ties == 0.0) {
        *stat = NAN;
        return 1.0;
    }
    const double ssbn = R1 * R1 / (double)n1 + R2 * R2 / (double)n2;
    const double H = (12.0 / (N * (N + 1.0)) * ssbn - 3.0 * (N + 1.0)) / ties;
    *stat = H;
    return H > 0.0 ? erfc(sqrt(H / 2.0)) : 1.0;
}

// sf: the table of the size pair, n1 n2 + 1 entries, or NULL when the sizes have none (then the asymptotic branch is taken)
SP_RW_HD double sp_rw_mwu(int n1, int n2, int64_t S1, int64_t T, const double *sf, double *stat) {
    const double N = (double)(n1 + n2), nn = (double)(n1 * n2);
    const double R1 = (double)S1 / 2.0;
    const double U1 = R1 - (double)(n1 * (n1 + 1)) / 2.0;
    const double U2 = nn - U1;
    const double U = U1 > U2 ? U1 : U2;
    *stat = U1;
    double p;
    if (T == 0 && sf) {
        int u = (int)U;     // no ties: U is an integer in [n1 n2 / 2, n1 n2]
        u = u < 0 ? 0 : u > n1 * n2 ? n1 * n2 : u;
        p = 2.0 * sf[u];
    } else {
        const double s = sqrt(nn / 12.0 * ((N + 1.0) - (double)T / (N * (N - 1.0))));
        const double z = (U - nn / 2.0 - 0.5) / s;
        p = 2.0 * (0.5 * erfc(z / 1.4142135623730951 /* sqrt(2) */));
    }
    return sp_rw_clip01(p);
}

SP_RW_HD double sp_rw_stat(int n1, int n2, int method, int64_t S1, int64_t S2, int64_t T, const double *sf, double *stat) {
    return method == SP_RW_KRUSKAL ? sp_rw_kruskal(n1, n2, S1, S2, T, stat) : sp_rw_mwu(n1, n2, S1, T, sf, stat);
}

// ---- host: the three integers of a pooled sample by the reference form above.  a and b are the two groups' values
// padded with +inf to P1 = sp_rw_pow2(n1) and P2 = sp_rw_pow2(n2) entries; both are sorted in place.
struct sp_rw_span {
    const double *p;
    double at(int i) const { return p[i]; }
};
static inline void sp_rw_sort(double *v, int n) {        // shell sort: no allocation, no library
    for (int gap = n / 2; gap > 0; gap /= 2)
        for (int i = gap; i < n; i++) {
            const double x = v[i];
            int j = i;
            for (; j >= gap && v[j - gap] > x; j -= gap) v[j] = v[j - gap];
            v[j] = x;
        }
}
static inline void sp_rw_ranks(double *a, int n1, double *b, int n2, int64_t *S1, int64_t *S2, int64_t *T) {
    const int P1 = sp_rw_pow2(n1), P2 = sp_rw_pow2(n2);
    sp_rw_sort(a, P1);
    sp_rw_sort(b, P2);
    const sp_rw_span va{a}, vb{b};
    int64_t s1 = 0, s2 = 0, t = 0;
    for (int i = 0; i < n1 + n2; i++) {
        int lt, eq;
        sp_rw_rank_one(va, P1, vb, P2, i < n1 ? a[i] : b[i - n1], &lt, &eq);
        const int64_t r2 = 2 * (int64_t)lt + eq + 1;
        if (i < n1) s1 += r2;
        else s2 += r2;
        t += (int64_t)eq * eq - 1;
    }
    *S1 = s1;
    *S2 = s2;
    *T = t;
}

// ---- host: the exact null distribution of the Mann-Whitney statistic for sizes (n1, n2), min(n1, n2) <= SP_RW_EXACT_MAX,
// max(n1, n2) <= SP_RW_MAXG: the Gaussian-binomial recurrence of sp_rt_exact_table in unsigned __int128 (the largest
// total, C(4104, 8), needs 81 bits; intermediate values wrap, the coefficients do not).  `work` holds n1 n2 + 1 entries.
// The counts are cumulated from the top as integers; sf[u] is one quotient: of two doubles where the total is below 2^53
// (both exact: the correctly rounded fraction, the bits sp_rt_exact_table gives), in long double rounded to double
// beyond -- the operands and the quotient are rounded to the 64-bit mantissa (a relative 2^-63 in all), then the quotient
// to 53 bits: within 1 ulp of the correctly rounded fraction.
// Writes n1 n2 + 1 entries; returns the total, C(n1 + n2, n1), or 0 for sizes outside the range.
typedef unsigned __int128 sp_rw_u128;
static inline sp_rw_u128 sp_rw_exact_table(int n1, int n2, sp_rw_u128 *work, double *sf) {
    const int m = n1 < n2 ? n1 : n2, n = n1 < n2 ? n2 : n1, D = m * n;
    if (m < 1 || m > SP_RW_EXACT_MAX || n > SP_RW_MAXG) return 0;
    sp_rw_u128 *c = work;
    for (int j = 0; j <= D; j++) c[j] = 0;
    c[0] = 1;
    for (int i = 1; i <= m; i++) {
        for (int j = D; j >= n + i; j--) c[j] -= c[j - (n + i)];
        for (int j = i; j <= D; j++) c[j] += c[j - i];
    }
    sp_rw_u128 total = 0, cum = 0;
    for (int j = 0; j <= D; j++) total += c[j];
    const bool small = total < ((sp_rw_u128)1 << 53);
    for (int j = D; j >= 0; j--) {
        cum += c[j];
        sf[j] = small ? (double)(uint64_t)cum / (double)(uint64_t)total : (double)((long double)cum / (long double)total);
    }
    return total;
}
