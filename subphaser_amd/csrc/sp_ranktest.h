// sp_ranktest.h -- the arithmetic of the two rank-sum k-mer tests (k7_ranktest, sp_ranktest.hip): Kruskal-Wallis and
// Mann-Whitney between the highest-mean and the second-highest-mean subgenome group of a k-mer, what the reference gets
// from scipy.stats.kruskal / mannwhitneyu per row (Cluster.py:178-194).  Both are functions of three integers of the
// pooled sample, so the statistic is bit-defined; only erfc is the platform's.
//
// __host__ __device__, so that tests/test_ranktest_host.py builds it with the host compiler and checks it against the
// numpy twin (tests/ranktest_ref.py).  Build with -ffp-contract=off: the orders below are scipy's, and a fused
// multiply-add changes the statistic.
//
// x[0 .. n1) are the values of the top group, x[n1 .. N) those of the second, N = n1 + n2, 1 <= n1, n2 <= SP_RT_MAXG.
// Ranks  r2[i] = 2 #{j: x[j] < x[i]} + e_i + 1,  e_i = #{j: x[j] == x[i]} (i itself included): twice the midrank, an
//        integer, found by N^2 comparisons -- no sort.  S1, S2 = the sums of r2 over the two groups; R1 = S1 / 2.0 and
//        R2 = S2 / 2.0 are the rank sums, exact.  T = sum_i (e_i^2 - 1) = scipy's sum over tie groups of t^3 - t.
// kruskal       ties = 1.0 - T / (N^3 - N); ties == 0 (all values identical): p = 1, stat = NaN.  Otherwise
//               ssbn = R1 * R1 / n1 + R2 * R2 / n2,  H = (12.0 / (N (N + 1)) * ssbn - 3 (N + 1)) / ties,  stat = H,
//               p = erfc(sqrt(H / 2)) for H > 0 and 1 otherwise: chdtrc(1, H).
// mannwhitneyu  (two-sided, use_continuity=True, method="auto" of scipy 1.15)
//               U1 = R1 - n1 (n1 + 1) / 2, U2 = n1 n2 - U1, U = max(U1, U2), stat = U1.
//               exact, when T == 0 and (n1 <= 8 or n2 <= 8): p = 2 sf[(int)U], sf[u] = P(statistic >= u) from the table
//               of the size pair (sp_rt_exact_table, host);
//               asymptotic otherwise: s = sqrt(n1 n2 / 12 * ((N + 1) - T / (N (N - 1)))), z = (U - n1 n2 / 2 - 0.5) / s
//               (s == 0, all values identical: z = -inf), p = 2 * (0.5 * erfc(z / sqrt(2))).
//               Both clipped to [0, 1].
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_RT_HD __host__ __device__ __forceinline__
#else
#define SP_RT_HD static inline
#endif

#define SP_RT_MAXG 64                                   // chromosomes per group
#define SP_RT_KRUSKAL 0
#define SP_RT_MWU 1
#define SP_RT_EXACT_MAX 8                               // exact Mann-Whitney null: the smaller group has at most this many
#define SP_RT_SF_MAX (SP_RT_EXACT_MAX * SP_RT_MAXG + 1) // entries of one table: u = 0 .. n1 n2
#define SP_RT_SF_SLOTS (SP_RT_EXACT_MAX * SP_RT_MAXG)   // size pairs that can have one

// slot of a size pair in the offset table handed to the kernel (the null distribution is symmetric in n1, n2)
SP_RT_HD int sp_rt_sf_slot(int n1, int n2) {
    const int lo = n1 < n2 ? n1 : n2, hi = n1 < n2 ? n2 : n1;
    return (lo - 1) * SP_RT_MAXG + (hi - 1);
}
SP_RT_HD bool sp_rt_exact_sizes(int n1, int n2) { return n1 <= SP_RT_EXACT_MAX || n2 <= SP_RT_EXACT_MAX; }

// numpy's float64 add.reduce of a contiguous vector of n <= 128 values (one leaf of its pairwise sum: eight lane sums,
// combined as a tree, then the n % 8 tail), what d_np_sum of sp_enrich.hip is; V: double at(int i)
template <class V>
SP_RT_HD double sp_rt_np_sum(const V &v, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; i++) r += v.at(i);
        return r;
    }
    double r0 = v.at(0), r1 = v.at(1), r2 = v.at(2), r3 = v.at(3), r4 = v.at(4), r5 = v.at(5), r6 = v.at(6), r7 = v.at(7);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += v.at(i);
        r1 += v.at(i + 1);
        r2 += v.at(i + 2);
        r3 += v.at(i + 3);
        r4 += v.at(i + 4);
        r5 += v.at(i + 5);
        r6 += v.at(i + 6);
        r7 += v.at(i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += v.at(i);
    return res;
}

// the three integers of a pooled sample of n1 + n2 values; V: double at(int i)
template <class V>
SP_RT_HD void sp_rt_ranks(const V &v, int n1, int n2, int *S1, int *S2, int *T) {
    const int N = n1 + n2;
    int s1 = 0, s2 = 0, t = 0;
    for (int i = 0; i < N; i++) {
        const double xi = v.at(i);
        int lt = 0, eq = 0;
        for (int j = 0; j < N; j++) {
            const double xj = v.at(j);
            lt += xj < xi ? 1 : 0;
            eq += xj == xi ? 1 : 0;
        }
        const int r2 = 2 * lt + eq + 1;
        if (i < n1) s1 += r2;
        else s2 += r2;
        t += eq * eq - 1;
    }
    *S1 = s1;
    *S2 = s2;
    *T = t;
}

SP_RT_HD double sp_rt_clip01(double p) { return p < 0.0 ? 0.0 : p > 1.0 ? 1.0 : p; }

SP_RT_HD double sp_rt_kruskal(int n1, int n2, int S1, int S2, int T, double *stat) {
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
SP_RT_HD double sp_rt_mwu(int n1, int n2, int S1, int T, const double *sf, double *stat) {
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
    return sp_rt_clip01(p);
}

// one row: p and the statistic of `method` for the pooled sample behind v
template <class V>
SP_RT_HD double sp_rt_row(const V &v, int n1, int n2, int method, const double *sf, double *stat) {
    int S1, S2, T;
    sp_rt_ranks(v, n1, n2, &S1, &S2, &T);
    return method == SP_RT_KRUSKAL ? sp_rt_kruskal(n1, n2, S1, S2, T, stat) : sp_rt_mwu(n1, n2, S1, T, sf, stat);
}

// ---- host: the exact null distribution of the Mann-Whitney statistic for sizes (n1, n2), min(n1, n2) <= SP_RT_EXACT_MAX,
// max(n1, n2) <= SP_RT_MAXG.  The number of arrangements with statistic u is the coefficient of q^u in the Gaussian
// binomial [m + n choose m]_q = prod_{i = 1..m} (1 - q^(n + i)) / (1 - q^i); each factor is applied to the coefficient
// vector in place, in uint64 (intermediate values wrap, the quotients do not: the largest total is C(72, 8) = 1.2e10).
// The counts are cumulated from the top as integers and divided once by the total, so sf[u] is the correctly rounded
// quotient of two integers below 2^53.  Writes n1 n2 + 1 entries; returns the total, C(n1 + n2, n1).
static inline uint64_t sp_rt_exact_table(int n1, int n2, double *sf) {
    const int m = n1 < n2 ? n1 : n2, n = n1 < n2 ? n2 : n1, D = m * n;
    uint64_t c[SP_RT_SF_MAX];
    if (m < 1 || m > SP_RT_EXACT_MAX || n > SP_RT_MAXG) return 0;
    for (int j = 0; j <= D; j++) c[j] = 0;
    c[0] = 1;
    for (int i = 1; i <= m; i++) {
        for (int j = D; j >= n + i; j--) c[j] -= c[j - (n + i)];
        for (int j = i; j <= D; j++) c[j] += c[j - i];
    }
    uint64_t total = 0, cum = 0;
    for (int j = 0; j <= D; j++) total += c[j];
    for (int j = D; j >= 0; j--) {
        cum += c[j];
        sf[j] = (double)cum / (double)total;
    }
    return total;
}
