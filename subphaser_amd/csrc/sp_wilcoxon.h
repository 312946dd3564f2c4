// sp_wilcoxon.h -- the arithmetic of the paired k-mer test (k7_wilcoxon, sp_wilcoxon.hip): the Wilcoxon signed-rank test
// between the highest-mean and the second-highest-mean subgenome group of a k-mer, what the reference gets from
// scipy.stats.wilcoxon per row (Cluster.py:178-194; scipy 1.13 .. 1.16, method="auto", correction=False, two-sided,
// zero_method="wilcox").  The statistic and two of the three p-value branches are functions of small integers, so they
// are bit-defined; only erfc is the platform's.
//
// __host__ __device__, so that tests/test_wilcoxon_host.py builds it with the host compiler and checks it against the
// numpy twin (tests/wilcoxon_ref.py).  Build with -ffp-contract=off: the orders below are scipy's.
//
// A row has n pairs, 2 <= n <= SP_WX_MAXG: d[j] = a[j] - b[j], a the top group and b the second in config order.
// Ranks  zeros of d are dropped; m = #{j: d[j] != 0}.  Among the nonzero |d|
//          r2[j] = 2 #{i nz: |d_i| < |d_j|} + e_j + 1,  e_j = #{i nz: |d_i| == |d_j|} (j itself included):
//        twice the midrank, an integer, found by n^2 comparisons -- no sort.  T = sum_nz (e_j^2 - 1) = scipy's sum over
//        tie groups of t^3 - t.  W2 = the sum of r2[j] over d[j] > 0; r_plus = W2 / 2.0, exact.
//        stat = min(r_plus, m (m + 1) / 2 - r_plus): scipy's two-sided statistic.
// Branch (what scipy's "auto" picks for the row)
//   exact        no zero, T == 0 and n <= 50:  p = clip(2 tab[W2 / 2], 0, 1),  tab[s] = min(P(W <= s), P(W >= s)) for W the
//                sum of a uniform random subset of {1 .. n} (sp_wx_exact_table, host: integers, one exact division).
//   permutation  a zero or a tie, n <= 13:  le = #{subsets of the m nonzero doubled ranks with sum <= W2} << (n - m), ge
//                the same for >= W2;  p = min(1, min(le, ge) / 2^n * 2).  Integers until one division by a power of two;
//                m = 0 gives 1.
//   asymptotic   everything else:  mn = m (m + 1.) * 0.25,  se = sqrt((m (m + 1.) (2. m + 1.) - T / 2) / 24),
//                z = (r_plus - mn) / se,  p = 2 * (0.5 * erfc(|z| / sqrt(2))).  m = 0: 0 / 0, p = NaN, as scipy returns.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_WX_HD __host__ __device__ __forceinline__
#else
#define SP_WX_HD static inline
#endif

#define SP_WX_MAXG 64                                   // pairs of a row: chromosomes per group
#define SP_WX_EXACT_MAX 50                              // scipy's exact null: up to this many pairs
#define SP_WX_PERM_MAX 13                               // scipy's deterministic permutation test: 2^13 < 9999 resamples
#define SP_WX_TAB_MAX (SP_WX_EXACT_MAX * (SP_WX_EXACT_MAX + 1) / 2 + 1)     // entries of the table: s = 0 .. n (n + 1) / 2
#define SP_WX_EXACT 0
#define SP_WX_PERM 1
#define SP_WX_ASYM 2

// the integers of a row.  V: double at(int i), void set(int i, double x).  v[0 .. n) holds d; the doubled ranks of the
// nonzero d are written to v[n .. n + m) in the order of j (what the permutation walk reads).
template <class V>
SP_WX_HD void sp_wx_ranks(const V &v, int n, int *m_out, int *W2_out, int *T_out) {
    int m = 0, w2 = 0, t = 0;
    for (int j = 0; j < n; j++) {
        const double dj = v.at(j);
        if (dj == 0.0) continue;
        const double aj = fabs(dj);
        int lt = 0, eq = 0;
        for (int i = 0; i < n; i++) {
            const double di = v.at(i);
            const double ai = fabs(di);
            lt += (di != 0.0 && ai < aj) ? 1 : 0;
            eq += ai == aj ? 1 : 0;           // aj > 0, so a zero never counts
        }
        const int r2 = 2 * lt + eq + 1;
        v.set(n + m, (double)r2);
        m++;
        if (dj > 0.0) w2 += r2;
        t += eq * eq - 1;
    }
    *m_out = m;
    *W2_out = w2;
    *T_out = t;
}

SP_WX_HD int sp_wx_branch(int n, int m, int T) {
    if (m == n && T == 0 && n <= SP_WX_EXACT_MAX) return SP_WX_EXACT;
    return n <= SP_WX_PERM_MAX ? SP_WX_PERM : SP_WX_ASYM;
}

SP_WX_HD double sp_wx_stat(int m, int W2) {
    const double r_plus = (double)W2 / 2.0, r_minus = (double)(m * (m + 1) - W2) / 2.0;
    return r_plus < r_minus ? r_plus : r_minus;
}

// the permutation branch: a Gray-code walk over the 2^m sign assignments of the doubled ranks in v[n .. n + m), one add or
// subtract and two compares per step; m <= n <= SP_WX_PERM_MAX, so the walk has at most 8192 steps and the counters fit
SP_WX_HD double sp_wx_perm_p(int n, int m, unsigned le, unsigned ge) {
    const unsigned lo = (le < ge ? le : ge) << (n - m);
    const double p = (double)lo / (double)(1u << n) * 2.0;
    return p > 1.0 ? 1.0 : p;
}
template <class V>
SP_WX_HD double sp_wx_perm_walk(const V &v, int n, int m, int W2) {
    unsigned le = W2 >= 0 ? 1u : 0u, ge = W2 <= 0 ? 1u : 0u;      // the empty subset: sum 0
    int s = 0;
    const unsigned steps = 1u << m;
    for (unsigned k = 1; k < steps; k++) {
        const int bit = __builtin_ctz(k);                         // the element the Gray code toggles at step k
        const int r2 = (int)v.at(n + bit);
        s += (((k ^ (k >> 1)) >> bit) & 1u) ? r2 : -r2;
        le += s <= W2 ? 1u : 0u;
        ge += s >= W2 ? 1u : 0u;
    }
    return sp_wx_perm_p(n, m, le, ge);
}

SP_WX_HD double sp_wx_asym(int m, int W2, int T) {
    const double c = (double)m, r_plus = (double)W2 / 2.0;
    const double mn = c * (c + 1.0) * 0.25;
    double se = c * (c + 1.0) * (2.0 * c + 1.0);
    se -= (double)T / 2.0;
    se = sqrt(se / 24.0);
    const double z = (r_plus - mn) / se;
    return 2.0 * (0.5 * erfc(fabs(z) / 1.4142135623730951 /* sqrt(2) */));
}

// tab: the table of n (sp_wx_exact_table), read only on the exact branch
SP_WX_HD double sp_wx_exact(int W2, const double *tab) {
    const double p = 2.0 * tab[W2 / 2];       // no ties: every r2 is even
    return p < 0.0 ? 0.0 : p > 1.0 ? 1.0 : p;
}

// one row: p, the statistic and the branch taken for the differences in v[0 .. n); v[n .. 2n) is overwritten
template <class V>
SP_WX_HD double sp_wx_row(const V &v, int n, const double *tab, double *stat, int *branch) {
    int m, W2, T;
    sp_wx_ranks(v, n, &m, &W2, &T);
    *stat = sp_wx_stat(m, W2);
    const int br = sp_wx_branch(n, m, T);
    *branch = br;
    if (br == SP_WX_EXACT) return sp_wx_exact(W2, tab);
    if (br == SP_WX_PERM) return sp_wx_perm_walk(v, n, m, W2);
    return sp_wx_asym(m, W2, T);
}

// ---- host: the exact null distribution of r_plus for n pairs without ties or zeros, 1 <= n <= SP_WX_EXACT_MAX.  The number
// of subsets of {1 .. n} with sum s is counted in uint64 (the total is 2^n <= 2^50), cumulated from both ends as integers,
// and min(#{W <= s}, #{W >= s}) divided once by 2^n: exact in fp64.  Writes n (n + 1) / 2 + 1 entries; returns the total.
static inline uint64_t sp_wx_exact_table(int n, double *tab) {
    if (n < 1 || n > SP_WX_EXACT_MAX) return 0;
    const int D = n * (n + 1) / 2;
    uint64_t c[SP_WX_TAB_MAX];
    for (int s = 0; s <= D; s++) c[s] = 0;
    c[0] = 1;
    for (int i = 1; i <= n; i++)
        for (int s = D; s >= i; s--) c[s] += c[s - i];
    const uint64_t total = (uint64_t)1 << n;
    uint64_t le = 0;
    for (int s = 0; s <= D; s++) {
        const uint64_t ge = total - le;      // #{W >= s}
        le += c[s];                          // #{W <= s}
        tab[s] = (double)(le < ge ? le : ge) / (double)total;
    }
    return le;
}
