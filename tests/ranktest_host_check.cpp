// Host check of subphaser_amd/csrc/sp_ranktest.h (tests/test_ranktest_host.py builds and runs it; -ffp-contract=off).
// Input file:  int64 n_cases, then per case int64 n1, n2, R and the R x (n1 + n2) pooled values (doubles, top group first);
//              int64 n_sums, then per vector int64 n (<= 128) and its n doubles.
// Output file: per row of every case int64 S1, S2, T, then doubles (kruskal stat, kruskal p, mannwhitneyu stat,
//              mannwhitneyu p); per vector the double sp_rt_np_sum gives; then for n1 = 1..8, n2 = 1..64 the uint64 total
//              of sp_rt_exact_table and its n1 n2 + 1 doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_ranktest.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }
template <typename T>
static bool put(FILE *f, const T *in, size_t n = 1) { return fwrite(in, sizeof(T), n, f) == n; }

// the accessor the kernel hands to the header, over a strided column like the kernel's
struct column {
    const double *p;
    int pitch;
    double at(int i) const { return p[(size_t)i * (size_t)pitch]; }
};

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int64_t n_cases = 0;
    if (!get(f, &n_cases)) return 3;
    std::vector<double> sf((size_t)SP_RT_SF_MAX);
    for (int64_t i = 0; i < n_cases; i++) {
        int64_t n1, n2, R;
        if (!get(f, &n1) || !get(f, &n2) || !get(f, &R)) return 3;
        if (n1 < 1 || n1 > SP_RT_MAXG || n2 < 1 || n2 > SP_RT_MAXG || R < 0) return 4;
        const int N = (int)(n1 + n2);
        std::vector<double> x((size_t)(R * N)), col((size_t)(R * N));
        if (!get(f, x.data(), x.size())) return 3;
        for (int64_t r = 0; r < R; r++)            // [i][r], as the kernel keeps v[i][tid]
            for (int c = 0; c < N; c++) col[(size_t)(c * R + r)] = x[(size_t)(r * N + c)];
        const bool has_table = sp_rt_exact_sizes((int)n1, (int)n2);
        if (has_table && sp_rt_exact_table((int)n1, (int)n2, sf.data()) == 0) return 4;
        for (int64_t r = 0; r < R; r++) {
            const column v{col.data() + r, (int)R};
            int S1, S2, T;
            sp_rt_ranks(v, (int)n1, (int)n2, &S1, &S2, &T);
            const int64_t ints[3] = {S1, S2, T};
            double out[4];
            out[1] = sp_rt_row(v, (int)n1, (int)n2, SP_RT_KRUSKAL, nullptr, &out[0]);
            out[3] = sp_rt_row(v, (int)n1, (int)n2, SP_RT_MWU, has_table ? sf.data() : nullptr, &out[2]);
            if (!put(o, ints, 3) || !put(o, out, 4)) return 5;
        }
    }
    int64_t n_sums = 0;
    if (!get(f, &n_sums)) return 3;
    for (int64_t i = 0; i < n_sums; i++) {
        int64_t n;
        if (!get(f, &n) || n < 0 || n > 128) return 3;
        std::vector<double> a((size_t)n + 1);
        if (!get(f, a.data(), (size_t)n)) return 3;
        const column v{a.data(), 1};
        const double s = sp_rt_np_sum(v, (int)n);
        if (!put(o, &s)) return 5;
    }
    for (int n1 = 1; n1 <= SP_RT_EXACT_MAX; n1++)
        for (int n2 = 1; n2 <= SP_RT_MAXG; n2++) {
            const uint64_t total = sp_rt_exact_table(n1, n2, sf.data());
            if (!put(o, &total) || !put(o, sf.data(), (size_t)(n1 * n2 + 1))) return 5;
        }
    fclose(f);
    return fclose(o) ? 5 : 0;
}
