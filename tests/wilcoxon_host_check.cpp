// Host check of subphaser_amd/csrc/sp_wilcoxon.h (tests/test_wilcoxon_host.py builds and runs it; -ffp-contract=off).
// Input file:  int64 n_cases, then per case int64 n, R and the R x 2n values of the rows (doubles: the n values of the top
//              group, then the n of the second).
// Output file: per row of every case int64 m, W2, T, branch, then doubles (stat, p); then for n = 1 .. 50 the uint64 total
//              of sp_wx_exact_table and its n (n + 1) / 2 + 1 doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_wilcoxon.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }
template <typename T>
static bool put(FILE *f, const T *in, size_t n = 1) { return fwrite(in, sizeof(T), n, f) == n; }

// the accessor the kernel hands to the header, over a strided column like the kernel's
struct column {
    double *p;
    int pitch;
    double at(int i) const { return p[(size_t)i * (size_t)pitch]; }
    void set(int i, double x) const { p[(size_t)i * (size_t)pitch] = x; }
};

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int64_t n_cases = 0;
    if (!get(f, &n_cases)) return 3;
    std::vector<double> tab((size_t)SP_WX_TAB_MAX);
    for (int64_t i = 0; i < n_cases; i++) {
        int64_t n64, R;
        if (!get(f, &n64) || !get(f, &R)) return 3;
        if (n64 < 2 || n64 > SP_WX_MAXG || R < 0) return 4;
        const int n = (int)n64, N = 2 * n;
        std::vector<double> x((size_t)(R * N)), col((size_t)(R * N));
        if (!get(f, x.data(), x.size())) return 3;
        for (int64_t r = 0; r < R; r++)            // [i][r], as the kernel keeps v[i][tid]
            for (int c = 0; c < N; c++) col[(size_t)(c * R + r)] = x[(size_t)(r * N + c)];
        if (n <= SP_WX_EXACT_MAX && sp_wx_exact_table(n, tab.data()) != ((uint64_t)1 << n)) return 4;
        for (int64_t r = 0; r < R; r++) {
            const column v{col.data() + r, (int)R};
            for (int j = 0; j < n; j++) v.set(j, v.at(j) - v.at(n + j));       // the kernel's d = a - b, in place
            int m, W2, T, branch;
            double out[2];
            out[1] = sp_wx_row(v, n, tab.data(), &out[0], &branch);
            const column w{col.data() + r, (int)R};
            sp_wx_ranks(w, n, &m, &W2, &T);                                    // d is still in v[0 .. n)
            const int64_t ints[4] = {m, W2, T, branch};
            if (!put(o, ints, 4) || !put(o, out, 2)) return 5;
        }
    }
    for (int n = 1; n <= SP_WX_EXACT_MAX; n++) {
        const uint64_t total = sp_wx_exact_table(n, tab.data());
        if (!put(o, &total) || !put(o, tab.data(), (size_t)(n * (n + 1) / 2 + 1))) return 5;
    }
    fclose(f);
    return fclose(o) ? 5 : 0;
}
