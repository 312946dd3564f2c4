// Host check of subphaser_amd/csrc/sp_rankwide.h (tests/test_rankwide_host.py builds and runs it; -ffp-contract=off).
// Input file:  int64 n_cases, then per case int64 n1, n2, R and the R x (n1 + n2) pooled values (doubles, top group first);
//              int64 n_tables, then per table int64 n1, n2.
// Output file: per row of every case int64 S1, S2, T, doubles (kruskal stat, kruskal p, mannwhitneyu stat, mannwhitneyu p)
//              of sp_rankwide.h, then the same four doubles of sp_ranktest.h (zeros where a group has more than 64 values);
//              per table the total of sp_rw_exact_table as uint64 low, high and its n1 n2 + 1 doubles.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sp_rankwide.h"
#include "sp_ranktest.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }
template <typename T>
static bool put(FILE *f, const T *in, size_t n = 1) { return fwrite(in, sizeof(T), n, f) == n; }

struct span {
    const double *p;
    double at(int i) const { return p[i]; }
};

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int64_t n_cases = 0;
    if (!get(f, &n_cases)) return 3;
    std::vector<sp_rw_u128> work((size_t)SP_RW_SF_MAX);
    std::vector<double> sf((size_t)SP_RW_SF_MAX), sf_narrow((size_t)SP_RT_SF_MAX);
    for (int64_t i = 0; i < n_cases; i++) {
        int64_t n1, n2, R;
        if (!get(f, &n1) || !get(f, &n2) || !get(f, &R)) return 3;
        if (n1 < 1 || n1 > SP_RW_MAXG || n2 < 1 || n2 > SP_RW_MAXG || R < 0) return 4;
        const int N = (int)(n1 + n2), P1 = sp_rw_pow2((int)n1), P2 = sp_rw_pow2((int)n2);
        std::vector<double> x((size_t)(R * N)), a((size_t)P1), b((size_t)P2);
        if (!get(f, x.data(), x.size())) return 3;
        const bool has_table = sp_rw_exact_sizes((int)n1, (int)n2);
        if (has_table && sp_rw_exact_table((int)n1, (int)n2, work.data(), sf.data()) == 0) return 4;
        const bool narrow = n1 <= SP_RT_MAXG && n2 <= SP_RT_MAXG;
        if (narrow && has_table && sp_rt_exact_table((int)n1, (int)n2, sf_narrow.data()) == 0) return 4;
        for (int64_t r = 0; r < R; r++) {
            const double *row = x.data() + r * N;
            for (int j = 0; j < P1; j++) a[(size_t)j] = j < n1 ? row[j] : std::numeric_limits<double>::infinity();
            for (int j = 0; j < P2; j++) b[(size_t)j] = j < n2 ? row[n1 + j] : std::numeric_limits<double>::infinity();
            int64_t ints[3];
            sp_rw_ranks(a.data(), (int)n1, b.data(), (int)n2, &ints[0], &ints[1], &ints[2]);
            double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            out[1] = sp_rw_stat((int)n1, (int)n2, SP_RW_KRUSKAL, ints[0], ints[1], ints[2], nullptr, &out[0]);
            out[3] = sp_rw_stat((int)n1, (int)n2, SP_RW_MWU, ints[0], ints[1], ints[2], has_table ? sf.data() : nullptr, &out[2]);
            if (narrow) {
                const span v{row};
                out[5] = sp_rt_row(v, (int)n1, (int)n2, SP_RT_KRUSKAL, nullptr, &out[4]);
                out[7] = sp_rt_row(v, (int)n1, (int)n2, SP_RT_MWU, has_table ? sf_narrow.data() : nullptr, &out[6]);
            }
            if (!put(o, ints, 3) || !put(o, out, 8)) return 5;
        }
    }
    int64_t n_tables = 0;
    if (!get(f, &n_tables)) return 3;
    for (int64_t i = 0; i < n_tables; i++) {
        int64_t n1, n2;
        if (!get(f, &n1) || !get(f, &n2)) return 3;
        const sp_rw_u128 total = sp_rw_exact_table((int)n1, (int)n2, work.data(), sf.data());
        if (total == 0) return 4;
        const uint64_t halves[2] = {(uint64_t)total, (uint64_t)(total >> 64)};
        if (!put(o, halves, 2) || !put(o, sf.data(), (size_t)(n1 * n2 + 1))) return 5;
    }
    fclose(f);
    return fclose(o) ? 5 : 0;
}
