// Host check of subphaser_amd/csrc/sp_kpca.h (tests/test_kpca_host.py builds and runs it; -ffp-contract=off).
// Input file:  int64 n_cases, then per case int64 M, C, n_comp, the C lengths (int64), the M x C counts (uint32) and
//              U (C x n_comp doubles).
// Output file: per case the M x 2 row statistics, the C x C Gram matrix (doubles), int64 n_bad, the n_comp sign rows
//              (int64) and their values (doubles).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_kpca.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }
template <typename T>
static bool put(FILE *f, const T *in, size_t n = 1) { return fwrite(in, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int64_t n_cases = 0;
    if (!get(f, &n_cases)) return 3;
    for (int64_t i = 0; i < n_cases; i++) {
        int64_t M, C, n_comp;
        if (!get(f, &M) || !get(f, &C) || !get(f, &n_comp)) return 3;
        if (M < 1 || C < 2 || C > SP_KP_MAXC || n_comp < 1 || n_comp > SP_KP_MAXCOMP) return 4;
        std::vector<int64_t> lengths((size_t)C), rows((size_t)n_comp);
        std::vector<uint32_t> counts((size_t)(M * C));
        std::vector<double> U((size_t)(C * n_comp)), len((size_t)C), stats((size_t)(2 * M)), gram((size_t)(C * C)),
            part((size_t)(C * C)), z((size_t)C), vals((size_t)n_comp), v((size_t)n_comp);
        if (!get(f, lengths.data(), lengths.size()) || !get(f, counts.data(), counts.size()) || !get(f, U.data(), U.size()))
            return 3;
        for (int64_t c = 0; c < C; c++) len[(size_t)c] = (double)lengths[(size_t)c];
        const int64_t n_bad = sp_kp_host_gram(counts.data(), M, (int)C, len.data(), stats.data(), gram.data(), part.data(), z.data());
        sp_kp_host_signs(counts.data(), M, (int)C, len.data(), U.data(), (int)n_comp, rows.data(), vals.data(), v.data());
        if (!put(o, stats.data(), stats.size()) || !put(o, gram.data(), gram.size()) || !put(o, &n_bad) ||
            !put(o, rows.data(), rows.size()) || !put(o, vals.data(), vals.size()))
            return 5;
    }
    fclose(f);
    return fclose(o) ? 5 : 0;
}
