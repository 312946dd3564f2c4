// Host check of subphaser_amd/csrc/sp_hclust.h (tests/test_hclust_host.py builds and runs it; -ffp-contract=off).
// Input file:  int64 n_cases, then per case int64 P, D and the P x D points (doubles).
// Output file: per case the P x P distance matrix before the first merge, the (P - 1) x 4 merges (doubles), then int64
//              status and int64 scans of the chain.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_hclust.h"

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
        int64_t P, D;
        if (!get(f, &P) || !get(f, &D)) return 3;
        if (P < 2 || P > SP_HC_MAXP || D < 1) return 4;
        std::vector<double> pts((size_t)(P * D)), dist((size_t)(P * P)), work, merges((size_t)((P - 1) * 4));
        std::vector<int> size((size_t)P), chain((size_t)P);
        if (!get(f, pts.data(), pts.size())) return 3;
        sp_hc_host_dist(pts.data(), (int)P, (int)D, dist.data());
        work = dist;
        int64_t scans = 0;
        const int64_t status = sp_hc_host_chain(work.data(), (int)P, size.data(), chain.data(), merges.data(), &scans);
        if (!put(o, dist.data(), dist.size()) || !put(o, merges.data(), merges.size()) || !put(o, &status) || !put(o, &scans))
            return 5;
    }
    fclose(f);
    return fclose(o) ? 5 : 0;
}
