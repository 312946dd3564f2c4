// Host check of subphaser_amd/csrc/sp_kboot.h (tests/test_kboot_host.py builds and runs it; -ffp-contract=off).
// Input file: int64 n_cases, then per case int64 C, K, uint64 seed, rep and the C x C Gram matrix (doubles);
//             int64 n_draws, then per draw uint64 seed, rep, i.
// Output:     "R <iters> <label 0> ... <label C-1>" per case, "U <u as %a>" per draw, "T <K> <trials>" for K = 1 .. 64.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_kboot.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n_cases = 0;
    if (!get(f, &n_cases)) return 3;
    std::vector<double> G, work;
    std::vector<int32_t> labels;
    for (int64_t i = 0; i < n_cases; i++) {
        int64_t C, K;
        uint64_t seed, rep;
        if (!get(f, &C) || !get(f, &K) || !get(f, &seed) || !get(f, &rep)) return 3;
        if (C < 1 || C > SP_KB_MAXC || K < 1 || K > SP_KB_MAXK || K > C) return 4;
        G.resize((size_t)(C * C));
        if (!get(f, G.data(), G.size())) return 3;
        work.assign((size_t)((SP_KB_MAXK + 1) * C), 0.0);
        labels.assign((size_t)C, -1);
        int it;
        if (i & 1) {     // the symmetric half the kernel keeps, on every other case
            std::vector<double> H((size_t)(C * (C + 1) / 2));
            for (int a = 0; a < C; a++)
                for (int b = 0; b <= a; b++) H[(size_t)sp_kb_tri(a, b)] = G[(size_t)(a * C + b)];
            it = sp_kb_solve(sp_kb_half{H.data()}, (int)C, (int)K, seed, rep, labels.data(), work.data());
        } else {
            it = sp_kb_solve(sp_kb_full{G.data(), (int)C}, (int)C, (int)K, seed, rep, labels.data(), work.data());
        }
        printf("R %d", it);
        for (int a = 0; a < C; a++) printf(" %d", (int)labels[(size_t)a]);
        printf("\n");
    }
    int64_t n_draws = 0;
    if (!get(f, &n_draws)) return 3;
    for (int64_t i = 0; i < n_draws; i++) {
        uint64_t v[3];
        if (!get(f, v, 3)) return 3;
        printf("U %a\n", sp_kb_u(v[0], v[1], v[2]));
    }
    for (int K = 1; K <= 64; K++) printf("T %d %d\n", K, sp_kb_trials(K));
    fclose(f);
    return 0;
}
