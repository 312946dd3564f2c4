// Host check of subphaser_amd/csrc/sp_ttest.h (compiled and run by tests/test_ttest_host.py).
// Input file (native endianness): int64 nvec; per vector int64 n, double np_sum, n doubles; int64 npairs; npairs x (double
// df, double t).  Every vector goes through the streaming accumulator in blocks of 8 as a kernel would feed it and must
// give np_sum bit for bit; then "SUMS <checked> <mismatches>" and one "P <df> <t> <sp_tt_pvalue>" line per pair (%.17g).
// Exit status 0 when no sum differed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sp_ttest.h"

struct HostStack {
    double s[SP_TT_DEPTH];
    double &at(int d) { return s[d]; }
};

static double stream_sum(const std::vector<double> &a, int *depth) {
    const int64_t n = (int64_t)a.size();
    std::vector<uint8_t> prog((size_t)(n / 8) + 1, 0xff);
    *depth = sp_tt_program(n, prog.data());
    if (*depth > SP_TT_DEPTH) return -1.0;
    sp_tt_acc acc;
    HostStack st;
    sp_tt_begin(acc);
    for (int64_t b = 0; b < n / 8; b++) {
        double v[8];
        for (int j = 0; j < 8; j++) v[j] = a[(size_t)(b * 8 + j)];
        sp_tt_block(acc, v, prog[(size_t)b], st);
    }
    for (int64_t i = n - n % 8; i < n; i++) sp_tt_tail(acc, a[(size_t)i]);
    return sp_tt_finish(acc, st);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t nvec = 0;
    if (std::fread(&nvec, 8, 1, f) != 1) return 2;
    long long checked = 0, bad = 0;
    int deepest = 0;
    for (int64_t i = 0; i < nvec; i++) {
        int64_t n = 0;
        double want = 0;
        if (std::fread(&n, 8, 1, f) != 1 || std::fread(&want, 8, 1, f) != 1) return 2;
        std::vector<double> a((size_t)n);
        if (n && std::fread(a.data(), 8, (size_t)n, f) != (size_t)n) return 2;
        int depth = 0;
        const double got = stream_sum(a, &depth);
        if (depth > deepest) deepest = depth;
        if (std::memcmp(&got, &want, 8) != 0) {
            if (bad++ < 20) std::printf("MISMATCH n=%lld got=%.17g expected=%.17g depth=%d\n", (long long)n, got, want, depth);
        }
        checked++;
    }
    std::printf("DEPTH %d of %d\n", deepest, SP_TT_DEPTH);
    std::printf("SUMS %lld %lld\n", checked, bad);
    int64_t npairs = 0;
    if (std::fread(&npairs, 8, 1, f) != 1) return 2;
    for (int64_t i = 0; i < npairs; i++) {
        double dt[2];
        if (std::fread(dt, 8, 2, f) != 2) return 2;
        std::printf("P %.17g %.17g %.17g\n", dt[0], dt[1], sp_tt_pvalue(dt[0], dt[1]));
    }
    std::fclose(f);
    return bad ? 1 : 0;
}
