// Host check of the ungapped prefilter of subphaser_amd/csrc/sp_domains.h (tests/test_domssv_host.py builds and runs it).
// Input file: records, each led by an int64 tag, until tag 0:
//   1  frame: int64 nres, M, then nres residue codes (bytes 0..21), M x 22 int32 emissions, M x 7 int32 transitions, int32
//      entry                                                                       -> int32 ssv (sp_dm_host_ssv_frame)
//   2  element: int64 n, M, then n base codes (bytes: 0..3, anything else invalid) and the tables as above
//                                                                                  -> 6 int32: the ssv of frames 0..5
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_domains.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return n == 0 || fread(out, sizeof(T), n, f) == n; }
template <typename T>
static bool put(FILE *f, const T *in, size_t n = 1) { return n == 0 || fwrite(in, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    long checks = 0;
    for (;;) {
        int64_t tag = 0;
        if (!get(f, &tag)) return 3;
        if (tag == 0) break;
        if (tag != 1 && tag != 2) return 4;
        int64_t n, M;
        if (!get(f, &n) || !get(f, &M)) return 3;
        if (n < 0 || n > SP_DM_MAXLEN || M < 1 || M > SP_DM_MAXM) return 4;
        std::vector<uint8_t> codes((size_t)n), res((size_t)(n / 3 + 1));
        std::vector<int32_t> emis((size_t)M * SP_DM_COLS), trans((size_t)M * 7), row((size_t)M + 1);
        int32_t entry;
        if (!get(f, codes.data(), codes.size()) || !get(f, emis.data(), emis.size()) || !get(f, trans.data(), trans.size()) || !get(f, &entry)) return 3;
        if (!sp_dm_tables_ok((int)M, emis.data(), trans.data(), entry)) return 6;
        if (tag == 1) {
            for (uint8_t c : codes)
                if (c >= SP_DM_COLS) return 4;
            const int32_t s = sp_dm_host_ssv_frame(codes.data(), (int32_t)n, (int)M, emis.data(), trans.data(), entry, row.data());
            if (!put(o, &s)) return 5;
        } else {
            int32_t out[6];
            for (int fr = 0; fr < 6; fr++) {
                sp_dm_host_translate(codes.data(), n, fr, res.data());
                out[fr] = sp_dm_host_ssv_frame(res.data(), sp_dm_nres(n, fr), (int)M, emis.data(), trans.data(), entry, row.data());
            }
            if (!put(o, out, 6)) return 5;
        }
        checks++;
    }
    fclose(f);
    if (fclose(o) != 0) return 5;
    printf("OK %ld\n", checks);
    return 0;
}
