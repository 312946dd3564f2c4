// Host check of subphaser_amd/csrc/sp_domalign.h (tests/test_domalign_host.py builds and runs it).
// Input file: records, each led by an int64 tag, until tag 0:
//   1  item: int64 n (bases), frame, i0, i1, M, then n base codes (bytes: 0..3, anything else invalid), M x 22 int32
//      emissions, M x 7 int32 transitions, int32 entry            -> 5 int32 (hit), M int32 (col), i1 - i0 + 1 bytes (residues)
//   2  rows: int64 N, C, then N x C bytes                          -> N x N int32 same, N x N int32 both (eight bytes a step)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sp_domalign.h"
#include "sp_swar.h"

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
        if (tag == 1) {
            int64_t n, fr, i0, i1, M;
            if (!get(f, &n) || !get(f, &fr) || !get(f, &i0) || !get(f, &i1) || !get(f, &M)) return 3;
            if (n < 0 || n > SP_DM_MAXLEN || M < 1 || M > SP_DM_MAXM || fr < 0 || fr > 5) return 4;
            const int32_t nres = sp_dm_nres(n, (int)fr);
            if (i0 < 0 || i0 > i1 || i1 >= nres || i1 - i0 + 1 > SP_DA_MAXWIN) return 4;
            const int32_t nwin = (int32_t)(i1 - i0 + 1);
            std::vector<uint8_t> codes((size_t)n), res((size_t)nres + 1), plane((size_t)nwin * SP_DA_PITCH(M));
            std::vector<int32_t> emis((size_t)M * SP_DM_COLS), trans((size_t)M * 7), col((size_t)M);
            std::vector<int64_t> row((size_t)(6 * (M + 1)));
            int32_t entry, hit[5];
            if (!get(f, codes.data(), codes.size()) || !get(f, emis.data(), emis.size()) || !get(f, trans.data(), trans.size()) || !get(f, &entry)) return 3;
            sp_dm_host_translate(codes.data(), n, (int)fr, res.data());
            sp_da_host_item(res.data() + i0, (int32_t)i0, nwin, (int)M, emis.data(), trans.data(), entry, row.data(), plane.data(), hit, col.data());
            if (!put(o, hit, 5) || !put(o, col.data(), col.size()) || !put(o, res.data() + i0, (size_t)nwin)) return 5;
        } else if (tag == 2) {
            int64_t N, C;
            if (!get(f, &N) || !get(f, &C)) return 3;
            if (N < 1 || N > 4096 || C < 1 || C > 8192) return 4;
            const size_t Cp = ((size_t)C + 7) & ~(size_t)7;
            std::vector<uint8_t> rows((size_t)N * Cp, (uint8_t)SP_DA_GAP);
            for (int64_t i = 0; i < N; i++)
                if (!get(f, rows.data() + (size_t)i * Cp, (size_t)C)) return 3;
            std::vector<int32_t> same((size_t)(N * N)), both((size_t)(N * N));
            for (int64_t a = 0; a < N; a++)
                for (int64_t b = 0; b < N; b++) {
                    uint32_t ns = 0, nb = 0;
                    for (size_t w = 0; w < Cp; w += 8) {
                        uint64_t x, y;
                        memcpy(&x, rows.data() + (size_t)a * Cp + w, 8);
                        memcpy(&y, rows.data() + (size_t)b * Cp + w, 8);
                        const uint64_t fl = sp_swar_lt20_bytes(x) & sp_swar_lt20_bytes(y);
                        nb += sp_swar_byte_count(fl);
                        ns += sp_swar_byte_count(fl & sp_swar_eq_bytes(x, y));
                    }
                    same[(size_t)(a * N + b)] = (int32_t)ns;
                    both[(size_t)(a * N + b)] = (int32_t)nb;
                }
            if (!put(o, same.data(), same.size()) || !put(o, both.data(), both.size())) return 5;
        } else
            return 4;
        checks++;
    }
    fclose(f);
    if (fclose(o) != 0) return 5;
    printf("OK %ld\n", checks);
    return 0;
}
