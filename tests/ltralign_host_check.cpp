// Stand-alone host check of subphaser_amd/csrc/sp_ltralign.h: aligns pairs with the header's cell update, row by row over
// two rolling rows of the band (the device sweeps anti-diagonals: another order over the same cells).
// input, per pair:  w la lb <la digits 0..4> <lb digits 0..4>
// output, per pair: score match mismatch gap skip flags
// usage: ltralign_host_check <pairs> <answers>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "sp_ltralign.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    long long w, la, lb;
    long checks = 0;
    std::vector<char> buf(2 * SP_LA_MAXLEN + 16);
    while (fscanf(in, "%lld %lld %lld", &w, &la, &lb) == 3) {
        if (w < 0 || la < 1 || lb < 1 || la > 2 * SP_LA_MAXLEN || lb > 2 * SP_LA_MAXLEN) return 3;
        std::string a, b;
        if (fscanf(in, "%16399s", buf.data()) != 1) return 3;
        a = buf.data();
        if (fscanf(in, "%16399s", buf.data()) != 1) return 3;
        b = buf.data();
        if ((long long)a.size() != la || (long long)b.size() != lb) return 3;
        int32_t res[6] = {0, 0, 0, 0, 0, 0};
        const int flag = sp_la_check(la, lb, w);
        if (flag) {
            res[5] = flag;
        } else {
            const int64_t dlo = sp_la_dlo(la, lb, w), dhi = sp_la_dhi(la, lb, w), width = dhi - dlo + 1;
            if (dlo > 0 || dhi < 0 || lb - la < dlo || lb - la > dhi || width > SP_LA_MAXBAND) return 4;      // both corners inside
            std::vector<sp_la_cell> prev((size_t)width, sp_la_none()), row((size_t)width, sp_la_none());
            for (int64_t i = 0; i <= la; i++) {
                for (int64_t d = dlo; d <= dhi; d++) {
                    const int64_t j = i + d, r = d - dlo;
                    row[(size_t)r] = sp_la_none();
                    if (j < 0 || j > lb) continue;
                    if (i == 0 && j == 0) {
                        row[(size_t)r] = sp_la_cell{0, 0};
                        continue;
                    }
                    const sp_la_cell diag = (i > 0 && j > 0) ? prev[(size_t)r] : sp_la_none();
                    const sp_la_cell up = (i > 0 && d < dhi) ? prev[(size_t)r + 1] : sp_la_none();
                    const sp_la_cell left = (j > 0 && d > dlo) ? row[(size_t)r - 1] : sp_la_none();
                    const unsigned x = i > 0 ? (unsigned)(a[(size_t)i - 1] - '0') : 0u, y = j > 0 ? (unsigned)(b[(size_t)j - 1] - '0') : 0u;
                    row[(size_t)r] = sp_la_update(diag, up, left, x, y, d, dlo, dhi, w);
                    if (row[(size_t)r].score <= SP_LA_NEG / 2) return 4;      // a cell inside always has a predecessor inside
                }
                prev.swap(row);
            }
            sp_la_result(prev[(size_t)(lb - la - dlo)], res);
        }
        fprintf(out, "%d %d %d %d %d %d\n", res[0], res[1], res[2], res[3], res[4], res[5]);
        checks++;
    }
    fclose(in);
    if (fclose(out) != 0) return 5;
    printf("OK %ld\n", checks);
    return 0;
}
