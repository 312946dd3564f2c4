// Stand-alone host check of subphaser_amd/csrc/sp_blocks.h: reads commands, one per line, and answers each with one line.
//   M key            -> mix(key)
//   S key s          -> 1 / 0: is the key sampled
//   C kb s bin       -> sp_bk_check
//   W len bin        -> number of windows
//   H mixed cap      -> home slot
//   V n (wb opp count) x n   -> win_b opp votes total of a window with these cells, by the packed maximum the device takes
// usage: blocks_host_check <commands> <answers>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sp_blocks.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char op;
    long checks = 0;
    while (fscanf(in, " %c", &op) == 1) {
        if (op == 'M') {
            unsigned long long key;
            if (fscanf(in, "%llu", &key) != 1) return 3;
            fprintf(out, "%llu\n", (unsigned long long)sp_bk_mix(key));
        } else if (op == 'S') {
            unsigned long long key;
            int s;
            if (fscanf(in, "%llu %d", &key, &s) != 2) return 3;
            const bool a = sp_bk_sampled(key, s), b = sp_bk_sampled_mix(sp_bk_mix(key), s);
            if (a != b) return 4;
            fprintf(out, "%d\n", a ? 1 : 0);
        } else if (op == 'C') {
            int kb, s;
            long long bin;
            if (fscanf(in, "%d %d %lld", &kb, &s, &bin) != 3) return 3;
            fprintf(out, "%d\n", sp_bk_check(kb, s, bin));
        } else if (op == 'W') {
            long long len, bin;
            if (fscanf(in, "%lld %lld", &len, &bin) != 2) return 3;
            fprintf(out, "%lld\n", (long long)sp_bk_nwin(len, bin));
        } else if (op == 'H') {
            unsigned long long mixed;
            unsigned cap;
            if (fscanf(in, "%llu %u", &mixed, &cap) != 2) return 3;
            const uint32_t h = sp_bk_home(mixed, cap);
            if (h >= cap) return 4;
            fprintf(out, "%u\n", h);
        } else if (op == 'V') {
            int n;
            if (fscanf(in, "%d", &n) != 1 || n < 0) return 3;
            std::vector<uint64_t> packed;
            long long total = 0;
            for (int i = 0; i < n; i++) {
                int wb, opp;
                unsigned count;
                if (fscanf(in, "%d %d %u", &wb, &opp, &count) != 3) return 3;
                const uint32_t cell = sp_bk_cell(wb, opp);
                const uint64_t v = sp_bk_vote_pack(count, cell);
                if (sp_bk_vote_count(v) != count || sp_bk_vote_wb(v) != wb || sp_bk_vote_opp(v) != opp) return 4;
                packed.push_back(v);
                total += count;
            }
            uint64_t best = 0;
            for (uint64_t v : packed) best = v > best ? v : best;
            int32_t win_b, votes, tot;
            uint8_t opp;
            sp_bk_vote_out(best, (int32_t)total, &win_b, &opp, &votes, &tot);
            fprintf(out, "%d %d %d %d\n", win_b, (int)opp, votes, tot);
        } else {
            return 3;
        }
        checks++;
    }
    fclose(in);
    if (fclose(out) != 0) return 5;
    printf("OK %ld\n", checks);
    return 0;
}
