// Stand-alone host check of subphaser_amd/csrc/sp_ltrdetect.h: the header's word, partner, seed and extension functions
// over whole sequences, as the device strings them together (elements sorted by word and position, one walk per element).
// input, per case:  L X dmin dmax maxlen len <len digits 0..4>
// output, per case: "C valid word_sum partner_pairs seeds", then "p q p0 n d" per seed, ascending (p, q)
// usage: ltrdetect_host_check <cases> <answers>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sp_ltrdetect.h"

struct Bases {
    const std::string *s;
    int operator()(int64_t g) const {
        if (g < 0 || g >= (int64_t)s->size()) abort();      // the header never looks outside the chromosome
        return (*s)[(size_t)g] - '0';
    }
};

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    long long L, X, dmin, dmax, maxlen, len;
    long checks = 0;
    while (fscanf(in, "%lld %lld %lld %lld %lld %lld", &L, &X, &dmin, &dmax, &maxlen, &len) == 6) {
        if (sp_ld_check((int)L, (int)X, dmin, dmax, maxlen) != 0 || len < 0 || len >= (1LL << SP_LD_POS_BITS)) return 3;
        std::string s((size_t)len, '4');
        for (long long i = 0; i < len; i++) {
            int c = fgetc(in);
            while (c == ' ' || c == '\n') c = fgetc(in);
            if (c < '0' || c > '4') return 3;
            s[(size_t)i] = (char)c;
        }
        const Bases B{&s};
        std::vector<unsigned long long> keys;
        unsigned long long wsum = 0;
        for (int64_t p = 0; p < len; p++) {
            uint64_t w;
            if (!sp_ld_word(B, len, p, (int)L, &w)) continue;
            wsum += w;
            keys.push_back(sp_ld_key(w, (uint32_t)p));
        }
        std::sort(keys.begin(), keys.end());
        long long pairs = 0;
        std::vector<std::vector<long long>> seeds;
        for (int64_t i = 0; i < (int64_t)keys.size(); i++) {
            uint32_t part[SP_LD_FANOUT];
            const int np = sp_ld_partners(keys.data(), (int64_t)keys.size(), i, dmin, dmax, part);
            pairs += np;
            const int64_t p = (int64_t)(keys[(size_t)i] & SP_LD_POS_MASK);
            for (int t = 0; t < np; t++) {
                const int64_t q = part[t];
                if (!sp_ld_is_seed(B, p, q)) continue;
                int64_t p0;
                int32_t n, p0b, nb, db;
                sp_ld_extend(B, len, p, q, (int)L, (int)X, maxlen, &p0, &n);
                sp_ld_hsp_unpack(sp_ld_hsp_pack(p0, n, q - p), &p0b, &nb, &db);
                if (p0b != p0 || nb != n || db != q - p) return 4;      // the HSP word holds the HSP
                seeds.push_back({p, q, p0, n, q - p});
            }
        }
        std::sort(seeds.begin(), seeds.end());
        fprintf(out, "C %zu %llu %lld %zu\n", keys.size(), wsum, pairs, seeds.size());
        for (const auto &r : seeds) fprintf(out, "%lld %lld %lld %lld %lld\n", r[0], r[1], r[2], r[3], r[4]);
        checks++;
    }
    fclose(in);
    if (fclose(out) != 0) return 5;
    printf("OK %ld\n", checks);
    return 0;
}
