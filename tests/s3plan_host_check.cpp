// Host check of subphaser_amd/csrc/sp_s3plan.h: the plan of the k = 16..32 count chain at every k against hand-worked
// values, s3_split_bits at the sizes the test chromosomes of tests/s3_cases.py use, and every threshold printed as a
// `NAME value` line for tests/test_s3plan_host.py to compare with the literals of tests/s3_cases.py.
#include <cstdio>
#include <cstdlib>

#include "sp_s3plan.h"

static int checks = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        checks++;                                                     \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    // k, B2, R1, R2, wide1, wide2: T = 2k bits, 10 go at level 1, 8 (k <= 17) or 9 at level 2
    static const int want[17][6] = {
        {16, 8, 22, 14, 0, 0}, {17, 8, 24, 16, 0, 0}, {18, 9, 26, 17, 0, 0}, {19, 9, 28, 19, 0, 0}, {20, 9, 30, 21, 0, 0},
        {21, 9, 32, 23, 0, 0}, {22, 9, 34, 25, 1, 0}, {23, 9, 36, 27, 1, 0}, {24, 9, 38, 29, 1, 0}, {25, 9, 40, 31, 1, 0},
        {26, 9, 42, 33, 1, 1}, {27, 9, 44, 35, 1, 1}, {28, 9, 46, 37, 1, 1}, {29, 9, 48, 39, 1, 1}, {30, 9, 50, 41, 1, 1},
        {31, 9, 52, 43, 1, 1}, {32, 9, 54, 45, 1, 1}};
    for (int i = 0; i < 17; i++) {
        const int k = want[i][0];
        CHECK(k == 16 + i);
        const s3_plan p = s3_make_plan(k);
        CHECK(p.T == 2 * k);
        CHECK(p.B1 == 10);
        CHECK(p.B2 == want[i][1]);
        CHECK(p.R1 == want[i][2]);
        CHECK(p.R2 == want[i][3]);
        CHECK(p.F1 == 1024);
        CHECK(p.F2 == (k <= 17 ? 256 : 512));
        CHECK((int)p.wide1 == want[i][4]);
        CHECK((int)p.wide2 == want[i][5]);
        // the all-ones EMPTY marker of the hash tables (32 or 64 one bits) is never a residual
        CHECK(p.R2 != 32 && p.R2 != 64 && p.R2 < 64);
        // the bitmap finish takes exactly k = 16, 17
        CHECK((p.R2 <= S3_BM_MAXBITS) == (k <= 17));
        // a packed 32-bit record: residual and 14-bit rank do not meet (bits 0..41 and 48..61)
        if (!p.wide1) CHECK(p.T <= 42);
    }
    CHECK(s3_make_plan(21).R1 == 32);
    CHECK(s3_make_plan(25).R2 == 31);
    CHECK(s3_make_plan(26).R2 == 33);
    CHECK(s3_make_plan(32).R2 == 45);

    // s3_split_bits: the smallest sb <= 8 with (n >> sb) <= 1024, at least 1; worked by hand:
    //   2049 >> 1 = 1024; 3074 >> 1 = 1537, >> 2 = 768; 4097 >> 1 = 2048, >> 2 = 1024; 6000 >> 2 = 1500, >> 3 = 750;
    //   65536 >> 5 = 2048, >> 6 = 1024; 2^19 >> 8 = 2048 and 2^22 + 1: the cap of 8
    static const unsigned ns[7] = {2049u, 3074u, 4097u, 6000u, 65536u, 1u << 19, (1u << 22) + 1u};
    static const int sbs[7] = {1, 2, 2, 3, 6, 8, 8};
    static const int r2s[5] = {14, 16, 17, 23, 45};
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 5; j++) CHECK(s3_split_bits(ns[i], r2s[j]) == sbs[i]);
    CHECK(s3_split_bits(65536u, 5) == 5);      // never more bits than the residual has
    CHECK(s3_split_bits(2048u + 1u, 0) == 0);
    CHECK(S3_SPLIT_BITS == 8 && S3_SORT_CAP == 2048);

#define SHOW(name) printf("%s %lld\n", #name, (long long)(name))
    SHOW(S3_P1_UNIT);
    SHOW(S3_P1T32);
    SHOW(S3_P1T64);
    SHOW(S3_P2_THREADS);
    SHOW(S3_P2_PER);
    SHOW(S3_P2_KEYS);
    SHOW(S3_SORT_THREADS);
    SHOW(S3_SORT_PER);
    SHOW(S3_SORT_CAP);
    SHOW(S3_SMALL_PER);
    SHOW(S3_SMALL_CAP);
    SHOW(S3_SPLIT_BITS);
    SHOW(S3_DIRECT_BITS);
    SHOW(S3_HASH_SLOTS);
    SHOW(S3_HASH_MAX);
    SHOW(S3H_COUNTERS);
    SHOW(S3H_SLOTS);
    SHOW(S3H_CAP);
    SHOW(S3H_PER);
    SHOW(S3_BM_MAXBITS);
    SHOW(S3_BM_CAP);
    SHOW(S3_BM_NMAX);
    SHOW(S3_BM_PER);
    SHOW(S3B_SPREAD);
    SHOW(S3B_KCAP);
    SHOW(S3B_MAXBIG);
    SHOW(S3_SAMPLE_MIN_LEN);
    printf("OK %d\n", checks);
    return 0;
}
