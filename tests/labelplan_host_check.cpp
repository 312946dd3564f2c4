// Host check of subphaser_amd/csrc/sp_labelplan.h, the choice and sizing of the label table of sp_labels_set, against
// values worked out by hand from the rules (compiled and run by tests/test_labelplan_host.py; exit status 0 and
// "OK <checks>" on success).
//
// The rules.  per-k-mer = more than 7 subgenomes or SP_MAP_ENGINE=1.  bb starts at 8 and grows while bb < 30 and
// 2^bb < factor * max(n, 1) (factor: SP_CTAB_FACTOR, default 2); then it is raised to sb - 2 (k <= 15) or sb - 34
// (k > 15), sb = 2 (k - 3): the tag keeps that many bits of the mixed (k-3)-mer.  A bucket table needs pair keys,
// S <= 3, bb <= min(sb, 27) and SP_CTAB != 0; at k <= 15 also k >= 5 and either SP_CTAB=1 or a direct table of 4^(k-1)
// words that is larger than 64 MiB and no smaller than four bucket tables' worth (16 << bb words).  Buckets are 16 bytes
// (k <= 15) or 32 bytes (k > 15), the overflow table has the least power of two >= max(4096, n / 2) entries of 8 or 16
// bytes.  The hash table of k > 15 has the least power of two >= max(1024, (pairs ? 4 : 2) n + 16) entries, 1024 beside
// the quad table.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "sp_labelplan.h"

static unsigned long long n_checks = 0;
static int n_bad = 0;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        n_checks++;                                                                 \
        if (!(cond) && n_bad++ < 40) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    } while (0)

static const int64_t KiB = 1024, MiB = 1024 * 1024, GiB = 1024 * MiB;
static const sp_label_env UNSET = {false, -1, 2};

static sp_label_env env(bool per_kmer, int ctab, int64_t factor) {
    sp_label_env E = {per_kmer, ctab, factor};
    return E;
}

static sp_label_plan plan(int k, int64_t n, int S, const sp_label_env &E = UNSET) {
    return sp_label_plan_make(k, n, S, k <= 15 ? (int64_t)1 << (2 * k - 1) : 0, E);
}

static bool same(const sp_label_plan &a, const sp_label_plan &b) {
    return a.kind == b.kind && a.bb == b.bb && a.bucket_bytes == b.bucket_bytes && a.ovf_n == b.ovf_n &&
           a.ovf_bytes == b.ovf_bytes && a.cap == b.cap && a.entries == b.entries;
}

static void no_buckets(const sp_label_plan &P) {
    CHECK(P.bb == 0 && P.bucket_bytes == 0 && P.ovf_n == 0 && P.ovf_bytes == 0);
}

static void dense() {
    sp_label_plan P = plan(15, 2000000, 3);       // 2^22 = 4 194 304 >= 4 000 000; 2^20 >= 1 000 000
    CHECK(P.kind == SP_LABELS_COMPACT && P.bb == 22 && P.bucket_bytes == 64 * MiB);
    CHECK(P.ovf_n == (1 << 20) && P.ovf_bytes == 8 * MiB && P.entries == (int64_t)1 << 28 && P.cap == 0);
    P = plan(15, 100000, 3);                      // 2^18 >= 200 000, raised to sb - 2 = 22; 65 536 >= 50 000
    CHECK(P.kind == SP_LABELS_COMPACT && P.bb == 22 && P.ovf_n == 65536 && P.ovf_bytes == 512 * KiB);
    P = plan(14, 100000, 3);                      // sb = 22: 20; the direct table is 256 MiB, four bucket tables 256 MiB
    CHECK(P.kind == SP_LABELS_COMPACT && P.bb == 20 && P.bucket_bytes == 16 * MiB);
    P = plan(13, 100000, 3);                      // the direct table is 64 MiB, which is not > 64 MiB
    CHECK(P.kind == SP_LABELS_DIRECT && P.entries == (int64_t)1 << 24);
    no_buckets(P);
    P = plan(13, 100000, 3, env(false, 1, 2));    // sb = 20: bb = 18 needs no raise
    CHECK(P.kind == SP_LABELS_COMPACT && P.bb == 18 && P.bucket_bytes == 4 * MiB);
    CHECK(plan(9, 100000, 3, env(false, 1, 2)).kind == SP_LABELS_DIRECT);      // bb 18 > sb 12
    CHECK(plan(4, 10, 3, env(false, 1, 2)).kind == SP_LABELS_DIRECT);          // k < 5
    CHECK(plan(4, 10, 3, env(false, 1, 2)).entries == 64);
    CHECK(plan(15, 10000000, 3).kind == SP_LABELS_DIRECT);                     // bb 25 > sb 24
    P = plan(15, 2000000, 3, env(false, 0, 2));
    CHECK(P.kind == SP_LABELS_DIRECT && P.entries * 4 == GiB);
    no_buckets(P);
    CHECK(plan(15, 2000000, 4).kind == SP_LABELS_DIRECT);                      // 2-bit label fields hold 3 subgenomes
    CHECK(plan(15, 2000000, 7).kind == SP_LABELS_DIRECT);
    CHECK(plan(15, 2000000, 8).kind == SP_LABELS_LABEL_BYTES);
    no_buckets(plan(15, 2000000, 8));
    CHECK(plan(15, 2000000, 3, env(true, -1, 2)).kind == SP_LABELS_LABEL_BYTES);
    CHECK(plan(15, 2000000, 3, env(true, 1, 2)).kind == SP_LABELS_LABEL_BYTES);
    CHECK(plan(15, 4000000, 3, env(false, -1, 1)).bb == 22);                   // 2^22 >= 4 000 000
    CHECK(plan(15, 4000000, 3, env(false, -1, 2)).bb == 23);                   // 2^23 >= 8 000 000
    CHECK(plan(15, 0, 3).kind == SP_LABELS_COMPACT && plan(15, 0, 3).bb == 22 && plan(15, 0, 3).ovf_n == 4096);
}

static void sparse() {
    sp_label_plan P = plan(17, 2000000, 3);
    CHECK(P.kind == SP_LABELS_QUAD && P.bb == 22 && P.bucket_bytes == 128 * MiB);
    CHECK(P.ovf_n == (1 << 20) && P.ovf_bytes == 16 * MiB && P.cap == 1024 && P.entries == 0);
    P = plan(21, 1000, 2);                        // 2^11 >= 2000
    CHECK(P.kind == SP_LABELS_QUAD && P.bb == 11 && P.bucket_bytes == 64 * KiB && P.ovf_n == 4096 && P.ovf_bytes == 64 * KiB);
    CHECK(plan(17, 0, 3).kind == SP_LABELS_QUAD && plan(17, 0, 3).bb == 8);
    // k = 32 / 31: bb is raised to sb - 34 whatever n is, 512 MiB / 128 MiB for a thousand labels.  Today's values --
    // the quad-table finding of ADVICE.md proposes the hash table there; that change has one expectation to update here.
    P = plan(32, 1000, 3);
    CHECK(P.kind == SP_LABELS_QUAD && P.bb == 24 && P.bucket_bytes == 512 * MiB);
    P = plan(31, 1000, 3);
    CHECK(P.kind == SP_LABELS_QUAD && P.bb == 22 && P.bucket_bytes == 128 * MiB);
    P = plan(16, 33554433, 3);                    // 2^26 < 67 108 866: bb 27 > sb 26; 4 n + 16 = 134 217 748 > 2^27
    CHECK(P.kind == SP_LABELS_PAIR_HASH && P.cap == (int64_t)1 << 28);
    no_buckets(P);
    P = plan(17, 1000, 5);                        // 4016
    CHECK(P.kind == SP_LABELS_PAIR_HASH && P.cap == 4096);
    CHECK(plan(17, 1000, 7).kind == SP_LABELS_PAIR_HASH);
    P = plan(17, 1000, 9);                        // 2016
    CHECK(P.kind == SP_LABELS_KMER_HASH && P.cap == 2048);
    no_buckets(P);
    CHECK(plan(17, 1000, 3, env(true, -1, 2)).kind == SP_LABELS_KMER_HASH);
    CHECK(plan(17, 0, 9).cap == 1024);
    P = plan(17, 2000000, 3, env(false, 0, 2));   // 8 000 016 <= 2^23 = 8 388 608
    CHECK(P.kind == SP_LABELS_PAIR_HASH && P.cap == 1 << 23);
    CHECK(same(plan(17, 2000000, 3, env(false, 1, 2)), plan(17, 2000000, 3)));      // SP_CTAB=1 forces nothing at k > 15
    CHECK(same(plan(16, 33554433, 3, env(false, 1, 2)), plan(16, 33554433, 3)));
    CHECK(plan(17, 4000000, 3, env(false, -1, 1)).bb == 22 && plan(17, 4000000, 3).bb == 23);
}

static void fallback() {
    sp_label_plan P = sp_label_plan_fallback(plan(17, 2000000, 3), 2000000);
    CHECK(P.kind == SP_LABELS_PAIR_HASH && P.cap == 1 << 23);
    no_buckets(P);
    CHECK(same(P, plan(17, 2000000, 3, env(false, 0, 2))));
    P = sp_label_plan_fallback(plan(17, 0, 3), 0);
    CHECK(P.kind == SP_LABELS_PAIR_HASH && P.cap == 1024);
    P = sp_label_plan_fallback(plan(15, 2000000, 3), 2000000);
    CHECK(P.kind == SP_LABELS_DIRECT && P.entries == (int64_t)1 << 28);
    no_buckets(P);
    CHECK(same(P, plan(15, 2000000, 3, env(false, 0, 2))));
}

static bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

static void sweep() {
    const int64_t ns[] = {0, 1, 2, 127, 128, 129, 1000, 8191, 8192, 8193, 100000, 2000000, 33554433, 100000000};
    const int Ss[] = {1, 2, 3, 4, 7, 8, 126};
    const sp_label_env Es[] = {UNSET, env(false, 0, 2), env(false, 1, 2), env(true, -1, 2), env(false, -1, 1), env(false, 1, 7)};
    for (int k = 1; k <= 32; k++)
        for (int64_t n : ns)
            for (int S : Ss)
                for (const sp_label_env &E : Es) {
                    const sp_label_plan P = plan(k, n, S, E);
                    const int sb = 2 * (k - 3);
                    const bool dense_kind = P.kind == SP_LABELS_DIRECT || P.kind == SP_LABELS_COMPACT || P.kind == SP_LABELS_LABEL_BYTES;
                    CHECK(dense_kind == (k <= 15));
                    CHECK((P.kind == SP_LABELS_LABEL_BYTES || P.kind == SP_LABELS_KMER_HASH) == (S > 7 || E.per_kmer));
                    if (k <= 15) CHECK(P.entries == (int64_t)1 << (2 * (k - 1)) && P.cap == 0);
                    else CHECK(pow2(P.cap) && P.cap >= 1024 && P.entries == 0);
                    if (P.kind == SP_LABELS_PAIR_HASH) CHECK(P.cap >= 4 * n + 16 && (P.cap == 1024 || P.cap / 2 < 4 * n + 16));
                    if (P.kind == SP_LABELS_KMER_HASH) CHECK(P.cap >= 2 * n + 16 && (P.cap == 1024 || P.cap / 2 < 2 * n + 16));
                    if (P.kind == SP_LABELS_COMPACT || P.kind == SP_LABELS_QUAD) {
                        CHECK(S <= 3 && E.ctab != 0);
                        CHECK(P.bb >= 1 && P.bb <= 27 && P.bb <= sb);
                        CHECK(((int64_t)1 << P.bb) >= E.factor * n);
                        CHECK(pow2(P.ovf_n) && P.ovf_n >= 4096 && P.ovf_n >= n / 2 && (P.ovf_n == 4096 || P.ovf_n / 2 < n / 2));
                        // the tag holds the bits of the mixed (k-3)-mer that the bucket number does not
                        if (P.kind == SP_LABELS_COMPACT) CHECK(sb - P.bb <= MAP_CT_MAX_TAG_BITS && k >= 5);
                        else CHECK(sb - P.bb <= SQ_TAG_BITS - 5);
                        CHECK(P.bucket_bytes == ((int64_t)(k <= 15 ? 16 : 32) << P.bb));
                        CHECK(P.ovf_bytes == P.ovf_n * (k <= 15 ? 8 : 16));
                        const sp_label_plan F = sp_label_plan_fallback(P, n);
                        CHECK(same(F, plan(k, n, S, env(E.per_kmer, 0, E.factor))));
                    } else {
                        no_buckets(P);
                    }
                }
}

// the switches as the process environment gives them
static void environment() {
    unsetenv("SP_MAP_ENGINE");
    unsetenv("SP_CTAB");
    unsetenv("SP_CTAB_FACTOR");
    sp_label_env E = sp_label_env_read();
    CHECK(!E.per_kmer && E.ctab == -1 && E.factor == 2);
    setenv("SP_MAP_ENGINE", "1", 1);
    setenv("SP_CTAB", "0", 1);
    setenv("SP_CTAB_FACTOR", "1", 1);
    E = sp_label_env_read();
    CHECK(E.per_kmer && E.ctab == 0 && E.factor == 1);
    setenv("SP_MAP_ENGINE", "0", 1);
    setenv("SP_CTAB", "1", 1);
    setenv("SP_CTAB_FACTOR", "-3", 1);
    E = sp_label_env_read();
    CHECK(!E.per_kmer && E.ctab == 1 && E.factor == 2);
    setenv("SP_CTAB", "yes", 1);
    setenv("SP_CTAB_FACTOR", "", 1);
    E = sp_label_env_read();
    CHECK(E.ctab == -1 && E.factor == 2);
}

int main() {
    dense();
    sparse();
    fallback();
    sweep();
    environment();
    if (n_bad) {
        std::printf("%d of %llu checks FAILED\n", n_bad, n_checks);
        return 1;
    }
    std::printf("OK %llu\n", n_checks);
    return 0;
}
