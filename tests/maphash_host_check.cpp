// maphash_host_check.cpp -- csrc/sp_maphash.h on the CPU (tests/test_maphash_host.py).
//   mix      map_ct_mix / map_ct_mix24 against the 32-bit form the table was built with; bijection for kb <= 16
//   probe K  no false negatives at k = K on both strands; the rolled walk's chain form == the generic map_bloom
//   quality K  false positives per pair and word-load variance / mean of the k <= 15 family against the round-6 family
// The reference functions (ref_*) are the round-6 functions, copied verbatim: never the code under test.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sp_maphash.h"

static long long n_checks = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        n_checks++;                                     \
        if (!(c)) {                                     \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            exit(1);                                    \
        }                                               \
    } while (0)

// ----------------------------------------------------------------- the round-6 functions (verbatim)
static uint32_t ref_ct_mix(uint32_t x, int kb) {
    const uint32_t m = kb >= 32 ? 0xFFFFFFFFu : ((1u << kb) - 1u);
    uint32_t h = (x * 0x9E3779B1u) & m;        // odd multiplier: a bijection of the kb-bit values
    h ^= h >> ((kb + 1) / 2);                  // xorshift by at least half the width: an involution-like bijection
    h = (h * 0x85EBCA6Bu) & m;
    h ^= h >> ((kb + 1) / 2);
    return h;
}
static uint32_t ref_core_hash(uint64_t t) {
    uint32_t x = (uint32_t)t ^ (uint32_t)(t >> 32);
    x *= 0x9E3779B1u;
    x ^= x >> 15;
    return x * 0x85EBCA6Bu;
}
static uint32_t ref_core_word(uint32_t hmin, int nbits) {
    const uint32_t n = ~hmin;
    const uint32_t sq = (uint32_t)(((unsigned long long)n * (unsigned long long)n) >> 32);
    return (~sq) >> (32 - (MAP_BLOOM_NBITS(nbits) - 5));
}
static uint32_t ref_bloom_bits3(uint64_t x64, uint32_t &h) {
    const uint32_t x = (uint32_t)x64 ^ (uint32_t)(x64 >> 32);
    h = x * 0x9E3779B1u;
    const uint32_t h2 = x * 0x85EBCA6Bu;
    return (1u << ((h >> 7) & 31u)) | (1u << ((h >> 2) & 31u)) | (1u << (h2 >> 27));
}
static map_bloom_probe ref_bloom(uint64_t x64, int k, int nbits) {
    map_bloom_probe p;
    uint32_t h;
    p.bits = ref_bloom_bits3(x64, h);
    if (!(nbits & MAP_BLOOM_CORE) || k < 5) {
        p.word = h >> (32 - (MAP_BLOOM_NBITS(nbits) - 5));
        return p;
    }
    const int cb = 2 * (k - 3);
    const uint64_t smask = (1ULL << cb) - 1ULL;
    const uint64_t a = x64 >> 4, b = x64 & smask;
    const uint64_t ar = sp_mh_revcomp(a, k - 3), br = sp_mh_revcomp(b, k - 3);
    const uint32_t ha = ref_core_hash(a < ar ? a : ar), hb = ref_core_hash(b < br ? b : br);
    p.word = ref_core_word(ha < hb ? ha : hb, nbits);
    return p;
}
// the sizing rule of sp_map_filter_build (MAP_BLOOM_MIN_BITS 12, MAP_BLOOM_MAX_BITS 25, MAP_FILL_MAX 0.40)
static const int MIN_BITS = 12, MAX_BITS = 25;
static const double FILL_MAX = 0.40;

static uint64_t rng_state = 0;
static uint64_t rnd() {      // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}
static std::vector<uint8_t> random_seq(size_t n) {
    std::vector<uint8_t> s(n);
    for (size_t i = 0; i < n; i += 32) {
        uint64_t r = rnd();
        for (size_t j = i; j < n && j < i + 32; j++, r >>= 2) s[j] = (uint8_t)(r & 3u);
    }
    return s;
}
static uint64_t mer_at(const std::vector<uint8_t> &s, size_t i, int len) {      // first base in the highest bits, as the keys have it
    uint64_t x = 0;
    for (int j = 0; j < len; j++) x = (x << 2) | s[i + j];
    return x;
}
static uint64_t canon(uint64_t x, int len) {
    const uint64_t r = sp_mh_revcomp(x, len);
    return x < r ? x : r;
}

// ----------------------------------------------------------------- (a)
static void check_mix() {
    for (int kb = 2; kb <= 16; kb++) {
        const uint32_t n = 1u << kb;
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t x = 0; x < n; x++) {
            const uint32_t h = map_ct_mix(x, kb);
            CHECK(h == ref_ct_mix(x, kb), "map_ct_mix(%u, %d) = %u, was %u", x, kb, h, ref_ct_mix(x, kb));
            CHECK(map_ct_mix24(x, kb) == h, "map_ct_mix24(%u, %d)", x, kb);
            CHECK(h < n && !seen[h], "map_ct_mix(., %d) is no bijection at %u", kb, x);
            seen[h] = 1;
        }
    }
    rng_state = 0x9E3779B97F4A7C15ULL;
    for (int kb = 17; kb <= 24; kb++)
        for (int i = 0; i < (1 << 20); i++) {
            const uint32_t x = (uint32_t)rnd() & ((1u << kb) - 1u);
            const uint32_t h = map_ct_mix(x, kb);
            CHECK(h == ref_ct_mix(x, kb), "map_ct_mix(%u, %d) = %u, was %u", x, kb, h, ref_ct_mix(x, kb));
            CHECK(map_ct_mix24(x, kb) == h, "map_ct_mix24(%u, %d)", x, kb);
        }
    // wider tables (none today) keep the 32-bit form
    for (int kb = 25; kb <= 32; kb++)
        for (int i = 0; i < 4096; i++) {
            const uint32_t x = (uint32_t)rnd() & (kb >= 32 ? 0xFFFFFFFFu : ((1u << kb) - 1u));
            CHECK(map_ct_mix(x, kb) == ref_ct_mix(x, kb), "map_ct_mix(%u, %d)", x, kb);
        }
}

// ----------------------------------------------------------------- (b)
static void check_probe(int k) {
    rng_state = 0xD1B54A32D192ED03ULL + (uint64_t)k;
    const int n_keys = 100000;
    const uint64_t kmask = (1ULL << (2 * k)) - 1ULL, m1mask = (1ULL << (2 * (k - 1))) - 1ULL;
    for (int mode = 0; mode < 2; mode++) {
        const int nbits = 18 | (mode ? MAP_BLOOM_CORE : 0);
        std::vector<uint32_t> bloom((size_t)1 << (18 - 5), 0u);
        std::vector<uint64_t> keys(n_keys);
        for (int i = 0; i < n_keys; i++) {
            const uint64_t o = rnd() & kmask;
            keys[i] = canon(o, k);
            // k4_pair_filter: prefix and suffix (k-1)-mer of the canonical key, each canonical
            const map_bloom_probe p = map_bloom(canon(keys[i] >> 2, k - 1), k, nbits), q = map_bloom(canon(keys[i] & m1mask, k - 1), k, nbits);
            CHECK(p.word < bloom.size() && q.word < bloom.size(), "word out of range at k = %d", k);
            CHECK(__builtin_popcount(p.bits) >= 1 && __builtin_popcount(p.bits) <= 3, "bits");
            bloom[p.word] |= p.bits;
            bloom[q.word] |= q.bits;
        }
        // a scan meets the k-mer on either strand: the pair's shared (k-1)-mer is the suffix of the k-mer at an even start,
        // the prefix of the one at an odd start, read as the strand has it and then made canonical
        for (int i = 0; i < n_keys; i++)
            for (int strand = 0; strand < 2; strand++) {
                const uint64_t o = strand ? sp_mh_revcomp(keys[i], k) : keys[i];
                const uint64_t xs[2] = {o >> 2, o & m1mask};
                for (int e = 0; e < 2; e++) {
                    const uint64_t f = xs[e], r = sp_mh_revcomp(f, k - 1);
                    const map_bloom_probe p = map_bloom(f < r ? f : r, k, nbits);
                    CHECK((bloom[p.word] & p.bits) == p.bits, "false negative: k = %d key %llx strand %d end %d", k, (unsigned long long)keys[i], strand, e);
                }
            }
    }
    // chain form (map_chain_start24 + map_quad_probes24, as map_unit_scan64 calls them) == generic form, on a sequence and on its reverse complement
    if (k >= 5) {
        const int nbits = 20 | MAP_BLOOM_CORE;
        const size_t n_quads = 25000;
        std::vector<uint8_t> s = random_seq(4 * n_quads + 64);
        for (int strand = 0; strand < 2; strand++) {
            if (strand) {
                std::reverse(s.begin(), s.end());
                for (auto &b : s) b = (uint8_t)(3 - b);
            }
            const uint32_t cmask = (1u << (2 * (k - 3))) - 1u;
            uint32_t h_carry = 0;
            for (size_t g = 0; g < n_quads; g++) {
                const size_t j = 4 * g;       // x1 = the (k-1)-mer at j + 1, x2 = at j + 3
                const uint64_t x1 = mer_at(s, j + 1, k - 1), x2 = mer_at(s, j + 3, k - 1);
                const uint64_t r1 = sp_mh_revcomp(x1, k - 1), r2 = sp_mh_revcomp(x2, k - 1);
                if (g % 16 == 0) h_carry = map_chain_start24((uint32_t)x1, (uint32_t)r1, cmask);      // a unit's first quad
                map_bloom_probe q1, q2;
                map_quad_probes24((uint32_t)x1, (uint32_t)r1, (uint32_t)x2, (uint32_t)r2, cmask, nbits, h_carry, q1, q2);
                const map_bloom_probe p1 = map_bloom(x1 < r1 ? x1 : r1, k, nbits), p2 = map_bloom(x2 < r2 ? x2 : r2, k, nbits);
                CHECK(p1.word == q1.word && p2.word == q2.word, "chain word != generic word: k = %d quad %zu strand %d", k, g, strand);
                CHECK(p1.bits == q1.bits && p2.bits == q2.bits, "chain bits != generic bits: k = %d quad %zu strand %d", k, g, strand);
            }
        }
    }
}

// ----------------------------------------------------------------- (c)
struct quality {
    int bits;
    double fill, fp, vmr;
    long long probes;
};
template <typename F>
static quality measure(const std::vector<uint64_t> &keys, const std::vector<uint64_t> &probes, int k, F &&bloom_of) {
    quality q;
    const long long n = (long long)keys.size();
    int bits = MIN_BITS;
    while (bits < MAX_BITS - 1 && ((long long)1 << bits) < 6 * n) bits++;
    std::vector<uint32_t> bloom, load;
    for (;;) {
        const size_t words = (size_t)1 << (bits - 5);
        bloom.assign(words, 0u);
        load.assign(words, 0u);
        for (uint64_t x : keys) {
            const map_bloom_probe p = bloom_of(x, k, bits | MAP_BLOOM_CORE);
            bloom[p.word] |= p.bits;
            load[p.word]++;
        }
        long long set = 0;
        for (uint32_t w : bloom) set += __builtin_popcount(w);
        q.fill = (double)set / (double)((long long)1 << bits);
        if (bits >= MAX_BITS || q.fill <= FILL_MAX) break;
        bits++;
    }
    q.bits = bits;
    double mean = (double)n / (double)load.size(), var = 0;
    for (uint32_t c : load) var += ((double)c - mean) * ((double)c - mean);
    q.vmr = var / (double)load.size() / mean;
    long long pass = 0;
    for (uint64_t x : probes) {
        const map_bloom_probe p = bloom_of(x, k, bits | MAP_BLOOM_CORE);
        pass += (bloom[p.word] & p.bits) == p.bits;
    }
    q.probes = (long long)probes.size();
    q.fp = (double)pass / (double)probes.size();
    return q;
}
// label set: the canonical (k-1)-mers of `n_rep` random "repeat" sequences of `rep_len` bases (what the k-mers of a repeat
// family leave in the filter: every (k-1)-mer of every copy); probes: the unlabelled (k-1)-mers of a random sequence, one
// per pair of starts
static void check_quality(int k, int n_rep, int rep_len) {
    rng_state = 0x2545F4914F6CDD1DULL ^ ((uint64_t)k << 32);
    std::vector<uint64_t> keys;
    for (int r = 0; r < n_rep; r++) {
        const std::vector<uint8_t> s = random_seq((size_t)rep_len + (size_t)(k - 2));
        for (int i = 0; i < rep_len; i++) keys.push_back(canon(mer_at(s, (size_t)i, k - 1), k - 1));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const size_t n_pairs = 1970000;
    const std::vector<uint8_t> g = random_seq(2 * n_pairs + (size_t)k);
    std::vector<uint64_t> probes;
    for (size_t i = 0; i < n_pairs; i++) {
        const uint64_t x = canon(mer_at(g, 2 * i + 1, k - 1), k - 1);
        if (!std::binary_search(keys.begin(), keys.end(), x)) probes.push_back(x);
    }
    const quality o = measure(keys, probes, k, ref_bloom), n = measure(keys, probes, k, map_bloom);
    printf("quality k = %d: %zu keys, %lld unlabelled probes\n", k, keys.size(), o.probes);
    printf("  round-6 family: 2^%d bits, fill %.4f, load var/mean %.4f, false positives per pair %.5f\n", o.bits, o.fill, o.vmr, o.fp);
    printf("  24-bit family:  2^%d bits, fill %.4f, load var/mean %.4f, false positives per pair %.5f\n", n.bits, n.fill, n.vmr, n.fp);
    CHECK(o.probes > 1000000, "too few unlabelled probes");
    if (k == 15) CHECK(o.bits == 24 && n.bits == 24, "the model's filter has 2^24 bits at k = 15");
    CHECK(n.bits == o.bits, "the families choose different sizes: 2^%d / 2^%d", o.bits, n.bits);
    CHECK(n.fp <= o.fp, "false positives per pair: %.5f > %.5f", n.fp, o.fp);
    CHECK(n.vmr <= 1.05 * o.vmr, "word load variance / mean: %.4f > 1.05 x %.4f", n.vmr, o.vmr);
}

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "";
    const int k = argc > 2 ? atoi(argv[2]) : 0;
    if (!strcmp(what, "mix")) check_mix();
    else if (!strcmp(what, "probe") && k >= 4 && k <= 15) check_probe(k);
    else if (!strcmp(what, "quality") && k == 15) check_quality(15, 36, 60000);
    // (k = 11: 36 x 4 kb label the same quarter of the 524 800 canonical 10-mers as 36 x 60 kb do of the 12-mers at k = 13)
    else if (!strcmp(what, "quality") && k == 13) check_quality(13, 36, 60000);
    else if (!strcmp(what, "quality") && k == 11) check_quality(11, 36, 4000);
    else {
        printf("usage: maphash_host_check mix | probe K | quality 15|13|11\n");
        return 2;
    }
    printf("OK %lld\n", n_checks);
    return 0;
}
