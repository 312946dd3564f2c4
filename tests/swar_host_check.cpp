// Host check of subphaser_amd/csrc/sp_swar.h against the per-slot definition of c2_count16's write-out
// (compiled and run by tests/test_swar_host.py; exit status 0 and "OK <cases>" on success).
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sp_swar.h"

static unsigned long long n_cases = 0;
static int n_bad = 0;

static void fail(const char *what, uint32_t lower, uint32_t w, uint32_t w2, unsigned long long got, unsigned long long exp) {
    if (n_bad++ < 20) std::printf("MISMATCH %s lower=%u w=%08x w2=%08x got=%llx expected=%llx\n", what, lower, w, w2, got, exp);
}

// one word against the slot-by-slot code (lower <= SP_SWAR_MAX_LOWER)
static void check_word(uint32_t lower, uint32_t w) {
    const uint32_t c[2] = {w & 0xffffu, w >> 16};
    uint32_t n = 0, s = 0, fexp = 0;
    for (int h = 0; h < 2; h++)
        if (c[h] >= lower) { n++; s += c[h]; fexp |= 0x8000u << (16 * h); }
    const uint32_t f = sp_swar_ge_flags(w, sp_swar_rep16(lower));
    if (f != fexp) fail("ge_flags", lower, w, 0, f, fexp);
    if (sp_swar_flag_count(f) != n) fail("flag_count", lower, w, 0, sp_swar_flag_count(f), n);
    if (sp_swar_flag_sum(w, f, 12345u) != 12345u + s) fail("flag_sum", lower, w, 0, sp_swar_flag_sum(w, f, 12345u), 12345u + s);
    n_cases++;
}
// two words: the table bytes and the "some counter >= 255" test
static void check_pair(uint32_t a, uint32_t b) {
    const uint32_t c[4] = {a & 0xffffu, a >> 16, b & 0xffffu, b >> 16};
    uint32_t bytes = 0, any = 0;
    for (int j = 0; j < 4; j++) {
        bytes |= (c[j] < 255u ? c[j] : 255u) << (8 * j);
        any |= c[j] >= 255u;
    }
    if (sp_swar_sat_bytes(a, b) != bytes) fail("sat_bytes", 0, a, b, sp_swar_sat_bytes(a, b), bytes);
    // every position of the pair among the four words, the others zero or small
    const uint32_t g[4][4] = {{a, b, 0, 0}, {0, 0, a, b}, {a, 3, 0x00fe00feu, b}, {0x00010002u, a, b, 0}};
    for (int t = 0; t < 4; t++) {
        const uint32_t got = sp_swar_any_ge255(g[t][0], g[t][1], g[t][2], g[t][3]) != 0u;
        if (got != any) fail("any_ge255", 0, a, b, got, any);
    }
    const uint32_t mn = sp_swar_min16(a, b), mx = sp_swar_max16(a, b);
    const uint32_t emn = (c[0] < c[2] ? c[0] : c[2]) | ((c[1] < c[3] ? c[1] : c[3]) << 16);
    const uint32_t emx = (c[0] > c[2] ? c[0] : c[2]) | ((c[1] > c[3] ? c[1] : c[3]) << 16);
    if (mn != emn) fail("min16", 0, a, b, mn, emn);
    if (mx != emx) fail("max16", 0, a, b, mx, emx);
    n_cases++;
}

int main() {
    const uint32_t lowers[] = {1, 2, 3, 254, 255, 256, 0x7FFF, 0x8000, 0x8001, 70000};
    for (uint32_t lower : lowers) {
        // the kernel's rule: larger values of `lower` go through the per-slot code, which is the definition itself
        const bool swar = lower <= SP_SWAR_MAX_LOWER;
        if (swar != (lower <= 0x8000u)) fail("SP_SWAR_MAX_LOWER", lower, 0, 0, swar, lower <= 0x8000u);
        if (!swar) continue;
        std::vector<uint32_t> vals = {0, 1, lower - 1, lower, lower + 1, 254, 255, 256, 0x7FFF, 0x8000, 0xFFFF};
        for (uint32_t &v : vals) v &= 0xffffu;
        for (uint32_t lo : vals)
            for (uint32_t hi : vals) check_word(lower, lo | (hi << 16));
        // all 2^16 values of one half against a fixed other half (several of them)
        for (uint32_t fixed : vals)
            for (uint32_t x = 0; x < 0x10000u; x++) {
                check_word(lower, x | (fixed << 16));
                check_word(lower, fixed | (x << 16));
            }
    }
    {
        const uint32_t vals[] = {0, 1, 2, 253, 254, 255, 256, 257, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF};
        for (uint32_t a0 : vals)
            for (uint32_t a1 : vals)
                for (uint32_t b0 : vals)
                    for (uint32_t b1 : vals) check_pair(a0 | (a1 << 16), b0 | (b1 << 16));
        for (uint32_t x = 0; x < 0x10000u; x++) {
            check_pair(x | (7u << 16), 0x00030004u);
            check_pair(0x00fe0001u, 9u | (x << 16));
        }
    }
    if (n_bad) {
        std::printf("FAILED: %d mismatches in %llu cases\n", n_bad, n_cases);
        return 1;
    }
    std::printf("OK %llu\n", n_cases);
    return 0;
}
