// sp_maphash.h -- the hash functions of the map stage: which word and which three bits of the pair filter a (k-1)-mer
// owns (sp_map.h: blocked Bloom filter, core addressing), and the bijective mix behind the compact pair table's buckets.
//
// Two families, chosen by k alone (build and probe always agree):
//   k <= 15  ("24"): every input fits 24 bits -- a core is a (k-3)-mer (<= 24 bits) and so is the table's t -- so every product
//            is a 24 x 24 one.  On gfx950 v_mul_u32_u24 issues no faster than v_mul_lo_u32 (tools/ubench_imul.hip: every
//            integer multiply takes 1.78 adds), but a 24 x 24 product shifted right by 16 and a multiply-add are ONE
//            instruction each, the three filter bits come from the two core hashes the walk has anyway, and the family has
//            a quarter fewer false positives than the one it replaces (profiles/map_hash_notes.md).  The walk of k <= 15
//            (map_unit_scan64) calls these directly: no choice per quad.
//   k >  15: the functions the filter has had since round 6, bit for bit (64-bit keys do not fit 24-bit multiplies).
// Everything here is plain integer arithmetic, __host__ __device__, so that tests/test_maphash_host.py checks it with the
// host compiler alone: new table mix == old table mix, no false negatives, chain form == generic form, filter quality.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_MH_HD __host__ __device__ __forceinline__
#else
#define SP_MH_HD static inline
#endif

#define MAP_BLOOM_CORE 0x100          // flag in the `nbits` argument of everything below (ctx->bloom_bits carries it)
#define MAP_BLOOM_NBITS(nb) ((nb) & 0xFF)
#define MAP_HASH24_MAX_K 15           // largest k of the 24-bit family

struct map_bloom_probe {
    uint32_t word, bits;
};

// low 32 bits of the product of the low 24 bits of a and b (the masks are what makes the compiler pick v_mul_u32_u24)
SP_MH_HD uint32_t sp_mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
// bits 16..47 of that 48-bit product (v_mul_hi_u32_u24, v_mul_u32_u24, v_alignbit_b32)
SP_MH_HD uint32_t sp_mul24_shr16(uint32_t a, uint32_t b) {
    return (uint32_t)(((unsigned long long)(a & 0xFFFFFFu) * (unsigned long long)(b & 0xFFFFFFu)) >> 16);
}
SP_MH_HD uint64_t sp_mh_revcomp(uint64_t x, int k) {       // (sp_revcomp of sp_common.h, which is not host-clean)
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFULL) | ((x & 0x00FF00FF00FF00FFULL) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFULL) | ((x & 0x0000FFFF0000FFFFULL) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64 - 2 * k);
}

// ----------------------------------------------------------------- k > 15: the round-6 functions, unchanged
SP_MH_HD uint32_t map_core_hash(uint64_t t) {       // of a canonical (k-3)-mer; well mixed in its HIGH bits
    uint32_t x = (uint32_t)t ^ (uint32_t)(t >> 32);
    x *= 0x9E3779B1u;
    x ^= x >> 15;
    return x * 0x85EBCA6Bu;      // (multiply - xorshift - multiply: the scan computes one of these per pair)
}
SP_MH_HD uint32_t map_core_word(uint32_t hmin /* the smaller of a (k-1)-mer's two core hashes */, int nbits) {
    const uint32_t n = ~hmin;
    const uint32_t sq = (uint32_t)(((unsigned long long)n * (unsigned long long)n) >> 32);      // (1 - u)^2
    return (~sq) >> (32 - (MAP_BLOOM_NBITS(nbits) - 5));
}
SP_MH_HD uint32_t map_bloom_bits3(uint64_t x64, uint32_t &h) {      // the three bits of a canonical (k-1)-mer
    const uint32_t x = (uint32_t)x64 ^ (uint32_t)(x64 >> 32);
    h = x * 0x9E3779B1u;
    const uint32_t h2 = x * 0x85EBCA6Bu;
    return (1u << ((h >> 7) & 31u)) | (1u << ((h >> 2) & 31u)) | (1u << (h2 >> 27));
}

// ----------------------------------------------------------------- k <= 15: the same three on 24-bit multiplies
// multiply - xorshift - multiply again; the second product takes the 24 well mixed HIGH bits of the first and the low byte
// rides along in the addend (v_mad_u32_u24), so that two cores differ in their hashes as surely as before
SP_MH_HD uint32_t map_core_hash24(uint32_t t /* a canonical (k-3)-mer, < 2^24 */) {
    uint32_t x = sp_mul24(t, 0xB2AE35u);
    x ^= x >> 15;
    return sp_mul24(x >> 8, 0xEBCA6Bu) + (x & 0xFFu);
}
// WHICH core addresses the word: the one with the LARGER hash here (the round-6 family takes the smaller one and
// 1 - (1 - u)^2; this is its mirror image without the two complements).  The maximum of two uniform hashes has the
// distribution u^2, so u^2 is uniform: a 24 x 24 product of the hash's 24 high bits, its bits 16..47.
SP_MH_HD uint32_t map_core_word24(uint32_t hmax /* the larger of a (k-1)-mer's two core hashes */, int nbits) {
    const uint32_t n = hmax >> 8;
    return sp_mul24_shr16(n, n) >> (32 - (MAP_BLOOM_NBITS(nbits) - 5));
}
// The three bits of a (k-1)-mer inside its word, from the two core hashes it has anyway.  Their sum is the same on both
// strands (the cores swap places); the keys that share a word share ONE core and differ in the other.  All three bits
// come from the high 15 bits of one more product (the round-6 function takes two of its three from bits 2..11 of a product,
// which depend on six bases only: 0.076 false positives per pair on the model of tests/maphash_host_check.cpp, 0.058 here).
SP_MH_HD uint32_t map_bits3_of(uint32_t h) { return (1u << (h >> 27)) | (1u << ((h >> 22) & 31u)) | (1u << ((h >> 17) & 31u)); }
SP_MH_HD uint32_t map_core_bits3_24(uint32_t ha, uint32_t hb) { return map_bits3_of(sp_mul24((ha + hb) >> 8, 0x3779B1u)); }
// Without core addressing (k < 5: cores of fewer than two bases; the cross-check mode) word and bits come from the
// (k-1)-mer itself: up to 28 bits, the first two bases folded onto the last two, multiply - xorshift - multiply.
// h: well mixed in its high bits (it addresses the word).
SP_MH_HD uint32_t map_bloom_bits3_24(uint32_t x /* a canonical (k-1)-mer, < 2^28 */, uint32_t &h) {
    uint32_t y = sp_mul24(x ^ (x >> 24), 0xD4EB2Fu);
    y ^= y >> 15;
    h = sp_mul24(y >> 8, 0x3779B1u);
    return map_bits3_of(h);
}
// The rolled walk of k <= 15 computes the same from the windows it holds: x1 and x2 are a quad's two shared (k-1)-mers, read
// forward (xf) and reverse-complemented (xr), and their cores form the chain a - x1 - b - x2 - c.  Canonical core = the
// smaller of the forward reading and its reverse complement, which is the OTHER end of the reverse-complemented
// (k-1)-mer.  A quad's a IS the previous quad's c (the same bases): its hash is carried in h_carry, which
// map_chain_start24 primes for a unit's first quad.
SP_MH_HD uint32_t map_chain_start24(uint32_t xf1, uint32_t xr1, uint32_t cmask /* 4^(k-3) - 1 */) {
    const uint32_t ta_f = xf1 >> 4, ta_r = xr1 & cmask;
    return map_core_hash24(ta_f < ta_r ? ta_f : ta_r);
}
SP_MH_HD void map_quad_probes24(uint32_t xf1, uint32_t xr1, uint32_t xf2, uint32_t xr2, uint32_t cmask, int nbits, uint32_t &h_carry,
                                map_bloom_probe &p1, map_bloom_probe &p2) {
    const uint32_t tb_f = xf1 & cmask, tb_r = xr1 >> 4, tc_f = xf2 & cmask, tc_r = xr2 >> 4;
    const uint32_t ha = h_carry;
    const uint32_t hb = map_core_hash24(tb_f < tb_r ? tb_f : tb_r);
    const uint32_t hc = map_core_hash24(tc_f < tc_r ? tc_f : tc_r);
    h_carry = hc;
    p1.word = map_core_word24(ha > hb ? ha : hb, nbits);
    p2.word = map_core_word24(hb > hc ? hb : hc, nbits);
    p1.bits = map_core_bits3_24(ha, hb);
    p2.bits = map_core_bits3_24(hb, hc);
}

// word + bits of the CANONICAL (k-1)-mer x64 of a k-mer pair (generic form: the filter build and the rolling scans; the rolled
// scans of sp_map.hip / sp_sparse.hip compute the same from the windows they already hold).  Cores of fewer than two bases
// (k < 5), or no MAP_BLOOM_CORE: the word is addressed by the hashed (k-1)-mer itself.
SP_MH_HD map_bloom_probe map_bloom(uint64_t x64, int k, int nbits) {
    map_bloom_probe p;
    uint32_t h;
    const bool h24 = k <= MAP_HASH24_MAX_K;
    if (!(nbits & MAP_BLOOM_CORE) || k < 5) {
        p.bits = h24 ? map_bloom_bits3_24((uint32_t)x64, h) : map_bloom_bits3(x64, h);
        p.word = h >> (32 - (MAP_BLOOM_NBITS(nbits) - 5));
        return p;
    }
    const int cb = 2 * (k - 3);
    const uint64_t smask = (1ULL << cb) - 1ULL;
    const uint64_t a = x64 >> 4, b = x64 & smask;               // first / last k-3 bases
    const uint64_t ar = sp_mh_revcomp(a, k - 3), br = sp_mh_revcomp(b, k - 3);
    const uint64_t ca = a < ar ? a : ar, cb2 = b < br ? b : br;
    if (h24) {
        const uint32_t ha = map_core_hash24((uint32_t)ca), hb = map_core_hash24((uint32_t)cb2);
        p.word = map_core_word24(ha > hb ? ha : hb, nbits);
        p.bits = map_core_bits3_24(ha, hb);
    } else {
        const uint32_t ha = map_core_hash(ca), hb = map_core_hash(cb2);
        p.bits = map_bloom_bits3(x64, h);
        p.word = map_core_word(ha < hb ? ha : hb, nbits);
    }
    return p;
}

// ----------------------------------------------------------------- compact pair table: bucket of a (k-3)-mer
// A bijection of the kb-bit values.  (x * C) & m depends on the low kb bits of x and of C alone, so for kb <= 24 -- every
// table there is: kb = 2 (k - 3), k <= 15 -- both products are 24 x 24 ones and the bits are what they always were.
SP_MH_HD uint32_t map_ct_mix24(uint32_t x, int kb /* <= 24 */) {
    const uint32_t m = (1u << kb) - 1u;
    uint32_t h = sp_mul24(x, 0x9E3779B1u) & m;        // odd multiplier: a bijection of the kb-bit values
    h ^= h >> ((kb + 1) / 2);                           // xorshift by at least half the width: an involution-like bijection
    h = sp_mul24(h, 0x85EBCA6Bu) & m;
    h ^= h >> ((kb + 1) / 2);
    return h;
}
SP_MH_HD uint32_t map_ct_mix(uint32_t x, int kb) {
    if (kb <= 24) return map_ct_mix24(x, kb);
    const uint32_t m = kb >= 32 ? 0xFFFFFFFFu : ((1u << kb) - 1u);
    uint32_t h = (x * 0x9E3779B1u) & m;
    h ^= h >> ((kb + 1) / 2);
    h = (h * 0x85EBCA6Bu) & m;
    h ^= h >> ((kb + 1) / 2);
    return h;
}
