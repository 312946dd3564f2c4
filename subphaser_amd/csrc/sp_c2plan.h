// sp_c2plan.h -- host planning of the k <= 15 partition chain (sp_count2.hip) as plain C++: no HIP types, so the host
// compiler alone builds it (tests/c2plan_host_check.cpp).  The geometry that kernels and sizing share, the sizing rule, the
// workspace layout and the lane-fit rule are stated here, once: the per-chromosome and the batched driver both run them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sp_carve.h"

#define C2_B3 15                      // slot bits resolved inside LDS
#define C2_FINE (1 << C2_B3)          // slots per fine bucket
#ifndef C2_P1_THREADS
#define C2_P1_THREADS 512             // part1: 512 threads x 32 k-mer starts
#endif
#define C2_P1_UNIT 32
#ifndef C2_P2_THREADS
#define C2_P2_THREADS 256             // (round 4, after the cursor fix: 256 x 24: 0.861 ms, 512 x 24: 0.897, 512 x 16: 0.990, 768 x 16: 1.20) part2 tile = threads x keys per thread.  Round 1 (software pipeline): 512 x 8 -> 1.37 ms per
                                      // 667-Mb chromosome, 768 x 12 -> 1.22.  Round 2 (rank from the histogram atomic, one table read
                                      // in the copy-out): 768 x 12 1.21, 768 x 16 1.31, 768 x 20 1.25, 1024 x 12 1.23, 1024 x 16 1.17,
                                      // 512 x 24 1.16 (adopted: 12 K-key tiles, 288-byte runs, three blocks per CU)
#endif
#ifndef C2_P2_PER
#define C2_P2_PER 24
#endif
#define C2_TILE_KEYS (C2_P2_THREADS * C2_P2_PER)  // keys per part2 tile
#define C2_MAXF 128                   // max fan-out per level (k <= 15: at most 2^29 slots = 7 + 7 + 15 bits)
// Cursors (round 4, tools/ubench_frag.hip).  Returning atomics on ONE cache line serialise: 128 cursors packed into
// 1 KiB held a 40 K-tile partition pass at 0.88 ms whatever it wrote; one cursor per 128-byte line 0.52 ms; eight
// sub-cursors per bucket on a line each 0.29 ms.  So every cursor owns a line, and a level-1 bucket is cut into
// C2_SPLIT sub-regions with a cursor each: tile t appends to sub-region t mod C2_SPLIT (a static, even deal of the
// tiles; with the blocks of a launch dealt round-robin to the XCDs, usually also a deal by L2).  Downstream a
// sub-region is just a level-1 "bucket" of its own: V1 = F1 * C2_SPLIT of them.
#define C2_SPLIT 8
#define C2_CSTRIDE 16                 // cursor stride in 8-byte words
#define C2_MAXV (C2_MAXF * C2_SPLIT)
// Layout (measured on one 667-Mb chain, part1 / part2 ms): every cursor on a line of its own 0.922 / 0.953; the 128
// cursors that ONE tile touches packed together -- sub-region m of all buckets in 1 KiB, the sub-regions apart --
// 0.883 / 0.899: a wave's atomics then touch 8 lines instead of 64, and only the tiles of one residue class (part1) or of
// one level-1 bucket (part2, whose concurrent tiles lie in different buckets) share them.
#ifndef C2_CSTRIDE2
#define C2_CSTRIDE2 1                 // stride of the fine (part2) cursors
#endif
#define C2_STRIPE 64                  // units per stripe: 2048 starts = 512 B of each packed stream, one wave
#define C2_SAMPLE_SHIFT 4             // one stripe in 16

struct c2_plan {
    int T;        // log2(nslots)
    int B1, B2;   // partition bits
    int F1, F2;
    int64_t n_fine;  // F1*F2
};

inline bool c2_make_plan(int64_t nslots, c2_plan &p) {
    int T = 0;
    while ((1LL << T) < nslots) T++;
    if ((1LL << T) != nslots) return false;
    int R = T - C2_B3;
    if (R < 2) return false;
    p.T = T;
    p.B1 = (R + 1) / 2;
    p.B2 = R / 2;
    if (p.B1 > 7 || p.B2 > 7) return false;
    p.F1 = 1 << p.B1;
    p.F2 = 1 << p.B2;
    p.n_fine = (int64_t)p.F1 * p.F2;
    return true;
}

// What a chromosome of `len` bases needs.  exact = false: the bucket regions are laid out from the 1-in-16 stripe
// sample; exact = true: from the full histogram, nothing can overrun.
struct c2_sizing {
    int64_t n_units32, n_tiles, n_visit;      // units of 32 starts; part1 tiles (16384 starts each); units the histogram visits
    int sample_shift, split;                  // split: sub-regions per level-1 bucket in use (C2_SPLIT, exact mode: 1)
    unsigned long long mult8, mult8_1;        // fine / level-1 region = histogram x mult / 8 ...
    unsigned long long slack, slack1;         // ... + slack
    unsigned long long pad1, sslack;          // pad records of a level-1 bucket; slack of a sub-region
    size_t cap_keys1, tiles2_max, cap_keys2;  // records the level-1 planes / buf2 hold at most; part2 tiles at most
    size_t cap_keys() const { return cap_keys1 > cap_keys2 ? cap_keys1 : cap_keys2; }
    // unordered (slot, count) pairs the list counter stages at most: a bucket's segment starts at floor(its first key / lower)
    size_t stage_pairs(int lower) const { return cap_keys() / (size_t)lower + C2_FINE + 16; }
};

// mult8_override / slack_override (the test hooks SP_C2_MULT8 / SP_C2_SLACK; negative: none) replace the fine multiplier and
// slack of estimate mode; an overridden value also goes for level 1 (mult8_1 = mult8, slack1 = slack).  Exact mode takes neither.
inline c2_sizing c2_size(const c2_plan &P, int64_t len, bool exact, long long mult8_override, long long slack_override) {
    c2_sizing S;
    const bool own_mult = !exact && mult8_override >= 0, own_slack = !exact && slack_override >= 0;
    S.n_units32 = (len + C2_P1_UNIT - 1) / C2_P1_UNIT;
    S.n_tiles = (S.n_units32 + C2_P1_THREADS - 1) / C2_P1_THREADS;
    // estimate mode: cap(f) = sample(f) * 16 * 9/8 + slack.  The slack absorbs what a 1-in-16 stripe sample cannot
    // see: a local array of one repeat shorter than 16 stripes (32 K starts) that falls between sampled stripes.
    S.sample_shift = exact ? 0 : C2_SAMPLE_SHIFT;
    S.mult8 = exact ? 8ULL : (unsigned long long)(own_mult ? mult8_override : (9 << C2_SAMPLE_SHIFT));
    int64_t sl = len / 64;
    sl = sl < 4096 ? 4096 : (sl > 32768 ? 32768 : sl);
    S.slack = exact ? 0ULL : (unsigned long long)(own_slack ? slack_override : sl);
    S.slack1 = own_slack ? S.slack : 4ULL * S.slack + 65536ULL;
    S.mult8_1 = (exact || own_mult) ? S.mult8 : (unsigned long long)(33 << (C2_SAMPLE_SHIFT - 2));   // x 1 1/32
    const int64_t n_stripes = (S.n_units32 + C2_STRIPE - 1) / C2_STRIPE;
    S.n_visit = exact ? S.n_units32 : ((n_stripes + (1 << C2_SAMPLE_SHIFT) - 1) >> C2_SAMPLE_SHIFT) * C2_STRIPE;
    // keys the regions can hold at most (rigorous bounds: the sample sees at most n_visit * 32 k-mers).  Pad records:
    // three per (part1 tile, level-1 bucket) and per (part2 tile, fine bucket) at most -- c2_offsets adds the same terms.
    S.pad1 = 3ULL * (unsigned long long)S.n_tiles + 3ULL * C2_SPLIT;
    // estimate mode: C2_SPLIT sub-regions per level-1 bucket, a quarter of the bucket's slack each; exact mode: one
    S.split = exact ? 1 : C2_SPLIT;
    S.sslack = exact ? 0ULL : S.slack1 / 4;
    const size_t nf = (size_t)P.n_fine, V1 = (size_t)P.F1 * C2_SPLIT;
    S.cap_keys1 = (exact ? (size_t)len : (size_t)(((unsigned long long)S.n_visit * C2_P1_UNIT * S.mult8_1 + 7) / 8) +
                                             (size_t)P.F1 * (size_t)S.slack1) +
                  (size_t)P.F1 * (size_t)(S.pad1 + 4) + V1 * (size_t)(S.sslack + 8);
    S.tiles2_max = S.cap_keys1 / C2_TILE_KEYS + 2 * V1;
    S.cap_keys2 = (exact ? (size_t)len + 4 * nf
                         : (size_t)(((unsigned long long)S.n_visit * C2_P1_UNIT * S.mult8 + 7) / 8) + nf * (size_t)(S.slack + 4)) +
                  3 * (size_t)P.F2 * S.tiles2_max;
    return S;
}

// A chromosome's workspace.  The head is zeroed with one memset before the chain runs; the body is written before it is
// read.  Arrays of HIP vector types are carved as bytes (span: ulonglong2 per fine bucket, stage: uint2 per pair).
struct c2_layout {
    unsigned long long *ghist, *off_fine, *off1, *tile_start, *cur1, *cur2;      // head
    unsigned char *span;
    uint16_t *lo1;               // level-1 records: 3 bytes per key in two planes
    uint8_t *hi1;
    uint16_t *buf2;
    uint32_t *seg_base, *seg_cnt, *seg_off;      // overflow / list segments: base, count, offsets per fine bucket
    unsigned char *stage;        // batched list count: the unordered pairs (a per-chromosome chain stages elsewhere)
    size_t lo1_bytes() const { return (size_t)((const unsigned char *)hi1 - (const unsigned char *)lo1); }
};
// The batched driver keeps the heads of all its chromosomes back to back (one memset), then their bodies: two carvers.
// A single chromosome passes one carver for both.
inline c2_layout c2_lay(const c2_plan &P, const c2_sizing &S, size_t stage_pairs, sp_carve &head, sp_carve &body) {
    const size_t nf = (size_t)P.n_fine, V1 = (size_t)P.F1 * C2_SPLIT;
    c2_layout L;
    L.ghist = head.take<unsigned long long>(nf);
    L.off_fine = head.take<unsigned long long>(nf + 1);
    L.off1 = head.take<unsigned long long>(2 * (V1 + 1));                  // level-1 sub-region starts, then ends
    L.tile_start = head.take<unsigned long long>(V1 + 1);
    L.cur1 = head.take<unsigned long long>((size_t)C2_MAXV * C2_CSTRIDE);  // (any layout of C2_CUR1: sub-region m of bucket b)
    L.cur2 = head.take<unsigned long long>(nf * C2_CSTRIDE2);
    L.span = body.take<unsigned char>(nf * 16);
    L.lo1 = (uint16_t *)body.take<unsigned char>(S.cap_keys1 * 2 + 64 + V1 * 8);
    L.hi1 = body.take<uint8_t>(S.cap_keys1 + 64 + V1 * 4);
    L.buf2 = (uint16_t *)body.take<unsigned char>(S.cap_keys2 * 2 + 64);
    L.seg_base = body.take<uint32_t>(nf);
    L.seg_cnt = body.take<uint32_t>(nf);
    L.seg_off = body.take<uint32_t>(nf + 1);
    L.stage = body.take<unsigned char>(stage_pairs * 8);
    return L;
}

// Every counting lane owns a workspace; need[l] is what lane l still has to allocate.  Returns how many leading lanes fit
// what the device has free less a sixteenth of the device.  (A negative budget fits no lane, not even one that needs nothing.)
inline int sp_lanes_fit(const int64_t *need, int n, int64_t free_bytes, int64_t total_bytes) {
    int64_t budget = free_bytes - total_bytes / 16;      // keep a sixteenth of the device free
    int fit = 0;
    for (int l = 0; l < n; l++) {
        if (need[l] > budget) break;
        budget -= need[l];
        fit++;
    }
    return fit;
}
