// Host check of subphaser_amd/csrc/sp_c2plan.h, the host planning of the k <= 15 partition chain, against values worked
// out by hand from its rules (compiled and run by tests/test_c2plan_host.py; exit status 0 and "OK <checks>" on success).
//
// The rules.  Plan: nslots = 2^T; 15 bits are resolved in LDS, the other R = T - 15 are split B1 = ceil(R / 2),
// B2 = floor(R / 2), 1..7 bits each (R >= 2); F = 2^B.  Sizing of a chromosome of len bases: units of 32 starts, part1
// tiles of 512 units, stripes of 64 units; the estimate visits one stripe in 16, n_visit = ceil(stripes / 16) * 64 units.
// Estimate: mult8 = 144 (16 x 9/8), mult8_1 = 132 (16 x 33/32), slack = len / 64 clamped to [4096, 32768],
// slack1 = 4 slack + 65536, sslack = slack1 / 4; exact: 8, 8, 0, 65536 (unused), 0.  pad1 = 3 tiles + 24.
//   cap_keys1 = ceil(n_visit * 32 * mult8_1 / 8) + F1 slack1   (exact: len)   + F1 (pad1 + 4) + 8 F1 (sslack + 8)
//   tiles2_max = floor(cap_keys1 / 6144) + 16 F1
//   cap_keys2 = ceil(n_visit * 32 * mult8 / 8) + n_fine (slack + 4)   (exact: len + 4 n_fine)   + 3 F2 tiles2_max
// Layout, every array rounded up to 256 bytes: ghist 8 n_fine | off_fine 8 (n_fine + 1) | off1 16 (8 F1 + 1) |
// tile_start 8 (8 F1 + 1) | cur1 8 x 1024 x 16 | cur2 8 n_fine || span 16 n_fine | lo1 2 cap_keys1 + 64 + 64 F1 |
// hi1 cap_keys1 + 64 + 32 F1 | buf2 2 cap_keys2 + 64 | seg_base 4 n_fine | seg_cnt 4 n_fine | seg_off 4 (n_fine + 1) |
// stage 8 per pair.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "sp_c2plan.h"

static unsigned long long n_checks = 0;
static int n_bad = 0;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        n_checks++;                                                                 \
        if (!(cond) && n_bad++ < 40) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    } while (0)

static c2_plan plan_of(int T) {
    c2_plan P;
    CHECK(c2_make_plan(1LL << T, P));
    return P;
}

static void plans() {
    c2_plan P = plan_of(29);      // R = 14 = 7 + 7
    CHECK(P.T == 29 && P.B1 == 7 && P.B2 == 7 && P.F1 == 128 && P.F2 == 128 && P.n_fine == 16384);
    P = plan_of(28);              // R = 13 = 7 + 6
    CHECK(P.T == 28 && P.B1 == 7 && P.B2 == 6 && P.F1 == 128 && P.F2 == 64 && P.n_fine == 8192);
    P = plan_of(17);              // the smallest: R = 2 = 1 + 1
    CHECK(P.T == 17 && P.B1 == 1 && P.B2 == 1 && P.F1 == 2 && P.F2 == 2 && P.n_fine == 4);
    P = plan_of(18);              // R = 3 = 2 + 1
    CHECK(P.B1 == 2 && P.B2 == 1 && P.n_fine == 8);
    c2_plan Q;
    CHECK(!c2_make_plan(1LL << 16, Q));             // R = 1
    CHECK(!c2_make_plan(3LL << 17, Q));             // no power of two
    CHECK(!c2_make_plan((1LL << 29) - 1, Q));
    CHECK(!c2_make_plan(1LL << 30, Q));             // R = 15: B1 = 8
}

// offsets of a layout run on a null base
static size_t at(const void *p) { return (size_t)(uintptr_t)p; }

// the properties every layout has: 256-byte offsets, arrays in order without overlap, the head contiguous from 0
static void check_layout(const c2_plan &P, const c2_sizing &S, size_t stage_pairs) {
    const size_t nf = (size_t)P.n_fine, V1 = (size_t)P.F1 * 8;
    sp_carve w;
    const c2_layout L = c2_lay(P, S, stage_pairs, w, w);
    const size_t off[] = {at(L.ghist), at(L.off_fine), at(L.off1), at(L.tile_start), at(L.cur1), at(L.cur2), at(L.span), at(L.lo1),
                          at(L.hi1), at(L.buf2), at(L.seg_base), at(L.seg_cnt), at(L.seg_off), at(L.stage), w.off};
    const size_t bytes[] = {8 * nf, 8 * (nf + 1), 16 * (V1 + 1), 8 * (V1 + 1), 8 * 1024 * 16, 8 * nf, 16 * nf, 2 * S.cap_keys1 + 64 + 8 * V1,
                            S.cap_keys1 + 64 + 4 * V1, 2 * S.cap_keys2 + 64, 4 * nf, 4 * nf, 4 * (nf + 1), 8 * stage_pairs};
    CHECK(off[0] == 0);
    for (int i = 0; i < 14; i++) {
        CHECK(off[i] % 256 == 0);
        CHECK(off[i + 1] >= off[i] + bytes[i]);          // no overlap
        CHECK(off[i + 1] < off[i] + bytes[i] + 256);     // and no hole: the head is contiguous from 0 to the span
    }
    CHECK(at(L.cur2) - at(L.cur1) == (size_t)C2_MAXV * C2_CSTRIDE * 8);     // whatever F1 is
    CHECK(L.lo1_bytes() == at(L.hi1) - at(L.lo1));
    // the batched use: heads of two chromosomes back to back, then their bodies -- same offsets inside head and body
    const size_t zero_bytes = at(L.span);
    sp_carve head, body;
    const c2_layout A = c2_lay(P, S, stage_pairs, head, body);
    CHECK(head.off == zero_bytes && body.off == w.off - zero_bytes);
    const c2_layout B = c2_lay(P, S, stage_pairs, head, body);
    CHECK(head.off == 2 * zero_bytes && body.off == 2 * (w.off - zero_bytes));
    CHECK(at(A.ghist) == 0 && at(A.off_fine) == at(L.off_fine) && at(A.off1) == at(L.off1) && at(A.tile_start) == at(L.tile_start) &&
          at(A.cur1) == at(L.cur1) && at(A.cur2) == at(L.cur2));
    CHECK(at(A.span) == 0 && at(A.lo1) == at(L.lo1) - zero_bytes && at(A.hi1) == at(L.hi1) - zero_bytes &&
          at(A.buf2) == at(L.buf2) - zero_bytes && at(A.seg_base) == at(L.seg_base) - zero_bytes &&
          at(A.seg_cnt) == at(L.seg_cnt) - zero_bytes && at(A.seg_off) == at(L.seg_off) - zero_bytes &&
          at(A.stage) == at(L.stage) - zero_bytes);
    CHECK(at(B.ghist) == zero_bytes && at(B.cur2) == zero_bytes + at(L.cur2));
    CHECK(at(B.span) == w.off - zero_bytes && at(B.stage) == w.off - zero_bytes + at(A.stage));
}

static void case1() {
    // 2^29 slots, 20 000 000 bases: 625 000 units, ceil(625000 / 512) = 1221 tiles, 9766 stripes, 611 sampled: 39104 units
    const c2_plan P = plan_of(29);
    c2_sizing S = c2_size(P, 20000000, false, -1, -1);
    CHECK(S.n_units32 == 625000 && S.n_tiles == 1221 && S.n_visit == 39104);
    CHECK(S.sample_shift == 4 && S.split == 8);
    CHECK(S.mult8 == 144 && S.mult8_1 == 132);
    CHECK(S.slack == 32768 && S.slack1 == 196608);       // 312500 clamped; 4 x 32768 + 65536
    CHECK(S.pad1 == 3687 && S.sslack == 49152);          // 3 x 1221 + 24; 196608 / 4
    // 39104 x 32 = 1251328 sampled k-mers: x 132 / 8 = 20646912; + 128 x 196608 + 128 x 3691 + 1024 x 49160
    CHECK(S.cap_keys1 == 96625024);
    CHECK(S.tiles2_max == 17774);                        // 15726 + 2048
    // 1251328 x 144 / 8 = 22523904; + 16384 x 32772 + 384 x 17774
    CHECK(S.cap_keys2 == 566285568);
    CHECK(S.cap_keys() == 566285568);
    CHECK(S.stage_pairs(3) == 188761856 + 32768 + 16);
    sp_carve w;
    c2_layout L = c2_lay(P, S, 0, w, w);
    // head: 131072 + 131328 + 16640 + 8448 + 131072 + 131072
    CHECK(at(L.ghist) == 0 && at(L.off_fine) == 131072 && at(L.off1) == 262400 && at(L.tile_start) == 279040 &&
          at(L.cur1) == 287488 && at(L.cur2) == 418560);
    CHECK(at(L.span) == 549632);
    CHECK(at(L.lo1) == 811776 && at(L.hi1) == 194070272 && at(L.buf2) == 290699520);
    CHECK(at(L.seg_base) == 1423270912 && at(L.seg_cnt) == 1423336448 && at(L.seg_off) == 1423401984);
    CHECK(at(L.stage) == 1423467776 && w.off == 1423467776);      // no stage: the end
    check_layout(P, S, 0);
    check_layout(P, S, S.stage_pairs(3));
    // exact mode: the full histogram, one sub-region per level-1 bucket, no slack
    S = c2_size(P, 20000000, true, -1, -1);
    CHECK(S.n_units32 == 625000 && S.n_tiles == 1221 && S.n_visit == 625000);
    CHECK(S.sample_shift == 0 && S.split == 1 && S.mult8 == 8 && S.mult8_1 == 8 && S.slack == 0 && S.sslack == 0 && S.pad1 == 3687);
    CHECK(S.cap_keys1 == 20480640);                      // 20000000 + 128 x 3691 + 1024 x 8
    CHECK(S.tiles2_max == 5381);                         // 3333 + 2048
    CHECK(S.cap_keys2 == 22131840);                      // 20000000 + 65536 + 384 x 5381
    sp_carve x;
    L = c2_lay(P, S, 0, x, x);
    CHECK(at(L.span) == 549632 && x.off == 106727168);
    check_layout(P, S, 0);
    // the overrides do not reach exact mode
    const c2_sizing X = c2_size(P, 20000000, true, 16, 64);
    CHECK(X.mult8 == 8 && X.mult8_1 == 8 && X.slack == 0 && X.slack1 == S.slack1 && X.sslack == 0 && X.cap_keys1 == 20480640 &&
          X.cap_keys2 == 22131840 && X.tiles2_max == 5381);
}

static void overrides() {
    const c2_plan P = plan_of(29);
    // both: the multiplier and the slack of the fine buckets go for level 1 as well
    c2_sizing S = c2_size(P, 20000000, false, 16, 64);
    CHECK(S.mult8 == 16 && S.mult8_1 == 16 && S.slack == 64 && S.slack1 == 64 && S.sslack == 16 && S.split == 8 && S.n_visit == 39104);
    CHECK(S.cap_keys1 == 3007872);       // 1251328 x 16 / 8 = 2502656; + 128 x 64 + 128 x 3691 + 1024 x 24
    CHECK(S.tiles2_max == 2537);         // 489 + 2048
    CHECK(S.cap_keys2 == 4590976);       // 2502656 + 16384 x 68 + 384 x 2537
    check_layout(P, S, S.stage_pairs(1));
    S = c2_size(P, 20000000, false, 16, -1);
    CHECK(S.mult8 == 16 && S.mult8_1 == 16 && S.slack == 32768 && S.slack1 == 196608 && S.sslack == 49152);
    S = c2_size(P, 20000000, false, -1, 64);
    CHECK(S.mult8 == 144 && S.mult8_1 == 132 && S.slack == 64 && S.slack1 == 64 && S.sslack == 16);
    S = c2_size(P, 20000000, false, -1, 0);      // a slack of nothing is an override too
    CHECK(S.slack == 0 && S.slack1 == 0 && S.sslack == 0 && S.mult8 == 144);
}

static void smallest() {
    // 2^17 slots (F1 = F2 = 2, 4 fine buckets, 16 sub-regions), 5000 bases: 157 units, one tile, 3 stripes, one sampled
    const c2_plan P = plan_of(17);
    c2_sizing S = c2_size(P, 5000, false, -1, -1);
    CHECK(S.n_units32 == 157 && S.n_tiles == 1 && S.n_visit == 64);
    CHECK(S.slack == 4096 && S.slack1 == 81920 && S.pad1 == 27 && S.sslack == 20480);
    CHECK(S.cap_keys1 == 525502);        // 64 x 32 x 132 / 8 = 33792; + 2 x 81920 + 2 x 31 + 16 x 20488
    CHECK(S.tiles2_max == 117);          // 85 + 32
    CHECK(S.cap_keys2 == 53966);         // 64 x 32 x 144 / 8 = 36864; + 4 x 4100 + 6 x 117
    sp_carve w;
    c2_layout L = c2_lay(P, S, 0, w, w);
    // head: 256 + 256 + 512 + 256 + 131072 + 256; span 256; lo1 1051196 -> 1051392; hi1 525630 -> 525824; buf2 107996 -> 108032
    CHECK(at(L.span) == 132608 && at(L.lo1) == 132864 && at(L.hi1) == 1184256 && at(L.buf2) == 1710080);
    CHECK(at(L.seg_base) == 1818112 && at(L.seg_cnt) == 1818368 && at(L.seg_off) == 1818624 && w.off == 1818880);
    check_layout(P, S, 0);
    check_layout(P, S, S.stage_pairs(2));
    // shorter than one stripe (2048 starts): still one whole stripe is visited, one tile
    for (int64_t len : {1000, 1, 2048}) {
        S = c2_size(P, len, false, -1, -1);
        CHECK(S.n_units32 == (len + 31) / 32 && S.n_tiles == 1 && S.n_visit == 64);
        CHECK(S.cap_keys1 == 525502 && S.tiles2_max == 117 && S.cap_keys2 == 53966);
        check_layout(P, S, 0);
    }
    S = c2_size(P, 1000, true, -1, -1);
    CHECK(S.n_visit == 32 && S.cap_keys1 == 1000 + 2 * 31 + 16 * 8 && S.tiles2_max == 32 && S.cap_keys2 == 1000 + 16 + 6 * 32);
    check_layout(P, S, 0);
    S = c2_size(P, 2049, false, -1, -1);         // 65 units: a second stripe, still one sampled
    CHECK(S.n_units32 == 65 && S.n_visit == 64);
    S = c2_size(P, 16 * 2048 + 1, false, -1, -1);     // a 17th stripe: a second sampled one
    CHECK(S.n_units32 == 1025 && S.n_tiles == 3 && S.n_visit == 128 && S.pad1 == 33);
}

static void clamps() {
    const c2_plan P = plan_of(27);
    struct { int64_t len; unsigned long long slack; } cases[] = {
        {64 * 4096 - 1, 4096}, {64 * 4096, 4096}, {64 * 4096 + 63, 4096}, {64 * 4096 + 64, 4097}, {100, 4096},
        {64 * 32768 - 1, 32767}, {64 * 32768, 32768}, {64 * 32768 + 64, 32768}, {1LL << 30, 32768}};
    for (const auto &c : cases) {
        const c2_sizing S = c2_size(P, c.len, false, -1, -1);
        CHECK(S.slack == c.slack);
        CHECK(S.slack1 == 4 * c.slack + 65536 && S.sslack == c.slack + 16384);
    }
}

static void lanes() {
    const int64_t G = 1LL << 30;
    {   // 16 GiB device, 10 GiB free: 9 GiB to give away
        const int64_t need[3] = {4 * G, 4 * G, 4 * G};
        CHECK(sp_lanes_fit(need, 3, 10 * G, 16 * G) == 2);
        CHECK(sp_lanes_fit(need, 2, 10 * G, 16 * G) == 2);
        CHECK(sp_lanes_fit(need, 0, 10 * G, 16 * G) == 0);
        CHECK(sp_lanes_fit(need, 3, 13 * G, 16 * G) == 3);      // 12 GiB: exactly enough
        CHECK(sp_lanes_fit(need, 3, 13 * G - 1, 16 * G) == 2);
    }
    {
        const int64_t need[3] = {0, 0, 10 * G};
        CHECK(sp_lanes_fit(need, 3, 10 * G, 16 * G) == 2);
    }
    {   // only LEADING lanes count: a lane that does not fit ends the row
        const int64_t need[3] = {10 * G, 0, 0};
        CHECK(sp_lanes_fit(need, 3, 10 * G, 16 * G) == 0);
    }
    {   // Less than a sixteenth free: the budget is negative and `0 > budget` holds, so not even lanes whose buffers exist
        // already (need = 0) fit.  This is what the drivers have always done; it is pinned here as it is, not endorsed.
        const int64_t need[2] = {0, 0};
        CHECK(sp_lanes_fit(need, 2, G / 2, 16 * G) == 0);
        CHECK(sp_lanes_fit(need, 2, G, 16 * G) == 2);            // budget 0: nothing to give, nothing needed
    }
}

int main() {
    plans();
    case1();
    overrides();
    smallest();
    clamps();
    lanes();
    if (n_bad) {
        std::printf("%d of %llu checks FAILED\n", n_bad, n_checks);
        return 1;
    }
    std::printf("OK %llu\n", n_checks);
    return 0;
}
