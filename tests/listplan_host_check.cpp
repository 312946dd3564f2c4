// Host check of subphaser_amd/csrc/sp_listplan.h, the host planning of the list filter's join, against values worked
// out by hand from its rules (compiled and run by tests/test_listplan_host.py; exit status 0 and "OK <checks>" on success).
//
// The rules.  Keys have `bits` bits: 2k (at most 64), in list mode ceil(log2(nslots)).  A range is sized for
// per_range = 682 entries (two thirds of a 1024-entry round), with more than 64 lists for 32 per list.  rb is the smallest
// number of range bits with 2^rb * per_range >= total, at most 23 and at most `bits`; `key >> 64` is no shift, so
// bits - rb <= 63.  R = 2^rb, shift = bits - rb.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sp_listplan.h"

static unsigned long long n_checks = 0;
static int n_bad = 0;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        n_checks++;                                                                 \
        if (!(cond) && n_bad++ < 40) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    } while (0)

template <typename T>
static bool same(const std::vector<T> &a, std::initializer_list<T> b) { return a == std::vector<T>(b); }

// the ranges cover the key space: the largest key falls into the last range
static void check_cover(const sp_range_plan &P) {
    CHECK(P.shift >= 0 && P.shift <= 63);
    CHECK(P.R == 1LL << P.rb && P.shift + P.rb == P.bits);
    const unsigned long long top = P.bits == 64 ? ~0ULL : (1ULL << P.bits) - 1;
    CHECK((long long)(top >> P.shift) == P.R - 1);
}

static void check_range(int64_t total, int C, int k, int64_t nslots, int bits, int rb, int shift, long long R, int64_t per_range) {
    const sp_range_plan P = sp_plan_ranges(total, C, k, nslots);
    CHECK(P.bits == bits);
    CHECK(P.rb == rb);
    CHECK(P.shift == shift);
    CHECK(P.R == R);
    CHECK(P.per_range == per_range);
    CHECK(P.wide == (C > 64));
    check_cover(P);
}

static void ranges() {
    for (int64_t total = 1; total <= 3; total++) {
        // the k32_join shape: one range would mean `key >> 64`
        const sp_range_plan P = sp_plan_ranges(total, 4, 32, 0);
        CHECK(P.shift <= 63);
        CHECK(P.R >= 2);
        check_range(total, 4, 32, 0, 64, 1, 63, 2, 682);
        check_range(total, 4, 31, 0, 62, 0, 62, 1, 682);
        check_range(total, 4, 24, 0, 48, 0, 48, 1, 682);
        check_range(total, 4, 17, 0, 34, 0, 34, 1, 682);
        check_range(total, 4, 16, 0, 32, 0, 32, 1, 682);
    }
    // list mode: 100000 / 682 = 146.6 -> 256 ranges; 10^7 / 682 = 14662.8 -> 16384 ranges
    check_range(100000, 4, 15, 1LL << 17, 17, 8, 9, 256, 682);
    check_range(10000000, 4, 15, 1LL << 29, 29, 14, 15, 16384, 682);
    check_range(100000, 4, 9, (1LL << 17) + 1, 18, 8, 10, 256, 682);      // not a power of two: one bit more
    check_range(1000000000, 4, 9, 1LL << 17, 17, 17, 0, 1LL << 17, 682);  // no more range bits than key bits
    // 10^10 / 682 = 1.47e7 > 2^23: the cap
    check_range(10000000000LL, 4, 21, 0, 42, 23, 19, 1LL << 23, 682);
    check_range(10000000000LL, 4, 32, 0, 64, 23, 41, 1LL << 23, 682);
    // 10^6 entries at k = 21: 1466.3 rounds' worth -> 2048; wide from 65 lists on: 10^6 / 2080 = 480.8 -> 512,
    // 10^6 / 32768 = 30.5 -> 32
    check_range(1000000, 1, 21, 0, 42, 11, 31, 2048, 682);
    check_range(1000000, 64, 21, 0, 42, 11, 31, 2048, 682);
    check_range(1000000, 65, 21, 0, 42, 9, 33, 512, 32 * 65);
    check_range(1000000, 1024, 21, 0, 42, 5, 37, 32, 32 * 1024);
    // exact fits: 2 * 682 entries need one range bit, one more needs two
    check_range(682, 4, 21, 0, 42, 0, 42, 1, 682);
    check_range(683, 4, 21, 0, 42, 1, 41, 2, 682);
    check_range(1364, 4, 21, 0, 42, 1, 41, 2, 682);
    check_range(1365, 4, 21, 0, 42, 2, 40, 4, 682);
}

static void row_caps() {
    // total / 16 rows, at least min(total, 2^20), plus a 256-row chunk for each of 16 workgroups per CU
    const unsigned long long slack = 256ULL * 16 * 256;
    CHECK(sp_plan_row_cap(100, 256) == 100 + slack);
    CHECK(sp_plan_row_cap(1LL << 21, 256) == (1ULL << 20) + slack);
    CHECK(sp_plan_row_cap(1LL << 24, 256) == (1ULL << 20) + slack);
    CHECK(sp_plan_row_cap(1LL << 26, 256) == (1ULL << 22) + slack);
    CHECK(sp_plan_row_cap(1LL << 26, 8) == (1ULL << 22) + 8ULL * 16 * 256);
    CHECK(sp_plan_row_retry(5000000, 256) == 5000000 + slack);
}

static void walks() {
    // set 0: units {0, 1} {2} {3}; a singleton set {8}; set 1: units {4} {5, 6} {7}
    const int32_t so[] = {0, 3, 4, 7}, uo[] = {0, 2, 3, 4, 5, 6, 8, 9}, uc[] = {0, 1, 2, 3, 8, 4, 5, 6, 7};
    const double inv[] = {0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125};
    const int UE = 1 << 20, SE = 1 << 21, BI1 = 1 << 22;
    {
        const sp_walk_plan W = sp_plan_walk(3, so, uo, uc, inv, 1, false);
        CHECK(W.fast == 1);
        CHECK(same<int32_t>(W.rd, {0, 1 | UE, 2 | UE, 3 | UE | SE | BI1, 4 | UE, 5, 6 | UE, 7 | UE | SE | BI1}));
        CHECK(same<float>(W.rinv, {0.0f, 0.5f, 0.25f, 0.125f, 0.03125f, 0.0f, 0.015625f, 0.0078125f}));
    }
    {
        const sp_walk_plan W = sp_plan_walk(3, so, uo, uc, inv, -1, false);      // the smallest of three: no BI1
        CHECK(W.fast == 1);
        CHECK(same<int32_t>(W.rd, {0, 1 | UE, 2 | UE, 3 | UE | SE, 4 | UE, 5, 6 | UE, 7 | UE | SE}));
        CHECK(same<float>(W.rinv, {0.0f, 0.5f, 0.25f, 0.125f, 0.03125f, 0.0f, 0.015625f, 0.0078125f}));
    }
    {
        const sp_walk_plan W = sp_plan_walk(3, so, uo, uc, inv, -2, false);      // the second of three, counted from the end
        CHECK(W.fast == 1 && (W.rd[3] & BI1) && (W.rd[7] & BI1));
    }
    {
        const sp_walk_plan W = sp_plan_walk(3, so, uo, uc, inv, 2, false);       // the last of three, as -1
        CHECK(W.fast == 1 && W.rd.size() == 8 && !(W.rd[3] & BI1));
    }
    for (int b : {0, -3}) {           // a baseline other than 1 / -1: the largest frequency itself
        const sp_walk_plan W = sp_plan_walk(3, so, uo, uc, inv, b, false);
        CHECK(W.fast == 0 && W.rd.empty() && W.rinv.empty());
    }
    {
        const int32_t so4[] = {0, 4}, uo4[] = {0, 1, 2, 3, 4}, uc4[] = {0, 1, 2, 3};
        const sp_walk_plan W = sp_plan_walk(1, so4, uo4, uc4, inv, 2, false);    // four units: 2 is neither 1 nor the last
        CHECK(W.fast == 0 && W.rd.empty() && W.rinv.empty());
    }
    {
        const sp_walk_plan W = sp_plan_walk(3, so, uo, uc, inv, 1, true);        // SP_JOIN_GENERIC
        CHECK(W.fast == 0 && W.rd.empty() && W.rinv.empty());
    }
    {
        const int32_t so1[] = {0, 1, 2}, uo1[] = {0, 1, 2}, uc1[] = {0, 1};      // singleton sets only
        const sp_walk_plan W = sp_plan_walk(2, so1, uo1, uc1, inv, 1, false);
        CHECK(W.fast == 0 && W.rd.empty() && W.rinv.empty());
    }
    {
        const int32_t so2[] = {0, 2}, uo2[] = {0, 2, 2}, uc2[] = {0, 1};         // an empty unit
        const sp_walk_plan W = sp_plan_walk(1, so2, uo2, uc2, inv, 1, false);
        CHECK(W.fast == 0 && W.rd.empty() && W.rinv.empty());
    }
    for (int per : {64, 65}) {        // 128 descriptors fit, 130 do not
        const int32_t so3[] = {0, 2}, uo3[] = {0, per, 2 * per};
        std::vector<int32_t> uc3;
        for (int c = 0; c < 2 * per; c++) uc3.push_back(c);
        const sp_walk_plan W = sp_plan_walk(1, so3, uo3, uc3.data(), inv, 1, false);
        CHECK(W.fast == (per == 64 ? 1 : 0));
        CHECK(W.rd.size() == (per == 64 ? 128u : 0u) && W.rinv.size() == W.rd.size());
    }
}

static void masks() {
    // set 0: units {0} {1}; a singleton set {4}; set 1: units {1} {2}; chromosome 3 in no set
    const int32_t so[] = {0, 2, 3, 5}, uo[] = {0, 1, 2, 3, 4, 5}, uc[] = {0, 1, 4, 1, 2};
    {
        const sp_mask_plan M = sp_plan_masks(5, 3, so, uo, uc, false, 2.0);
        CHECK(M.screen == 1);
        CHECK(same<unsigned long long>(M.cs, {1, 3, 2, 0, 0}));
    }
    CHECK(sp_plan_masks(5, 3, so, uo, uc, false, 0.0).screen == 1);
    CHECK(sp_plan_masks(5, 3, so, uo, uc, true, 0.0).screen == 0);      // phase A: an all-zero set passes min_fold <= 0
    CHECK(sp_plan_masks(5, 3, so, uo, uc, true, -1.0).screen == 0);
    CHECK(sp_plan_masks(5, 3, so, uo, uc, true, 2.0).screen == 1);
    {
        std::vector<int32_t> cso, cs;
        sp_plan_wide_csr(5, 3, so, uo, uc, cso, cs);      // sets by their config numbers: 0 and 2
        CHECK(same<int32_t>(cso, {0, 1, 3, 4, 4, 4}));
        CHECK(same<int32_t>(cs, {0, 0, 2, 2}));
    }
    for (int n : {32, 33}) {          // n sets of two units {2s} {2s + 1}: 32-bit masks hold 32 sets
        std::vector<int32_t> s_o, u_o, u_c;
        for (int s = 0; s <= n; s++) s_o.push_back(2 * s);
        for (int u = 0; u <= 2 * n; u++) u_o.push_back(u);
        for (int c = 0; c < 2 * n; c++) u_c.push_back(c);
        const sp_mask_plan M = sp_plan_masks(2 * n, n, s_o.data(), u_o.data(), u_c.data(), false, 2.0);
        CHECK(M.screen == (n == 32 ? 1 : 0));
        CHECK(M.cs[0] == 1 && M.cs[1] == 1 && M.cs[62] == 1ULL << 31 && M.cs[63] == 1ULL << 31);
        if (n == 33) CHECK(M.cs[64] == 0 && M.cs[65] == 0);
    }
}

static void passengers() {
    // set 0: units {5} {2}; a singleton set {0}; set 1: units {2, 6} {3}; chromosomes 1 and 4 in no set
    const int32_t so[] = {0, 2, 3, 5}, uo[] = {0, 1, 2, 3, 5, 6}, uc[] = {5, 2, 0, 2, 6, 3};
    const double den[] = {10, 11, 12, 13, 14, 0.5, 0.25, 0.125, 0.0625, 0.03125};
    const sp_passenger_plan P = sp_plan_passengers(7, 3, so, uo, uc, den);
    CHECK(same<int>(P.pick, {2, 3, 5, 6}));
    CHECK(same<int>(P.num, {-1, -1, 0, 1, -1, 2, 3}));
    CHECK(same<int32_t>(P.a_so, {0, 2, 4}));
    CHECK(same<int32_t>(P.a_uo, {0, 1, 2, 4, 5}));
    CHECK(same<int32_t>(P.a_uc, {2, 0, 0, 3, 1, /* the pad */ 0}));
    CHECK(same<double>(P.a_den, {10, 11, 13, 14, 0.5, 0.25, 0.0625, 0.03125}));
    // 1025 set chromosomes (one more than the list filter takes) among 1030: the caller reports them
    std::vector<int32_t> u_c;
    for (int c = 0; c < 1025; c++) u_c.push_back(1029 - c);
    const int32_t so2[] = {0, 2}, uo2[] = {0, 513, 1025};
    const double den2[] = {1, 1, 1, 1};
    const sp_passenger_plan Q = sp_plan_passengers(1030, 1, so2, uo2, u_c.data(), den2);
    CHECK(Q.pick.size() == 1025 && Q.pick.size() > 1024);
    CHECK(Q.pick.front() == 5 && Q.pick.back() == 1029 && Q.num[4] == -1 && Q.num[5] == 0 && Q.num[1029] == 1024);
    for (size_t i = 1; i < Q.pick.size(); i++) CHECK(Q.pick[i - 1] < Q.pick[i]);
    CHECK(Q.a_uc[0] == 1024 && Q.a_uc[1024] == 0);
}

int main() {
    ranges();
    row_caps();
    walks();
    masks();
    passengers();
    if (n_bad) {
        std::printf("FAILED: %d of %llu checks\n", n_bad, n_checks);
        return 1;
    }
    std::printf("OK %llu\n", n_checks);
    return 0;
}
