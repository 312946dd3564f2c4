// Host check of subphaser_amd/csrc/sp_culimit.h, the parse of the SP_CU_LIMIT switch (compiled and run by
// tests/test_culimit_host.py; exit status 0 and "OK <checks>" on success).
//
// The rule: a decimal integer 1 <= n < n_cu, nothing before or after it, replaces the device's compute-unit count;
// everything else leaves it alone.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "sp_culimit.h"

static unsigned long long n_checks = 0;
static int n_bad = 0;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        n_checks++;                                                                 \
        if (!(cond) && n_bad++ < 40) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    const int real[] = {256, 304, 64, 2, 1};
    for (int n_cu : real) {
        CHECK(sp_cu_limit(nullptr, n_cu) == n_cu);                        // unset
        CHECK(sp_cu_limit("", n_cu) == n_cu);                             // empty
        for (const char *junk : {"x", "abc", "3x", "x3", "1.5", "1e1", "0x2", " 1", "1 ", "+1", "1\n", "--1", "1,2", "\t"})
            CHECK(sp_cu_limit(junk, n_cu) == n_cu);                       // garbage
        CHECK(sp_cu_limit("0", n_cu) == n_cu);
        CHECK(sp_cu_limit("00", n_cu) == n_cu);
        CHECK(sp_cu_limit("-1", n_cu) == n_cu);                           // negative
        CHECK(sp_cu_limit("-3", n_cu) == n_cu);
        char buf[64];
        std::snprintf(buf, sizeof buf, "%d", n_cu);
        CHECK(sp_cu_limit(buf, n_cu) == n_cu);                            // the real count: no limit
        std::snprintf(buf, sizeof buf, "%d", n_cu + 1);
        CHECK(sp_cu_limit(buf, n_cu) == n_cu);                            // above it
        CHECK(sp_cu_limit("100000", n_cu) == n_cu);
        CHECK(sp_cu_limit("4294967297", n_cu) == n_cu);                   // 2^32 + 1: no wrap to 1
        CHECK(sp_cu_limit("99999999999999999999999999", n_cu) == n_cu);   // out of range of long long
        for (int n = 1; n < n_cu; n++) {                                  // every valid value
            std::snprintf(buf, sizeof buf, "%d", n);
            CHECK(sp_cu_limit(buf, n_cu) == n);
        }
        if (n_cu > 3) CHECK(sp_cu_limit("003", n_cu) == 3);               // leading zeros are still decimal
    }
    CHECK(sp_cu_limit("1", 256) == 1);
    CHECK(sp_cu_limit("3", 256) == 3);
    CHECK(sp_cu_limit("255", 256) == 255);
    CHECK(sp_cu_limit("1", 1) == 1 && sp_cu_limit("1", 2) == 1);
    // the environment itself, as sp_ctx_create reads it
    unsetenv("SP_CU_LIMIT");
    CHECK(sp_cu_limit(getenv("SP_CU_LIMIT"), 256) == 256);
    setenv("SP_CU_LIMIT", "", 1);
    CHECK(sp_cu_limit(getenv("SP_CU_LIMIT"), 256) == 256);
    setenv("SP_CU_LIMIT", "3", 1);
    CHECK(sp_cu_limit(getenv("SP_CU_LIMIT"), 256) == 3);
    if (n_bad) {
        std::printf("FAILED: %d of %llu checks\n", n_bad, n_checks);
        return 1;
    }
    std::printf("OK %llu\n", n_checks);
    return 0;
}
