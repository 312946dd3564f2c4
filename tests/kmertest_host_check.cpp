// Host check of subphaser_amd/csrc/sp_ktlayout.h, the host-clean part of the k-mer tests' shared driver (compiled and
// run by tests/test_kmertest_host.py; exit status 0 and "OK <checks>" on success).
// The layout on a null base: every array starts at a 256-byte multiple, arrays follow one another without overlap in
// the order rows | len | goff | gch | top | sec | p | [stat] | means | extra, the total is the end of the last array, the
// rows take no room when they are on the device already, and the sizing and the placing pass agree.  The group check:
// its verdicts on hand-made lists, the first fault in group order.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>
#include "sp_ktlayout.h"

static unsigned long long n_checks = 0;
static int n_bad = 0;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        n_checks++;                                                                 \
        if (!(cond) && n_bad++ < 40) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    } while (0)

static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t at(const void *p) { return (size_t)(uintptr_t)p; }

static void layout(int64_t M, int C, int G, bool on_device, bool with_stat, size_t extra_doubles) {
    const sp_kt_shape s{M, C, G, (size_t)C, on_device, with_stat};
    double *extra = nullptr;
    int runs = 0;
    auto hook = [&](sp_carve &cv) {
        runs++;
        if (extra_doubles) extra = cv.take<double>(extra_doubles);
    };
    sp_kt_arrays a;
    sp_carve sizes;
    const size_t need = sp_kt_layout(sizes, s, a, hook);
    CHECK(runs == 1 && need == sizes.off);
    const size_t m = (size_t)M;
    struct arr { size_t at, bytes; };
    std::vector<arr> A = {{at(a.rows), on_device ? 0 : m * C * 4}, {at(a.len), (size_t)C * 8}, {at(a.goff), (size_t)(G + 1) * 4},
                          {at(a.gch), (size_t)C * 4}, {at(a.top), m * 4}, {at(a.sec), m * 4}, {at(a.p), m * 8}};
    if (with_stat) A.push_back({at(a.stat), m * 8});
    else CHECK(a.stat == nullptr);
    A.push_back({at(a.means), m * G * 8});
    if (extra_doubles) A.push_back({at(extra), extra_doubles * 8});
    size_t end = 0;
    for (const arr &x : A) {
        CHECK(x.at % 256 == 0);
        CHECK(x.at == end);                 // behind the one before: no overlap, no hole beyond the rounding
        end = x.at + up(x.bytes);
    }
    CHECK(need == end);
    CHECK(at(a.rows) == 0 && (on_device ? at(a.len) == 0 : at(a.len) == up(m * C * 4)));
    // the placing pass on a buffer: the same offsets from its base
    const size_t base = 1 << 20;
    sp_kt_arrays b;
    double *first = extra;
    sp_carve cv((void *)base);
    CHECK(sp_kt_layout(cv, s, b, hook) == need && runs == 2);
    CHECK(at(b.rows) == base + at(a.rows) && at(b.len) == base + at(a.len) && at(b.goff) == base + at(a.goff));
    CHECK(at(b.gch) == base + at(a.gch) && at(b.top) == base + at(a.top) && at(b.sec) == base + at(a.sec));
    CHECK(at(b.p) == base + at(a.p) && at(b.means) == base + at(a.means));
    CHECK(with_stat ? at(b.stat) == base + at(a.stat) : b.stat == nullptr);
    if (extra_doubles) CHECK(at(extra) == base + at(first));
}

static void groups() {
    const int32_t off[] = {0, 3, 5, 6}, ch[] = {0, 1, 2, 5, 4, 3};
    CHECK(sp_kt_groups_verdict(6, 3, off, ch, 3).what == SP_KT_GROUPS_OK);
    sp_kt_verdict v = sp_kt_groups_verdict(6, 3, off, ch, 2);
    CHECK(v.what == SP_KT_GROUP_BIG && v.g == 0 && v.n == 3);
    v = sp_kt_groups_verdict(5, 3, off, ch, 3);                     // index 5 of group 1 with 5 chromosomes
    CHECK(v.what == SP_KT_CHROM_RANGE && v.g == 1);
    const int32_t neg[] = {0, 1, 2, 5, 4, -1};
    v = sp_kt_groups_verdict(6, 3, off, neg, 3);
    CHECK(v.what == SP_KT_CHROM_RANGE && v.g == 2);
    CHECK(sp_kt_groups_verdict(6, 2, off, neg, 3).what == SP_KT_GROUPS_OK);      // the bad entry lies behind the lists
    const int32_t empty[] = {0, 3, 3, 6}, back[] = {0, 3, 2, 6};
    v = sp_kt_groups_verdict(6, 3, empty, ch, 3);
    CHECK(v.what == SP_KT_GROUP_EMPTY && v.g == 1 && v.n == 0);
    v = sp_kt_groups_verdict(6, 3, back, ch, 4);
    CHECK(v.what == SP_KT_GROUP_EMPTY && v.g == 1 && v.n == -1);
    v = sp_kt_groups_verdict(5, 3, empty, ch, 2);                   // the first fault in group order: group 0 is too big
    CHECK(v.what == SP_KT_GROUP_BIG && v.g == 0);
}

int main() {
    for (int64_t M : {1, 129})
        for (int G : {1, 2, 3})
            for (int on_device = 0; on_device < 2; on_device++)
                for (int with_stat = 0; with_stat < 2; with_stat++)
                    for (size_t extra : {(size_t)0, (size_t)1, (size_t)73}) layout(M, 6, G, on_device, with_stat, extra);
    groups();
    if (n_bad) {
        std::printf("%d of %llu checks FAILED\n", n_bad, n_checks);
        return 1;
    }
    std::printf("OK %llu\n", n_checks);
    return 0;
}
