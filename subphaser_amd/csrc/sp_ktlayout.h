// sp_ktlayout.h -- the host-clean part of the k-mer tests' shared driver (sp_kmertest.h): the group check's logic and the
// workspace layout.  Plain C++ (no HIP types): tests/kmertest_host_check.cpp runs both with the host compiler alone.
#pragma once
#include "sp_carve.h"

// the first thing wrong with the subgenome lists: group `g` of `n` chromosomes, or nothing (what == SP_KT_GROUPS_OK)
enum { SP_KT_GROUPS_OK = 0, SP_KT_GROUP_EMPTY, SP_KT_GROUP_BIG, SP_KT_CHROM_RANGE };
struct sp_kt_verdict {
    int what, g, n;
};
inline sp_kt_verdict sp_kt_groups_verdict(int C, int n_groups, const int32_t *group_off, const int32_t *group_chrom, int max_group) {
    for (int g = 0; g < n_groups; g++) {
        const int n = group_off[g + 1] - group_off[g];
        if (n < 1) return {SP_KT_GROUP_EMPTY, g, n};
        if (n > max_group) return {SP_KT_GROUP_BIG, g, n};
        for (int j = group_off[g]; j < group_off[g + 1]; j++)
            if (group_chrom[j] < 0 || group_chrom[j] >= C) return {SP_KT_CHROM_RANGE, g, n};
    }
    return {SP_KT_GROUPS_OK, 0, 0};
}

// what sizes the common arrays of a call
struct sp_kt_shape {
    int64_t M;                  // rows
    int C, G;                   // chromosomes, groups
    size_t nuc;                 // entries of the chromosome lists: group_off[G]
    bool rows_on_device;        // the caller's rows are read in place: no slot for them
    bool with_stat;             // the test has a statistic besides p
};
// the device arrays every k-mer test has
struct sp_kt_arrays {
    uint32_t *rows;             // [M][C], empty when the rows are on the device already
    double *len;                // [C]
    int *goff, *gch;            // [G + 1], [nuc]
    int *top, *sec;             // [M]
    double *p, *stat, *means;   // [M], [M] or null, [M][G]
};
// The one layout: the common arrays, then whatever `extra` takes (a test's own tables).  Run on sp_carve() it sizes the
// workspace, run on sp_carve(buffer) it places the arrays; either way it returns the bytes used.
template <class Extra>
inline size_t sp_kt_layout(sp_carve &cv, const sp_kt_shape &s, sp_kt_arrays &a, Extra &&extra) {
    const size_t M = (size_t)s.M;
    a.rows = cv.take<uint32_t>(s.rows_on_device ? 0 : M * (size_t)s.C);
    a.len = cv.take<double>((size_t)s.C);
    a.goff = cv.take<int>((size_t)s.G + 1);
    a.gch = cv.take<int>(s.nuc);
    a.top = cv.take<int>(M);
    a.sec = cv.take<int>(M);
    a.p = cv.take<double>(M);
    a.stat = s.with_stat ? cv.take<double>(M) : nullptr;
    a.means = cv.take<double>(M * (size_t)s.G);
    extra(cv);
    return cv.off;
}
