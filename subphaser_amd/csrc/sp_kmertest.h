// sp_kmertest.h -- what the per-k-mer tests of Cluster.output_kmers share: sp_kmer_ttest and sp_kmer_ttest_wide
// (sp_enrich.hip), sp_kmer_ranktest (sp_ranktest.hip), sp_kmer_ranktest_wide (sp_rankwide.hip) and sp_kmer_wilcoxon
// (sp_wilcoxon.hip).  Included from .hip units only.
//   host    sp_kt_check_groups / sp_kt_check_lengths validate the arguments; sp_kt_begin decides whether the rows are read
//           in place (sp_on_device), lays the workspace out in ctx->b_tt (sp_ktlayout.h: the common arrays, then the
//           entry's own through its hook) and uploads lengths, lists and host rows; sp_kt_finish copies the results back
//           and waits.  An entry reads: checks, its own tables, begin, its launches, finish.
//   device  the row prologue of the kernels: the LDS column view, dividing a group's counts into it, the means in numpy's
//           order and the top / second update with ties in group order.
// k7_ttest keeps its register arrays and d_np_sum, and the wide kernels their tw_group: d_np_sum also serves k6_enrich on
// the benchmarked path, so merging it with sp_rt_np_sum is left alone here.
#pragma once
#include <limits.h>

#include "sp_common.h"
#include "sp_ktlayout.h"
#include "sp_ranktest.h"

// ---------------------------------------------------------------- host
// One call: the arguments every entry takes (stat null for the t-tests) and, from sp_kt_begin on, its device side: `d` the
// common arrays, `rows` the counts the kernels read (the caller's, or d.rows), `hl` the lengths as doubles -- the source
// of an asynchronous copy, so it lives until sp_kt_finish has waited for the stream.
struct sp_kt_call {
    sp_ctx *ctx;
    const char *who;            // the entry's name: the prefix of its messages
    const uint32_t *counts;
    int64_t M;
    int C;
    const int64_t *lengths;
    int n_groups;
    const int32_t *group_off, *group_chrom;
    int32_t *top, *second;
    double *pvals, *means, *stat;
    sp_kt_arrays d;
    const uint32_t *rows;
    std::vector<double> hl;
};
// null pointers, then the subgenome lists: every group has 1..max_group chromosomes (SP_EUNSUP beyond; an empty group is
// `empty_rc`: SP_EUNSUP for the t-tests, which count it as out of that range, SP_EINVAL elsewhere), every index is in [0, C)
inline int sp_kt_check_groups(const sp_kt_call &k, int max_group, int empty_rc) {
    if (!k.ctx || k.M < 0 || k.C < 1 || k.n_groups < 1 || !k.lengths || !k.group_off || !k.group_chrom ||
        (k.M > 0 && (!k.counts || !k.top || !k.second || !k.pvals || !k.means)))
        return sp_fail(k.ctx, SP_EINVAL, "%s: bad arguments", k.who);
    const sp_kt_verdict v = sp_kt_groups_verdict(k.C, k.n_groups, k.group_off, k.group_chrom, max_group);
    if (v.what == SP_KT_CHROM_RANGE) return sp_fail(k.ctx, SP_EINVAL, "%s: chromosome index out of range", k.who);
    if (v.what == SP_KT_GROUP_BIG || (v.what == SP_KT_GROUP_EMPTY && empty_rc == SP_EUNSUP))
        return sp_fail(k.ctx, SP_EUNSUP, "%s: a subgenome with %d chromosomes (1..%d supported)", k.who, v.n, max_group);
    if (v.what == SP_KT_GROUP_EMPTY) return sp_fail(k.ctx, empty_rc, "%s: subgenome %d has %d chromosomes", k.who, v.g, v.n);
    return SP_OK;
}
inline int sp_kt_check_lengths(const sp_kt_call &k) {
    for (int c = 0; c < k.C; c++)
        if (k.lengths[c] <= 0)
            return sp_fail(k.ctx, SP_EINVAL, "%s: chromosome %d has length %lld", k.who, c, (long long)k.lengths[c]);
    return SP_OK;
}

// M > 0.  `extra(cv)` takes the entry's own arrays behind the common ones; it runs twice, sizing and placing.
template <class Extra>
int sp_kt_begin(sp_kt_call &k, bool with_stat, Extra &&extra) {
    sp_ctx *ctx = k.ctx;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    // `counts` may be a host or a DEVICE pointer (a caller that staged the rows earlier, Context.stage_rows): rows that
    // already live on this device are read in place -- no second M x C copy inside the workspace
    const sp_kt_shape shape{k.M, k.C, k.n_groups, (size_t)k.group_off[k.n_groups], sp_on_device(ctx, k.counts), with_stat};
    sp_carve sizes;
    const size_t need = sp_kt_layout(sizes, shape, k.d, extra);
    const int rc = sp_buf_ensure(ctx, ctx->b_tt, (int64_t)need);
    if (rc == SP_ENOMEM) {
        (void)hipGetLastError();     // or the context's next launch check would report this allocation
        return sp_fail(ctx, SP_ENOMEM, "%s: a workspace of %lld bytes (%lld rows x %d chromosomes%s, %d groups) does not fit on the device",
                       k.who, (long long)need, (long long)k.M, k.C, shape.rows_on_device ? ", read in place" : " and their upload",
                       k.n_groups);
    }
    if (rc) return rc;
    sp_carve cv(ctx->b_tt.p);
    sp_kt_layout(cv, shape, k.d, extra);
    k.rows = shape.rows_on_device ? k.counts : k.d.rows;
    k.hl.assign(k.lengths, k.lengths + k.C);
    if (!shape.rows_on_device)
        SP_HIP(ctx, hipMemcpyAsync(k.d.rows, k.counts, (size_t)k.M * k.C * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(k.d.len, k.hl.data(), (size_t)k.C * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(k.d.goff, k.group_off, (size_t)(k.n_groups + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(k.d.gch, k.group_chrom, shape.nuc * 4, hipMemcpyHostToDevice, ctx->stream));
    return SP_OK;
}
inline int sp_kt_finish(const sp_kt_call &k) {
    sp_ctx *ctx = k.ctx;
    const size_t M = (size_t)k.M;
    SP_HIP(ctx, hipMemcpyAsync(k.top, k.d.top, M * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(k.second, k.d.sec, M * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(k.pvals, k.d.p, M * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(k.means, k.d.means, M * k.n_groups * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (k.stat) SP_HIP(ctx, hipMemcpyAsync(k.stat, k.d.stat, M * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

// ---------------------------------------------------------------- device: the row prologue
// Column tid of a workgroup's LDS array v[i][tid]: element i of all the threads of a wave lies in 64 consecutive 8-byte
// words, so every access is conflict-free, and values indexed with a run-time i never become a stack array in scratch.
struct sp_kt_col {
    double *p;
    int pitch;
    __device__ __forceinline__ double at(int i) const { return p[i * pitch]; }
    __device__ __forceinline__ void set(int i, double x) const { p[i * pitch] = x; }
};
// the statistic or p-value of a test with nothing to compare (one group; no degrees of freedom)
__device__ __forceinline__ double sp_kt_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
// The two best groups so far and their order keys.  sp_kt_top2 lets group g with key `key` in: descending, ties in group
// order.  By value: through references the compiler merges the two branches' stores into one store through a selected
// address before it inlines, and t1 .. k2 end up in scratch.
struct sp_kt_best {
    int t1 = -1, t2 = -1;
    double k1 = 0, k2 = 0;
};
__device__ __forceinline__ sp_kt_best sp_kt_top2(int g, double key, sp_kt_best b) {
    if (b.t1 < 0 || key > b.k1) { b.t2 = b.t1; b.k2 = b.k1; b.t1 = g; b.k1 = key; }
    else if (b.t2 < 0 || key > b.k2) { b.t2 = g; b.k2 = key; }
    return b;
}
// col[at + i] = the frequency of chromosome gchrom[o + i], i < n.  (An index, not the pointer gchrom + o: the pointer form
// costs k7_ranktest and k7_wilcoxon registers and a step of occupancy.)
__device__ __forceinline__ void sp_kt_load(const sp_kt_col &col, int at, const uint32_t *__restrict__ row,
                                           const int *__restrict__ gchrom, int o, int n, const double *__restrict__ chrom_len) {
    for (int i = 0; i < n; i++) {
        const int c = gchrom[o + i];
        col.set(at + i, (double)row[c] / chrom_len[c]);
    }
}
// where group g's chromosome list starts in gchrom and how long it is: by offsets, or G lists of n back to back
struct sp_kt_groups_off {
    const int *__restrict__ goff;
    __device__ __forceinline__ int start(int g) const { return goff[g]; }
    __device__ __forceinline__ int size(int g) const { return goff[g + 1] - goff[g]; }
};
struct sp_kt_groups_even {
    int n;
    __device__ __forceinline__ int start(int g) const { return g * n; }
    __device__ __forceinline__ int size(int) const { return n; }
};
// means_out[g] = the mean of every group in numpy's summation order (the column serves as the buffer); returns the groups
// of the highest and second-highest mean (t2 = t1 for a single group)
template <class Groups>
__device__ __forceinline__ sp_kt_best sp_kt_means_top2(const sp_kt_col &col, const uint32_t *__restrict__ row,
                                                       const double *__restrict__ chrom_len, int G, const Groups &groups,
                                                       const int *__restrict__ gchrom, double *__restrict__ means_out) {
    sp_kt_best b;
    for (int g = 0; g < G; g++) {
        const int n = groups.size(g);
        sp_kt_load(col, 0, row, gchrom, groups.start(g), n, chrom_len);
        const double mean = sp_rt_np_sum(col, n) / (double)n;
        means_out[g] = mean;
        b = sp_kt_top2(g, mean, b);
    }
    if (b.t2 < 0) b.t2 = b.t1;
    return b;
}
