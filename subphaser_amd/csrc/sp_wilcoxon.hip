// sp_wilcoxon.hip -- Cluster.output_kmers for test_method = wilcoxon (Cluster.py:178-194) on the device: per differential
// k-mer the frequencies count / length are grouped by subgenome, the groups ordered by mean exactly as k7_ttest and
// k7_ranktest order them, and the signed-rank test of sp_wilcoxon.h runs on the pairs (j-th chromosome of the top group,
// j-th chromosome of the second), both in config order.  Every subgenome has the same number n of chromosomes.
//   k7_wilcoxon   one thread per k-mer row, no barrier, no atomics, nothing shared between threads.  A thread owns column
//                 tid of an LDS array v[i][tid] (i < 2n): element i of all the threads of a wave lies in 64 consecutive
//                 8-byte words, so every access is conflict-free, and the values a thread indexes with a run-time i never
//                 become a stack array in scratch.  A group's values are divided once into the column and summed there in
//                 numpy's order (the means, sp_rt_np_sum); the two chosen groups are then written side by side, the
//                 differences overwrite the first and the doubled ranks of the nonzero ones the second.
//                 Permutation branch (n <= 13, a zero or a tie in the row): a Gray-code walk over the 2^m sign assignments
//                 of the m nonzero ranks -- one LDS read (the rank of element ctz(k)), one add or subtract and two
//                 compares per step, no storage beyond the column; at most 2^13 = 8192 steps, the only loop of the kernel
//                 not bounded by n^2 <= 4096.  Rows of one wave may take different branches and walks of different
//                 length; the wave then runs as long as its longest row.
//                 The workgroup is 128 threads up to n = 32 and 64 threads beyond, so the column array is
//                 2n x threads x 8 <= 64 KiB, the default limit of a workgroup; at n = 7 (wheat) it is 14 KiB.
// Resources (`make resources`) are in profiles/wilcoxon_notes.md.
#include "sp_common.h"
#include "sp_ranktest.h"
#include "sp_wilcoxon.h"

#define SP_WX_THREADS 128
#define SP_WX_THREADS_WIDE 64       // n > 32

namespace {
// column tid of the workgroup's LDS array
struct wx_col {
    double *p;
    int pitch;
    __device__ __forceinline__ double at(int i) const { return p[i * pitch]; }
    __device__ __forceinline__ void set(int i, double x) const { p[i * pitch] = x; }
};
}  // namespace

__global__ void __launch_bounds__(SP_WX_THREADS)
k7_wilcoxon(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G, int n,
            const int *__restrict__ gchrom, const double *__restrict__ tab, int *__restrict__ top, int *__restrict__ second,
            double *__restrict__ pvals, double *__restrict__ means, double *__restrict__ stat) {
    extern __shared__ double s_v[];      // [2n][blockDim.x]
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;                  // no barrier below
    const wx_col col{s_v + threadIdx.x, (int)blockDim.x};
    const uint32_t *row = counts + r * C;
    int t1 = -1, t2 = -1;
    double m1 = 0, m2 = 0;
    for (int g = 0; g < G; g++) {        // means in numpy's summation order; descending, ties in group order (k7_ranktest)
        const int o = g * n;
        for (int i = 0; i < n; i++) {
            const int c = gchrom[o + i];
            col.set(i, (double)row[c] / chrom_len[c]);
        }
        const double mean = sp_rt_np_sum(col, n) / (double)n;
        means[r * G + g] = mean;
        if (t1 < 0 || mean > m1) { t2 = t1; m2 = m1; t1 = g; m1 = mean; }
        else if (t2 < 0 || mean > m2) { t2 = g; m2 = mean; }
    }
    if (t2 < 0) t2 = t1;
    top[r] = t1;
    second[r] = t2;
    double p = 1.0, st = __longlong_as_double(0x7ff8000000000000LL);     // one group: nothing to compare
    if (t2 != t1) {
        const int o1 = t1 * n, o2 = t2 * n;
        for (int i = 0; i < n; i++) {
            const int c = gchrom[o1 + i];
            col.set(i, (double)row[c] / chrom_len[c]);
        }
        for (int i = 0; i < n; i++) {
            const int c = gchrom[o2 + i];
            col.set(n + i, (double)row[c] / chrom_len[c]);
        }
        for (int i = 0; i < n; i++) col.set(i, col.at(i) - col.at(n + i));
        int branch;
        p = sp_wx_row(col, n, tab, &st, &branch);
    }
    pvals[r] = p;
    stat[r] = st;
}

extern "C" int sp_kmer_wilcoxon(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                                const int32_t *group_off, const int32_t *group_chrom, int32_t *top, int32_t *second,
                                double *pvals, double *means, double *stat) {
    if (!ctx || M < 0 || C < 1 || n_groups < 1 || !lengths || !group_off || !group_chrom ||
        (M > 0 && (!counts || !top || !second || !pvals || !means)))
        return sp_fail(ctx, SP_EINVAL, "sp_kmer_wilcoxon: bad arguments");
    if (group_off[0] < 0) return sp_fail(ctx, SP_EINVAL, "sp_kmer_wilcoxon: group_off[0] = %d", group_off[0]);
    for (int g = 0; g < n_groups; g++) {
        const int sz = group_off[g + 1] - group_off[g];
        if (sz < 1) return sp_fail(ctx, SP_EINVAL, "sp_kmer_wilcoxon: subgenome %d has %d chromosomes", g, sz);
        for (int j = group_off[g]; j < group_off[g + 1]; j++)
            if (group_chrom[j] < 0 || group_chrom[j] >= C) return sp_fail(ctx, SP_EINVAL, "sp_kmer_wilcoxon: chromosome index out of range");
    }
    for (int c = 0; c < C; c++)
        if (lengths[c] <= 0) return sp_fail(ctx, SP_EINVAL, "sp_kmer_wilcoxon: chromosome %d has length %lld", c, (long long)lengths[c]);
    const int n = group_off[1] - group_off[0];           // pairs of a row
    for (int g = 1; g < n_groups; g++)
        if (group_off[g + 1] - group_off[g] != n)
            return sp_fail(ctx, SP_EUNSUP, "sp_kmer_wilcoxon: subgenomes of %d and %d chromosomes (the paired test needs one size)", n,
                           group_off[g + 1] - group_off[g]);
    if (n < 2 || n > SP_WX_MAXG)
        return sp_fail(ctx, SP_EUNSUP, "sp_kmer_wilcoxon: subgenomes of %d chromosomes (2..%d supported)", n, SP_WX_MAXG);
    if (M == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> h_tab(1, 0.0);                   // the exact null of n pairs; one table, a call has one n
    if (n <= SP_WX_EXACT_MAX) {
        h_tab.resize((size_t)(n * (n + 1) / 2 + 1));
        sp_wx_exact_table(n, h_tab.data());
    }
    const size_t nuc = (size_t)n_groups * (size_t)n;        // the lists back to back, n each
    bool on_device = false;              // rows staged on this device earlier are read in place, as in sp_kmer_ranktest
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, counts) == hipSuccess)
            on_device = at.type == hipMemoryTypeDevice && at.device == ctx->device;
        else
            (void)hipGetLastError();     // a plain malloc'ed pointer is "invalid value" for this query on some runtimes
    }
    auto layout = [&](sp_carve &cv, uint32_t *&d_rows, double *&d_len, int *&d_gch, double *&d_tab, int *&d_top, int *&d_sec,
                      double *&d_p, double *&d_stat, double *&d_means) {
        d_rows = cv.take<uint32_t>(on_device ? 0 : (size_t)M * (size_t)C);
        d_len = cv.take<double>((size_t)C);
        d_gch = cv.take<int>(nuc);
        d_tab = cv.take<double>(h_tab.size());
        d_top = cv.take<int>((size_t)M);
        d_sec = cv.take<int>((size_t)M);
        d_p = cv.take<double>((size_t)M);
        d_stat = cv.take<double>((size_t)M);
        d_means = cv.take<double>((size_t)M * (size_t)n_groups);
    };
    uint32_t *d_rows;
    double *d_len, *d_tab, *d_p, *d_stat, *d_means;
    int *d_gch, *d_top, *d_sec;
    sp_carve sizes;
    layout(sizes, d_rows, d_len, d_gch, d_tab, d_top, d_sec, d_p, d_stat, d_means);
    const int rc = sp_buf_ensure(ctx, ctx->b_tt, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_kmer_wilcoxon: a workspace of %lld bytes (%lld rows x %d chromosomes%s, %d groups) does not fit on the device",
                       (long long)sizes.off, (long long)M, C, on_device ? ", read in place" : " and their upload", n_groups);
    if (rc) return rc;
    sp_carve cv(ctx->b_tt.p);
    layout(cv, d_rows, d_len, d_gch, d_tab, d_top, d_sec, d_p, d_stat, d_means);
    const uint32_t *d_counts = on_device ? counts : d_rows;
    std::vector<double> hl((size_t)C);
    for (int c = 0; c < C; c++) hl[(size_t)c] = (double)lengths[c];
    if (!on_device) SP_HIP(ctx, hipMemcpyAsync(d_rows, counts, (size_t)M * C * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_len, hl.data(), (size_t)C * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_gch, group_chrom + group_off[0], nuc * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_tab, h_tab.data(), h_tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    const int threads = 2 * n <= 64 ? SP_WX_THREADS : SP_WX_THREADS_WIDE;
    const size_t lds = (size_t)(2 * n) * (size_t)threads * 8;   // <= 64 KiB: 2n <= 64 x 128 threads, 2n <= 128 x 64 threads
    SP_LAUNCH(ctx, "k7_wilcoxon", k7_wilcoxon, dim3((unsigned)((M + threads - 1) / threads)), dim3((unsigned)threads), lds, d_counts,
              (long long)M, C, (const double *)d_len, n_groups, n, (const int *)d_gch, (const double *)d_tab, d_top, d_sec, d_p,
              d_means, d_stat);
    SP_HIP(ctx, hipMemcpyAsync(top, d_top, (size_t)M * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(second, d_sec, (size_t)M * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(pvals, d_p, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(means, d_means, (size_t)M * n_groups * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (stat) SP_HIP(ctx, hipMemcpyAsync(stat, d_stat, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}
