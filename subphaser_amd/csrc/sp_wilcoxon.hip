// sp_wilcoxon.hip -- Cluster.output_kmers for test_method = wilcoxon (Cluster.py:178-194) on the device: per differential
// k-mer the frequencies count / length are grouped by subgenome, the groups ordered by mean exactly as k7_ttest and
// k7_ranktest order them, and the signed-rank test of sp_wilcoxon.h runs on the pairs (j-th chromosome of the top group,
// j-th chromosome of the second), both in config order.  Every subgenome has the same number n of chromosomes.
// Validation, staging, the workspace and the row prologue (sp_kt_col, the means, top / second) are the shared ones of
// sp_kmertest.h.
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
#include "sp_kmertest.h"
#include "sp_wilcoxon.h"

#define SP_WX_THREADS 128
#define SP_WX_THREADS_WIDE 64       // n > 32

__global__ void __launch_bounds__(SP_WX_THREADS)
k7_wilcoxon(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G, int n,
            const int *__restrict__ gchrom /* G lists of n, back to back */, const double *__restrict__ tab, int *__restrict__ top,
            int *__restrict__ second, double *__restrict__ pvals, double *__restrict__ means, double *__restrict__ stat) {
    extern __shared__ double s_v[];      // [2n][blockDim.x]
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;                  // no barrier below
    const sp_kt_col col{s_v + threadIdx.x, (int)blockDim.x};
    const uint32_t *row = counts + r * C;
    const sp_kt_best best = sp_kt_means_top2(col, row, chrom_len, G, sp_kt_groups_even{n}, gchrom, means + r * G);
    const int t1 = best.t1, t2 = best.t2;
    top[r] = t1;
    second[r] = t2;
    double p = 1.0, st = sp_kt_nan();    // one group: nothing to compare
    if (t2 != t1) {
        sp_kt_load(col, 0, row, gchrom, t1 * n, n, chrom_len);
        sp_kt_load(col, n, row, gchrom, t2 * n, n, chrom_len);
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
    sp_kt_call k{ctx, "sp_kmer_wilcoxon", counts, M, C, lengths, n_groups, group_off, group_chrom, top, second, pvals, means, stat};
    if (group_off && group_off[0] < 0) return sp_fail(ctx, SP_EINVAL, "%s: group_off[0] = %d", k.who, group_off[0]);
    int rc = sp_kt_check_groups(k, INT_MAX, SP_EINVAL);
    if (!rc) rc = sp_kt_check_lengths(k);
    if (rc) return rc;
    const int n = group_off[1] - group_off[0];           // pairs of a row
    for (int g = 1; g < n_groups; g++)
        if (group_off[g + 1] - group_off[g] != n)
            return sp_fail(ctx, SP_EUNSUP, "%s: subgenomes of %d and %d chromosomes (the paired test needs one size)", k.who, n,
                           group_off[g + 1] - group_off[g]);
    if (n < 2 || n > SP_WX_MAXG)
        return sp_fail(ctx, SP_EUNSUP, "%s: subgenomes of %d chromosomes (2..%d supported)", k.who, n, SP_WX_MAXG);
    if (M == 0) return SP_OK;
    std::vector<double> h_tab(1, 0.0);                   // the exact null of n pairs; one table, a call has one n
    if (n <= SP_WX_EXACT_MAX) {
        h_tab.resize((size_t)(n * (n + 1) / 2 + 1));
        sp_wx_exact_table(n, h_tab.data());
    }
    double *d_tab;
    rc = sp_kt_begin(k, true, [&](sp_carve &cv) { d_tab = cv.take<double>(h_tab.size()); });
    if (rc) return rc;
    SP_HIP(ctx, hipMemcpyAsync(d_tab, h_tab.data(), h_tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    const int threads = 2 * n <= 64 ? SP_WX_THREADS : SP_WX_THREADS_WIDE;
    const size_t lds = (size_t)(2 * n) * (size_t)threads * 8;   // <= 64 KiB: 2n <= 64 x 128 threads, 2n <= 128 x 64 threads
    SP_LAUNCH(ctx, "k7_wilcoxon", k7_wilcoxon, dim3((unsigned)((M + threads - 1) / threads)), dim3((unsigned)threads), lds, k.rows,
              (long long)M, C, (const double *)k.d.len, n_groups, n, (const int *)k.d.gch + group_off[0], (const double *)d_tab,
              k.d.top, k.d.sec, k.d.p, k.d.means, k.d.stat);
    return sp_kt_finish(k);
}
