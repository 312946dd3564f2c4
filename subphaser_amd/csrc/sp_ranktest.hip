// sp_ranktest.hip -- Cluster.output_kmers for test_method = kruskal and mannwhitneyu (Cluster.py:178-194) on the device:
// per differential k-mer the frequencies count / length are grouped by subgenome, the groups ordered by mean exactly as
// k7_ttest orders them, and the rank-sum test of sp_ranktest.h runs between the top and the second group.  Validation,
// staging, the workspace and the row prologue (sp_kt_col, the means, top / second) are the shared ones of sp_kmertest.h.
//   k7_ranktest   one thread per k-mer row, no barrier, no atomics, nothing shared between threads.  A thread owns column
//                 tid of an LDS array v[i][tid] (i < N, the largest n1 + n2 of the call): element i of all the threads
//                 of a wave lies in 64 consecutive 8-byte words, so every access is conflict-free, and the values
//                 a thread indexes with a run-time i never become a stack array in scratch.  A group's values are divided
//                 once into the column and summed there in numpy's order (the means); the two chosen groups are then
//                 written side by side and ranked by N^2 comparisons on LDS.  Every loop is bounded by N <= 128.
//                 The workgroup is 128 threads up to N = 64 and 64 threads beyond, so the column array is N x threads x 8
//                 <= 64 KiB, the default limit of a workgroup; at N = 14 (wheat, three groups of 7) it is 14 KiB.
// Resources (`make resources`) are in profiles/ranktest_notes.md.
#include "sp_kmertest.h"

#define SP_RT_THREADS 128
#define SP_RT_THREADS_WIDE 64       // N > 64

__global__ void __launch_bounds__(SP_RT_THREADS)
k7_ranktest(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G,
            const int *__restrict__ goff, const int *__restrict__ gchrom, int method, const int *__restrict__ sf_off,
            const double *__restrict__ sf, int *__restrict__ top, int *__restrict__ second, double *__restrict__ pvals,
            double *__restrict__ means, double *__restrict__ stat) {
    extern __shared__ double s_v[];      // [N][blockDim.x]
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;                  // no barrier below
    const sp_kt_col col{s_v + threadIdx.x, (int)blockDim.x};
    const uint32_t *row = counts + r * C;
    const sp_kt_best best = sp_kt_means_top2(col, row, chrom_len, G, sp_kt_groups_off{goff}, gchrom, means + r * G);
    const int t1 = best.t1, t2 = best.t2;
    top[r] = t1;
    second[r] = t2;
    double p = 1.0, st = sp_kt_nan();    // one group: nothing to compare
    if (t2 != t1) {
        const int o1 = goff[t1], n1 = goff[t1 + 1] - o1, o2 = goff[t2], n2 = goff[t2 + 1] - o2;
        sp_kt_load(col, 0, row, gchrom, o1, n1, chrom_len);
        sp_kt_load(col, n1, row, gchrom, o2, n2, chrom_len);
        const int off = sp_rt_exact_sizes(n1, n2) ? sf_off[sp_rt_sf_slot(n1, n2)] : -1;
        p = sp_rt_row(col, n1, n2, method, off >= 0 ? sf + off : nullptr, &st);
    }
    pvals[r] = p;
    stat[r] = st;
}

extern "C" int sp_kmer_ranktest(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                                const int32_t *group_off, const int32_t *group_chrom, int method, int32_t *top, int32_t *second,
                                double *pvals, double *means, double *stat) {
    sp_kt_call k{ctx, "sp_kmer_ranktest", counts, M, C, lengths, n_groups, group_off, group_chrom, top, second, pvals, means, stat};
    if (method != SP_RT_KRUSKAL && method != SP_RT_MWU)
        return sp_fail(ctx, SP_EINVAL, "%s: method %d (0 kruskal, 1 mannwhitneyu)", k.who, method);
    int rc = sp_kt_check_groups(k, SP_RT_MAXG, SP_EINVAL);
    if (!rc) rc = sp_kt_check_lengths(k);
    if (rc || M == 0) return rc;
    int biggest = 0, next = 0;           // the two largest groups: the largest n1 + n2 a row can have
    for (int g = 0; g < n_groups; g++) {
        const int n = group_off[g + 1] - group_off[g];
        if (n > biggest) { next = biggest; biggest = n; }
        else if (n > next) next = n;
    }
    // the exact Mann-Whitney tables of the size pairs this call can meet, one per unordered pair
    std::vector<int> h_off((size_t)SP_RT_SF_SLOTS, -1);
    std::vector<double> h_sf;
    if (method == SP_RT_MWU)
        for (int a = 0; a < n_groups; a++)
            for (int b = a + 1; b < n_groups; b++) {
                const int n1 = group_off[a + 1] - group_off[a], n2 = group_off[b + 1] - group_off[b];
                if (!sp_rt_exact_sizes(n1, n2)) continue;
                int &off = h_off[(size_t)sp_rt_sf_slot(n1, n2)];
                if (off >= 0) continue;
                off = (int)h_sf.size();
                h_sf.resize(h_sf.size() + (size_t)(n1 * n2 + 1));
                sp_rt_exact_table(n1, n2, h_sf.data() + off);
            }
    int *d_sfoff;
    double *d_sf;
    rc = sp_kt_begin(k, true, [&](sp_carve &cv) {
        d_sfoff = cv.take<int>((size_t)SP_RT_SF_SLOTS);
        d_sf = cv.take<double>(h_sf.size() ? h_sf.size() : 1);
    });
    if (rc) return rc;
    SP_HIP(ctx, hipMemcpyAsync(d_sfoff, h_off.data(), (size_t)SP_RT_SF_SLOTS * 4, hipMemcpyHostToDevice, ctx->stream));
    if (h_sf.size()) SP_HIP(ctx, hipMemcpyAsync(d_sf, h_sf.data(), h_sf.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    const int N = n_groups > 1 ? biggest + next : biggest;      // rows of the LDS array: a group alone, or the two chosen
    const int threads = N <= 64 ? SP_RT_THREADS : SP_RT_THREADS_WIDE;
    const size_t lds = (size_t)N * (size_t)threads * 8;         // <= 64 KiB: N <= 64 x 128 threads, N <= 128 x 64 threads
    SP_LAUNCH(ctx, "k7_ranktest", k7_ranktest, dim3((unsigned)((M + threads - 1) / threads)), dim3((unsigned)threads), lds, k.rows,
              (long long)M, C, (const double *)k.d.len, n_groups, (const int *)k.d.goff, (const int *)k.d.gch, method,
              (const int *)d_sfoff, (const double *)d_sf, k.d.top, k.d.sec, k.d.p, k.d.means, k.d.stat);
    return sp_kt_finish(k);
}
