// sp_ranktest.hip -- Cluster.output_kmers for test_method = kruskal and mannwhitneyu (Cluster.py:178-194) on the device:
// per differential k-mer the frequencies count / length are grouped by subgenome, the groups ordered by mean exactly as
// k7_ttest orders them, and the rank-sum test of sp_ranktest.h runs between the top and the second group.
//   k7_ranktest   one thread per k-mer row, no barrier, no atomics, nothing shared between threads.  A thread owns column
//                 tid of an LDS array v[i][tid] (i < N, the largest n1 + n2 of the call): element i of all the threads
//                 of a wave lies in 64 consecutive 8-byte words, so every access is conflict-free, and the values
//                 a thread indexes with a run-time i never become a stack array in scratch.  A group's values are divided
//                 once into the column and summed there in numpy's order (the means); the two chosen groups are then
//                 written side by side and ranked by N^2 comparisons on LDS.  Every loop is bounded by N <= 128.
//                 The workgroup is 128 threads up to N = 64 and 64 threads beyond, so the column array is N x threads x 8
//                 <= 64 KiB, the default limit of a workgroup; at N = 14 (wheat, three groups of 7) it is 14 KiB.
// Resources (`make resources`) are in profiles/ranktest_notes.md.
#include "sp_common.h"
#include "sp_ranktest.h"

#define SP_RT_THREADS 128
#define SP_RT_THREADS_WIDE 64       // N > 64

namespace {
// column tid of the workgroup's LDS array
struct rt_col {
    double *p;
    int pitch;
    __device__ __forceinline__ double at(int i) const { return p[i * pitch]; }
    __device__ __forceinline__ void set(int i, double x) const { p[i * pitch] = x; }
};
}  // namespace

__global__ void __launch_bounds__(SP_RT_THREADS)
k7_ranktest(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len, int G,
            const int *__restrict__ goff, const int *__restrict__ gchrom, int method, const int *__restrict__ sf_off,
            const double *__restrict__ sf, int *__restrict__ top, int *__restrict__ second, double *__restrict__ pvals,
            double *__restrict__ means, double *__restrict__ stat) {
    extern __shared__ double s_v[];      // [N][blockDim.x]
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;                  // no barrier below
    const rt_col col{s_v + threadIdx.x, (int)blockDim.x};
    const uint32_t *row = counts + r * C;
    int t1 = -1, t2 = -1;
    double m1 = 0, m2 = 0;
    for (int g = 0; g < G; g++) {        // means in numpy's summation order; descending, ties in group order (k7_ttest)
        const int o = goff[g], n = goff[g + 1] - o;
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
        const int o1 = goff[t1], n1 = goff[t1 + 1] - o1, o2 = goff[t2], n2 = goff[t2 + 1] - o2;
        for (int i = 0; i < n1; i++) {
            const int c = gchrom[o1 + i];
            col.set(i, (double)row[c] / chrom_len[c]);
        }
        for (int i = 0; i < n2; i++) {
            const int c = gchrom[o2 + i];
            col.set(n1 + i, (double)row[c] / chrom_len[c]);
        }
        const int off = sp_rt_exact_sizes(n1, n2) ? sf_off[sp_rt_sf_slot(n1, n2)] : -1;
        p = sp_rt_row(col, n1, n2, method, off >= 0 ? sf + off : nullptr, &st);
    }
    pvals[r] = p;
    stat[r] = st;
}

extern "C" int sp_kmer_ranktest(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                                const int32_t *group_off, const int32_t *group_chrom, int method, int32_t *top, int32_t *second,
                                double *pvals, double *means, double *stat) {
    if (!ctx || M < 0 || C < 1 || n_groups < 1 || !lengths || !group_off || !group_chrom ||
        (M > 0 && (!counts || !top || !second || !pvals || !means)))
        return sp_fail(ctx, SP_EINVAL, "sp_kmer_ranktest: bad arguments");
    if (method != SP_RT_KRUSKAL && method != SP_RT_MWU)
        return sp_fail(ctx, SP_EINVAL, "sp_kmer_ranktest: method %d (0 kruskal, 1 mannwhitneyu)", method);
    int biggest = 0, next = 0;           // the two largest groups: the largest n1 + n2 a row can have
    for (int g = 0; g < n_groups; g++) {
        const int n = group_off[g + 1] - group_off[g];
        if (n < 1) return sp_fail(ctx, SP_EINVAL, "sp_kmer_ranktest: subgenome %d has %d chromosomes", g, n);
        if (n > SP_RT_MAXG)
            return sp_fail(ctx, SP_EUNSUP, "sp_kmer_ranktest: a subgenome with %d chromosomes (1..%d supported)", n, SP_RT_MAXG);
        for (int j = group_off[g]; j < group_off[g + 1]; j++)
            if (group_chrom[j] < 0 || group_chrom[j] >= C) return sp_fail(ctx, SP_EINVAL, "sp_kmer_ranktest: chromosome index out of range");
        if (n > biggest) { next = biggest; biggest = n; }
        else if (n > next) next = n;
    }
    for (int c = 0; c < C; c++)
        if (lengths[c] <= 0) return sp_fail(ctx, SP_EINVAL, "sp_kmer_ranktest: chromosome %d has length %lld", c, (long long)lengths[c]);
    if (M == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
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
    const size_t nuc = (size_t)group_off[n_groups], n_sf = h_sf.size() ? h_sf.size() : 1;
    bool on_device = false;              // rows staged on this device earlier are read in place, as in sp_kmer_ttest
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, counts) == hipSuccess)
            on_device = at.type == hipMemoryTypeDevice && at.device == ctx->device;
        else
            (void)hipGetLastError();     // a plain malloc'ed pointer is "invalid value" for this query on some runtimes
    }
    auto layout = [&](sp_carve &cv, uint32_t *&d_rows, double *&d_len, int *&d_goff, int *&d_gch, int *&d_sfoff, double *&d_sf,
                      int *&d_top, int *&d_sec, double *&d_p, double *&d_stat, double *&d_means) {
        d_rows = cv.take<uint32_t>(on_device ? 0 : (size_t)M * (size_t)C);
        d_len = cv.take<double>((size_t)C);
        d_goff = cv.take<int>((size_t)n_groups + 1);
        d_gch = cv.take<int>(nuc);
        d_sfoff = cv.take<int>((size_t)SP_RT_SF_SLOTS);
        d_sf = cv.take<double>(n_sf);
        d_top = cv.take<int>((size_t)M);
        d_sec = cv.take<int>((size_t)M);
        d_p = cv.take<double>((size_t)M);
        d_stat = cv.take<double>((size_t)M);
        d_means = cv.take<double>((size_t)M * (size_t)n_groups);
    };
    uint32_t *d_rows;
    double *d_len, *d_sf, *d_p, *d_stat, *d_means;
    int *d_goff, *d_gch, *d_sfoff, *d_top, *d_sec;
    sp_carve sizes;
    layout(sizes, d_rows, d_len, d_goff, d_gch, d_sfoff, d_sf, d_top, d_sec, d_p, d_stat, d_means);
    const int rc = sp_buf_ensure(ctx, ctx->b_tt, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_kmer_ranktest: a workspace of %lld bytes (%lld rows x %d chromosomes%s, %d groups) does not fit on the device",
                       (long long)sizes.off, (long long)M, C, on_device ? ", read in place" : " and their upload", n_groups);
    if (rc) return rc;
    sp_carve cv(ctx->b_tt.p);
    layout(cv, d_rows, d_len, d_goff, d_gch, d_sfoff, d_sf, d_top, d_sec, d_p, d_stat, d_means);
    const uint32_t *d_counts = on_device ? counts : d_rows;
    std::vector<double> hl((size_t)C);
    for (int c = 0; c < C; c++) hl[(size_t)c] = (double)lengths[c];
    if (!on_device) SP_HIP(ctx, hipMemcpyAsync(d_rows, counts, (size_t)M * C * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_len, hl.data(), (size_t)C * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_goff, group_off, (size_t)(n_groups + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_gch, group_chrom, nuc * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_sfoff, h_off.data(), (size_t)SP_RT_SF_SLOTS * 4, hipMemcpyHostToDevice, ctx->stream));
    if (h_sf.size()) SP_HIP(ctx, hipMemcpyAsync(d_sf, h_sf.data(), h_sf.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    const int N = n_groups > 1 ? biggest + next : biggest;      // rows of the LDS array: a group alone, or the two chosen
    const int threads = N <= 64 ? SP_RT_THREADS : SP_RT_THREADS_WIDE;
    const size_t lds = (size_t)N * (size_t)threads * 8;         // <= 64 KiB: N <= 64 x 128 threads, N <= 128 x 64 threads
    SP_LAUNCH(ctx, "k7_ranktest", k7_ranktest, dim3((unsigned)((M + threads - 1) / threads)), dim3((unsigned)threads), lds, d_counts,
              (long long)M, C, (const double *)d_len, n_groups, (const int *)d_goff, (const int *)d_gch, method, (const int *)d_sfoff,
              (const double *)d_sf, d_top, d_sec, d_p, d_means, d_stat);
    SP_HIP(ctx, hipMemcpyAsync(top, d_top, (size_t)M * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(second, d_sec, (size_t)M * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(pvals, d_p, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(means, d_means, (size_t)M * n_groups * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (stat) SP_HIP(ctx, hipMemcpyAsync(stat, d_stat, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}
