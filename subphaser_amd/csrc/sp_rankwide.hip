// sp_rankwide.hip -- Cluster.output_kmers for test_method = kruskal and mannwhitneyu when a subgenome has more than the
// SP_RT_MAXG = 64 chromosomes k7_ranktest takes (scaffold-level assemblies), up to SP_RW_MAXG = 4096 per group.
// Validation, staging, the workspace and the copies back are the shared ones of sp_kmertest.h; sp_rankwide.h states the
// arithmetic.  Two passes over the rows:
//   pass 1  k7_ttest_wide_means (sp_enrich.hip, through sp_tw_means_launch): means = numpy's pairwise np.mean, top / second
//           by the reference's order key -sum(x) / len(x), added left to right, ties in group order.
//   pass 2  k7_ranktest_wide, one workgroup per row.  It divides the counts of the row's top and second group by their
//           lengths into two LDS segments, each padded with +inf to a power of two, sorts both with one bitonic network
//           (a comparator index runs over the two segments back to back; a step beyond a segment's size skips it), and
//           then every thread ranks its elements by the lower and upper bounds in both segments (sp_rw_rank_one).  S1, S2
//           and T are summed in 64-bit integers: per thread, per wave by shuffles, then over the waves through LDS -- the
//           segments' own memory, after a barrier, so a row of 4096 + 4096 values needs the 64 KiB of its values and no
//           more.  One lane forms the statistic and p.  Every loop bound and every barrier depends on the row's size pair
//           alone: uniform within the workgroup.
//   LDS     a comparator reads elements lo and lo + j.  For j >= 32 the 32 lanes of a ds_read_b64 group read 32
//           consecutive doubles: all 64 banks once.  For j < 32 the 32 comparators of a group span 64 doubles and their
//           low elements fall on 16 of the 32 double-wide bank pairs, twice each; so the comparators whose low element
//           lies in the upper half of that span read their high element first: each of the two loads then touches every
//           bank pair once.  The stores (16-lane groups) keep a 2-way conflict for j < 16; they are issued only by
//           comparators that swap.  The binary searches read data-dependent addresses.
//   shape   threads = (P1 + P2) / SP_RW_PER_THREAD for the two largest groups of the call, padded, within 64 .. 1024: four
//           comparators and eight elements per thread, so that the barriers of a sorting step join few waves and several
//           rows share a CU.  Measured with 2, 4, 8 and 16 per thread (profiles/ranktest_wide_notes.md): fewer waves per
//           row were faster at every step down to 8; 16 was not tried on the 64-KiB rows, where it halves the resident waves.
// Resources (`make resources`) are in profiles/ranktest_wide_notes.md.
#include "sp_internal.h"
#include "sp_kmertest.h"
#include "sp_rankwide.h"

#define SP_RW_THREADS_MIN 64
#define SP_RW_THREADS_MAX 1024
#define SP_RW_LDS_MIN 512        // the reduction's 3 sums of up to 16 waves
#ifndef SP_RW_PER_THREAD
#define SP_RW_PER_THREAD 8       // padded values of a row per thread: half as many comparators
#endif

struct rw_seg {
    const double *p;
    __device__ __forceinline__ double at(int i) const { return p[i]; }
};

__device__ __forceinline__ long long rw_wave_sum(long long v) {
    for (int d = SP_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, SP_WAVE);
    return v;
}

__global__ void __launch_bounds__(SP_RW_THREADS_MAX)
k7_ranktest_wide(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ chrom_len,
                 const int *__restrict__ goff, const int *__restrict__ gchrom, int method, const long long *__restrict__ sf_off,
                 const double *__restrict__ sf, const int *__restrict__ top, const int *__restrict__ second,
                 double *__restrict__ pvals, double *__restrict__ stat) {
    extern __shared__ double s_x[];      // [P1] the top group's values, [P2] the second's; then the waves' sums
    const int tid = threadIdx.x, nt = blockDim.x;
    for (long long r = blockIdx.x; r < M; r += gridDim.x) {
        const int t1 = top[r], t2 = second[r];
        if (t1 == t2) {                  // one group: nothing to compare
            if (tid == 0) {
                pvals[r] = 1.0;
                stat[r] = sp_kt_nan();
            }
            continue;
        }
        const uint32_t *row = counts + r * C;
        const int o1 = goff[t1], n1 = goff[t1 + 1] - o1, o2 = goff[t2], n2 = goff[t2 + 1] - o2;
        const int P1 = sp_rw_pow2(n1), P2 = sp_rw_pow2(n2), P = P1 + P2;
        for (int i = tid; i < P; i += nt) {
            const bool first = i < P1;
            const int j = first ? i : i - P1;
            double v = __longlong_as_double(0x7ff0000000000000LL);      // +inf: the padding sorts behind every value
            if (j < (first ? n1 : n2)) {
                const int c = gchrom[(first ? o1 : o2) + j];
                v = (double)row[c] / chrom_len[c];
            }
            s_x[i] = v;
        }
        __syncthreads();
        const int half1 = P1 >> 1, nc = half1 + (P2 >> 1), Pmax = P1 > P2 ? P1 : P2;
        for (int k = 2; k <= Pmax; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = tid; q < nc; q += nt) {
                    const bool first = q < half1;
                    if (k > (first ? P1 : P2)) continue;
                    const int c = first ? q : q - half1;
                    const int lo = (first ? 0 : P1) + (((c & ~(j - 1)) << 1) | (c & (j - 1))), hi = lo + j;
                    const bool up = ((first ? lo : lo - P1) & k) == 0;
                    const bool flip = j < 32 && (lo & 32);
                    const double v0 = s_x[flip ? hi : lo], v1 = s_x[flip ? lo : hi];
                    const double a = flip ? v1 : v0, b = flip ? v0 : v1;
                    if ((a > b) == up) {
                        s_x[lo] = b;
                        s_x[hi] = a;
                    }
                }
                __syncthreads();
            }
        const rw_seg A{s_x}, B{s_x + P1};
        long long s1 = 0, s2 = 0, t = 0;
        for (int i = tid; i < P; i += nt) {
            const bool first = i < P1;
            if ((first ? i : i - P1) >= (first ? n1 : n2)) continue;
            int lt, eq;
            sp_rw_rank_one(A, P1, B, P2, s_x[i], &lt, &eq);
            const long long r2 = 2LL * lt + eq + 1;
            if (first) s1 += r2;
            else s2 += r2;
            t += (long long)eq * eq - 1;
        }
        s1 = rw_wave_sum(s1);
        s2 = rw_wave_sum(s2);
        t = rw_wave_sum(t);
        __syncthreads();                 // every search has read the segments: their memory takes the waves' sums
        long long *red = (long long *)s_x;
        const int wave = tid / SP_WAVE, nw = nt / SP_WAVE;
        if (tid % SP_WAVE == 0) {
            red[wave * 3] = s1;
            red[wave * 3 + 1] = s2;
            red[wave * 3 + 2] = t;
        }
        __syncthreads();
        if (tid == 0) {
            long long S1 = 0, S2 = 0, T = 0;
            for (int w = 0; w < nw; w++) {
                S1 += red[w * 3];
                S2 += red[w * 3 + 1];
                T += red[w * 3 + 2];
            }
            const double *tab = nullptr;
            if (method == SP_RW_MWU && sp_rw_exact_sizes(n1, n2)) {
                const long long off = sf_off[sp_rw_sf_slot(n1, n2)];
                if (off >= 0) tab = sf + off;
            }
            double st;
            pvals[r] = sp_rw_stat(n1, n2, method, S1, S2, T, tab, &st);
            stat[r] = st;
        }
        __syncthreads();                 // the next row's values overwrite the sums
    }
}

extern "C" int sp_kmer_ranktest_wide(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                                     const int32_t *group_off, const int32_t *group_chrom, int method, int32_t *top,
                                     int32_t *second, double *pvals, double *means, double *stat) {
    sp_kt_call k{ctx, "sp_kmer_ranktest_wide", counts, M, C, lengths, n_groups, group_off, group_chrom, top, second, pvals, means, stat};
    if (method != SP_RW_KRUSKAL && method != SP_RW_MWU)
        return sp_fail(ctx, SP_EINVAL, "%s: method %d (0 kruskal, 1 mannwhitneyu)", k.who, method);
    int rc = sp_kt_check_groups(k, SP_RW_MAXG, SP_EINVAL);
    if (!rc) rc = sp_kt_check_lengths(k);
    if (rc || M == 0) return rc;
    int biggest = 0, next = 0;           // the two largest groups: the most LDS a row can need
    std::map<int, int> sizes;            // size -> groups of that size
    for (int g = 0; g < n_groups; g++) {
        const int n = group_off[g + 1] - group_off[g];
        sizes[n]++;
        if (n > biggest) { next = biggest; biggest = n; }
        else if (n > next) next = n;
    }
    // the exact Mann-Whitney tables of the distinct size pairs this call can meet that have one
    std::vector<long long> h_off;
    std::vector<double> h_sf;
    if (method == SP_RW_MWU) {
        h_off.assign((size_t)SP_RW_SF_SLOTS, -1);
        std::vector<sp_rw_u128> work;
        for (auto a = sizes.begin(); a != sizes.end() && a->first <= SP_RW_EXACT_MAX; ++a)
            for (auto b = a; b != sizes.end(); ++b) {
                if (b == a && a->second < 2) continue;
                const int n1 = a->first, n2 = b->first;
                const size_t at = h_sf.size(), len = (size_t)n1 * (size_t)n2 + 1;
                h_off[(size_t)sp_rw_sf_slot(n1, n2)] = (long long)at;
                h_sf.resize(at + len);
                work.resize(len);
                sp_rw_exact_table(n1, n2, work.data(), h_sf.data() + at);
            }
    }
    sp_tw_plan plan;
    rc = sp_tw_means_plan(ctx, k.who, n_groups, group_off, plan);
    if (rc) return rc;
    int *d_poff;
    uint8_t *d_prog;
    long long *d_sfoff;
    double *d_sf;
    rc = sp_kt_begin(k, true, [&](sp_carve &cv) {
        d_poff = cv.take<int>(plan.poff.size());
        d_prog = cv.take<uint8_t>(plan.prog.size());
        d_sfoff = cv.take<long long>(h_off.size() ? h_off.size() : 1);
        d_sf = cv.take<double>(h_sf.size() ? h_sf.size() : 1);
    });
    if (rc) return rc;
    if (h_off.size()) SP_HIP(ctx, hipMemcpyAsync(d_sfoff, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (h_sf.size()) SP_HIP(ctx, hipMemcpyAsync(d_sf, h_sf.data(), h_sf.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = sp_tw_means_launch(ctx, plan, d_poff, d_prog, k.rows, M, C, k.d.len, n_groups, k.d.goff, k.d.gch, k.d.top, k.d.sec, k.d.means);
    if (rc) return rc;
    const int P = n_groups > 1 ? sp_rw_pow2(biggest) + sp_rw_pow2(next) : 0;      // a group alone is never ranked
    int threads = P / SP_RW_PER_THREAD;
    threads = threads < SP_RW_THREADS_MIN ? SP_RW_THREADS_MIN : threads > SP_RW_THREADS_MAX ? SP_RW_THREADS_MAX : threads;
    threads = (threads + SP_WAVE - 1) / SP_WAVE * SP_WAVE;      // a share of 2^a + 2^b need not be a whole number of waves
    const size_t lds = (size_t)P * 8 > SP_RW_LDS_MIN ? (size_t)P * 8 : SP_RW_LDS_MIN;      // <= 64 KiB
    const int64_t grid = M < 0x7fffffffLL ? M : 0x7fffffffLL;
    SP_LAUNCH(ctx, "k7_ranktest_wide", k7_ranktest_wide, dim3((unsigned)grid), dim3((unsigned)threads), lds, k.rows, (long long)M, C,
              (const double *)k.d.len, (const int *)k.d.goff, (const int *)k.d.gch, method, (const long long *)d_sfoff,
              (const double *)d_sf, (const int *)k.d.top, (const int *)k.d.sec, k.d.p, k.d.stat);
    return sp_kt_finish(k);
}
