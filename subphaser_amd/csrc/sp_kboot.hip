// sp_kboot.hip -- the k-means bootstrap of Cluster.bootstrap on the device: one workgroup per replicate.
//
// A replicate is a k-means fit on n columns of the C x M Z-score matrix drawn with replacement.  k-means on C points
// needs only their C x C Gram matrix over those columns, so the workgroup
//   1. gathers its columns SP_KB_TILE at a time into an LDS tile and accumulates G, one lane per pair (a, b <= a), in
//      draw order (product rounded, then added: bit-defined, the numpy twin is `for t: G += outer(z_t, z_t)`);
//   2. runs greedy k-means++ and Lloyd from sp_kboot.h on the LDS Gram, a lane per point / cluster / trial, the serial
//      sums (potential, running sum, cluster totals) on one lane each in the order the header states.
// G is kept as its symmetric half (66 KB at C = 128); the tile's LDS holds the K x C member sums afterwards.  Three
// instances by C (<= 32, <= 64, <= 128) so that the usual two dozen chromosomes do not pay the LDS of 128:
//   MAXC   LDS         VGPRs   scratch   workgroups of 256 per CU
//    32     13680 B    41      0         8 (the wave limit)
//    64     34928 B    41      0         4
//   128    102000 B    50      0         1
// (`make resources`).  The gather is one 8-byte read per (chromosome, column): the rows of z are M * 8 bytes apart, so
// nothing coalesces, and a replicate's time at C = 21 is the latency of its n / 32 chunks; 1000 replicates are resident
// at once.
#include "sp_common.h"
#include "sp_kboot.h"

#define SP_KB_THREADS 256
#define SP_KB_LD (SP_KB_TILE + 1)     // tile row stride in doubles: odd, rows a and a + 1 start on different banks

template <int MAXC>
__global__ void __launch_bounds__(SP_KB_THREADS)
kb_bootstrap(const double *__restrict__ z, int C, long long M, const long long *__restrict__ cols, int n, int K,
             unsigned long long seed, int *__restrict__ labels, int *__restrict__ iters, double *__restrict__ gram) {
    static_assert(MAXC * SP_KB_LD >= SP_KB_MAXK * MAXC, "the member sums reuse the tile");
    __shared__ double s_g[MAXC * (MAXC + 1) / 2];
    __shared__ double s_tile[MAXC * SP_KB_LD];
    __shared__ double s_closest[MAXC], s_T[SP_KB_MAXK], s_newpot[SP_KB_MAXTRIALS], s_pot;
    __shared__ int s_lab[MAXC], s_centre[SP_KB_MAXK], s_cnt[SP_KB_MAXK], s_cand[SP_KB_MAXTRIALS], s_changed;
    const int tid = threadIdx.x;
    const unsigned long long rep = blockIdx.x;
    const long long *mycols = cols + rep * (unsigned long long)n;
    const int P = C * (C + 1) / 2;

    // ---- phase 1: Gram
    for (int t0 = 0; t0 < n; t0 += SP_KB_TILE) {
        const int nt = min(SP_KB_TILE, n - t0);
        __syncthreads();     // the previous chunk has been read
        for (int e = tid; e < C * nt; e += SP_KB_THREADS) {
            const int c = e / nt, t = e - c * nt;
            s_tile[c * SP_KB_LD + t] = z[(long long)c * M + mycols[t0 + t]];
        }
        __syncthreads();
        for (int p = tid; p < P; p += SP_KB_THREADS) {
            int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
            while (a * (a + 1) / 2 > p) a--;
            while ((a + 1) * (a + 2) / 2 <= p) a++;
            const int b = p - a * (a + 1) / 2;
            const double *za = s_tile + a * SP_KB_LD, *zb = s_tile + b * SP_KB_LD;
            double acc = t0 ? s_g[p] : 0.0;
            for (int t = 0; t < nt; t++) acc += za[t] * zb[t];
            s_g[p] = acc;
        }
    }
    __syncthreads();
    const sp_kb_half G{s_g};
    if (gram)
        for (int e = tid; e < C * C; e += SP_KB_THREADS) gram[rep * (unsigned long long)(C * C) + e] = G(e / C, e % C);

    // ---- phase 2: k-means++ on the Gram
    double *s_S = s_tile;     // [K][C]
    const int trials = sp_kb_trials(K);
    if (tid == 0) s_centre[0] = sp_kb_first_centre(seed, rep, C);
    __syncthreads();
    if (tid < C) s_closest[tid] = sp_kb_d2(G, s_centre[0], tid);
    __syncthreads();
    if (tid == 0) s_pot = sp_kb_potential(s_closest, C);
    __syncthreads();
    for (int c = 1; c < K; c++) {
        if (tid < trials)
            sp_kb_trial(G, C, s_closest, s_pot, sp_kb_u(seed, rep, 1 + (unsigned long long)(c - 1) * trials + tid),
                        &s_cand[tid], &s_newpot[tid]);
        __syncthreads();
        if (tid == 0) {
            const int b = sp_kb_best_trial(s_newpot, trials);
            s_centre[c] = s_cand[b];
            s_pot = s_newpot[b];
        }
        __syncthreads();
        if (tid < C) s_closest[tid] = sp_kb_closer(G, s_centre[c], tid, s_closest[tid]);
        __syncthreads();
    }
    if (tid < C) s_lab[tid] = sp_kb_nearest_centre(G, K, s_centre, tid);
    __syncthreads();

    // ---- Lloyd
    int it = 0;
    for (;;) {
        it++;
        if (tid == 0) s_changed = 0;
        if (tid < C) sp_kb_point_sums(G, C, K, s_lab, tid, s_S, C);
        __syncthreads();
        if (tid < K) s_cnt[tid] = sp_kb_cluster_total(C, s_lab, tid, s_S, C, &s_T[tid]);
        __syncthreads();
        int next = 0;
        if (tid < C) {
            next = sp_kb_point_assign(G, K, tid, s_S, C, s_T, s_cnt);
            if (next != s_lab[tid]) s_changed = 1;
        }
        __syncthreads();     // every label has been read, the flag is complete
        if (tid < C) s_lab[tid] = next;
        const int changed = s_changed;
        __syncthreads();     // ... and read, before the next iteration clears it
        if (!changed || it >= SP_KB_MAXIT) break;
    }
    if (tid < C) labels[rep * (unsigned long long)C + tid] = s_lab[tid];
    if (tid == 0) iters[rep] = it;
}

extern "C" int sp_kmeans_bootstrap(sp_ctx *ctx, const double *z, int C, int64_t M, const int64_t *cols, int R, int n,
                                   int K, uint64_t seed, int32_t *labels, int32_t *iters, double *gram) {
    if (!ctx || !z || !cols || !labels || !iters || C < 1 || M < 1 || R < 0)
        return sp_fail(ctx, SP_EINVAL, "sp_kmeans_bootstrap: bad arguments");
    if (K < 1 || K > C) return sp_fail(ctx, SP_EINVAL, "sp_kmeans_bootstrap: %d clusters for %d points", K, C);
    if (n < 1) return sp_fail(ctx, SP_EINVAL, "sp_kmeans_bootstrap: %d columns per replicate", n);
    if (C > SP_KB_MAXC || K > SP_KB_MAXK)
        return sp_fail(ctx, SP_EUNSUP, "sp_kmeans_bootstrap: %d points in %d clusters (up to %d in %d supported)", C, K,
                       SP_KB_MAXC, SP_KB_MAXK);
    const size_t ncols = (size_t)R * (size_t)n;
    for (size_t i = 0; i < ncols; i++)
        if (cols[i] < 0 || cols[i] >= M)
            return sp_fail(ctx, SP_EINVAL, "sp_kmeans_bootstrap: column index %lld of replicate %lld outside [0, %lld)",
                           (long long)cols[i], (long long)(i / (size_t)n), (long long)M);
    if (R == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const bool on_device = sp_on_device(ctx, z);     // a matrix staged on this device earlier is read in place
    sp_carve sizes;
    auto layout = [&](sp_carve &cv, long long *&d_cols, int *&d_lab, int *&d_it, double *&d_gram) {
        d_cols = cv.take<long long>(ncols);
        d_lab = cv.take<int>((size_t)R * C);
        d_it = cv.take<int>((size_t)R);
        d_gram = gram ? cv.take<double>((size_t)R * C * C) : nullptr;
    };
    long long *d_cols;
    int *d_lab, *d_it;
    double *d_gram;
    layout(sizes, d_cols, d_lab, d_it, d_gram);
    int rc = sp_buf_ensure(ctx, ctx->b_kb, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_kmeans_bootstrap: a workspace of %lld bytes (%d replicates of %d columns) does not fit on the device",
                       (long long)sizes.off, R, n);
    if (rc) return rc;
    sp_carve cv(ctx->b_kb.p);
    layout(cv, d_cols, d_lab, d_it, d_gram);
    const size_t zbytes = (size_t)C * (size_t)M * 8;
    sp_tmp<double> d_z;      // the upload, released on every return
    if (!on_device) {
        const hipError_t e = d_z.alloc((size_t)C * (size_t)M);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP,
                           "sp_kmeans_bootstrap: the %d x %lld matrix, %lld bytes, does not fit on the device (%s)", C,
                           (long long)M, (long long)zbytes, hipGetErrorString(e));
        }
        SP_HIP(ctx, hipMemcpyAsync(d_z.p, z, zbytes, hipMemcpyHostToDevice, ctx->stream));
    }
    SP_HIP(ctx, hipMemcpyAsync(d_cols, cols, ncols * 8, hipMemcpyHostToDevice, ctx->stream));
    const double *zz = on_device ? z : d_z.p;
    const dim3 grid((unsigned)R), block(SP_KB_THREADS);
    if (C <= 32)
        SP_LAUNCH(ctx, "kb_bootstrap", kb_bootstrap<32>, grid, block, 0, zz, C, (long long)M, (const long long *)d_cols, n, K,
                  (unsigned long long)seed, d_lab, d_it, d_gram);
    else if (C <= 64)
        SP_LAUNCH(ctx, "kb_bootstrap", kb_bootstrap<64>, grid, block, 0, zz, C, (long long)M, (const long long *)d_cols, n, K,
                  (unsigned long long)seed, d_lab, d_it, d_gram);
    else
        SP_LAUNCH(ctx, "kb_bootstrap", kb_bootstrap<SP_KB_MAXC>, grid, block, 0, zz, C, (long long)M,
                  (const long long *)d_cols, n, K, (unsigned long long)seed, d_lab, d_it, d_gram);
    SP_HIP(ctx, hipMemcpyAsync(labels, d_lab, (size_t)R * C * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(iters, d_it, (size_t)R * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (gram) SP_HIP(ctx, hipMemcpyAsync(gram, d_gram, (size_t)R * C * C * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}
