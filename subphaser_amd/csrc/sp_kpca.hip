// sp_kpca.hip -- the passes of the k-mer PCA (Cluster.pca) over the M x C count rows, on the device.
//
// sklearn's PCA of the C x M Z-score matrix needs the C x C Gram matrix G = Z Z^T and, for the component signs, the row of
// largest |u_j^T z| per component; the eigen-decomposition in between is C x C work on the host.  Z is never materialised:
// every pass recomputes z from the uint32 counts, the lengths and the row's (mean, sd), as sp_kpca.h defines them.
//   kp_rowstats   a thread per row, 256 rows per workgroup; the counts pass through an LDS tile of 256 x SP_KP_COLS so
//                 that global reads run along the rows while every thread walks ITS row left to right (the tile's odd
//                 pitch keeps the 256 rows on different banks).  Writes (mean, sd) per row and counts the bad rows
//                 (an integer count: one atomic per wave).
//   kp_gram       a workgroup owns one lower-triangle tile of SP_KP_T x SP_KP_T chromosome pairs and one chunk of
//                 SP_KP_ROWS rows.  It stages the z values of its two chromosome ranges SP_KP_RB rows at a time in LDS
//                 (one range on a diagonal tile) and every thread keeps its 2 x 2 pairs (a = ty + 16 i, b = tx + 16 j) in
//                 registers across the chunk, adding the rows in order.  One partial per pair per chunk: no atomics and
//                 no MFMA, whose order of addition is not ours to state.
//   kp_gram_sum   a thread per pair adds the chunk partials in chunk order and mirrors the triangle.
//   kp_signs<NC>  a thread per row as in kp_rowstats, up to NC projections in registers, U staged beside the counts
//                 SP_KP_COLS rows of it at a time; per component the workgroup reduces to its best row by sp_kp_better
//                 (shuffles in the wave, LDS across the four waves) and writes one candidate per component.
//   kp_signs_final  a workgroup per component reduces the candidates.
// Resources per instance (`make resources`) are in profiles/kpca_notes.md.
#include "sp_common.h"
#include "sp_kpca.h"

#define SP_KP_THREADS 256
#define SP_KP_COLS 32                 // columns staged per step of the row-walking kernels
#define SP_KP_PITCH (SP_KP_COLS + 1)  // odd: thread r reads [r][c], consecutive rows on consecutive banks
#define SP_KP_T 32                    // chromosomes per side of a Gram tile
#define SP_KP_RB 32                   // rows staged per step of kp_gram
#define SP_KP_LD (SP_KP_T + 1)        // pitch of a staged row in doubles, padded as kb_bootstrap's tile is

// counts[row0 .. row0 + nrows)[c0 .. c0 + nc) -> tile[r * SP_KP_PITCH + c], consecutive threads along a row
__device__ __forceinline__ void kp_stage_counts(const uint32_t *__restrict__ counts, int C, long long row0, int nrows, int c0,
                                                int nc, uint32_t *tile) {
    for (int e = threadIdx.x; e < nrows * nc; e += SP_KP_THREADS) {
        const int r = e / nc, c = e - r * nc;
        tile[r * SP_KP_PITCH + c] = counts[(row0 + r) * (long long)C + c0 + c];
    }
}

__global__ void __launch_bounds__(SP_KP_THREADS)
kp_rowstats(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ len,
            double *__restrict__ stats, unsigned long long *__restrict__ n_bad) {
    __shared__ uint32_t s_tile[SP_KP_THREADS * SP_KP_PITCH];
    __shared__ double s_len[SP_KP_COLS];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * SP_KP_THREADS;
    const int nrows = (int)min((long long)SP_KP_THREADS, M - row0);
    double sum = 0.0, ss = 0.0, mean = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        for (int c0 = 0; c0 < C; c0 += SP_KP_COLS) {
            const int nc = min(SP_KP_COLS, C - c0);
            __syncthreads();     // the previous step has been read
            kp_stage_counts(counts, C, row0, nrows, c0, nc, s_tile);
            if (tid < nc) s_len[tid] = len[c0 + tid];
            __syncthreads();
            if (tid < nrows) {
                const uint32_t *row = s_tile + tid * SP_KP_PITCH;
                if (pass == 0)
                    for (int c = 0; c < nc; c++) sum += sp_kp_x(row[c], s_len[c]);
                else
                    for (int c = 0; c < nc; c++) ss += sp_kp_dev2(sp_kp_x(row[c], s_len[c]), mean);
            }
        }
        if (pass == 0) mean = sp_kp_mean(sum, C);
    }
    bool bad = false;
    if (tid < nrows) {
        const double sd = sp_kp_sd(ss, C);
        stats[2 * (row0 + tid)] = mean;
        stats[2 * (row0 + tid) + 1] = sd;
        bad = sp_kp_bad(mean, sd);
    }
    const unsigned long long b = __ballot(bad);
    if ((tid & 63) == 0 && b) atomicAdd(n_bad, (unsigned long long)__popcll(b));
}

__global__ void __launch_bounds__(SP_KP_THREADS)
kp_gram(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ len,
        const double *__restrict__ stats, double *__restrict__ partial) {
    __shared__ double s_z[2][SP_KP_RB * SP_KP_LD];
    __shared__ int s_bad[SP_KP_RB];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // tile pair blockIdx.y = ta (ta + 1) / 2 + tb, tb <= ta
    int ta = (int)((sqrtf(8.0f * (float)blockIdx.y + 1.0f) - 1.0f) * 0.5f);
    while (ta * (ta + 1) / 2 > (int)blockIdx.y) ta--;
    while ((ta + 1) * (ta + 2) / 2 <= (int)blockIdx.y) ta++;
    const int tb = (int)blockIdx.y - ta * (ta + 1) / 2;
    const bool diag = ta == tb;
    const int a0 = ta * SP_KP_T, b0 = tb * SP_KP_T;
    const int na = min(SP_KP_T, C - a0), nb = min(SP_KP_T, C - b0);
    const long long chunk = blockIdx.x;
    const long long row_lo = chunk * SP_KP_ROWS, row_hi = min(M, row_lo + SP_KP_ROWS);
    const double *A = s_z[0], *B = diag ? s_z[0] : s_z[1];
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (long long r0 = row_lo; r0 < row_hi; r0 += SP_KP_RB) {
        const int nr = (int)min((long long)SP_KP_RB, row_hi - r0);
        __syncthreads();     // the previous block has been read
        for (int e = tid; e < SP_KP_RB * SP_KP_T; e += SP_KP_THREADS) {
            const int r = e / SP_KP_T, c = e - r * SP_KP_T;
            double za = 0.0, zb = 0.0;
            if (r < nr) {
                const long long row = r0 + r;
                const double mean = stats[2 * row], sd = stats[2 * row + 1];
                const bool bad = sp_kp_bad(mean, sd);
                if (c == 0) s_bad[r] = bad;
                if (!bad) {
                    if (c < na) za = sp_kp_z(counts[row * (long long)C + a0 + c], len[a0 + c], mean, sd);
                    if (!diag && c < nb) zb = sp_kp_z(counts[row * (long long)C + b0 + c], len[b0 + c], mean, sd);
                }
            }
            s_z[0][r * SP_KP_LD + c] = za;
            if (!diag) s_z[1][r * SP_KP_LD + c] = zb;
        }
        __syncthreads();
        for (int r = 0; r < nr; r++) {
            if (s_bad[r]) continue;     // the same row for every thread: uniform
            const double al = A[r * SP_KP_LD + ty], ah = A[r * SP_KP_LD + ty + 16];
            const double bl = B[r * SP_KP_LD + tx], bh = B[r * SP_KP_LD + tx + 16];
            acc[0][0] += al * bl;
            acc[0][1] += al * bh;
            acc[1][0] += ah * bl;
            acc[1][1] += ah * bh;
        }
    }
    const long long P = sp_kp_tri(C - 1, C - 1) + 1;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) {
            const int a = a0 + ty + 16 * i, b = b0 + tx + 16 * j;
            if (a < C && b <= a) partial[chunk * P + sp_kp_tri(a, b)] = acc[i][j];
        }
}

__global__ void __launch_bounds__(SP_KP_THREADS)
kp_gram_sum(const double *__restrict__ partial, long long n_chunks, int C, double *__restrict__ gram) {
    const long long P = sp_kp_tri(C - 1, C - 1) + 1;
    const long long p = (long long)blockIdx.x * SP_KP_THREADS + threadIdx.x;
    if (p >= P) return;
    int a = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    while (sp_kp_tri(a, 0) > p) a--;
    while (sp_kp_tri(a + 1, 0) <= p) a++;
    const int b = (int)(p - sp_kp_tri(a, 0));
    double s = 0.0;
    for (long long k = 0; k < n_chunks; k++) s += partial[k * P + p];
    gram[(long long)a * C + b] = s;
    gram[(long long)b * C + a] = s;
}

struct kp_cand {
    double ab;          // |v|, or -1: no row
    long long row;
    double v;
};
__device__ __forceinline__ void kp_take(kp_cand &x, const kp_cand &o) {
    if (sp_kp_better(o.ab, o.row, x.ab, x.row)) x = o;
}
// the best candidate of the workgroup, valid on thread 0.  s_red: SP_KP_THREADS / 64 entries
__device__ __forceinline__ kp_cand kp_block_best(kp_cand x, kp_cand *s_red) {
    for (int off = 32; off; off >>= 1) {
        kp_cand o;
        o.ab = __shfl_down(x.ab, off);
        o.row = __shfl_down(x.row, off);
        o.v = __shfl_down(x.v, off);
        kp_take(x, o);
    }
    __syncthreads();     // s_red is free again
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < SP_KP_THREADS / 64; w++) kp_take(x, s_red[w]);
    return x;
}

template <int NC>
__global__ void __launch_bounds__(SP_KP_THREADS)
kp_signs(const uint32_t *__restrict__ counts, long long M, int C, const double *__restrict__ len,
         const double *__restrict__ stats, const double *__restrict__ U, int n_comp, long long *__restrict__ cand_row,
         double *__restrict__ cand_val) {
    __shared__ uint32_t s_tile[SP_KP_THREADS * SP_KP_PITCH];
    __shared__ double s_len[SP_KP_COLS];
    __shared__ double s_U[SP_KP_COLS * NC];
    __shared__ kp_cand s_red[SP_KP_THREADS / 64];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * SP_KP_THREADS;
    const int nrows = (int)min((long long)SP_KP_THREADS, M - row0);
    double mean = 0.0, sd = 0.0;
    bool good = false;
    if (tid < nrows) {
        mean = stats[2 * (row0 + tid)];
        sd = stats[2 * (row0 + tid) + 1];
        good = !sp_kp_bad(mean, sd);
    }
    double v[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) v[j] = 0.0;
    for (int c0 = 0; c0 < C; c0 += SP_KP_COLS) {
        const int nc = min(SP_KP_COLS, C - c0);
        __syncthreads();     // the previous step has been read
        kp_stage_counts(counts, C, row0, nrows, c0, nc, s_tile);
        if (tid < nc) s_len[tid] = len[c0 + tid];
        for (int e = tid; e < nc * NC; e += SP_KP_THREADS) {
            const int c = e / NC, j = e - c * NC;
            s_U[e] = j < n_comp ? U[(long long)(c0 + c) * n_comp + j] : 0.0;
        }
        __syncthreads();
        if (good) {
            const uint32_t *row = s_tile + tid * SP_KP_PITCH;
            for (int c = 0; c < nc; c++) {
                const double z = sp_kp_z(row[c], s_len[c], mean, sd);
#pragma unroll
                for (int j = 0; j < NC; j++) v[j] += s_U[c * NC + j] * z;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NC; j++) {
        if (j < n_comp) {     // uniform; no break: the loop has to unroll for v to stay in registers
            kp_cand x;
            x.ab = good ? fabs(v[j]) : -1.0;
            x.row = good ? row0 + tid : LLONG_MAX;
            x.v = v[j];
            x = kp_block_best(x, s_red);
            if (tid == 0) {
                cand_row[(long long)blockIdx.x * n_comp + j] = x.row;
                cand_val[(long long)blockIdx.x * n_comp + j] = x.ab < 0.0 ? NAN : x.v;     // NaN marks "no good row in this block"
            }
        }
    }
}

__global__ void __launch_bounds__(SP_KP_THREADS)
kp_signs_final(const long long *__restrict__ cand_row, const double *__restrict__ cand_val, long long n_blocks, int n_comp,
               long long *__restrict__ rows, double *__restrict__ vals) {
    __shared__ kp_cand s_red[SP_KP_THREADS / 64];
    const int j = blockIdx.x;
    kp_cand x{-1.0, LLONG_MAX, 0.0};
    for (long long k = threadIdx.x; k < n_blocks; k += SP_KP_THREADS) {
        const double v = cand_val[k * n_comp + j];
        if (v != v) continue;
        kp_take(x, kp_cand{fabs(v), cand_row[k * n_comp + j], v});
    }
    x = kp_block_best(x, s_red);
    if (threadIdx.x == 0) {
        rows[j] = x.ab < 0.0 ? -1 : x.row;
        vals[j] = x.ab < 0.0 ? 0.0 : x.v;
    }
}

// ---------------------------------------------------------------- host side
namespace {
// arguments both entries check
int kp_check(sp_ctx *ctx, const char *who, const uint32_t *counts, int64_t M, int C, const int64_t *lengths) {
    if (!ctx || !counts || !lengths) return sp_fail(ctx, SP_EINVAL, "%s: bad arguments", who);
    if (M < 1) return sp_fail(ctx, SP_EINVAL, "%s: %lld rows", who, (long long)M);
    if (C < 2) return sp_fail(ctx, SP_EINVAL, "%s: %d chromosomes (a PCA needs two)", who, C);
    if (C > SP_KP_MAXC) return sp_fail(ctx, SP_EUNSUP, "%s: %d chromosomes (up to %d supported)", who, C, SP_KP_MAXC);
    for (int c = 0; c < C; c++)
        if (lengths[c] <= 0) return sp_fail(ctx, SP_EINVAL, "%s: chromosome %d has length %lld", who, c, (long long)lengths[c]);
    return SP_OK;
}
// rows that already live on this device are read in place, as in sp_kmer_ttest; host rows are uploaded into `up`
int kp_rows(sp_ctx *ctx, const char *who, const uint32_t *counts, int64_t M, int C, sp_tmp<uint32_t> &up, const uint32_t **out) {
    if (sp_on_device(ctx, counts)) {
        *out = counts;
        return SP_OK;
    }
    const size_t n = (size_t)M * (size_t)C;
    const hipError_t e = up.alloc(n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "%s: the %lld x %d rows, %lld bytes, do not fit on the device (%s)",
                       who, (long long)M, C, (long long)(n * 4), hipGetErrorString(e));
    }
    SP_HIP(ctx, hipMemcpyAsync(up.p, counts, n * 4, hipMemcpyHostToDevice, ctx->stream));
    *out = up.p;
    return SP_OK;
}
int kp_launch_stats(sp_ctx *ctx, const uint32_t *d_counts, int64_t M, int C, const double *d_len, double *d_stats,
                    unsigned long long *d_bad) {
    SP_HIP(ctx, hipMemsetAsync(d_bad, 0, 8, ctx->stream));
    SP_LAUNCH(ctx, "kp_rowstats", kp_rowstats, dim3((unsigned)((M + SP_KP_THREADS - 1) / SP_KP_THREADS)), dim3(SP_KP_THREADS), 0,
              d_counts, (long long)M, C, d_len, d_stats, d_bad);
    return SP_OK;
}
}  // namespace

extern "C" int sp_kmer_pca_gram(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, double *gram,
                                int64_t *n_bad, double *stats) {
    int rc = kp_check(ctx, "sp_kmer_pca_gram", counts, M, C, lengths);
    if (rc) return rc;
    if (!gram || !n_bad) return sp_fail(ctx, SP_EINVAL, "sp_kmer_pca_gram: bad arguments");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n_chunks = sp_kp_chunks(M), P = sp_kp_tri(C - 1, C - 1) + 1;
    const int n_tiles = (C + SP_KP_T - 1) / SP_KP_T, n_tpairs = n_tiles * (n_tiles + 1) / 2;
    auto layout = [&](sp_carve &cv, double *&d_len, double *&d_stats, double *&d_part, double *&d_gram, unsigned long long *&d_bad) {
        d_len = cv.take<double>((size_t)C);
        d_stats = cv.take<double>((size_t)M * 2);
        d_part = cv.take<double>((size_t)n_chunks * (size_t)P);
        d_gram = cv.take<double>((size_t)C * C);
        d_bad = cv.take<unsigned long long>(1);
    };
    double *d_len, *d_stats, *d_part, *d_gram;
    unsigned long long *d_bad;
    sp_carve sizes;
    layout(sizes, d_len, d_stats, d_part, d_gram, d_bad);
    rc = sp_buf_ensure(ctx, ctx->b_kp, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_kmer_pca_gram: a workspace of %lld bytes (%lld chunks x %lld pairs x 8 and %lld rows x 16) does not fit on the device",
                       (long long)sizes.off, (long long)n_chunks, (long long)P, (long long)M);
    if (rc) return rc;
    sp_carve cv(ctx->b_kp.p);
    layout(cv, d_len, d_stats, d_part, d_gram, d_bad);
    sp_tmp<uint32_t> up;     // the upload of host rows, released on every return
    const uint32_t *d_counts;
    rc = kp_rows(ctx, "sp_kmer_pca_gram", counts, M, C, up, &d_counts);
    if (rc) return rc;
    std::vector<double> hl((size_t)C);
    for (int c = 0; c < C; c++) hl[(size_t)c] = (double)lengths[c];
    SP_HIP(ctx, hipMemcpyAsync(d_len, hl.data(), (size_t)C * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = kp_launch_stats(ctx, d_counts, M, C, d_len, d_stats, d_bad);
    if (rc) return rc;
    SP_LAUNCH(ctx, "kp_gram", kp_gram, dim3((unsigned)n_chunks, (unsigned)n_tpairs), dim3(SP_KP_THREADS), 0, d_counts, (long long)M,
              C, (const double *)d_len, (const double *)d_stats, d_part);
    SP_LAUNCH(ctx, "kp_gram_sum", kp_gram_sum, dim3((unsigned)((P + SP_KP_THREADS - 1) / SP_KP_THREADS)), dim3(SP_KP_THREADS), 0,
              (const double *)d_part, (long long)n_chunks, C, d_gram);
    unsigned long long h_bad = 0;
    SP_HIP(ctx, hipMemcpyAsync(gram, d_gram, (size_t)C * C * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (stats) SP_HIP(ctx, hipMemcpyAsync(stats, d_stats, (size_t)M * 16, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_bad = (int64_t)h_bad;
    return SP_OK;
}

extern "C" int sp_kmer_pca_signs(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, const double *U,
                                 int n_comp, int64_t *rows, double *vals) {
    int rc = kp_check(ctx, "sp_kmer_pca_signs", counts, M, C, lengths);
    if (rc) return rc;
    if (!U || !rows || !vals) return sp_fail(ctx, SP_EINVAL, "sp_kmer_pca_signs: bad arguments");
    if (n_comp < 1 || n_comp > SP_KP_MAXCOMP)
        return sp_fail(ctx, SP_EINVAL, "sp_kmer_pca_signs: %d components (1..%d)", n_comp, SP_KP_MAXCOMP);
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n_blocks = (M + SP_KP_THREADS - 1) / SP_KP_THREADS;
    auto layout = [&](sp_carve &cv, double *&d_len, double *&d_stats, double *&d_U, long long *&d_crow, double *&d_cval,
                      long long *&d_rows, double *&d_vals, unsigned long long *&d_bad) {
        d_len = cv.take<double>((size_t)C);
        d_stats = cv.take<double>((size_t)M * 2);
        d_U = cv.take<double>((size_t)C * n_comp);
        d_crow = cv.take<long long>((size_t)n_blocks * n_comp);
        d_cval = cv.take<double>((size_t)n_blocks * n_comp);
        d_rows = cv.take<long long>((size_t)n_comp);
        d_vals = cv.take<double>((size_t)n_comp);
        d_bad = cv.take<unsigned long long>(1);
    };
    double *d_len, *d_stats, *d_U, *d_cval, *d_vals;
    long long *d_crow, *d_rows;
    unsigned long long *d_bad;
    sp_carve sizes;
    layout(sizes, d_len, d_stats, d_U, d_crow, d_cval, d_rows, d_vals, d_bad);
    rc = sp_buf_ensure(ctx, ctx->b_kp, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_kmer_pca_signs: a workspace of %lld bytes (%lld rows, %d components) does not fit on the device",
                       (long long)sizes.off, (long long)M, n_comp);
    if (rc) return rc;
    sp_carve cv(ctx->b_kp.p);
    layout(cv, d_len, d_stats, d_U, d_crow, d_cval, d_rows, d_vals, d_bad);
    sp_tmp<uint32_t> up;
    const uint32_t *d_counts;
    rc = kp_rows(ctx, "sp_kmer_pca_signs", counts, M, C, up, &d_counts);
    if (rc) return rc;
    std::vector<double> hl((size_t)C);
    for (int c = 0; c < C; c++) hl[(size_t)c] = (double)lengths[c];
    SP_HIP(ctx, hipMemcpyAsync(d_len, hl.data(), (size_t)C * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_U, U, (size_t)C * n_comp * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = kp_launch_stats(ctx, d_counts, M, C, d_len, d_stats, d_bad);     // recomputed: the call stands alone
    if (rc) return rc;
    const dim3 grid((unsigned)n_blocks), block(SP_KP_THREADS);
    if (n_comp <= 4)
        SP_LAUNCH(ctx, "kp_signs", kp_signs<4>, grid, block, 0, d_counts, (long long)M, C, (const double *)d_len,
                  (const double *)d_stats, (const double *)d_U, n_comp, d_crow, d_cval);
    else
        SP_LAUNCH(ctx, "kp_signs", kp_signs<SP_KP_MAXCOMP>, grid, block, 0, d_counts, (long long)M, C, (const double *)d_len,
                  (const double *)d_stats, (const double *)d_U, n_comp, d_crow, d_cval);
    SP_LAUNCH(ctx, "kp_signs_final", kp_signs_final, dim3((unsigned)n_comp), block, 0, (const long long *)d_crow,
              (const double *)d_cval, (long long)n_blocks, n_comp, d_rows, d_vals);
    static_assert(sizeof(long long) == sizeof(int64_t), "rows are copied out as they are");
    SP_HIP(ctx, hipMemcpyAsync(rows, d_rows, (size_t)n_comp * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(vals, d_vals, (size_t)n_comp * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}
