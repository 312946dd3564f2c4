// sp_hclust.hip -- complete-linkage clustering of the heatmap's two axes (Cluster.heatmap) on the device: the P x P
// Euclidean distance matrix and the nearest-neighbour chain on it, as sp_hclust.h defines them.
//   hc_dist    a workgroup owns one SP_HC_T x SP_HC_T tile of the matrix.  It stages SP_HC_DB coordinates of its two point
//              ranges in LDS (one range on a diagonal tile; the pitch is odd, so the 16 points a wave reads lie on
//              different banks) and every thread keeps its 2 x 2 pairs (i = ty + 16 a, j = tx + 16 b) in registers while
//              it walks the coordinates left to right.  Both triangles are computed: (a - b)^2 == (b - a)^2, so they
//              agree to the bit and nothing is mirrored.  The same kernel serves many points in few dimensions
//              (10 000 x 21: 98 000 tiles of one step) and few points in many (21 x 10 000: one tile of 313 steps).
//   hc_chain   ONE workgroup of SP_HC_THREADS threads runs the whole chain.  A scan is a coalesced read of row x: thread t
//              takes columns t, t + 1024, ...; the (value, index) minimum is reduced by shuffles in the wave, through LDS
//              across the 16 waves, and thread 0 decides between push and merge.  The chain and size[] are thread 0's
//              alone (global memory); which slots are live is a bit mask in LDS.  After a merge all threads rewrite row y
//              (coalesced) and column y (one store per live row) from rows x and y -- the matrix stays symmetric, so
//              D[i][x] is read as D[x][i].  No second workgroup, no cooperative launch, no flag to wait for; the loop
//              ends after P - 1 merges, or when the scan count passes sp_hc_max_scans(P), or when a chain of one finds no
//              neighbour (status word; the entry reports SP_ESTATE).
//              Visibility of the rewritten row and column to the other waves: every store to the matrix is followed by a
//              __syncthreads() before any thread loads from it again (the barrier at the top of the next scan).
//              __syncthreads() is a workgroup-scope release + barrier + acquire: each wave waits for its own stores
//              (s_waitcnt vmcnt(0)) before it arrives, and the waves of one workgroup share their CU's write-through L1
//              (the library is not built for threadgroup-split mode), so no cache action is needed at workgroup scope.
//              The matrix is never read through a const __restrict__ pointer, so no load is hoisted over a barrier.
// Resources per kernel (`make resources`) are in profiles/heatmap_notes.md.
#include "sp_common.h"
#include "sp_hclust.h"

#include <limits.h>

#define SP_HC_DTHREADS 256
#define SP_HC_T 32                    // points per side of a distance tile
#define SP_HC_DB 32                   // coordinates staged per step
#define SP_HC_LD (SP_HC_DB + 1)       // pitch of a staged point in doubles
#define SP_HC_THREADS 1024
#define SP_HC_WAVES (SP_HC_THREADS / SP_WAVE)

__global__ void __launch_bounds__(SP_HC_DTHREADS)
hc_dist(const double *__restrict__ pts, int P, int D, double *__restrict__ dist) {
    __shared__ double s_p[2][SP_HC_T * SP_HC_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * SP_HC_T, j0 = blockIdx.x * SP_HC_T;
    const int ni = min(SP_HC_T, P - i0), nj = min(SP_HC_T, P - j0);
    const bool diag = i0 == j0;
    const double *A = s_p[0], *B = diag ? s_p[0] : s_p[1];
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int d0 = 0; d0 < D; d0 += SP_HC_DB) {
        const int nd = min(SP_HC_DB, D - d0);
        __syncthreads();     // the previous step has been read
        for (int e = tid; e < SP_HC_T * SP_HC_DB; e += SP_HC_DTHREADS) {
            const int r = e / SP_HC_DB, c = e - r * SP_HC_DB;
            double a = 0.0, b = 0.0;
            if (c < nd) {
                if (r < ni) a = pts[(long long)(i0 + r) * D + d0 + c];
                if (!diag && r < nj) b = pts[(long long)(j0 + r) * D + d0 + c];
            }
            s_p[0][r * SP_HC_LD + c] = a;
            if (!diag) s_p[1][r * SP_HC_LD + c] = b;
        }
        __syncthreads();
        for (int c = 0; c < nd; c++) {
            const double al = A[ty * SP_HC_LD + c], ah = A[(ty + 16) * SP_HC_LD + c];
            const double bl = B[tx * SP_HC_LD + c], bh = B[(tx + 16) * SP_HC_LD + c];
            acc[0][0] += sp_hc_term(al, bl);
            acc[0][1] += sp_hc_term(al, bh);
            acc[1][0] += sp_hc_term(ah, bl);
            acc[1][1] += sp_hc_term(ah, bh);
        }
    }
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < P && j < P) dist[(long long)i * P + j] = sqrt(acc[a][b]);
        }
}

// what thread 0 tells the workgroup after a scan
#define HC_PUSH 0
#define HC_MERGE 1        // rewrite row and column y, then scan on
#define HC_STOP 2         // the last merge is recorded, or the status word is set

__global__ void __launch_bounds__(SP_HC_THREADS)
hc_chain(double *D, int P, int *size, int *chain, double *merges, long long *status /* [0] status, [1] scans */) {
    __shared__ uint32_t s_live[SP_HC_MAXP / 32];
    __shared__ double s_rv[SP_HC_WAVES];
    __shared__ int s_ri[SP_HC_WAVES];
    __shared__ double s_cur;
    __shared__ int s_x, s_prev, s_op, s_mx, s_my;
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += SP_HC_THREADS) size[i] = 1;
    for (int w = tid; w < SP_HC_MAXP / 32; w += SP_HC_THREADS) {
        const int n = P - w * 32;
        s_live[w] = n >= 32 ? 0xFFFFFFFFu : n > 0 ? (1u << n) - 1u : 0u;
    }
    // thread 0's own state
    int len = 0, first = 0, done = 0;
    long long scans = 0;
    __syncthreads();     // s_live and size[] are set
    for (;;) {
        if (tid == 0) {
            if (len == 0) {
                while (first < P && !((s_live[first >> 5] >> (first & 31)) & 1u)) first++;     // slots only die: amortised O(P)
                if (first >= P) first = P - 1;     // cannot happen (two live slots remain before every merge): keeps row x in bounds
                chain[len++] = first;
            }
            s_x = chain[len - 1];
            s_prev = len > 1 ? chain[len - 2] : -1;
        }
        __syncthreads();     // s_x, s_prev; and the row and column the last merge rewrote (see the header comment)
        const int x = s_x, prev = s_prev;
        const double *row = D + (long long)x * P;
        double bv = INFINITY;
        int bi = INT_MAX;
        for (int i = tid; i < P; i += SP_HC_THREADS) {
            const double d = row[i];     // loaded whether or not slot i is live: no branch around the load
            if (i == prev) s_cur = d;    // one thread: D[x][prev], which the scan passes anyway
            const bool ok = ((s_live[i >> 5] >> (i & 31)) & 1u) && i != x;
            if (ok && sp_hc_less(d, i, bv, bi)) {
                bv = d;
                bi = i;
            }
        }
        for (int off = 32; off; off >>= 1) {
            const double ov = __shfl_down(bv, off);
            const int oi = __shfl_down(bi, off);
            if (sp_hc_less(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            s_rv[tid >> 6] = bv;
            s_ri[tid >> 6] = bi;
        }
        __syncthreads();     // the wave minima and s_cur
        if (tid == 0) {
            for (int w = 1; w < SP_HC_WAVES; w++)
                if (sp_hc_less(s_rv[w], s_ri[w], bv, bi)) {
                    bv = s_rv[w];
                    bi = s_ri[w];
                }
            const double cur = prev >= 0 ? s_cur : INFINITY;
            int op;
            scans++;
            const bool push = bi != INT_MAX && bv < cur;
            if (scans > sp_hc_max_scans(P) || (push && len >= P)) {     // a push finds len < P: the chain holds live slots, each once
                status[0] = SP_HC_SCANS;
                op = HC_STOP;
            } else if (push) {
                chain[len++] = bi;
                op = HC_PUSH;
            } else if (prev < 0) {
                status[0] = SP_HC_NONE;
                op = HC_STOP;
            } else {
                len -= 2;
                const int a = min(x, prev), b = max(x, prev);
                const int na = size[a], nb = size[b];
                double *m = merges + 4 * (long long)done;
                m[0] = (double)a;
                m[1] = (double)b;
                m[2] = cur;
                m[3] = (double)(na + nb);
                size[a] = 0;
                size[b] = na + nb;
                s_live[a >> 5] &= ~(1u << (a & 31));
                s_mx = a;
                s_my = b;
                done++;
                op = done == P - 1 ? HC_STOP : HC_MERGE;
            }
            if (op == HC_STOP) status[1] = scans;
            s_op = op;
        }
        __syncthreads();     // s_op, s_mx, s_my, s_live
        const int op = s_op;
        if (op == HC_STOP) break;
        if (op == HC_MERGE) {
            const int mx = s_mx, my = s_my;
            const double *rx = D + (long long)mx * P;
            double *ry = D + (long long)my * P;
            for (int i = tid; i < P; i += SP_HC_THREADS) {
                const double v = sp_hc_max(rx[i], ry[i]);
                if (((s_live[i >> 5] >> (i & 31)) & 1u) && i != my) {
                    ry[i] = v;
                    D[(long long)i * P + my] = v;
                }
            }
        }
    }
}

extern "C" int sp_hclust_complete(sp_ctx *ctx, const double *pts, int P, int D, double *merges, double *dist) {
    if (!ctx || !pts || !merges) return sp_fail(ctx, SP_EINVAL, "sp_hclust_complete: bad arguments");
    if (P < 2 || D < 1) return sp_fail(ctx, SP_EINVAL, "sp_hclust_complete: %d points in %d dimensions (2 and 1 at least)", P, D);
    if (P > SP_HC_MAXP)
        return sp_fail(ctx, SP_EUNSUP, "sp_hclust_complete: %d points (up to %d supported)", P, SP_HC_MAXP);
    const size_t n_pts = (size_t)P * (size_t)D;
    for (size_t i = 0; i < n_pts; i++)
        if (!isfinite(pts[i]))
            return sp_fail(ctx, SP_EINVAL, "sp_hclust_complete: coordinate %d of point %lld is not finite", (int)(i % (size_t)D),
                           (long long)(i / (size_t)D));
    SP_HIP(ctx, hipSetDevice(ctx->device));
    auto layout = [&](sp_carve &cv, double *&d_pts, double *&d_dist, double *&d_merges, int *&d_size, int *&d_chain, long long *&d_status) {
        d_pts = cv.take<double>(n_pts);
        d_dist = cv.take<double>((size_t)P * (size_t)P);
        d_merges = cv.take<double>((size_t)(P - 1) * 4);
        d_size = cv.take<int>((size_t)P);
        d_chain = cv.take<int>((size_t)P);
        d_status = cv.take<long long>(2);
    };
    double *d_pts, *d_dist, *d_merges;
    int *d_size, *d_chain;
    long long *d_status;
    sp_carve sizes;
    layout(sizes, d_pts, d_dist, d_merges, d_size, d_chain, d_status);
    int rc = sp_buf_ensure(ctx, ctx->b_hc, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_hclust_complete: a workspace of %lld bytes (the %d x %d distance matrix and %d x %d points) does not fit on the device",
                       (long long)sizes.off, P, P, P, D);
    if (rc) return rc;
    sp_carve cv(ctx->b_hc.p);
    layout(cv, d_pts, d_dist, d_merges, d_size, d_chain, d_status);
    SP_HIP(ctx, hipMemcpyAsync(d_pts, pts, n_pts * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemsetAsync(d_status, 0, 16, ctx->stream));
    const unsigned n_tiles = (unsigned)((P + SP_HC_T - 1) / SP_HC_T);
    SP_LAUNCH(ctx, "hc_dist", hc_dist, dim3(n_tiles, n_tiles), dim3(SP_HC_DTHREADS), 0, (const double *)d_pts, P, D, d_dist);
    if (dist) SP_HIP(ctx, hipMemcpyAsync(dist, d_dist, (size_t)P * (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_LAUNCH(ctx, "hc_chain", hc_chain, dim3(1), dim3(SP_HC_THREADS), 0, d_dist, P, d_size, d_chain, d_merges, d_status);
    long long h_status[2] = {0, 0};
    SP_HIP(ctx, hipMemcpyAsync(h_status, d_status, 16, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(merges, d_merges, (size_t)(P - 1) * 32, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_status[0] == SP_HC_SCANS)
        return sp_fail(ctx, SP_ESTATE, "sp_hclust_complete: the chain ran %lld scans for %d points (at most %lld expected)",
                       h_status[1], P, (long long)sp_hc_max_scans(P));
    if (h_status[0] != SP_HC_OK)
        return sp_fail(ctx, SP_ESTATE, "sp_hclust_complete: a point has no neighbour at a finite distance (the squared differences overflow)");
    return SP_OK;
}
