// sp_ltrtree.hip -- the LTR-RT tree on the device: MinHash sketches of the elements, their pairwise comparison, and
// neighbour joining (definition: sp_ltrtree.h).
//
//   lt_sketch   ONE workgroup per element, longest first.  The hashes of an element do not fit one LDS sort, so the element
//               is worked in chunks of `chunk` starts: LDS holds M = a power of two >= s + chunk words -- the running
//               bottom-s in front (unused entries UINT64_MAX), the chunk's hashes behind it (a thread builds the window of
//               its start from three packed words and two mask words; invalid starts give UINT64_MAX).  A bitonic sort of
//               the M words, then every thread looks at its M / 1024 consecutive words, keeps those that differ from their
//               predecessor, and a block scan packs the first s of the kept ones to the front.  "The s smallest distinct" is
//               associative, so the chunk size changes nothing.
//   lt_pairs    a workgroup owns a T x T tile of the upper triangle of the pair matrix, stages its 2 T sketches in LDS once
//               (T on a diagonal tile; the pitch s + 1 is odd, so the lanes of a wave start on different banks), and one
//               lane walks one pair's merge (sp_lt_pair) and writes (i, j) and (j, i); a diagonal tile walks a pair once.  T = min(16, 8192 / s): the
//               2 T sketches fill at most 128 KiB.
//   neighbour joining, two drivers over the same state (matrix, sums, live mask):
//     nj_loop   ONE workgroup of 1024 threads runs all N - 2 joins: a wave takes a live row, its lanes the live columns
//               behind the diagonal (a 64-column group whose live bits are all clear is skipped), the (Q, i, j) minimum is
//               reduced by shuffles and through LDS, and then thread k updates D(i, k), D(k, i) and R_k.  The sums live in
//               LDS.  Every store to the matrix is followed by a __syncthreads() before any thread loads from it again --
//               a workgroup-scope release and acquire; the waves of a workgroup share their CU's write-through L1 -- and
//               the matrix is never read through a const __restrict__ pointer (the argument of hc_chain, sp_hclust.hip).
//     nj_rowmin + nj_join   per join two launches on the stream: N workgroups, one per row, each write their row's best
//               (Q, j) -- dead rows a sentinel --, then one workgroup reduces the N row results, writes the record and
//               updates row and column i, the sums and the live mask.  2 (N - 2) launches are enqueued at once; the join
//               count is known before the first.  A set status word (the guard; its limit is sp_nj_set_guard's, for tests) makes every later launch return at once.
//   No cooperative launch, no workgroup waits on another, every loop is bounded by N or by the element's length.  No kernel
//   of this unit caps its grid: the grids are n elements, the tiles of the pair triangle, and N rows.
// Which driver runs at which N was measured (profiles/ltrtree_notes.md): SP_LT_NJ_LOOP_MAX.
// Resources per kernel (`make resources`) are in profiles/ltrtree_notes.md.
#include <algorithm>
#include <limits.h>
#include <new>
#include <vector>

#include "sp_ltrtree.h"
#include "sp_common.h"
#include "sp_carve.h"
#include "sp_internal.h"

#define SP_LT_THREADS 1024
#define SP_LT_WAVES (SP_LT_THREADS / SP_WAVE)
#define SP_LT_PTHREADS 256
#define SP_LT_RTHREADS 256
#define SP_LT_PAIR_WORDS 8192         // sketch words one side of a pair tile may hold
#define SP_LT_UPLOAD (32LL << 20)     // bytes of sketches sp_ltr_sketch_pairs takes
#define SP_LT_NJ_LOOP_MAX 128         // up to this N the looping workgroup runs the joins (measured: profiles/ltrtree_notes.md)

// ---------------------------------------------------------------- sketches
struct lt_elem {
    const uint32_t *pk, *nm;   // the chromosome's packed codes and invalid mask
    int64_t start;
    int32_t len, out;          // bases; the caller's row
};

// hash of the k-mer at base g, or SP_LT_NONE when one of its bases is invalid.  The window's 32 bases lie in three packed
// words and two mask words; the words behind a chromosome's last are padding (SP_PAD_WORDS, marked invalid).
__device__ __forceinline__ unsigned long long lt_hash_at(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, int64_t g, int k) {
    const int64_t w = g >> 4, m = g >> 5;
    const uint32_t inv = __builtin_amdgcn_alignbit(nm[m + 1], nm[m], (int)(g & 31));
    if (inv & (0xffffffffu >> (32 - k))) return SP_LT_NONE;
    const uint32_t p0 = pk[w], p1 = pk[w + 1], p2 = pk[w + 2];
    const int r = 2 * (int)(g & 15);
    const uint64_t win = (uint64_t)__builtin_amdgcn_alignbit(p1, p0, r) | ((uint64_t)__builtin_amdgcn_alignbit(p2, p1, r) << 32);
    return sp_lt_hash(win, k);
}

// exclusive prefix sum of one int per thread over the SP_LT_THREADS threads; s_w: SP_LT_WAVES ints
__device__ __forceinline__ int lt_excl_scan(int v, int *s_w, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < SP_LT_WAVES; w++) {
        const int t = s_w[w];
        if (w < wave) base += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// M: a power of two, SP_LT_THREADS <= M <= 2 SP_LT_SMAX, s + chunk <= M
__global__ void __launch_bounds__(SP_LT_THREADS)
lt_sketch(const lt_elem *__restrict__ elems, int k, int s, int chunk, int M, unsigned long long *__restrict__ sketch, int32_t *__restrict__ len) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lt_buf[];
    __shared__ int s_w[SP_LT_WAVES];
    const lt_elem e = elems[blockIdx.x];
    const int tid = threadIdx.x, per = M / SP_LT_THREADS;      // 1, 2, 4 or 8
    for (int i = tid; i < M; i += SP_LT_THREADS) lt_buf[i] = SP_LT_NONE;
    __syncthreads();
    int cur = 0;
    const int n_starts = e.len - k + 1;
    for (int c0 = 0; c0 < n_starts; c0 += chunk) {
        const int nc = min(chunk, n_starts - c0);
        for (int t = tid; t < M - s; t += SP_LT_THREADS) lt_buf[s + t] = t < nc ? lt_hash_at(e.pk, e.nm, e.start + c0 + t, k) : SP_LT_NONE;
        for (int kk = 2; kk <= M; kk <<= 1)
            for (int j = kk >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (int i = tid; i < M; i += SP_LT_THREADS) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long a = lt_buf[i], b = lt_buf[l];
                        if ((a > b) == ((i & kk) == 0)) {
                            lt_buf[i] = b;
                            lt_buf[l] = a;
                        }
                    }
                }
            }
        __syncthreads();
        // this thread's `per` consecutive words: the distinct ones, packed to the front
        const int b0 = tid * per;
        unsigned long long vals[8];
        unsigned keep = 0;
        int cnt = 0;
        unsigned long long prev = b0 > 0 ? lt_buf[b0 - 1] : SP_LT_NONE;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (q < per) {
                const unsigned long long v = lt_buf[b0 + q];
                vals[q] = v;
                if (v != SP_LT_NONE && (b0 + q == 0 || v != prev)) {
                    keep |= 1u << q;
                    cnt++;
                }
                prev = v;
            }
        int total;
        int off = lt_excl_scan(cnt, s_w, total);      // (its barriers: every word is read before one is written)
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (q < per && ((keep >> q) & 1u)) {
                if (off < s) lt_buf[off] = vals[q];
                off++;
            }
        cur = min(total, s);
        for (int i = cur + tid; i < s; i += SP_LT_THREADS) lt_buf[i] = SP_LT_NONE;
        __syncthreads();
    }
    __syncthreads();
    for (int t = tid; t < s; t += SP_LT_THREADS) sketch[(int64_t)blockIdx.x * s + t] = lt_buf[t];
    if (tid == 0) len[blockIdx.x] = cur;
}

// ---------------------------------------------------------------- pairs
__global__ void __launch_bounds__(SP_LT_PTHREADS)
lt_pairs(const unsigned long long *__restrict__ sketch, const int32_t *__restrict__ len, int n, int s, int T, int32_t *__restrict__ shared,
         int32_t *__restrict__ denom) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lt_sk[];      // [2][T][s + 1]
    if (blockIdx.x < blockIdx.y) return;      // the lower triangle is written by its mirror tile
    const int pitch = s + 1, i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const int ni = min(T, n - i0), nj = min(T, n - j0);
    const bool diag = i0 == j0;
    unsigned long long *A = lt_sk, *B = diag ? lt_sk : lt_sk + (size_t)T * pitch;
    for (int e = threadIdx.x; e < ni * s; e += SP_LT_PTHREADS) {
        const int r = e / s, c = e - r * s;
        A[r * pitch + c] = sketch[(int64_t)(i0 + r) * s + c];
    }
    if (!diag)
        for (int e = threadIdx.x; e < nj * s; e += SP_LT_PTHREADS) {
            const int r = e / s, c = e - r * s;
            B[r * pitch + c] = sketch[(int64_t)(j0 + r) * s + c];
        }
    __syncthreads();
    for (int p = threadIdx.x; p < ni * nj; p += SP_LT_PTHREADS) {
        const int a = p / nj, b = p - a * nj, i = i0 + a, j = j0 + b;
        if (diag && b < a) continue;      // (b, a) writes both
        int32_t sh, dn;
        sp_lt_pair((const uint64_t *)A + a * pitch, len[i], (const uint64_t *)B + b * pitch, len[j], s, &sh, &dn);
        shared[(int64_t)i * n + j] = sh;
        denom[(int64_t)i * n + j] = dn;
        shared[(int64_t)j * n + i] = sh;
        denom[(int64_t)j * n + i] = dn;
    }
}

// ---------------------------------------------------------------- neighbour joining
struct lt_best {
    long long q;
    int i, j;
};
__device__ __forceinline__ lt_best lt_none() { return lt_best{LLONG_MAX, INT_MAX, INT_MAX}; }
__device__ __forceinline__ void lt_take(lt_best &b, long long q, int i, int j) {
    if (sp_lt_less(q, i, j, b.q, b.i, b.j)) b = lt_best{q, i, j};
}
// the minimum over the workgroup, in every thread; s_q, s_i, s_j: one entry per wave
__device__ __forceinline__ lt_best lt_block_min(lt_best b, long long *s_q, int *s_i, int *s_j) {
    for (int off = 32; off; off >>= 1) {
        const long long oq = __shfl_down(b.q, off);
        const int oi = __shfl_down(b.i, off), oj = __shfl_down(b.j, off);
        lt_take(b, oq, oi, oj);
    }
    const int wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) {
        s_q[wave] = b.q;
        s_i[wave] = b.i;
        s_j[wave] = b.j;
    }
    __syncthreads();
    lt_best r = lt_none();
    for (int w = 0; w < nw; w++) lt_take(r, s_q[w], s_i[w], s_j[w]);
    __syncthreads();
    return r;
}
// the sum over the workgroup, in every thread
__device__ __forceinline__ long long lt_block_sum(long long v, long long *s_q) {
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    const int wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) s_q[wave] = v;
    __syncthreads();
    long long t = 0;
    for (int w = 0; w < nw; w++) t += s_q[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ bool lt_live(const unsigned long long *live, int i) { return (live[i >> 6] >> (i & 63)) & 1ULL; }
// the best live column behind the diagonal of live row i, over the lanes of the calling waves: wave `w` of `nw` takes
// every nw-th group of 64 columns
__device__ __forceinline__ void lt_scan_row(const long long *row, int N, int i, int n, long long ri, const long long *R,
                                            const unsigned long long *live, int w, int nw, lt_best &b) {
    const int lane = threadIdx.x & 63;
    for (int c0 = ((i + 1) & ~63) + 64 * w; c0 < N; c0 += 64 * nw) {
        const unsigned long long m = live[c0 >> 6];
        if (!m) continue;
        const int j = c0 + lane;
        if (j > i && j < N && ((m >> lane) & 1ULL)) lt_take(b, sp_lt_q(n, row[j], ri, R[j]), i, j);
    }
}
// the two slots left: the last record (one thread)
__device__ void lt_last_record(const long long *D, int N, const unsigned long long *live, long long *m) {
    int a = -1, b = -1;
    for (int i = 0; i < N; i++)
        if (lt_live(live, i)) {
            if (a < 0) a = i;
            else if (b < 0) b = i;
        }
    if (a < 0 || b < 0) return;      // (cannot happen: two slots are live when the joins are done)
    m[0] = a;
    m[1] = b;
    m[2] = D[(long long)a * N + b];
    m[3] = 0;
    m[4] = 0;
}
// join (i, j) of n live slots: the record, then row and column i, the sums and the live mask.  All threads of the ONE
// workgroup call it; R and live may be LDS or global.  Returns whether the guard fired (in every thread).
__device__ __forceinline__ bool lt_join(long long *D, int N, int i, int j, long long *R, unsigned long long *live, long long *rec,
                                        long long *s_q, long long limit) {
    const long long dij = D[(long long)i * N + j];
    if (threadIdx.x == 0) {
        rec[0] = i;
        rec[1] = j;
        rec[2] = dij;
        rec[3] = R[i];
        rec[4] = R[j];
    }
    long long sum = 0;
    int bad = 0;
    long long *ri = D + (long long)i * N;
    const long long *rj = D + (long long)j * N;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        if (!lt_live(live, k) || k == i || k == j) continue;
        const long long a = ri[k], b = rj[k], v = sp_lt_update(a, b, dij);
        if (sp_lt_guard(v, limit)) bad = 1;
        ri[k] = v;
        D[(long long)k * N + i] = v;
        R[k] += v - a - b;      // thread k % blockDim.x alone touches R[k]
        sum += v;
    }
    sum = lt_block_sum(sum, s_q);      // (its barriers: the live mask and R[i], R[j] are read before thread 0 rewrites them)
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        R[i] = sum;
        live[j >> 6] &= ~(1ULL << (j & 63));
    }
    __syncthreads();
    return bad != 0;
}

// state: [0] live slots, [1] records written, [2] status
__global__ void __launch_bounds__(SP_LT_THREADS)
nj_loop(long long *D, int N, long long *merges, int *state, long long limit) {
    __shared__ long long s_R[SP_LT_MAXN];
    __shared__ unsigned long long s_live[SP_LT_MAXN / 64];
    __shared__ long long s_q[SP_LT_WAVES];
    __shared__ int s_i[SP_LT_WAVES], s_j[SP_LT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int w = tid; w < SP_LT_MAXN / 64; w += SP_LT_THREADS) {
        const int n = N - w * 64;
        s_live[w] = n >= 64 ? ~0ULL : n > 0 ? (1ULL << n) - 1ULL : 0ULL;
    }
    for (int i = wave; i < N; i += SP_LT_WAVES) {
        long long r = 0;
        for (int k = lane; k < N; k += 64) r += D[(long long)i * N + k];
        for (int off = 32; off; off >>= 1) r += __shfl_down(r, off);
        if (lane == 0) s_R[i] = r;
    }
    __syncthreads();
    int done = 0;
    for (int n = N; n > 2; n--) {
        lt_best b = lt_none();
        for (int i = wave; i < N; i += SP_LT_WAVES)
            if (lt_live(s_live, i)) lt_scan_row(D + (long long)i * N, N, i, n, s_R[i], s_R, s_live, 0, 1, b);
        b = lt_block_min(b, s_q, s_i, s_j);
        if (b.i >= N || b.j >= N) break;      // (cannot happen with n > 2 live slots: keeps the rows in bounds)
        const bool bad = lt_join(D, N, b.i, b.j, s_R, s_live, merges + 5 * (long long)done, s_q, limit);
        done++;
        if (bad) {
            if (tid == 0) state[2] = SP_LT_GUARD;
            return;
        }
    }
    if (tid == 0) lt_last_record(D, N, s_live, merges + 5 * (long long)done);
}

__global__ void __launch_bounds__(SP_LT_RTHREADS)
nj_rowsum(const long long *__restrict__ D, int N, long long *__restrict__ R) {
    __shared__ long long s_q[SP_LT_RTHREADS / SP_WAVE];
    const int i = blockIdx.x;
    long long r = 0;
    for (int k = threadIdx.x; k < N; k += SP_LT_RTHREADS) r += D[(long long)i * N + k];
    r = lt_block_sum(r, s_q);
    if (threadIdx.x == 0) R[i] = r;
}
// row blockIdx.x: its best (Q, j), or the sentinel when the row is dead or has no live column behind the diagonal
__global__ void __launch_bounds__(SP_LT_RTHREADS)
nj_rowmin(const long long *D, int N, const long long *R, const unsigned long long *live, const int *state, long long *pq, int *pj) {
    __shared__ long long s_q[SP_LT_RTHREADS / SP_WAVE];
    __shared__ int s_i[SP_LT_RTHREADS / SP_WAVE], s_j[SP_LT_RTHREADS / SP_WAVE];
    if (state[2]) return;
    const int i = blockIdx.x;
    lt_best b = lt_none();
    if (lt_live(live, i)) lt_scan_row(D + (long long)i * N, N, i, state[0], R[i], R, live, threadIdx.x >> 6, SP_LT_RTHREADS / SP_WAVE, b);
    b = lt_block_min(b, s_q, s_i, s_j);
    if (threadIdx.x == 0) {
        pq[i] = b.q;
        pj[i] = b.j;
    }
}
__global__ void __launch_bounds__(SP_LT_THREADS)
nj_join(long long *D, int N, long long *R, unsigned long long *live, int *state, const long long *pq, const int *pj, long long *merges,
        long long limit) {
    __shared__ long long s_q[SP_LT_WAVES];
    __shared__ int s_i[SP_LT_WAVES], s_j[SP_LT_WAVES];
    if (state[2]) return;
    const int done = state[1];
    lt_best b = lt_none();
    for (int r = threadIdx.x; r < N; r += SP_LT_THREADS)
        if (pj[r] != INT_MAX) lt_take(b, pq[r], r, pj[r]);
    b = lt_block_min(b, s_q, s_i, s_j);      // (its barriers: state[1] is read before thread 0 rewrites it)
    if (b.i >= N || b.j >= N) return;         // (cannot happen with more than 2 live slots)
    const bool bad = lt_join(D, N, b.i, b.j, R, live, merges + 5 * (long long)done, s_q, limit);
    if (threadIdx.x == 0) {
        state[0] -= 1;
        state[1] = done + 1;
        if (bad) state[2] = SP_LT_GUARD;
    }
}
__global__ void nj_last(const long long *D, int N, const unsigned long long *live, const int *state, long long *merges) {
    if (threadIdx.x == 0 && !state[2]) lt_last_record(D, N, live, merges + 5 * (long long)state[1]);
}

extern "C" {

int sp_ltr_sketch_set_chunk(sp_ctx *ctx, int starts) {
    if (!ctx || starts < 0 || starts > SP_LT_SMAX)
        return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch_set_chunk: %d is outside 0..%d", starts, SP_LT_SMAX);
    ctx->lt_chunk = starts;
    return SP_OK;
}

int sp_nj_set_mode(sp_ctx *ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return sp_fail(ctx, SP_EINVAL, "sp_nj_set_mode: %d is outside 0..2", mode);
    ctx->lt_mode = mode;
    return SP_OK;
}

int sp_nj_set_guard(sp_ctx *ctx, int64_t limit) {
    if (!ctx || limit < 0 || limit > SP_LT_DMAX) return sp_fail(ctx, SP_EINVAL, "sp_nj_set_guard: %lld is outside 0..2^40", (long long)limit);
    ctx->lt_guard = limit;
    return SP_OK;
}

int sp_ltr_sketch(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int k, int s, uint64_t *sketch,
                  int32_t *len) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: ctx is NULL");
    if (n < 0 || (n > 0 && (!chrom || !start || !end || !sketch || !len))) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: bad arguments");
    const int bad = sp_lt_check(k, s);
    if (bad == 1) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: k = %d is not an odd number in %d..%d", k, SP_LT_KMIN, SP_LT_KMAX);
    if (bad) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: s = %d is outside %d..%d", s, SP_LT_SMIN, SP_LT_SMAX);
    const int C = (int)ctx->chroms.size();
    if (C == 0) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: no genome loaded (sp_genome_add first)");
    if (n > 0x7fffffffLL) return sp_fail(ctx, SP_EUNSUP, "sp_ltr_sketch: %lld elements in one call, at most %d", (long long)n, 0x7fffffff);
    try {      // (the host lists below grow with n: a failed allocation is SP_ENOMEM, not an exception through the C entry)
    std::vector<lt_elem> elems;
    elems.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (chrom[i] < 0 || chrom[i] >= C) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: element %lld: chromosome %d out of range", (long long)i, chrom[i]);
        const sp_chrom &c = ctx->chroms[(size_t)chrom[i]];
        if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: element %lld: chromosome %d has no packed sequence (sp_genome_add first)", (long long)i, chrom[i]);
        if (start[i] < 0 || end[i] <= start[i] || end[i] > c.len)
            return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch: element %lld = [%lld, %lld) is empty or outside chromosome %d (%lld bases)", (long long)i,
                           (long long)start[i], (long long)end[i], chrom[i], (long long)c.len);
        elems.push_back(lt_elem{c.d_pk, c.d_nm, start[i], (int32_t)std::min<int64_t>(end[i] - start[i], 0x7fffffff), (int32_t)i});
    }
    for (int64_t i = 0; i < n; i++)
        if (end[i] - start[i] > SP_LT_MAXLEN)
            return sp_fail(ctx, SP_EUNSUP, "sp_ltr_sketch: element %lld has %lld bases (up to %d supported)", (long long)i, (long long)(end[i] - start[i]), SP_LT_MAXLEN);
    if (n == 0) return SP_OK;
    std::stable_sort(elems.begin(), elems.end(), [](const lt_elem &x, const lt_elem &y) { return x.len > y.len; });
    // the LDS words: the running sketch and one chunk
    int M = SP_LT_THREADS, chunk = ctx->lt_chunk;
    if (chunk == 0) {
        while (M < 2 * s) M *= 2;
        if (M < 2048) M = 2048;
        chunk = M - s;
    } else
        while (M < s + chunk) M *= 2;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_tmp<unsigned char> wsp;
    const size_t m = (size_t)n;
    sp_carve cv;
    cv.take<lt_elem>(m);
    cv.take<unsigned long long>(m * (size_t)s);
    cv.take<int32_t>(m);
    const hipError_t e = wsp.alloc(cv.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_ltr_sketch: %lld sketches of %d hashes, %lld bytes, do not fit on the device (%s)",
                       (long long)n, s, (long long)cv.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    lt_elem *d_elems = at.take<lt_elem>(m);
    unsigned long long *d_sk = at.take<unsigned long long>(m * (size_t)s);
    int32_t *d_len = at.take<int32_t>(m);
    std::vector<uint64_t> h_sk(m * (size_t)s);      // rows in the order of `elems`
    std::vector<int32_t> h_len(m);
    SP_HIP(ctx, hipMemcpyAsync(d_elems, elems.data(), m * sizeof(lt_elem), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipFuncSetAttribute((const void *)lt_sketch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)M * 8)));
    SP_LAUNCH(ctx, "lt_sketch", lt_sketch, dim3((unsigned)m), dim3(SP_LT_THREADS), (size_t)M * 8, (const lt_elem *)d_elems, k, s, chunk, M, d_sk, d_len);
    SP_HIP(ctx, hipMemcpyAsync(h_sk.data(), d_sk, m * (size_t)s * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(h_len.data(), d_len, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < m; q++) {
        memcpy(sketch + (size_t)elems[q].out * (size_t)s, h_sk.data() + q * (size_t)s, (size_t)s * 8);
        len[elems[q].out] = h_len[q];
    }
    return SP_OK;
    } catch (const std::bad_alloc &) {
        return sp_fail(ctx, SP_ENOMEM, "sp_ltr_sketch: the host lists of %lld elements with %d hashes each do not fit in memory", (long long)n, s);
    }
}

int sp_ltr_sketch_pairs(sp_ctx *ctx, int n, int s, const uint64_t *sketch, const int32_t *len, int32_t *shared, int32_t *denom) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch_pairs: ctx is NULL");
    if (n < 0 || (n > 0 && (!sketch || !len || !shared || !denom))) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch_pairs: bad arguments");
    if (sp_lt_check(SP_LT_KMIN, s)) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch_pairs: s = %d is outside %d..%d", s, SP_LT_SMIN, SP_LT_SMAX);
    for (int i = 0; i < n; i++)
        if (len[i] < 0 || len[i] > s) return sp_fail(ctx, SP_EINVAL, "sp_ltr_sketch_pairs: sketch %d has len = %d, outside 0..%d", i, len[i], s);
    const int64_t up = (int64_t)n * s * 8;
    if (up > SP_LT_UPLOAD)
        return sp_fail(ctx, SP_EUNSUP, "sp_ltr_sketch_pairs: %d sketches of %d hashes are %lld bytes (up to %lld are taken)", n, s, (long long)up, (long long)SP_LT_UPLOAD);
    if (n == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n * (size_t)n;
    sp_tmp<unsigned char> wsp;
    sp_carve cv;
    cv.take<unsigned long long>((size_t)n * (size_t)s);
    cv.take<int32_t>((size_t)n);
    cv.take<int32_t>(nn);
    cv.take<int32_t>(nn);
    const hipError_t e = wsp.alloc(cv.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_ltr_sketch_pairs: %d sketches and two %d x %d matrices, %lld bytes, do not fit on the device (%s)",
                       n, n, n, (long long)cv.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    unsigned long long *d_sk = at.take<unsigned long long>((size_t)n * (size_t)s);
    int32_t *d_len = at.take<int32_t>((size_t)n);
    int32_t *d_sh = at.take<int32_t>(nn), *d_dn = at.take<int32_t>(nn);
    int T = SP_LT_PAIR_WORDS / s;
    T = T > 16 ? 16 : T < 1 ? 1 : T;
    const size_t lds = 2 * (size_t)T * (size_t)(s + 1) * 8;      // at most 2 * (8192 + 16) * 8 bytes
    SP_HIP(ctx, hipFuncSetAttribute((const void *)lt_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SP_HIP(ctx, hipMemcpyAsync(d_sk, sketch, (size_t)n * (size_t)s * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_len, len, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    const unsigned nt = (unsigned)((n + T - 1) / T);
    SP_LAUNCH(ctx, "lt_pairs", lt_pairs, dim3(nt, nt), dim3(SP_LT_PTHREADS), lds, (const unsigned long long *)d_sk, (const int32_t *)d_len, n, s, T, d_sh, d_dn);
    SP_HIP(ctx, hipMemcpyAsync(shared, d_sh, nn * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(denom, d_dn, nn * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_nj_tree(sp_ctx *ctx, const int64_t *dist, int N, int64_t *merges) {
    if (!ctx || !dist || !merges) return sp_fail(ctx, SP_EINVAL, "sp_nj_tree: bad arguments");
    if (N < 2) return sp_fail(ctx, SP_EINVAL, "sp_nj_tree: %d slots (2 at least)", N);
    if (N > SP_LT_MAXN) return sp_fail(ctx, SP_EUNSUP, "sp_nj_tree: %d slots (up to %d supported)", N, SP_LT_MAXN);
    for (int i = 0; i < N; i++) {
        const int64_t *row = dist + (int64_t)i * N;
        if (row[i] != 0) return sp_fail(ctx, SP_EINVAL, "sp_nj_tree: D(%d, %d) = %lld is not zero", i, i, (long long)row[i]);
        for (int j = i + 1; j < N; j++) {
            if (row[j] < 0 || row[j] >= SP_LT_DIN)
                return sp_fail(ctx, SP_EINVAL, "sp_nj_tree: D(%d, %d) = %lld is outside [0, 2^31)", i, j, (long long)row[j]);
            if (row[j] != dist[(int64_t)j * N + i])
                return sp_fail(ctx, SP_EINVAL, "sp_nj_tree: D(%d, %d) = %lld but D(%d, %d) = %lld", i, j, (long long)row[j], j, i, (long long)dist[(int64_t)j * N + i]);
        }
    }
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)N * (size_t)N;
    long long *d_D, *d_R, *d_pq, *d_merges;
    unsigned long long *d_live;
    int *d_pj, *d_state;
    auto layout = [&](sp_carve &cv) {
        d_D = cv.take<long long>(nn);
        d_R = cv.take<long long>((size_t)N);
        d_pq = cv.take<long long>((size_t)N);
        d_merges = cv.take<long long>((size_t)(N - 1) * 5);
        d_live = cv.take<unsigned long long>(SP_LT_MAXN / 64);
        d_pj = cv.take<int>((size_t)N);
        d_state = cv.take<int>(4);
    };
    sp_carve sizes;
    layout(sizes);
    const int rc = sp_buf_ensure(ctx, ctx->b_lt, (int64_t)sizes.off);
    if (rc == SP_ENOMEM)
        return sp_fail(ctx, SP_ENOMEM, "sp_nj_tree: a workspace of %lld bytes (the %d x %d matrix) does not fit on the device", (long long)sizes.off, N, N);
    if (rc) return rc;
    sp_carve cv(ctx->b_lt.p);
    layout(cv);
    unsigned long long h_live[SP_LT_MAXN / 64];
    for (int w = 0; w < SP_LT_MAXN / 64; w++) {
        const int n = N - w * 64;
        h_live[w] = n >= 64 ? ~0ULL : n > 0 ? (1ULL << n) - 1ULL : 0ULL;
    }
    int h_state[4] = {N, 0, SP_LT_OK, 0};
    SP_HIP(ctx, hipMemcpyAsync(d_D, dist, nn * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_live, h_live, sizeof h_live, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_state, h_state, sizeof h_state, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // h_live and h_state are on this frame
    const long long limit = ctx->lt_guard ? (long long)ctx->lt_guard : (long long)SP_LT_DMAX;
    const bool loop = ctx->lt_mode == 1 || (ctx->lt_mode == 0 && N <= SP_LT_NJ_LOOP_MAX);
    if (loop) {
        SP_LAUNCH(ctx, "nj_loop", nj_loop, dim3(1), dim3(SP_LT_THREADS), 0, d_D, N, d_merges, d_state, limit);
    } else {
        SP_LAUNCH(ctx, "nj_rowsum", nj_rowsum, dim3((unsigned)N), dim3(SP_LT_RTHREADS), 0, (const long long *)d_D, N, d_R);
        for (int t = 0; t < N - 2; t++) {
            SP_LAUNCH(ctx, "nj_rowmin", nj_rowmin, dim3((unsigned)N), dim3(SP_LT_RTHREADS), 0, (const long long *)d_D, N, (const long long *)d_R,
                      (const unsigned long long *)d_live, (const int *)d_state, d_pq, d_pj);
            SP_LAUNCH(ctx, "nj_join", nj_join, dim3(1), dim3(SP_LT_THREADS), 0, d_D, N, d_R, d_live, d_state, (const long long *)d_pq, (const int *)d_pj, d_merges, limit);
        }
        SP_LAUNCH(ctx, "nj_last", nj_last, dim3(1), dim3(SP_WAVE), 0, (const long long *)d_D, N, (const unsigned long long *)d_live, (const int *)d_state, d_merges);
    }
    SP_HIP(ctx, hipMemcpyAsync(h_state, d_state, sizeof h_state, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(merges, d_merges, (size_t)(N - 1) * 40, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_state[2] != SP_LT_OK)
        return sp_fail(ctx, SP_ESTATE, "sp_nj_tree: a derived distance reached %lld in magnitude (the guard; %d slots); the matrix is far from a tree's", limit, N);
    return SP_OK;
}

}  // extern "C"
