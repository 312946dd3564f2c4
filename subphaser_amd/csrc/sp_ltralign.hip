// sp_ltralign.hip -- banded global alignment of LTR pairs on the resident genome (definition: sp_ltralign.h).
//
// One workgroup of one wave owns a pair.  It unpacks both LTRs once from the 2-bit words and the validity mask into LDS,
// a byte per base, and sweeps the band by anti-diagonals s = i + j.  The cells of one anti-diagonal lie on the diagonals
// d = j - i of one parity, so the lanes take every second diagonal (and loop when the band has more than 128); a cell's
// predecessors are its own diagonal two steps back and the two neighbouring diagonals one step back.  One entry per
// diagonal is therefore all the state there is: a step's cells overwrite their own entry and read entries of the other
// parity, which nobody writes in that step.  Entries of the two parities live in separate halves of the arrays, so the
// lanes of a step touch consecutive words.  Nothing proportional to la * lb exists anywhere, nothing spills, and a
// pair's six results are written by one lane.
//
// The host checks every interval, flags the pairs that are not aligned (sp_la_check) and hands the others out longest
// first: workgroups are dispatched in grid order, so the long pairs start at once and the short ones fill in behind them.
#include <algorithm>

#include "sp_ltralign.h"
#include "sp_common.h"
#include "sp_internal.h"

#define SP_LA_THREADS 64

struct la_pair {
    const uint32_t *pk, *nm;   // the chromosome's packed codes and invalid mask
    int64_t a0, b0;            // first base of either LTR
    int32_t la, lb;
    int32_t out, pad;          // the caller's row (the kernel writes row blockIdx.x)
};

__device__ __forceinline__ int la_slot(int rel) { return (rel & 1) * (SP_LA_MAXBAND / 2) + (rel >> 1); }

__device__ __forceinline__ void la_unpack(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, int64_t g0, int n,
                                          uint8_t *dst) {
    for (int p = (int)threadIdx.x; p < n; p += SP_LA_THREADS) {
        const int64_t g = g0 + p;
        const uint32_t code = (pk[g >> 4] >> (2 * (int)(g & 15))) & 3u, inv = (nm[g >> 5] >> (int)(g & 31)) & 1u;
        dst[p] = (uint8_t)(inv ? SP_LA_INVALID : code);
    }
}

__global__ void __launch_bounds__(SP_LA_THREADS)
la_align(const la_pair *__restrict__ pairs, int w, int32_t *__restrict__ out) {
    __shared__ uint8_t sa[SP_LA_MAXLEN], sb[SP_LA_MAXLEN];
    __shared__ int32_t hs[SP_LA_MAXBAND];
    __shared__ unsigned long long hc[SP_LA_MAXBAND];
    const la_pair P = pairs[blockIdx.x];
    const int la = P.la, lb = P.lb;
    if (la < 1 || lb < 1 || sp_la_check(la, lb, w)) return;      // (the host sends none of these)
    la_unpack(P.pk, P.nm, P.a0, la, sa);
    la_unpack(P.pk, P.nm, P.b0, lb, sb);
    const int dlo = (int)sp_la_dlo(la, lb, w), dhi = (int)sp_la_dhi(la, lb, w);
    if (threadIdx.x == 0) {
        hs[la_slot(-dlo)] = 0;
        hc[la_slot(-dlo)] = 0;
    }
    __syncthreads();
    for (int s = 1; s <= la + lb; s++) {
        // the cells of this anti-diagonal: d of the parity of s, inside the band and the matrix
        int lo = max(dlo, max(-s, s - 2 * la));
        const int hi = min(dhi, min(s, 2 * lb - s));
        lo += (lo - s) & 1;
        for (int d = lo + 2 * (int)threadIdx.x; d <= hi; d += 2 * SP_LA_THREADS) {
            const int i = (s - d) >> 1, j = (s + d) >> 1, rel = d - dlo;
            sp_la_cell diag = sp_la_none(), up = sp_la_none(), left = sp_la_none();
            if (i > 0 && j > 0) diag = sp_la_cell{hs[la_slot(rel)], hc[la_slot(rel)]};
            if (i > 0 && d < dhi) up = sp_la_cell{hs[la_slot(rel + 1)], hc[la_slot(rel + 1)]};
            if (j > 0 && d > dlo) left = sp_la_cell{hs[la_slot(rel - 1)], hc[la_slot(rel - 1)]};
            const unsigned x = i > 0 ? sa[i - 1] : 0u, y = j > 0 ? sb[j - 1] : 0u;
            const sp_la_cell r = sp_la_update(diag, up, left, x, y, d, dlo, dhi, w);
            hs[la_slot(rel)] = r.score;
            hc[la_slot(rel)] = r.cnt;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int rel = lb - la - dlo;
        int32_t res[6];
        sp_la_result(sp_la_cell{hs[la_slot(rel)], hc[la_slot(rel)]}, res);
        for (int q = 0; q < 6; q++) out[(int64_t)blockIdx.x * 6 + q] = res[q];
    }
}

extern "C" {

int sp_ltr_align(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *a_start, const int32_t *a_len, const int64_t *b_start,
                 const int32_t *b_len, int band, int32_t *out) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: ctx is NULL");
    if (n < 0 || (n > 0 && (!chrom || !a_start || !a_len || !b_start || !b_len || !out)))
        return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: bad arguments");
    if (band < 0) return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: band = %d is below 0", band);
    const int C = (int)ctx->chroms.size();
    if (C == 0) return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: no genome loaded (sp_genome_add first)");
    if (n > 0x7fffffffLL / 6) return sp_fail(ctx, SP_EUNSUP, "sp_ltr_align: %lld pairs in one call, at most %d", (long long)n, 0x7fffffff / 6);
    std::vector<la_pair> pairs;
    pairs.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (chrom[i] < 0 || chrom[i] >= C) return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: pair %lld: chromosome %d out of range", (long long)i, chrom[i]);
        const sp_chrom &c = ctx->chroms[(size_t)chrom[i]];
        if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: pair %lld: chromosome %d has no packed sequence (sp_genome_add first)", (long long)i, chrom[i]);
        const int64_t st[2] = {a_start[i], b_start[i]}, ln[2] = {a_len[i], b_len[i]};
        for (int q = 0; q < 2; q++)
            if (ln[q] < 1 || st[q] < 0 || st[q] > c.len || ln[q] > c.len - st[q])
                return sp_fail(ctx, SP_EINVAL, "sp_ltr_align: pair %lld: %s LTR = [%lld, %lld + %lld) outside chromosome %d (%lld bases)", (long long)i,
                               q ? "right" : "left", (long long)st[q], (long long)st[q], (long long)ln[q], chrom[i], (long long)c.len);
        if (sp_la_check(ln[0], ln[1], band) == 0) pairs.push_back(la_pair{c.d_pk, c.d_nm, st[0], st[1], (int32_t)ln[0], (int32_t)ln[1], (int32_t)i, 0});
    }
    if (n == 0) return SP_OK;
    memset(out, 0, (size_t)n * 6 * sizeof(int32_t));
    for (int64_t i = 0; i < n; i++) out[i * 6 + 5] = sp_la_check(a_len[i], b_len[i], band);      // (the kernel writes the other rows)
    const size_t m = pairs.size();
    if (m == 0) return SP_OK;
    std::stable_sort(pairs.begin(), pairs.end(), [](const la_pair &x, const la_pair &y) { return x.la + x.lb > y.la + y.lb; });
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_tmp<unsigned char> wsp;
    const size_t o_out = (m * sizeof(la_pair) + 255) & ~(size_t)255, bytes = o_out + m * 6 * sizeof(int32_t);
    const hipError_t e = wsp.alloc(bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_ltr_align: %lld pairs, %lld bytes, do not fit on the device (%s)", (long long)n,
                       (long long)bytes, hipGetErrorString(e));
    }
    la_pair *d_pairs = (la_pair *)wsp.p;
    int32_t *d_out = (int32_t *)(wsp.p + o_out);
    std::vector<int32_t> res(m * 6);      // rows in the order of `pairs`
    SP_HIP(ctx, hipMemcpyAsync(d_pairs, pairs.data(), m * sizeof(la_pair), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemsetAsync(d_out, 0, m * 6 * sizeof(int32_t), ctx->stream));
    SP_LAUNCH(ctx, "la_align", la_align, dim3((unsigned)m), dim3(SP_LA_THREADS), 0, (const la_pair *)d_pairs, band, d_out);
    SP_HIP(ctx, hipMemcpyAsync(res.data(), d_out, m * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < m; q++) memcpy(out + (size_t)pairs[q].out * 6, res.data() + q * 6, 6 * sizeof(int32_t));
    return SP_OK;
}

}  // extern "C"
