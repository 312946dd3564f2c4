// sp_ltrdetect.hip -- de novo LTR-RT detection on the resident genome: exact seeds at a bounded distance and their gapless
// extensions (definition: sp_ltrdetect.h).  The chaining of the HSPs and everything after it is the host's (ltr.py).
//
// A chromosome is worked in CHUNKS.  A chunk owns the starts p of its body and also holds the dmax + L bases behind it, so
// every partner of an owned start lies in the chunk and every pair is found exactly once, whatever the body size.
//   ld_words   one 64-bit element per valid start of the chunk, (word << 24) | position in the chunk; a thread builds
//              the 32 starts of a unit from the packed words and the mask (sp_scan32_valid64) and appends its valid ones
//              in one piece -- the order is the sort's business
//   sort       rocprim::radix_sort_keys over the 2L + 24 significant bits: equal words sit together, ascending position
//   ld_seeds   one lane per sorted element: the partner walk of sp_ld_partners, left-maximality on the genome, and the
//              surviving (p, q) appended to the chromosome's seed list.  The list has a capacity; the counter runs on
//              when it is full, and the host then sizes the list from the count and runs the chunk again.
//   ld_extend  one lane per seed: both extensions, 16 bases of either copy at a time from the packed words and the mask;
//              a block of 16 equal valid bases is one step
//   per chromosome: sort of the HSP words, rocprim::unique
#include <cstring>
#include <utility>
#include <rocprim/rocprim.hpp>

#include "sp_ltrdetect.h"
#include "sp_ltralign.h"
#include "sp_blocks.h"
#include "sp_common.h"
#include "sp_device.h"
#include "sp_internal.h"

static_assert(SP_LD_MAXLEN == SP_LA_MAXLEN, "every candidate is aligned by sp_ltr_align");
static_assert(SP_LD_BODY + SP_LD_MAXDIST + SP_LD_LMAX <= (1 << SP_LD_POS_BITS), "chunk positions travel in 24 bits");

#define SP_LD_THREADS 256

struct sp_ltrdetect_state {
    int64_t body = SP_LD_BODY, seed_cap = SP_LD_SEED_CAP;
    sp_buf b_hsp;                // the HSP words of the last sp_ltr_seeds
    int64_t n_hsp = -1;          // -1: no list to answer for
};

struct ld_bases {
    const uint32_t *pk, *nm;
    __device__ __forceinline__ int operator()(int64_t g) const {
        if ((nm[g >> 5] >> (int)(g & 31)) & 1u) return SP_LD_INVALID;
        return (int)((pk[g >> 4] >> (2 * (int)(g & 15))) & 3u);
    }
};

// ---------------------------------------------------------------- words
// starts [c0, c1) of the chromosome; units of 32 starts from u0 on.  cnt[0]: elements written.
__global__ void __launch_bounds__(SP_LD_THREADS)
ld_words(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, int64_t u0, int64_t n_units,
         int64_t c0, int64_t c1, sp_kparams kp, unsigned long long *__restrict__ keys, unsigned long long *__restrict__ cnt) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s0 = (u0 + u) * 32;
        // the valid starts of the unit that the chunk holds: one reservation, then the elements behind one another
        uint32_t ok = ~(uint32_t)sp_bad_starts64(nm, s0, kp.k);
        if (s0 < c0) ok &= (c0 - s0 >= 32) ? 0u : (0xffffffffu << (int)(c0 - s0));
        if (s0 + 32 > c1) ok &= (c1 <= s0) ? 0u : (0xffffffffu >> (int)(s0 + 32 - c1));
        unsigned long long at = ok ? atomicAdd(cnt, (unsigned long long)__popc(ok)) : 0ULL;
        // (the scan takes the first k bases off the top of a 32-base window: good for k = 12..15 as for the 16..32 it was written for)
        sp_scan32_valid64(pk, pm, nm, s0, kp, [&](int64_t pos, uint64_t fwd, uint64_t) {
            if ((ok >> (int)(pos - s0)) & 1u) keys[at++] = sp_ld_key(fwd, (uint32_t)(pos - c0));
        });
    }
}

// ---------------------------------------------------------------- seeds
// cnt[1]: seeds found so far in the chromosome (it runs on past `cap`: nothing is written there, the host sees the count)
__global__ void __launch_bounds__(SP_LD_THREADS)
ld_seeds(const unsigned long long *__restrict__ keys, int64_t n, int64_t c0, int64_t body, int64_t dmin, int64_t dmax, ld_bases G,
         unsigned long long *__restrict__ seeds, unsigned long long cap, unsigned long long *__restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t cp = (int64_t)(keys[i] & SP_LD_POS_MASK);
        if (cp >= body) continue;           // a start of the next chunk's
        const int64_t p = c0 + cp;
        sp_ld_partners_each(keys, n, i, dmin, dmax, [&](uint32_t qpos) {
            const int64_t q = c0 + qpos;
            if (!sp_ld_is_seed(G, p, q)) return;
            const unsigned long long at = atomicAdd(cnt + 1, 1ULL);
            if (at < cap) seeds[at] = ((unsigned long long)p << 32) | (unsigned long long)q;
        });
    }
}

// ---------------------------------------------------------------- extension
// 16 bases from base g on (0 <= g < len; the padding behind a chromosome is marked invalid): codes LSB-first, invalid bits
__device__ __forceinline__ void ld_fetch16(const ld_bases &G, int64_t g, uint32_t &codes, uint32_t &inv) {
    const int64_t w = g >> 4, m = g >> 5;
    codes = __builtin_amdgcn_alignbit(G.pk[w + 1], G.pk[w], 2 * (int)(g & 15));
    inv = __builtin_amdgcn_alignbit(G.nm[m + 1], G.nm[m], (int)(g & 31)) & 0xffffu;
}

__global__ void __launch_bounds__(SP_LD_THREADS)
ld_extend(const unsigned long long *__restrict__ seeds, int64_t n, ld_bases G, int64_t len, int L, int X, int64_t maxlen,
          unsigned long long *__restrict__ hsps) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = (int64_t)(seeds[i] >> 32), q = (int64_t)(seeds[i] & 0xffffffffULL), d = q - p;
        const int cap = (int)(d < maxlen ? d : maxlen);
        // right: columns e with e < cap and q + e < len
        const int rlim = (int)((int64_t)cap < len - q ? (int64_t)cap : len - q);
        int e = L, s = 0, best = 0, r = L;
        bool go = true;
        while (go && e < rlim) {
            const int nb = rlim - e < 16 ? rlim - e : 16;
            uint32_t ca, ia, cb, ib;
            ld_fetch16(G, p + e, ca, ia);
            ld_fetch16(G, q + e, cb, ib);
            const uint32_t x = ca ^ cb, inv = ia | ib;
            if (nb == 16 && x == 0u && inv == 0u) {      // 16 matches: the score only rises, the best follows it or stays
                s += 16 * SP_LD_MATCH;
                e += 16;
                if (s > best) {
                    best = s;
                    r = e;
                }
                continue;
            }
            for (int j = 0; j < nb; j++) {
                if ((inv >> j) & 1u) {
                    go = false;
                    break;
                }
                if (!sp_ld_step(((x >> (2 * j)) & 3u) == 0u, X, s, best, e, r)) {
                    go = false;
                    break;
                }
            }
        }
        // left: columns e with e < p and r + e < cap; the block of a step ends before base p - e
        const int llim = (int)(p < (int64_t)(cap - r) ? p : (int64_t)(cap - r));
        int l = 0;
        e = 0, s = 0, best = 0;
        go = true;
        while (go && e < llim) {
            const int nb = llim - e < 16 ? llim - e : 16;
            uint32_t ca, ia, cb, ib;
            ld_fetch16(G, p - e - nb, ca, ia);
            ld_fetch16(G, q - e - nb, cb, ib);
            const uint32_t x = ca ^ cb, inv = ia | ib;
            if (nb == 16 && x == 0u && inv == 0u) {
                s += 16 * SP_LD_MATCH;
                e += 16;
                if (s > best) {
                    best = s;
                    l = e;
                }
                continue;
            }
            for (int j = nb - 1; j >= 0; j--) {
                if ((inv >> j) & 1u) {
                    go = false;
                    break;
                }
                if (!sp_ld_step(((x >> (2 * j)) & 3u) == 0u, X, s, best, e, l)) {
                    go = false;
                    break;
                }
            }
        }
        hsps[i] = sp_ld_hsp_pack(p - l, r + l, d);
    }
}

// ---------------------------------------------------------------- host
static sp_ltrdetect_state *ld_state(sp_ctx *ctx) {
    if (!ctx->ltrdetect) ctx->ltrdetect = new sp_ltrdetect_state();
    return ctx->ltrdetect;
}
void sp_ltrdetect_destroy(sp_ctx *ctx) {
    if (!ctx->ltrdetect) return;
    sp_buf_free(ctx->ltrdetect->b_hsp);
    delete ctx->ltrdetect;
    ctx->ltrdetect = nullptr;
}
static unsigned ld_grid(sp_ctx *ctx, int64_t items) {
    int64_t g = (items + SP_LD_THREADS - 1) / SP_LD_THREADS;
    const int64_t most = 8LL * ctx->n_cu;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}
static int ld_nomem(sp_ctx *ctx, hipError_t e, const char *what, int chrom, size_t bytes) {
    (void)hipGetLastError();
    return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_ltr_seeds: %s of chromosome %d, %lld bytes, do not fit on the device (%s)", what,
                   chrom, (long long)bytes, hipGetErrorString(e));
}
// (the library's kernels are timed as one entry of sp_prof_report under `name`)
static int ld_sort(sp_ctx *ctx, const char *name, int chrom, unsigned long long *in, unsigned long long *out, int64_t n, unsigned end_bit) {
    size_t tmp_bytes = 0;
    SP_HIP(ctx, rocprim::radix_sort_keys(nullptr, tmp_bytes, in, out, (size_t)n, 0u, end_bit, ctx->stream));
    sp_tmp<unsigned char> tmp;
    const hipError_t e = tmp.alloc(tmp_bytes + 256);
    if (e != hipSuccess) return ld_nomem(ctx, e, "the sort's workspace", chrom, tmp_bytes + 256);
    sp_prof_begin(ctx, name, dim3(1));
    const hipError_t es = rocprim::radix_sort_keys((void *)tmp.p, tmp_bytes, in, out, (size_t)n, 0u, end_bit, ctx->stream);
    sp_prof_end(ctx);
    SP_HIP(ctx, es);
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the workspace goes at scope exit)
    return SP_OK;
}

extern "C" {

int sp_ltr_detect_set_chunk(sp_ctx *ctx, int64_t body_bases) {
    if (!ctx || body_bases < 0 || body_bases > SP_LD_BODY)
        return sp_fail(ctx, SP_EINVAL, "sp_ltr_detect_set_chunk: %lld is outside 0..%d", (long long)body_bases, SP_LD_BODY);
    ld_state(ctx)->body = body_bases ? body_bases : SP_LD_BODY;
    return SP_OK;
}

int sp_ltr_detect_set_capacity(sp_ctx *ctx, int64_t seeds) {
    if (!ctx || seeds < 0 || seeds > (1LL << 40))
        return sp_fail(ctx, SP_EINVAL, "sp_ltr_detect_set_capacity: %lld is outside 0..2^40", (long long)seeds);
    ld_state(ctx)->seed_cap = seeds ? seeds : SP_LD_SEED_CAP;
    return SP_OK;
}

int sp_ltr_seeds(sp_ctx *ctx, int chrom, int seed_len, int xdrop, int64_t dmin, int64_t dmax, int32_t maxlen, int64_t *n_seeds, int64_t *n_hsps) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: ctx is NULL");
    sp_ltrdetect_state *st = ld_state(ctx);
    st->n_hsp = -1;
    if (!n_seeds || !n_hsps) return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: an output pointer is NULL");
    if (chrom < 0 || chrom >= (int)ctx->chroms.size())
        return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: chromosome %d is outside the genome (0..%d)", chrom, (int)ctx->chroms.size() - 1);
    const sp_chrom &c = ctx->chroms[(size_t)chrom];
    if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: chromosome %d has no packed sequence (sp_genome_add first)", chrom);
    switch (sp_ld_check(seed_len, xdrop, dmin, dmax, maxlen)) {
    case 1: return sp_fail(ctx, SP_EUNSUP, "sp_ltr_seeds: seed length %d is outside %d..%d", seed_len, SP_LD_LMIN, SP_LD_LMAX);
    case 2: return sp_fail(ctx, SP_EUNSUP, "sp_ltr_seeds: maximum distance %lld is above %d: the distance travels in 15 bits", (long long)dmax, SP_LD_MAXDIST);
    case 3: return sp_fail(ctx, SP_EUNSUP, "sp_ltr_seeds: maximum LTR length %d is above %d, what the alignment takes", maxlen, SP_LD_MAXLEN);
    case 4: return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: distances %lld..%lld: the minimum is below 1 or above the maximum", (long long)dmin, (long long)dmax);
    case 5: return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: X-drop %d is below 0", xdrop);
    case 6: return sp_fail(ctx, SP_EINVAL, "sp_ltr_seeds: maximum LTR length %d is below 1", maxlen);
    }
    if (c.len > SP_BK_MAXLEN)
        return sp_fail(ctx, SP_EUNSUP, "sp_ltr_seeds: chromosome %d has %lld bases, positions travel in 31 bits", chrom, (long long)c.len);
    *n_seeds = *n_hsps = 0;
    const int L = seed_len;
    const int64_t n_starts = c.len - L + 1;
    if (n_starts < 1) {
        st->n_hsp = 0;
        return SP_OK;
    }
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t body = st->body, tail = dmax;      // starts behind the body that a partner may be
    const int64_t most = n_starts < body + tail ? n_starts : body + tail;      // elements of one chunk
    const size_t key_bytes = ((size_t)most * 8 + 255) & ~(size_t)255;
    sp_tmp<unsigned char> wk, ws;
    hipError_t e = wk.alloc(2 * key_bytes + 256);
    if (e != hipSuccess) return ld_nomem(ctx, e, "the words of a chunk", chrom, 2 * key_bytes + 256);
    unsigned long long *A = (unsigned long long *)wk.p, *B = (unsigned long long *)(wk.p + key_bytes), *cnt = (unsigned long long *)(wk.p + 2 * key_bytes);
    int64_t cap = st->seed_cap;
    e = ws.alloc((size_t)cap * 8);
    if (e != hipSuccess) return ld_nomem(ctx, e, "the seed list", chrom, (size_t)cap * 8);
    SP_HIP(ctx, hipMemsetAsync(cnt, 0, 16, ctx->stream));
    const sp_kparams kp = sp_make_kparams(L);
    const ld_bases G{c.d_pk, c.d_nm};
    unsigned long long h[2] = {0, 0};
    int64_t have = 0;                                   // seeds of the chunks done
    for (int64_t c0 = 0; c0 < n_starts; c0 += body) {
        const int64_t c1 = c0 + body + tail < n_starts ? c0 + body + tail : n_starts;
        const int64_t u0 = c0 >> 5, n_units = ((c1 + 31) >> 5) - u0;
        SP_HIP(ctx, hipMemsetAsync(cnt, 0, 8, ctx->stream));
        SP_LAUNCH(ctx, "ld_words", ld_words, dim3(ld_grid(ctx, n_units)), dim3(SP_LD_THREADS), 0, c.d_pk, c.d_pm, c.d_nm, u0, n_units, c0, c1, kp, A, cnt);
        SP_HIP(ctx, hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const int64_t nv = (int64_t)h[0];
        if (nv > c1 - c0) return sp_fail(ctx, SP_EHIP, "sp_ltr_seeds: chromosome %d: %lld words from %lld starts", chrom, (long long)nv, (long long)(c1 - c0));
        if (nv < 2) continue;
        int rc = ld_sort(ctx, "ld_sort_words", chrom, A, B, nv, (unsigned)(2 * L + SP_LD_POS_BITS));
        if (rc) return rc;
        for (;;) {
            SP_LAUNCH(ctx, "ld_seeds", ld_seeds, dim3(ld_grid(ctx, nv)), dim3(SP_LD_THREADS), 0, (const unsigned long long *)B, nv, c0, body, dmin, dmax, G,
                      (unsigned long long *)ws.p, (unsigned long long)cap, cnt);
            SP_HIP(ctx, hipMemcpyAsync(h + 1, cnt + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
            SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if ((int64_t)h[1] <= cap) break;
            // the list is full: a new one sized from the count (twice the old at least), the seeds of the earlier chunks
            // moved over, and this chunk once more
            const int64_t want = (int64_t)h[1] > 2 * cap ? (int64_t)h[1] : 2 * cap;
            sp_tmp<unsigned char> bigger;
            e = bigger.alloc((size_t)want * 8);
            if (e != hipSuccess) return ld_nomem(ctx, e, "the seed list", chrom, (size_t)want * 8);
            if (have) SP_HIP(ctx, hipMemcpyAsync(bigger.p, ws.p, (size_t)have * 8, hipMemcpyDeviceToDevice, ctx->stream));
            const unsigned long long back = (unsigned long long)have;
            SP_HIP(ctx, hipMemcpyAsync(cnt + 1, &back, 8, hipMemcpyHostToDevice, ctx->stream));
            SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            std::swap(ws.p, bigger.p);
            cap = want;
        }
        have = (int64_t)h[1];
    }
    *n_seeds = have;
    if (have == 0) {
        st->n_hsp = 0;
        return SP_OK;
    }
    // one HSP per seed, sorted, the duplicates dropped
    const size_t hsp_bytes = ((size_t)have * 8 + 255) & ~(size_t)255;
    sp_tmp<unsigned char> wh;
    e = wh.alloc(2 * hsp_bytes + 256);
    if (e != hipSuccess) return ld_nomem(ctx, e, "the HSPs", chrom, 2 * hsp_bytes + 256);
    unsigned long long *H = (unsigned long long *)wh.p, *S = (unsigned long long *)(wh.p + hsp_bytes), *d_n = (unsigned long long *)(wh.p + 2 * hsp_bytes);
    int rc = sp_buf_ensure(ctx, st->b_hsp, (int64_t)hsp_bytes);
    if (rc) return rc;
    SP_LAUNCH(ctx, "ld_extend", ld_extend, dim3(ld_grid(ctx, have)), dim3(SP_LD_THREADS), 0, (const unsigned long long *)ws.p, have, G, c.len, L, xdrop,
              (int64_t)maxlen, H);
    if ((rc = ld_sort(ctx, "ld_sort_hsps", chrom, H, S, have, 64u))) return rc;
    size_t tmp_bytes = 0;
    SP_HIP(ctx, rocprim::unique(nullptr, tmp_bytes, S, (unsigned long long *)st->b_hsp.p, d_n, (size_t)have, rocprim::equal_to<unsigned long long>(), ctx->stream));
    sp_tmp<unsigned char> tmp;
    e = tmp.alloc(tmp_bytes + 256);
    if (e != hipSuccess) return ld_nomem(ctx, e, "the workspace of the duplicate removal", chrom, tmp_bytes + 256);
    sp_prof_begin(ctx, "ld_unique", dim3(1));
    const hipError_t eu = rocprim::unique((void *)tmp.p, tmp_bytes, S, (unsigned long long *)st->b_hsp.p, d_n, (size_t)have, rocprim::equal_to<unsigned long long>(), ctx->stream);
    sp_prof_end(ctx);
    SP_HIP(ctx, eu);
    unsigned long long nu = 0;
    SP_HIP(ctx, hipMemcpyAsync(&nu, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    st->n_hsp = (int64_t)nu;
    *n_hsps = (int64_t)nu;
    return SP_OK;
}

int sp_ltr_hsps(sp_ctx *ctx, int32_t *p0, int32_t *len, int32_t *d, int64_t n) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_ltr_hsps: ctx is NULL");
    sp_ltrdetect_state *st = ctx->ltrdetect;
    if (!st || st->n_hsp < 0) return sp_fail(ctx, SP_EINVAL, "sp_ltr_hsps: no list to answer for (sp_ltr_seeds first)");
    if (n != st->n_hsp) return sp_fail(ctx, SP_EINVAL, "sp_ltr_hsps: the last call found %lld HSPs, not %lld", (long long)st->n_hsp, (long long)n);
    if (n == 0) return SP_OK;
    if (!p0 || !len || !d) return sp_fail(ctx, SP_EINVAL, "sp_ltr_hsps: an output array is NULL");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> h((size_t)n);
    SP_HIP(ctx, hipMemcpyAsync(h.data(), st->b_hsp.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < n; i++) sp_ld_hsp_unpack(h[(size_t)i], &p0[i], &len[i], &d[i]);
    return SP_OK;
}

}  // extern "C"
