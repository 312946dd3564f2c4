// sp_domains.hip -- the protein-domain search of the LTR stage on the resident genome (definition: sp_domains.h).
//
//   dm_translate  one workgroup per element writes the residues of its six frames, a byte each, to the workspace once.
//   dm_search     ONE wave owns an item = (element, frame, profile); the host hands the items out longest first by
//                 residues x nodes (workgroups are dispatched in grid order).  Lane l owns the B = ceil(M / 64) nodes
//                 l B + 1 .. (l + 1) B.  The rows run in sequence over two sets of M, I, D words in LDS (previous and
//                 current row, entry 0 of each is "does not exist").  M and I of a row need the previous row only.  The D
//                 chain of a row runs along the nodes: a lane folds its block into the map x -> max(x + A, d) (A: the sum
//                 of its d->d transitions, d: the block's last D when nothing comes in), an inclusive (max, +) scan of
//                 these maps over the 64 lanes gives every lane the D that enters its block -- exact, because the maps
//                 compose associatively over the pair order (sp_domains.h) --, and the lane walks its block again with
//                 it.  No iteration to a fixed point.  The residues of the next 64 rows are fetched while the current 64
//                 run (one per lane, broadcast by a shuffle): a fixed register stage, not a tunable chunk -- every frame
//                 of more than 64 residues crosses it.
//                 The profile's tables (emissions transposed to [22][M], transitions to [7][M], so that the lanes of a
//                 row read neighbouring words) sit in LDS when M <= SP_DM_TABM and are read from global memory (L2) above.
//                 Items of the two kinds go in two launches, each with the LDS its largest profile needs.
//   dm_pick       one thread per (element, profile): the best of the six frames, the six output numbers.
//   No kernel caps its grid (elements; items; entries), none waits on another workgroup, every loop is bounded by the
//   residues of a frame or the nodes of a profile.
#include <algorithm>
#include <new>
#include <vector>

#include "sp_domains.h"
#include "sp_common.h"
#include "sp_carve.h"
#include "sp_internal.h"

#define SP_DM_THREADS 64
#define SP_DM_TTHREADS 256
#define SP_DM_TABM 512                   // profiles up to this many nodes keep their tables in LDS
#define SP_DM_MAXOUT (1LL << 24)         // (element, profile) entries one call returns

struct dm_elem {
    const uint32_t *pk, *nm;   // the chromosome's packed codes and invalid mask
    int64_t start, roff;       // first base; where the element's residues start in the workspace
    int32_t len, pad;
};
struct dm_item {
    int64_t roff;              // the frame's residues
    int32_t nres, prof, slot, pad;   // slot: (element * P + profile) * 6 + frame
};
struct dm_prof {
    int32_t M, off, entry, pad;      // off: nodes in front of this profile in the tables
};

__device__ __forceinline__ unsigned dm_base(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, int64_t g) {
    const uint32_t code = (pk[g >> 4] >> (2 * (int)(g & 15))) & 3u, inv = (nm[g >> 5] >> (int)(g & 31)) & 1u;
    return inv ? (unsigned)SP_DM_INVALID : code;
}

__global__ void __launch_bounds__(SP_DM_TTHREADS)
dm_translate(const dm_elem *__restrict__ elems, uint8_t *__restrict__ res) {
    const dm_elem e = elems[blockIdx.x];
    const int64_t n = e.len;
    int64_t off = e.roff;
    for (int f = 0; f < 6; f++) {
        const int nr = sp_dm_nres(n, f);
        for (int j = threadIdx.x; j < nr; j += SP_DM_TTHREADS) {
            unsigned c[3];
#pragma unroll
            for (int t = 0; t < 3; t++) c[t] = sp_dm_strand(f, dm_base(e.pk, e.nm, e.start + sp_dm_pos(n, f, j, t)));
            res[off + j] = (uint8_t)sp_dm_codon(c[0], c[1], c[2]);
        }
        off += nr;
    }
}

// cap: words of one state array (the launch's largest M, plus 1); tabM: nodes the LDS table area holds (0: none)
__global__ void __launch_bounds__(SP_DM_THREADS)
dm_search(const dm_item *__restrict__ items, const dm_prof *__restrict__ profs, const int32_t *__restrict__ emisT, const int32_t *__restrict__ transT,
          const uint8_t *__restrict__ res, int cap, int tabM, sp_dm_hit *__restrict__ hits) {
    extern __shared__ __attribute__((aligned(16))) long long dm_lds[];
    const dm_item it = items[blockIdx.x];
    const dm_prof pf = profs[it.prof];
    const int M = pf.M, lane = threadIdx.x;
    if (M < 1 || M + 1 > cap || it.nres < 1) return;      // (the host sends none of these)
    long long *pM = dm_lds, *pI = pM + cap, *pD = pI + cap, *cM = pD + cap, *cI = cM + cap, *cD = cI + cap;
    for (int q = lane; q < 6 * cap; q += SP_DM_THREADS) dm_lds[q] = SP_DM_NONE;
    const int32_t *E = emisT + (int64_t)SP_DM_COLS * pf.off, *T = transT + (int64_t)7 * pf.off;
    if (M <= tabM) {
        int32_t *tab = (int32_t *)(dm_lds + 6 * (int64_t)cap);
        for (int q = lane; q < SP_DM_COLS * M; q += SP_DM_THREADS) tab[q] = E[q];
        for (int q = lane; q < 7 * M; q += SP_DM_THREADS) tab[SP_DM_COLS * M + q] = T[q];
        E = tab;
        T = tab + SP_DM_COLS * M;
    }
    __syncthreads();
    const int B = (M + SP_DM_THREADS - 1) / SP_DM_THREADS;
    const int k0 = lane * B + 1, k1 = min(M, k0 + B - 1);      // this lane's nodes; none when k0 > M
    const long long UNIT = 1LL << SP_DM_STARTBITS;
    sp_dm_hit best = sp_dm_nohit();
    int nxt = lane < it.nres ? res[it.roff + lane] : SP_DM_X;
    for (int i0 = 0; i0 < it.nres; i0 += 64) {
        const int cur = nxt;
        nxt = i0 + 64 + lane < it.nres ? res[it.roff + i0 + 64 + lane] : SP_DM_X;
        const int rows = min(64, it.nres - i0);
        for (int r = 0; r < rows; r++) {
            const int i = i0 + r, x = __shfl(cur, r);
            const int32_t *Ex = E + x * M;
            // M and I of this row, from the previous row
            for (int k = k0; k <= k1; k++) {
                const int kp = k >= 2 ? k - 2 : 0;      // node k - 1 in the tables (not used at k = 1: its predecessors do not exist)
                const long long m = sp_dm_match(pM[k - 1], pI[k - 1], pD[k - 1], T[SP_DM_MM * M + kp], T[SP_DM_IM * M + kp], T[SP_DM_DM * M + kp],
                                                pf.entry, (long long)i * 2048 + (k - 1), Ex[k - 1]);
                cM[k] = m;
                cI[k] = k <= M - 1 ? sp_dm_insert(pM[k], pI[k], T[SP_DM_MI * M + k - 1], T[SP_DM_II * M + k - 1]) : SP_DM_NONE;
                const sp_dm_hit h = sp_dm_hit{m, i, k};
                if (sp_dm_better(h, best)) best = h;
            }
            __syncthreads();
            // D of this row: the block as a map, the scan of the maps, the block again
            long long A = 0, d = SP_DM_NONE;
            for (int k = max(k0, 2); k <= k1; k++) {
                d = sp_dm_delete(cM[k - 1], d, T[SP_DM_MD * M + k - 2], T[SP_DM_DD * M + k - 2]);
                A += (long long)T[SP_DM_DD * M + k - 2] * UNIT;
            }
            for (int o = 1; o < 64; o <<= 1) {
                const long long pa = __shfl_up(A, o), pd = __shfl_up(d, o);
                if (lane >= o) {
                    // the map of the lanes in front, then this one
                    const long long through = pd == SP_DM_NONE ? SP_DM_NONE : pd + A;
                    d = through > d ? through : d;
                    A += pa;
                }
            }
            long long din = __shfl_up(d, 1);
            if (lane == 0) din = SP_DM_NONE;
            for (int k = k0; k <= k1; k++) {
                din = k >= 2 ? sp_dm_delete(cM[k - 1], din, T[SP_DM_MD * M + k - 2], T[SP_DM_DD * M + k - 2]) : SP_DM_NONE;
                cD[k] = din;
            }
            __syncthreads();
            long long *t;
            t = pM, pM = cM, cM = t;
            t = pI, pI = cI, cI = t;
            t = pD, pD = cD, cD = t;
        }
    }
    for (int o = 32; o; o >>= 1) {
        sp_dm_hit h;
        h.w = __shfl_down(best.w, o);
        h.i = __shfl_down(best.i, o);
        h.k = __shfl_down(best.k, o);
        if (sp_dm_better(h, best)) best = h;
    }
    if (lane == 0) hits[it.slot] = best;
}

__global__ void __launch_bounds__(SP_DM_TTHREADS)
dm_pick(const sp_dm_hit *__restrict__ hits, int64_t entries, int32_t *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * SP_DM_TTHREADS + threadIdx.x;
    if (q >= entries) return;
    sp_dm_hit fr[6];
    for (int f = 0; f < 6; f++) fr[f] = hits[q * 6 + f];
    int32_t r[6];
    sp_dm_result(fr, r);
    for (int c = 0; c < 6; c++) out[q * 6 + c] = r[c];
}

extern "C" {

int sp_dom_search(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P, const int32_t *moff,
                  const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t *out) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_dom_search: ctx is NULL");
    if (P < 1) return sp_fail(ctx, SP_EINVAL, "sp_dom_search: %d profiles (1 at least)", P);
    if (n < 0 || (n > 0 && (!chrom || !start || !end || !out)) || !moff || !emis || !trans || !entry)
        return sp_fail(ctx, SP_EINVAL, "sp_dom_search: bad arguments");
    if (P > SP_DM_MAXP) return sp_fail(ctx, SP_EUNSUP, "sp_dom_search: %d profiles (up to %d supported)", P, SP_DM_MAXP);
    const int C = (int)ctx->chroms.size();
    if (C == 0) return sp_fail(ctx, SP_EINVAL, "sp_dom_search: no genome loaded (sp_genome_add first)");
    if (moff[0] != 0) return sp_fail(ctx, SP_EINVAL, "sp_dom_search: the node offsets start at %d, not at 0", moff[0]);
    for (int p = 0; p < P; p++)
        if (moff[p + 1] <= moff[p])
            return sp_fail(ctx, SP_EINVAL, "sp_dom_search: profile %d has %lld nodes (1 at least; the offsets ascend)", p, (long long)moff[p + 1] - moff[p]);
    for (int64_t i = 0; i < n; i++) {
        if (chrom[i] < 0 || chrom[i] >= C) return sp_fail(ctx, SP_EINVAL, "sp_dom_search: element %lld: chromosome %d out of range", (long long)i, chrom[i]);
        const sp_chrom &c = ctx->chroms[(size_t)chrom[i]];
        if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "sp_dom_search: element %lld: chromosome %d has no packed sequence (sp_genome_add first)", (long long)i, chrom[i]);
        if (start[i] < 0 || end[i] < start[i] || end[i] > c.len)
            return sp_fail(ctx, SP_EINVAL, "sp_dom_search: element %lld = [%lld, %lld) is outside chromosome %d (%lld bases) or ends before it starts",
                           (long long)i, (long long)start[i], (long long)end[i], chrom[i], (long long)c.len);
    }
    int maxM[2] = {0, 0};      // the largest profile with its tables in LDS, and above
    for (int p = 0; p < P; p++) {
        const int M = moff[p + 1] - moff[p];
        if (M > SP_DM_MAXM) return sp_fail(ctx, SP_EUNSUP, "sp_dom_search: profile %d has %d nodes (up to %d supported)", p, M, SP_DM_MAXM);
        maxM[M > SP_DM_TABM] = std::max(maxM[M > SP_DM_TABM], M);
    }
    for (int64_t i = 0; i < n; i++)
        if (end[i] - start[i] > SP_DM_MAXLEN)
            return sp_fail(ctx, SP_EUNSUP, "sp_dom_search: element %lld has %lld bases (up to %d supported)", (long long)i, (long long)(end[i] - start[i]), SP_DM_MAXLEN);
    if (n * (int64_t)P > SP_DM_MAXOUT)
        return sp_fail(ctx, SP_EUNSUP, "sp_dom_search: %lld elements x %d profiles in one call (up to %lld entries)", (long long)n, P, (long long)SP_DM_MAXOUT);
    for (int p = 0; p < P; p++)
        if (!sp_dm_tables_ok(moff[p + 1] - moff[p], emis + (int64_t)moff[p] * SP_DM_COLS, trans + (int64_t)moff[p] * 7, entry[p]))
            return sp_fail(ctx, SP_EINVAL, "sp_dom_search: profile %d has a score outside its range (-2^20 <= transitions, entry <= 0; -2^20 <= emissions <= 2^15)", p);
    if (n == 0) return SP_OK;
    const size_t nodes = (size_t)moff[P], entries = (size_t)n * (size_t)P;
    try {      // (the host lists below grow with n x P: a failed allocation is SP_ENOMEM, not an exception through the C entry)
    std::vector<dm_elem> elems((size_t)n);
    std::vector<dm_prof> profs((size_t)P);
    std::vector<int32_t> emisT(nodes * SP_DM_COLS), transT(nodes * 7);
    for (int p = 0; p < P; p++) {
        const int M = moff[p + 1] - moff[p];
        profs[(size_t)p] = dm_prof{M, moff[p], entry[p], 0};
        const int32_t *e = emis + (int64_t)moff[p] * SP_DM_COLS, *t = trans + (int64_t)moff[p] * 7;
        int32_t *eT = emisT.data() + (size_t)moff[p] * SP_DM_COLS, *tT = transT.data() + (size_t)moff[p] * 7;
        for (int k = 0; k < M; k++) {
            for (int x = 0; x < SP_DM_COLS; x++) eT[(size_t)x * M + k] = e[(size_t)k * SP_DM_COLS + x];
            for (int x = 0; x < 7; x++) tT[(size_t)x * M + k] = t[(size_t)k * 7 + x];
        }
    }
    int64_t total = 0;
    std::vector<dm_item> items;
    items.reserve(entries * 6);
    for (int64_t i = 0; i < n; i++) {
        const sp_chrom &c = ctx->chroms[(size_t)chrom[i]];
        const int64_t len = end[i] - start[i];
        elems[(size_t)i] = dm_elem{c.d_pk, c.d_nm, start[i], total, (int32_t)len, 0};
        for (int f = 0; f < 6; f++) {
            const int32_t nr = sp_dm_nres(len, f);
            if (nr > 0)
                for (int p = 0; p < P; p++) items.push_back(dm_item{total, nr, p, (int32_t)((i * P + p) * 6 + f), 0});
            total += nr;
        }
    }
    // the items whose tables sit in LDS first, each kind longest first
    std::stable_sort(items.begin(), items.end(), [&](const dm_item &a, const dm_item &b) {
        const int Ma = profs[(size_t)a.prof].M, Mb = profs[(size_t)b.prof].M;
        const bool ga = Ma > SP_DM_TABM, gb = Mb > SP_DM_TABM;
        if (ga != gb) return gb;
        return (int64_t)a.nres * Ma > (int64_t)b.nres * Mb;
    });
    size_t n_lds = 0;
    while (n_lds < items.size() && profs[(size_t)items[n_lds].prof].M <= SP_DM_TABM) n_lds++;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    dm_elem *d_elems;
    dm_item *d_items;
    dm_prof *d_profs;
    int32_t *d_emis, *d_trans, *d_out;
    uint8_t *d_res;
    sp_dm_hit *d_hits;
    auto layout = [&](sp_carve &cv) {
        d_elems = cv.take<dm_elem>((size_t)n);
        d_items = cv.take<dm_item>(items.size() + 1);
        d_profs = cv.take<dm_prof>((size_t)P);
        d_hits = cv.take<sp_dm_hit>(entries * 6);
        d_emis = cv.take<int32_t>(nodes * SP_DM_COLS);
        d_trans = cv.take<int32_t>(nodes * 7);
        d_out = cv.take<int32_t>(entries * 6);
        d_res = cv.take<uint8_t>((size_t)total + 64);
    };
    sp_carve sizes;
    layout(sizes);
    sp_tmp<unsigned char> wsp;
    const hipError_t e = wsp.alloc(sizes.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_dom_search: %lld elements x %d profiles, %lld residues, %lld bytes, do not fit on the device (%s)",
                       (long long)n, P, (long long)total, (long long)sizes.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    layout(at);
    SP_HIP(ctx, hipMemcpyAsync(d_elems, elems.data(), elems.size() * sizeof(dm_elem), hipMemcpyHostToDevice, ctx->stream));
    if (!items.empty()) SP_HIP(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(dm_item), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_profs, profs.data(), profs.size() * sizeof(dm_prof), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_emis, emisT.data(), emisT.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_trans, transT.data(), transT.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemsetAsync(d_hits, 0, entries * 6 * sizeof(sp_dm_hit), ctx->stream));      // k = 0: no hit
    SP_LAUNCH(ctx, "dm_translate", dm_translate, dim3((unsigned)n), dim3(SP_DM_TTHREADS), 0, (const dm_elem *)d_elems, d_res);
    const size_t cnt[2] = {n_lds, items.size() - n_lds};
    size_t lds_max = 0;
    for (int g = 0; g < 2; g++)
        if (cnt[g]) lds_max = std::max(lds_max, (size_t)6 * (size_t)(maxM[g] + 1) * 8 + (g == 0 ? (size_t)29 * (size_t)maxM[0] * 4 : 0));
    if (lds_max) SP_HIP(ctx, hipFuncSetAttribute((const void *)dm_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    for (int g = 0; g < 2; g++) {
        if (!cnt[g]) continue;
        const int cap = maxM[g] + 1, tabM = g == 0 ? maxM[0] : 0;
        const size_t lds = (size_t)6 * (size_t)cap * 8 + (size_t)29 * (size_t)tabM * 4;      // at most 6 * 2049 * 8 = 98352 and 6 * 513 * 8 + 29 * 512 * 4 = 84016 bytes
        SP_LAUNCH(ctx, g == 0 ? "dm_search" : "dm_search_wide", dm_search, dim3((unsigned)cnt[g]), dim3(SP_DM_THREADS), lds,
                  (const dm_item *)(d_items + (g == 0 ? 0 : n_lds)), (const dm_prof *)d_profs, (const int32_t *)d_emis, (const int32_t *)d_trans,
                  (const uint8_t *)d_res, cap, tabM, d_hits);
    }
    SP_LAUNCH(ctx, "dm_pick", dm_pick, dim3((unsigned)((entries + SP_DM_TTHREADS - 1) / SP_DM_TTHREADS)), dim3(SP_DM_TTHREADS), 0,
              (const sp_dm_hit *)d_hits, (int64_t)entries, d_out);
    SP_HIP(ctx, hipMemcpyAsync(out, d_out, entries * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
    } catch (const std::bad_alloc &) {
        return sp_fail(ctx, SP_ENOMEM, "sp_dom_search: the host lists of %lld elements x %d profiles do not fit in memory", (long long)n, P);
    }
}

}  // extern "C"
