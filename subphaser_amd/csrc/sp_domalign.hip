// sp_domalign.hip -- the profile alignment of the domain trees on the resident genome (definition: sp_domalign.h), and the
// pair comparison of the aligned rows.
//
//   da_residues   one workgroup per item writes the residues of the item's WINDOW, a byte each (not of six whole frames):
//                 sp_dm_codon / sp_dm_pos / sp_dm_strand as they are.  sp_dom_peptide is this kernel alone.
//   da_fill       ONE wave per item, built like dm_search (sp_domains.hip): lanes own contiguous node blocks, two sets of
//                 M, I, D words in LDS, the exact (max, +) scan for the D chain, the tables in LDS up to SP_DA_TABM nodes,
//                 the 64-row residue stage.  While a lane walks its block it has the predecessors of its cells in hand and
//                 forms the back-pointer codes (sp_da_bp_*): M and I in the first walk, D in the second.  A lane's cells
//                 are ceil(M / 64) bytes apart from its neighbour's, so the bytes are NOT stored from the lanes: they go
//                 to a row of SP_DA_PITCH(M) bytes in LDS (two rows, used in turn, so that a row is rewritten only after
//                 two barriers), and the wave then stores the row to the plane as whole 32-bit words, neighbouring lanes
//                 neighbouring words.  The plane's pitch is a multiple of 4 for that.  It also keeps the best M cell.
//   da_trace      one wave per item: the lanes set col to -1, then lane 0 walks the plane back from the hit
//                 (sp_da_trace), a serial chain of dependent byte loads.
//   da_pairs      a workgroup of 256 threads owns a tile of 32 x 32 row pairs of the upper triangle, stages the 32 + 32
//                 rows in LDS one chunk of 1024 columns at a time (64 rows of 1032 bytes: 66048; a diagonal tile stages 32), and compares 8
//                 bytes per step (sp_swar.h).  Thread t owns row a = t % 32 of the first side and the four rows
//                 4 (t / 32) .. + 3 of the second: the lanes of a wave read 32 different rows of the first side -- the
//                 pitch of 1032 bytes puts them on different banks -- and one row of the second, a broadcast.
//   A batch of items runs as launches on the context's stream (da_fill for the items with tables in LDS, da_fill for those
//   above, da_trace), so no question of visibility inside a kernel arises.  No kernel caps its grid (items; items; tiles
//   of the pair triangle), none waits on another workgroup, every loop is bounded by the window, the nodes or the columns.
#include <algorithm>
#include <new>
#include <string.h>
#include <vector>

#include "sp_domalign.h"
#include "sp_common.h"
#include "sp_swar.h"
#include "sp_carve.h"
#include "sp_internal.h"

#define SP_DA_THREADS 64
#define SP_DA_RTHREADS 256
#define SP_DA_TABM 512                    // profiles up to this many nodes keep their tables in LDS
#define SP_DA_CAP (1LL << 30)             // bytes of back-pointer planes one batch holds
#define SP_DA_TILE 32                     // rows of one side of a pair tile
#define SP_DA_CHUNK 1024                  // columns staged at a time
#define SP_DA_LPITCH (SP_DA_CHUNK + 8)    // bytes of a staged row: 258 words, so 32 rows start on 32 different even banks
#define SP_DA_PTHREADS 256

struct da_item {
    const uint32_t *pk, *nm;   // the chromosome's packed codes and invalid mask
    int64_t start;             // first base of the interval
    int64_t roff;              // where the window's residues lie
    int64_t plane;             // where the item's plane starts in its batch's workspace
    int64_t coff;              // where its columns start
    int32_t len, frame, i0, nwin, prof, out;   // interval bases; out: the caller's item
};
struct da_prof {
    int32_t M, off, entry, pad;
};

__device__ __forceinline__ unsigned da_base(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, int64_t g) {
    const uint32_t code = (pk[g >> 4] >> (2 * (int)(g & 15))) & 3u, inv = (nm[g >> 5] >> (int)(g & 31)) & 1u;
    return inv ? (unsigned)SP_DM_INVALID : code;
}

__global__ void __launch_bounds__(SP_DA_RTHREADS)
da_residues(const da_item *__restrict__ items, uint8_t *__restrict__ res) {
    const da_item e = items[blockIdx.x];
    const int64_t n = e.len;
    for (int j = threadIdx.x; j < e.nwin; j += SP_DA_RTHREADS) {
        unsigned c[3];
#pragma unroll
        for (int t = 0; t < 3; t++) c[t] = sp_dm_strand(e.frame, da_base(e.pk, e.nm, e.start + sp_dm_pos(n, e.frame, (int64_t)e.i0 + j, t)));
        res[e.roff + j] = (uint8_t)sp_dm_codon(c[0], c[1], c[2]);
    }
}

// cap: words of one state array (the launch's largest M, plus 1); tabM: nodes the LDS table area holds (0: none).
// LDS: 6 cap words, then 2 * SP_DA_PITCH(cap - 1) bytes of back-pointer rows, then the tables.
__global__ void __launch_bounds__(SP_DA_THREADS)
da_fill(const da_item *__restrict__ items, const da_prof *__restrict__ profs, const int32_t *__restrict__ emisT, const int32_t *__restrict__ transT,
        const uint8_t *__restrict__ res, int cap, int tabM, uint8_t *__restrict__ planes, sp_dm_hit *__restrict__ hits) {
    extern __shared__ __attribute__((aligned(16))) long long da_lds[];
    const da_item it = items[blockIdx.x];
    const da_prof pf = profs[it.prof];
    const int M = pf.M, lane = threadIdx.x;
    if (M < 1 || M + 1 > cap || it.nwin < 1) return;      // (the host sends none of these)
    long long *pM = da_lds, *pI = pM + cap, *pD = pI + cap, *cM = pD + cap, *cI = cM + cap, *cD = cI + cap;
    for (int q = lane; q < 6 * cap; q += SP_DA_THREADS) da_lds[q] = SP_DM_NONE;
    const int bpitch = SP_DA_PITCH(cap - 1), pitch = SP_DA_PITCH(M);
    uint8_t *bp = (uint8_t *)(da_lds + 6 * (int64_t)cap);      // two rows of bpitch bytes
    for (int q = lane; q < 2 * bpitch / 4; q += SP_DA_THREADS) ((uint32_t *)bp)[q] = 0u;
    const int32_t *E = emisT + (int64_t)SP_DM_COLS * pf.off, *T = transT + (int64_t)7 * pf.off;
    if (M <= tabM) {
        int32_t *tab = (int32_t *)(bp + 2 * bpitch);
        for (int q = lane; q < SP_DM_COLS * M; q += SP_DA_THREADS) tab[q] = E[q];
        for (int q = lane; q < 7 * M; q += SP_DA_THREADS) tab[SP_DM_COLS * M + q] = T[q];
        E = tab;
        T = tab + SP_DM_COLS * M;
    }
    __syncthreads();
    const int B = (M + SP_DA_THREADS - 1) / SP_DA_THREADS;
    const int k0 = lane * B + 1, k1 = min(M, k0 + B - 1);      // this lane's nodes; none when k0 > M
    const long long UNIT = 1LL << SP_DM_STARTBITS;
    uint8_t *plane = planes + it.plane;
    sp_dm_hit best = sp_dm_nohit();
    int nxt = lane < it.nwin ? res[it.roff + lane] : SP_DM_X;
    for (int r0 = 0; r0 < it.nwin; r0 += 64) {
        const int cur = nxt;
        nxt = r0 + 64 + lane < it.nwin ? res[it.roff + r0 + 64 + lane] : SP_DM_X;
        const int rows = min(64, it.nwin - r0);
        for (int r = 0; r < rows; r++) {
            const int i = it.i0 + r0 + r, x = __shfl(cur, r);
            const int32_t *Ex = E + x * M;
            uint8_t *brow = bp + ((r0 + r) & 1) * bpitch;
            // M and I of this row and their codes, from the previous row
            for (int k = k0; k <= k1; k++) {
                const int kp = k >= 2 ? k - 2 : 0;
                const long long m1 = pM[k - 1], i1 = pI[k - 1], d1 = pD[k - 1], start = (long long)i * 2048 + (k - 1);
                const int tmm = T[SP_DM_MM * M + kp], tim = T[SP_DM_IM * M + kp], tdm = T[SP_DM_DM * M + kp];
                const long long m = sp_dm_match(m1, i1, d1, tmm, tim, tdm, pf.entry, start, Ex[k - 1]);
                int code = sp_da_bp_match(m1, i1, d1, tmm, tim, tdm, pf.entry, start);
                cM[k] = m;
                long long ins = SP_DM_NONE;
                if (k <= M - 1) {
                    const int tmi = T[SP_DM_MI * M + k - 1], tii = T[SP_DM_II * M + k - 1];
                    ins = sp_dm_insert(pM[k], pI[k], tmi, tii);
                    code |= sp_da_bp_insert(pM[k], pI[k], tmi, tii) << 2;
                }
                cI[k] = ins;
                brow[k - 1] = (uint8_t)code;
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
                    const long long through = pd == SP_DM_NONE ? SP_DM_NONE : pd + A;
                    d = through > d ? through : d;
                    A += pa;
                }
            }
            long long din = __shfl_up(d, 1);
            if (lane == 0) din = SP_DM_NONE;
            for (int k = k0; k <= k1; k++) {
                if (k >= 2) {
                    const long long m1 = cM[k - 1];
                    const int tmd = T[SP_DM_MD * M + k - 2], tdd = T[SP_DM_DD * M + k - 2];
                    brow[k - 1] |= (uint8_t)(sp_da_bp_delete(m1, din, tmd, tdd) << 3);      // (this lane's own byte)
                    din = sp_dm_delete(m1, din, tmd, tdd);
                } else
                    din = SP_DM_NONE;
                cD[k] = din;
            }
            __syncthreads();
            // the row of bytes, as words
            uint32_t *dst = (uint32_t *)(plane + (int64_t)(r0 + r) * pitch);
            for (int q = lane; q < pitch / 4; q += SP_DA_THREADS) dst[q] = ((const uint32_t *)brow)[q];
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
    if (lane == 0) hits[blockIdx.x] = best;
}

__global__ void __launch_bounds__(SP_DA_THREADS)
da_trace(const da_item *__restrict__ items, const da_prof *__restrict__ profs, const uint8_t *__restrict__ planes, const sp_dm_hit *__restrict__ hits,
         int32_t *__restrict__ hit, int32_t *__restrict__ col) {
    const da_item it = items[blockIdx.x];
    const int M = profs[it.prof].M;
    int32_t *c = col + it.coff;
    for (int k = threadIdx.x; k < M; k += SP_DA_THREADS) c[k] = -1;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const sp_dm_hit h = hits[blockIdx.x];
    int32_t r[5] = {INT32_MIN, 0, 0, 0, 0};
    if (h.k >= 1 && h.k <= M && h.i >= it.i0 && h.i < it.i0 + it.nwin) {      // (always: the window has a residue)
        sp_da_result(h, r);
        sp_da_trace(planes + it.plane, M, it.i0, it.nwin, h.i, h.k, c);
    }
    for (int q = 0; q < 5; q++) hit[(int64_t)it.out * 5 + q] = r[q];
}

// rows: N rows of Cp bytes (Cp a multiple of 8, the columns behind C are SP_DA_GAP)
__global__ void __launch_bounds__(SP_DA_PTHREADS)
da_pairs(const uint8_t *__restrict__ rows, int N, int Cp, int32_t *__restrict__ same, int32_t *__restrict__ both) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long da_rows[];      // [2][SP_DA_TILE][SP_DA_LPITCH / 8]
    if (blockIdx.x < blockIdx.y) return;      // the lower triangle is written by its mirror tile
    const int i0 = blockIdx.y * SP_DA_TILE, j0 = blockIdx.x * SP_DA_TILE, W = SP_DA_LPITCH / 8;
    const bool diag = i0 == j0;
    unsigned long long *SA = da_rows, *SB = diag ? da_rows : da_rows + SP_DA_TILE * W;
    const int a = threadIdx.x & (SP_DA_TILE - 1), b0 = (threadIdx.x >> 5) * 4;
    uint32_t ns[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
    for (int c0 = 0; c0 < Cp; c0 += SP_DA_CHUNK) {
        const int cw = min(SP_DA_CHUNK, Cp - c0) / 8;      // words of this chunk
        __syncthreads();
        for (int e = threadIdx.x; e < SP_DA_TILE * cw; e += SP_DA_PTHREADS) {
            const int r = e / cw, w = e - r * cw;
            SA[r * W + w] = i0 + r < N ? *(const unsigned long long *)(rows + (int64_t)(i0 + r) * Cp + c0 + 8 * w) : ~0ULL;
            if (!diag) SB[r * W + w] = j0 + r < N ? *(const unsigned long long *)(rows + (int64_t)(j0 + r) * Cp + c0 + 8 * w) : ~0ULL;
        }
        __syncthreads();
        for (int w = 0; w < cw; w++) {
            const unsigned long long x = SA[a * W + w], fx = sp_swar_lt20_bytes(x);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned long long y = SB[(b0 + q) * W + w], f = fx & sp_swar_lt20_bytes(y);
                nb[q] += sp_swar_byte_count(f);
                ns[q] += sp_swar_byte_count(f & sp_swar_eq_bytes(x, y));
            }
        }
    }
    const int i = i0 + a;
    if (i >= N) return;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int j = j0 + b0 + q;
        if (j >= N) continue;
        same[(int64_t)i * N + j] = (int32_t)ns[q];
        both[(int64_t)i * N + j] = (int32_t)nb[q];
        same[(int64_t)j * N + i] = (int32_t)ns[q];      // (a diagonal tile writes (i, j) and (j, i) from two threads: equal values)
        both[(int64_t)j * N + i] = (int32_t)nb[q];
    }
}

// what the two item entries check alike; on SP_OK `items` holds one entry per caller's item (roff, plane, coff unset)
static int da_check_items(sp_ctx *ctx, const char *who, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, const int32_t *frame,
                          const int32_t *i0, const int32_t *i1) {
    const int C = (int)ctx->chroms.size();
    if (C == 0) return sp_fail(ctx, SP_EINVAL, "%s: no genome loaded (sp_genome_add first)", who);
    for (int64_t q = 0; q < n; q++) {
        if (chrom[q] < 0 || chrom[q] >= C) return sp_fail(ctx, SP_EINVAL, "%s: item %lld: chromosome %d out of range", who, (long long)q, chrom[q]);
        const sp_chrom &c = ctx->chroms[(size_t)chrom[q]];
        if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "%s: item %lld: chromosome %d has no packed sequence (sp_genome_add first)", who, (long long)q, chrom[q]);
        if (start[q] < 0 || end[q] < start[q] || end[q] > c.len)
            return sp_fail(ctx, SP_EINVAL, "%s: item %lld = [%lld, %lld) is outside chromosome %d (%lld bases) or ends before it starts", who,
                           (long long)q, (long long)start[q], (long long)end[q], chrom[q], (long long)c.len);
        if (frame[q] < 0 || frame[q] > 5) return sp_fail(ctx, SP_EINVAL, "%s: item %lld: frame %d is outside 0..5", who, (long long)q, frame[q]);
        if (i0[q] < 0 || i0[q] > i1[q])
            return sp_fail(ctx, SP_EINVAL, "%s: item %lld: the window [%d, %d] is empty or starts below 0", who, (long long)q, i0[q], i1[q]);
        // (an interval above the limit is SP_EUNSUP below; its frame is long enough for this test either way)
        const int64_t nres = (end[q] - start[q] - frame[q] % 3) / 3;
        if (end[q] - start[q] < frame[q] % 3 || i1[q] >= nres)
            return sp_fail(ctx, SP_EINVAL, "%s: item %lld: the window [%d, %d] ends beyond the %lld residues of frame %d", who, (long long)q, i0[q], i1[q],
                           (long long)(end[q] - start[q] < frame[q] % 3 ? 0 : nres), frame[q]);
    }
    return SP_OK;
}
static int da_check_limits(sp_ctx *ctx, const char *who, int64_t n, const int64_t *start, const int64_t *end, const int32_t *i0, const int32_t *i1) {
    for (int64_t q = 0; q < n; q++) {
        if (end[q] - start[q] > SP_DM_MAXLEN)
            return sp_fail(ctx, SP_EUNSUP, "%s: item %lld has %lld bases (up to %d supported)", who, (long long)q, (long long)(end[q] - start[q]), SP_DM_MAXLEN);
        if ((int64_t)i1[q] - i0[q] + 1 > SP_DA_MAXWIN)
            return sp_fail(ctx, SP_EUNSUP, "%s: item %lld has a window of %lld residues (up to %d supported)", who, (long long)q,
                           (long long)i1[q] - i0[q] + 1, SP_DA_MAXWIN);
    }
    return SP_OK;
}

extern "C" {

int sp_dom_align_set_batch(sp_ctx *ctx, int64_t items) {
    if (!ctx || items < 0) return sp_fail(ctx, SP_EINVAL, "sp_dom_align_set_batch: %lld is below 0", (long long)items);
    ctx->da_batch = items;
    return SP_OK;
}

int sp_dom_peptide(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, const int32_t *frame, const int32_t *i0,
                   const int32_t *i1, const int64_t *poff, uint8_t *pep) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_dom_peptide: ctx is NULL");
    if (n < 0 || !poff || (n > 0 && (!chrom || !start || !end || !frame || !i0 || !i1 || !pep))) return sp_fail(ctx, SP_EINVAL, "sp_dom_peptide: bad arguments");
    int rc = da_check_items(ctx, "sp_dom_peptide", n, chrom, start, end, frame, i0, i1);
    if (rc) return rc;
    if (poff[0] != 0) return sp_fail(ctx, SP_EINVAL, "sp_dom_peptide: the peptide offsets start at %lld, not at 0", (long long)poff[0]);
    for (int64_t q = 0; q < n; q++)
        if (poff[q + 1] - poff[q] != (int64_t)i1[q] - i0[q] + 1)
            return sp_fail(ctx, SP_EINVAL, "sp_dom_peptide: item %lld: the offsets leave %lld bytes for a window of %lld residues", (long long)q,
                           (long long)(poff[q + 1] - poff[q]), (long long)i1[q] - i0[q] + 1);
    rc = da_check_limits(ctx, "sp_dom_peptide", n, start, end, i0, i1);
    if (rc) return rc;
    if (n > 0x7fffffffLL) return sp_fail(ctx, SP_EUNSUP, "sp_dom_peptide: %lld items in one call, at most %d", (long long)n, 0x7fffffff);
    if (n == 0) return SP_OK;
    try {
    std::vector<da_item> items((size_t)n);
    for (int64_t q = 0; q < n; q++) {
        const sp_chrom &c = ctx->chroms[(size_t)chrom[q]];
        items[(size_t)q] = da_item{c.d_pk, c.d_nm, start[q], poff[q], 0, 0, (int32_t)(end[q] - start[q]), frame[q], i0[q], i1[q] - i0[q] + 1, 0, (int32_t)q};
    }
    const size_t total = (size_t)poff[n];
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_carve sizes;
    sizes.take<da_item>((size_t)n);
    sizes.take<uint8_t>(total);
    sp_tmp<unsigned char> wsp;
    const hipError_t e = wsp.alloc(sizes.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_dom_peptide: %lld items, %lld residues, %lld bytes, do not fit on the device (%s)",
                       (long long)n, (long long)total, (long long)sizes.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    da_item *d_items = at.take<da_item>((size_t)n);
    uint8_t *d_res = at.take<uint8_t>(total);
    SP_HIP(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(da_item), hipMemcpyHostToDevice, ctx->stream));
    SP_LAUNCH(ctx, "da_residues", da_residues, dim3((unsigned)n), dim3(SP_DA_RTHREADS), 0, (const da_item *)d_items, d_res);
    SP_HIP(ctx, hipMemcpyAsync(pep, d_res, total, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
    } catch (const std::bad_alloc &) {
        return sp_fail(ctx, SP_ENOMEM, "sp_dom_peptide: the host list of %lld items does not fit in memory", (long long)n);
    }
}

int sp_dom_align(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, const int32_t *frame, const int32_t *i0,
                 const int32_t *i1, const int32_t *prof, int P, const int32_t *moff, const int32_t *emis, const int32_t *trans, const int32_t *entry,
                 int32_t *hit, const int64_t *coff, int32_t *col) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_dom_align: ctx is NULL");
    if (P < 1) return sp_fail(ctx, SP_EINVAL, "sp_dom_align: %d profiles (1 at least)", P);
    if (n < 0 || !moff || !emis || !trans || !entry || !coff || (n > 0 && (!chrom || !start || !end || !frame || !i0 || !i1 || !prof || !hit || !col)))
        return sp_fail(ctx, SP_EINVAL, "sp_dom_align: bad arguments");
    if (P > SP_DM_MAXP) return sp_fail(ctx, SP_EUNSUP, "sp_dom_align: %d profiles (up to %d supported)", P, SP_DM_MAXP);
    if (moff[0] != 0) return sp_fail(ctx, SP_EINVAL, "sp_dom_align: the node offsets start at %d, not at 0", moff[0]);
    for (int p = 0; p < P; p++)
        if (moff[p + 1] <= moff[p])
            return sp_fail(ctx, SP_EINVAL, "sp_dom_align: profile %d has %lld nodes (1 at least; the offsets ascend)", p, (long long)moff[p + 1] - moff[p]);
    int rc = da_check_items(ctx, "sp_dom_align", n, chrom, start, end, frame, i0, i1);
    if (rc) return rc;
    if (coff[0] != 0) return sp_fail(ctx, SP_EINVAL, "sp_dom_align: the column offsets start at %lld, not at 0", (long long)coff[0]);
    for (int64_t q = 0; q < n; q++) {
        if (prof[q] < 0 || prof[q] >= P) return sp_fail(ctx, SP_EINVAL, "sp_dom_align: item %lld: profile %d is outside 0..%d", (long long)q, prof[q], P - 1);
        const int M = moff[prof[q] + 1] - moff[prof[q]];
        if (coff[q + 1] - coff[q] != M)
            return sp_fail(ctx, SP_EINVAL, "sp_dom_align: item %lld: the offsets leave %lld columns for a profile of %d nodes", (long long)q,
                           (long long)(coff[q + 1] - coff[q]), M);
    }
    int maxM[2] = {0, 0};      // the largest profile with its tables in LDS, and above
    for (int p = 0; p < P; p++) {
        const int M = moff[p + 1] - moff[p];
        if (M > SP_DM_MAXM) return sp_fail(ctx, SP_EUNSUP, "sp_dom_align: profile %d has %d nodes (up to %d supported)", p, M, SP_DM_MAXM);
    }
    rc = da_check_limits(ctx, "sp_dom_align", n, start, end, i0, i1);
    if (rc) return rc;
    if (n > 0x7fffffffLL) return sp_fail(ctx, SP_EUNSUP, "sp_dom_align: %lld items in one call, at most %d", (long long)n, 0x7fffffff);
    for (int p = 0; p < P; p++)
        if (!sp_dm_tables_ok(moff[p + 1] - moff[p], emis + (int64_t)moff[p] * SP_DM_COLS, trans + (int64_t)moff[p] * 7, entry[p]))
            return sp_fail(ctx, SP_EINVAL, "sp_dom_align: profile %d has a score outside its range (-2^20 <= transitions, entry <= 0; -2^20 <= emissions <= 2^15)", p);
    if (n == 0) return SP_OK;
    const size_t nodes = (size_t)moff[P];
    try {
    std::vector<da_prof> profs((size_t)P);
    std::vector<int32_t> emisT(nodes * SP_DM_COLS), transT(nodes * 7);
    for (int p = 0; p < P; p++) {
        const int M = moff[p + 1] - moff[p];
        profs[(size_t)p] = da_prof{M, moff[p], entry[p], 0};
        const int32_t *e = emis + (int64_t)moff[p] * SP_DM_COLS, *t = trans + (int64_t)moff[p] * 7;
        int32_t *eT = emisT.data() + (size_t)moff[p] * SP_DM_COLS, *tT = transT.data() + (size_t)moff[p] * 7;
        for (int k = 0; k < M; k++) {
            for (int x = 0; x < SP_DM_COLS; x++) eT[(size_t)x * M + k] = e[(size_t)k * SP_DM_COLS + x];
            for (int x = 0; x < 7; x++) tT[(size_t)x * M + k] = t[(size_t)k * 7 + x];
        }
    }
    // the items in the caller's order, cut into batches whose planes fit the cap; inside a batch the items whose tables sit
    // in LDS first, each kind longest first
    std::vector<da_item> items((size_t)n);
    std::vector<size_t> cut(1, 0);      // batch b = items cut[b] .. cut[b + 1]
    int64_t total = 0, used = 0, largest = 0;
    for (int64_t q = 0; q < n; q++) {
        const sp_chrom &c = ctx->chroms[(size_t)chrom[q]];
        const int M = profs[(size_t)prof[q]].M, nwin = i1[q] - i0[q] + 1;
        maxM[M > SP_DA_TABM] = std::max(maxM[M > SP_DA_TABM], M);
        const int64_t bytes = (((int64_t)nwin * SP_DA_PITCH(M)) + 255) & ~255LL;
        const size_t in_batch = (size_t)q - cut.back();
        if (in_batch > 0 && (used + bytes > SP_DA_CAP || (ctx->da_batch > 0 && (int64_t)in_batch >= ctx->da_batch))) {
            cut.push_back((size_t)q);
            used = 0;
        }
        items[(size_t)q] = da_item{c.d_pk, c.d_nm, start[q], total, used, coff[q], (int32_t)(end[q] - start[q]), frame[q], i0[q], nwin, prof[q], (int32_t)q};
        used += bytes;
        largest = std::max(largest, used);
        total += nwin;
    }
    cut.push_back((size_t)n);
    std::vector<size_t> n_lds(cut.size() - 1);
    for (size_t b = 0; b + 1 < cut.size(); b++) {
        std::stable_sort(items.begin() + (ptrdiff_t)cut[b], items.begin() + (ptrdiff_t)cut[b + 1], [&](const da_item &x, const da_item &y) {
            const int Mx = profs[(size_t)x.prof].M, My = profs[(size_t)y.prof].M;
            const bool gx = Mx > SP_DA_TABM, gy = My > SP_DA_TABM;
            if (gx != gy) return gy;
            return (int64_t)x.nwin * Mx > (int64_t)y.nwin * My;
        });
        size_t m = cut[b];
        while (m < cut[b + 1] && profs[(size_t)items[m].prof].M <= SP_DA_TABM) m++;
        n_lds[b] = m - cut[b];
    }
    SP_HIP(ctx, hipSetDevice(ctx->device));
    da_item *d_items;
    da_prof *d_profs;
    int32_t *d_emis, *d_trans, *d_hit, *d_col;
    uint8_t *d_res, *d_planes;
    sp_dm_hit *d_hits;
    const size_t ncol = (size_t)coff[n];
    auto layout = [&](sp_carve &cv) {
        d_items = cv.take<da_item>((size_t)n);
        d_profs = cv.take<da_prof>((size_t)P);
        d_hits = cv.take<sp_dm_hit>((size_t)n);
        d_emis = cv.take<int32_t>(nodes * SP_DM_COLS);
        d_trans = cv.take<int32_t>(nodes * 7);
        d_hit = cv.take<int32_t>((size_t)n * 5);
        d_col = cv.take<int32_t>(ncol);
        d_res = cv.take<uint8_t>((size_t)total + 64);
        d_planes = cv.take<uint8_t>((size_t)largest);
    };
    sp_carve sizes;
    layout(sizes);
    sp_tmp<unsigned char> wsp;
    const hipError_t e = wsp.alloc(sizes.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_dom_align: %lld items, %lld residues, planes of %lld bytes, %lld bytes in all, do not fit on the device (%s)",
                       (long long)n, (long long)total, (long long)largest, (long long)sizes.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    layout(at);
    SP_HIP(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(da_item), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_profs, profs.data(), profs.size() * sizeof(da_prof), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_emis, emisT.data(), emisT.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_trans, transT.data(), transT.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_LAUNCH(ctx, "da_residues", da_residues, dim3((unsigned)n), dim3(SP_DA_RTHREADS), 0, (const da_item *)d_items, d_res);
    // LDS of a launch: six state arrays, two byte rows, the tables
    auto lds_of = [&](int g) {
        const size_t cap = (size_t)maxM[g] + 1;
        return 6 * cap * 8 + 2 * (size_t)SP_DA_PITCH(maxM[g]) + (g == 0 ? (size_t)29 * (size_t)maxM[0] * 4 : 0);      // at most 85040 (g = 0: 512 nodes with tables) and 102448 bytes (g = 1: 2048 nodes)
    };
    size_t lds_max = 0;
    for (int g = 0; g < 2; g++)
        if (maxM[g]) lds_max = std::max(lds_max, lds_of(g));
    SP_HIP(ctx, hipFuncSetAttribute((const void *)da_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    for (size_t b = 0; b + 1 < cut.size(); b++) {
        const size_t cnt[2] = {n_lds[b], cut[b + 1] - cut[b] - n_lds[b]}, first[2] = {cut[b], cut[b] + n_lds[b]};
        for (int g = 0; g < 2; g++) {
            if (!cnt[g]) continue;
            SP_LAUNCH(ctx, g == 0 ? "da_fill" : "da_fill_wide", da_fill, dim3((unsigned)cnt[g]), dim3(SP_DA_THREADS), lds_of(g), (const da_item *)(d_items + first[g]),
                      (const da_prof *)d_profs, (const int32_t *)d_emis, (const int32_t *)d_trans, (const uint8_t *)d_res, maxM[g] + 1, g == 0 ? maxM[0] : 0,
                      d_planes, d_hits + first[g]);
        }
        SP_LAUNCH(ctx, "da_trace", da_trace, dim3((unsigned)(cut[b + 1] - cut[b])), dim3(SP_DA_THREADS), 0, (const da_item *)(d_items + cut[b]),
                  (const da_prof *)d_profs, (const uint8_t *)d_planes, (const sp_dm_hit *)(d_hits + cut[b]), d_hit, d_col);
    }
    SP_HIP(ctx, hipMemcpyAsync(hit, d_hit, (size_t)n * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(col, d_col, ncol * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
    } catch (const std::bad_alloc &) {
        return sp_fail(ctx, SP_ENOMEM, "sp_dom_align: the host lists of %lld items and %d profiles do not fit in memory", (long long)n, P);
    }
}

int sp_aln_pairs(sp_ctx *ctx, int N, int C, const uint8_t *rows, int32_t *same, int32_t *both) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_aln_pairs: ctx is NULL");
    if (!rows || !same || !both) return sp_fail(ctx, SP_EINVAL, "sp_aln_pairs: bad arguments");
    if (N < 2 || C < 1) return sp_fail(ctx, SP_EINVAL, "sp_aln_pairs: %d rows of %d columns (2 rows and 1 column at least)", N, C);
    if (N > SP_DA_MAXN || C > SP_DA_MAXC)
        return sp_fail(ctx, SP_EUNSUP, "sp_aln_pairs: %d rows of %d columns (up to %d rows of %d columns supported)", N, C, SP_DA_MAXN, SP_DA_MAXC);
    const int Cp = (C + 7) & ~7;
    const size_t nn = (size_t)N * (size_t)N;
    try {
    std::vector<uint8_t> padded((size_t)N * (size_t)Cp, (uint8_t)SP_DA_GAP);
    for (int i = 0; i < N; i++) memcpy(padded.data() + (size_t)i * Cp, rows + (size_t)i * C, (size_t)C);
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_carve sizes;
    sizes.take<uint8_t>(padded.size());
    sizes.take<int32_t>(nn);
    sizes.take<int32_t>(nn);
    sp_tmp<unsigned char> wsp;
    const hipError_t e = wsp.alloc(sizes.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_aln_pairs: %d rows of %d columns and two %d x %d matrices, %lld bytes, do not fit on the device (%s)",
                       N, C, N, N, (long long)sizes.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    uint8_t *d_rows = at.take<uint8_t>(padded.size());
    int32_t *d_same = at.take<int32_t>(nn), *d_both = at.take<int32_t>(nn);
    const size_t lds = (size_t)2 * SP_DA_TILE * SP_DA_LPITCH;      // 66048 bytes
    SP_HIP(ctx, hipFuncSetAttribute((const void *)da_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SP_HIP(ctx, hipMemcpyAsync(d_rows, padded.data(), padded.size(), hipMemcpyHostToDevice, ctx->stream));
    const unsigned nt = (unsigned)((N + SP_DA_TILE - 1) / SP_DA_TILE);
    SP_LAUNCH(ctx, "da_pairs", da_pairs, dim3(nt, nt), dim3(SP_DA_PTHREADS), lds, (const uint8_t *)d_rows, N, Cp, d_same, d_both);
    SP_HIP(ctx, hipMemcpyAsync(same, d_same, nn * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(both, d_both, nn * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // `padded` is on this frame
    return SP_OK;
    } catch (const std::bad_alloc &) {
        return sp_fail(ctx, SP_ENOMEM, "sp_aln_pairs: the padded copy of %d rows of %d columns does not fit in memory", N, C);
    }
}

}  // extern "C"
