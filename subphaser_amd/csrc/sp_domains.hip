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
//   dm_ssv        the ungapped prefilter (sp_domains.h: S[i][k], ssv) of every (frame, profile).  A cell depends on its
//                 diagonal alone, so a LANE owns diagonals: it walks the nodes 1..M with one int32 per diagonal and never
//                 talks to another lane.  The frames with residues lie one behind the other in the workspace, in the
//                 order dm_translate wrote them; frame f of n residues has the n + M - 1 diagonals j = 0 .. n + M - 2
//                 (j = i - k + M), and the diagonals of all frames against one profile form ONE line of
//                 G = residues + frames * (M - 1) slots.  A workgroup of 256 lanes takes `span` consecutive slots of one
//                 profile's line (1024: four diagonals a lane, 256 slots apart, so that a wave reads 64 neighbouring
//                 residues), whichever frames they fall in: short frames share a workgroup, a long one is cut over
//                 several, and the profile's tables are read once per 1024 diagonals, not once per item.  The workgroup
//                 finds its first frame by bisection of the frame list, puts the slot at which each of its frames starts
//                 in LDS (at most `span` frames: every frame has a diagonal), and copies the residues its slots read
//                 to LDS -- one contiguous piece of the workspace of at most span + M bytes (below).  Then the nodes go
//                 by in TILES of `tile` (128) nodes: the tile's emissions NODE-major ([node][22]: the 22 words a step can
//                 read are 22 different banks; the lanes of a wave are on the same node) and its m->m transitions are
//                 loaded behind a barrier, and every lane carries its four S from tile to tile in registers, so LDS does
//                 not grow with M: 18.9 KB for any profile (86 VGPRs: 20 waves a CU).  A wave with no cell in a tile skips it.  The maximum of a
//                 diagonal goes to the item's int32 by atomicMax (one per wave where the wave's 64 diagonals are of
//                 one frame) -- a max of integers: any order gives the same bytes.  No result depends on `tile` or
//                 `span` (sp_dom_ssv_set_tile; the tests run several).
//                 Residues staged: the first slot g0 is diagonal j0 of frame f0 and reads residues i >= j0 - M + 1; the
//                 last slot is diagonal jl of frame fl and reads i <= jl; the frames between are read whole.  As the
//                 slots of a frame are its residues + M - 1, the piece [roff(f0) + max(0, j0 - M + 1), roff(fl) + min(n,
//                 jl + 1)) has at most span + M - 1 bytes.  Reads are clamped to the piece all the same.
//   No kernel caps its grid (elements; items; entries; spans of diagonals), none loops over items, none waits on another
//   workgroup, every loop is bounded by the residues of a frame, the nodes of a profile or the slots of a workgroup.
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

// ---- the ungapped prefilter
#define SP_DM_STHREADS 256
#define SP_DM_SDIAG 4                                   // diagonals a lane carries
#define SP_DM_SSPAN (SP_DM_STHREADS * SP_DM_SDIAG)      // slots of a workgroup, at most
#define SP_DM_STILE 128                                 // nodes of a tile, at most
#define SP_DM_SRES (SP_DM_SSPAN + SP_DM_MAXM)           // residue bytes a workgroup stages, at most (head comment)

struct dm_frame {
    int64_t roff;          // where the frame's residues start = the residues of the frames listed in front of it
    int32_t nres, ef;      // ef: element * 6 + frame
};

// frames: the F frames with residues, in workspace order; total: their residues; boff[p]: the workgroups in front of
// profile p's; emis, trans: the caller's tables ([node][22], [node][7])
__global__ void __launch_bounds__(SP_DM_STHREADS)
dm_ssv(const dm_frame *__restrict__ frames, int64_t F, int64_t total, const dm_prof *__restrict__ profs, const int64_t *__restrict__ boff, int P,
       const int32_t *__restrict__ emis, const int32_t *__restrict__ trans, const uint8_t *__restrict__ res, int tile, int span,
       int32_t *__restrict__ out) {
    __shared__ int32_t s_e[SP_DM_STILE * SP_DM_COLS];
    __shared__ int32_t s_t[SP_DM_STILE];
    __shared__ int32_t s_key[SP_DM_SSPAN];
    __shared__ __attribute__((aligned(16))) uint8_t s_res[SP_DM_SRES];
    __shared__ int s_nf;
    const int tid = threadIdx.x;
    if (tile < 1 || tile > SP_DM_STILE || span < 1 || span > SP_DM_SSPAN || F < 1) return;      // (the host sends none of these)
    const int64_t b = blockIdx.x;
    int p = 0;
    for (int hi = P; hi - p > 1;) {
        const int mid = (p + hi) >> 1;
        if (boff[mid] <= b) p = mid;
        else hi = mid;
    }
    const dm_prof pf = profs[p];
    const int M = pf.M;
    const int64_t step = M - 1;                              // frame f starts at slot frames[f].roff + f * step
    const int64_t G = total + F * step, g0 = (b - boff[p]) * span;
    if (M < 1 || g0 >= G) return;
    const int64_t g1 = min(G, g0 + span);                    // behind this workgroup's last slot
    int64_t f0 = 0;
    for (int64_t hi = F; hi - f0 > 1;) {
        const int64_t mid = (f0 + hi) >> 1;
        if (frames[mid].roff + mid * step <= g0) f0 = mid;
        else hi = mid;
    }
    if (tid == 0) s_nf = 0;
    __syncthreads();
    for (int q = tid; q < span; q += SP_DM_STHREADS) {
        const int64_t f = f0 + q;
        if (f >= F) break;
        const int64_t key = frames[f].roff + f * step;
        if (key >= g1) break;
        s_key[q] = (int32_t)(key - g0);                      // (below 0 for the first frame when it starts in front of g0)
        atomicMax(&s_nf, q + 1);
    }
    __syncthreads();
    const int nf = s_nf;
    const dm_frame first = frames[f0], last = frames[f0 + nf - 1];
    const int64_t j0 = g0 - (first.roff + f0 * step), jl = g1 - 1 - (last.roff + (f0 + nf - 1) * step);
    const int64_t A = first.roff + max((int64_t)0, j0 - M + 1), B = last.roff + min((int64_t)last.nres, jl + 1);
    const int cnt = (int)min(B - A, (int64_t)SP_DM_SRES);
    if (cnt < 1) return;                                     // (never: the first slot has a cell)
    for (int q = tid; q < cnt; q += SP_DM_STHREADS) s_res[q] = res[A + q];
    int d[SP_DM_SDIAG], n[SP_DM_SDIAG], rb[SP_DM_SDIAG], u[SP_DM_SDIAG], S[SP_DM_SDIAG], best[SP_DM_SDIAG];
    int64_t oidx[SP_DM_SDIAG];
#pragma unroll
    for (int r = 0; r < SP_DM_SDIAG; r++) {
        const int q = r * SP_DM_STHREADS + tid;
        d[r] = 0, n[r] = 0, rb[r] = 0, u[r] = -1, S[r] = SP_DM_SSV_NONE, best[r] = INT32_MIN, oidx[r] = 0;
        if (q < span && g0 + q < g1) {
            int lo = 0;
            for (int hi = nf; hi - lo > 1;) {
                const int mid = (lo + hi) >> 1;
                if (s_key[mid] <= q) lo = mid;
                else hi = mid;
            }
            const dm_frame fr = frames[f0 + lo];
            u[r] = lo;
            d[r] = q - s_key[lo] - M;                        // i - k of this diagonal: -M .. nres - 2
            n[r] = fr.nres;
            rb[r] = (int)(fr.roff - A);
            oidx[r] = ((int64_t)(fr.ef / 6) * P + p) * 6 + fr.ef % 6;
        }
    }
    const int32_t *E = emis + (int64_t)SP_DM_COLS * pf.off, *T = trans + (int64_t)7 * pf.off;
    const int entry = pf.entry;
    for (int kb0 = 0; kb0 < M; kb0 += tile) {
        const int tk = min(tile, M - kb0);                   // nodes kb0 + 1 .. kb0 + tk
        __syncthreads();                                     // the tile in front is read (first tile: the residues are there)
        for (int q = tid; q < tk * SP_DM_COLS; q += SP_DM_STHREADS) s_e[q] = E[(int64_t)kb0 * SP_DM_COLS + q];
        for (int q = tid; q < tk; q += SP_DM_STHREADS) s_t[q] = kb0 + q >= 1 ? T[(int64_t)(kb0 + q - 1) * 7 + SP_DM_MM] : 0;
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int r = 0; r < SP_DM_SDIAG; r++) any |= n[r] > 0 && max(1, -d[r]) <= kb0 + tk && min(M, n[r] - 1 - d[r]) >= kb0 + 1;
        if (!__any(any)) continue;                           // no cell of this wave in the tile
        for (int kk = 0; kk < tk; kk++) {
            const int k = kb0 + kk + 1, t = s_t[kk];
            const int32_t *row = s_e + kk * SP_DM_COLS;
#pragma unroll
            for (int r = 0; r < SP_DM_SDIAG; r++) {
                const int i = d[r] + k;
                const bool on = (unsigned)i < (unsigned)n[r];
                const int x = s_res[min(max(rb[r] + i, 0), cnt - 1)];
                const int32_t s = sp_dm_ssv_cell(S[r], t, entry, row[x]);
                S[r] = on ? s : SP_DM_SSV_NONE;
                best[r] = on && s > best[r] ? s : best[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < SP_DM_SDIAG; r++) {
        const int u0 = __shfl(u[r], 0);
        if (__all(u[r] == u0)) {                             // the wave's 64 diagonals are of one frame (or are none)
            if (u0 < 0) continue;
            int m = best[r];
            for (int o = 32; o; o >>= 1) m = max(m, __shfl_xor(m, o));
            if ((tid & 63) == 0) atomicMax(out + oidx[r], m);
        } else if (u[r] >= 0)
            atomicMax(out + oidx[r], best[r]);
    }
}

// what an entry of this unit runs
enum dm_mode { DM_SEARCH, DM_SSV, DM_PRE };

// The three entries: one set of checks, one element list, one translation.  DM_SEARCH is sp_dom_search as it always was.
// DM_SSV: translate, dm_ssv, the scores.  DM_PRE: translate, dm_ssv, the scores to the host, where the items with
// ssv >= threshold are listed and sorted as DM_SEARCH lists and sorts all of them, dm_search on those, dm_pick.
static int dm_run(sp_ctx *ctx, const char *who, dm_mode mode, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P,
                  const int32_t *moff, const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t threshold, int32_t *out, int64_t *stats) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "%s: ctx is NULL", who);
    if (P < 1) return sp_fail(ctx, SP_EINVAL, "%s: %d profiles (1 at least)", who, P);
    if (n < 0 || (n > 0 && (!chrom || !start || !end || !out)) || !moff || !emis || !trans || !entry || (mode == DM_PRE && !stats))
        return sp_fail(ctx, SP_EINVAL, "%s: bad arguments", who);
    if (P > SP_DM_MAXP) return sp_fail(ctx, SP_EUNSUP, "%s: %d profiles (up to %d supported)", who, P, SP_DM_MAXP);
    const int C = (int)ctx->chroms.size();
    if (C == 0) return sp_fail(ctx, SP_EINVAL, "%s: no genome loaded (sp_genome_add first)", who);
    if (moff[0] != 0) return sp_fail(ctx, SP_EINVAL, "%s: the node offsets start at %d, not at 0", who, moff[0]);
    for (int p = 0; p < P; p++)
        if (moff[p + 1] <= moff[p])
            return sp_fail(ctx, SP_EINVAL, "%s: profile %d has %lld nodes (1 at least; the offsets ascend)", who, p, (long long)moff[p + 1] - moff[p]);
    for (int64_t i = 0; i < n; i++) {
        if (chrom[i] < 0 || chrom[i] >= C) return sp_fail(ctx, SP_EINVAL, "%s: element %lld: chromosome %d out of range", who, (long long)i, chrom[i]);
        const sp_chrom &c = ctx->chroms[(size_t)chrom[i]];
        if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "%s: element %lld: chromosome %d has no packed sequence (sp_genome_add first)", who, (long long)i, chrom[i]);
        if (start[i] < 0 || end[i] < start[i] || end[i] > c.len)
            return sp_fail(ctx, SP_EINVAL, "%s: element %lld = [%lld, %lld) is outside chromosome %d (%lld bases) or ends before it starts",
                           who, (long long)i, (long long)start[i], (long long)end[i], chrom[i], (long long)c.len);
    }
    int maxM[2] = {0, 0};      // the largest profile with its tables in LDS, and above
    for (int p = 0; p < P; p++) {
        const int M = moff[p + 1] - moff[p];
        if (M > SP_DM_MAXM) return sp_fail(ctx, SP_EUNSUP, "%s: profile %d has %d nodes (up to %d supported)", who, p, M, SP_DM_MAXM);
        maxM[M > SP_DM_TABM] = std::max(maxM[M > SP_DM_TABM], M);
    }
    for (int64_t i = 0; i < n; i++)
        if (end[i] - start[i] > SP_DM_MAXLEN)
            return sp_fail(ctx, SP_EUNSUP, "%s: element %lld has %lld bases (up to %d supported)", who, (long long)i, (long long)(end[i] - start[i]), SP_DM_MAXLEN);
    if (n * (int64_t)P > SP_DM_MAXOUT)
        return sp_fail(ctx, SP_EUNSUP, "%s: %lld elements x %d profiles in one call (up to %lld entries)", who, (long long)n, P, (long long)SP_DM_MAXOUT);
    for (int p = 0; p < P; p++)
        if (!sp_dm_tables_ok(moff[p + 1] - moff[p], emis + (int64_t)moff[p] * SP_DM_COLS, trans + (int64_t)moff[p] * 7, entry[p]))
            return sp_fail(ctx, SP_EINVAL, "%s: profile %d has a score outside its range (-2^20 <= transitions, entry <= 0; -2^20 <= emissions <= 2^15)", who, p);
    if (stats) stats[0] = stats[1] = 0;
    if (n == 0) return SP_OK;
    const size_t nodes = (size_t)moff[P], entries = (size_t)n * (size_t)P;
    const bool search = mode != DM_SSV, ssv = mode != DM_SEARCH;
    try {      // (the host lists below grow with n x P: a failed allocation is SP_ENOMEM, not an exception through the C entry)
    std::vector<dm_elem> elems((size_t)n);
    std::vector<dm_prof> profs((size_t)P);
    std::vector<int32_t> emisT(search ? nodes * SP_DM_COLS : 0), transT(search ? nodes * 7 : 0);
    for (int p = 0; p < P; p++) {
        const int M = moff[p + 1] - moff[p];
        profs[(size_t)p] = dm_prof{M, moff[p], entry[p], 0};
        if (!search) continue;
        const int32_t *e = emis + (int64_t)moff[p] * SP_DM_COLS, *t = trans + (int64_t)moff[p] * 7;
        int32_t *eT = emisT.data() + (size_t)moff[p] * SP_DM_COLS, *tT = transT.data() + (size_t)moff[p] * 7;
        for (int k = 0; k < M; k++) {
            for (int x = 0; x < SP_DM_COLS; x++) eT[(size_t)x * M + k] = e[(size_t)k * SP_DM_COLS + x];
            for (int x = 0; x < 7; x++) tT[(size_t)x * M + k] = t[(size_t)k * 7 + x];
        }
    }
    // the elements, the frames with residues in the order dm_translate writes them, and (DM_SEARCH) the items
    int64_t total = 0;
    std::vector<dm_item> items;
    std::vector<dm_frame> frames;
    if (mode == DM_SEARCH) items.reserve(entries * 6);
    else frames.reserve((size_t)n * 6);
    for (int64_t i = 0; i < n; i++) {
        const sp_chrom &c = ctx->chroms[(size_t)chrom[i]];
        const int64_t len = end[i] - start[i];
        elems[(size_t)i] = dm_elem{c.d_pk, c.d_nm, start[i], total, (int32_t)len, 0};
        for (int f = 0; f < 6; f++) {
            const int32_t nr = sp_dm_nres(len, f);
            if (nr > 0) {
                if (mode == DM_SEARCH)
                    for (int p = 0; p < P; p++) items.push_back(dm_item{total, nr, p, (int32_t)((i * P + p) * 6 + f), 0});
                else
                    frames.push_back(dm_frame{total, nr, (int32_t)(i * 6 + f)});
            }
            total += nr;
        }
    }
    const size_t n_with = mode == DM_SEARCH ? items.size() : frames.size() * (size_t)P;      // items with residues
    // dm_ssv: the workgroups of every profile's line of slots
    const int tile = ctx->ds_tile > 0 ? ctx->ds_tile : SP_DM_STILE, span = ctx->ds_span > 0 ? ctx->ds_span : SP_DM_SSPAN;
    std::vector<int64_t> boff((size_t)P + 1, 0);
    if (ssv) {
        for (int p = 0; p < P; p++) {
            const int64_t G = frames.empty() ? 0 : total + (int64_t)frames.size() * (profs[(size_t)p].M - 1);
            boff[(size_t)p + 1] = boff[(size_t)p] + (G + span - 1) / span;
        }
        if (boff[(size_t)P] > INT32_MAX)
            return sp_fail(ctx, SP_EUNSUP, "%s: %lld elements x %d profiles are %lld spans of %d diagonals (up to %d in one call)", who, (long long)n, P,
                           (long long)boff[(size_t)P], span, INT32_MAX);
    }
    // the items whose tables sit in LDS first, each kind longest first
    size_t n_lds = 0;
    auto sort_items = [&]() {
        std::stable_sort(items.begin(), items.end(), [&](const dm_item &a, const dm_item &b) {
            const int Ma = profs[(size_t)a.prof].M, Mb = profs[(size_t)b.prof].M;
            const bool ga = Ma > SP_DM_TABM, gb = Mb > SP_DM_TABM;
            if (ga != gb) return gb;
            return (int64_t)a.nres * Ma > (int64_t)b.nres * Mb;
        });
        n_lds = 0;
        while (n_lds < items.size() && profs[(size_t)items[n_lds].prof].M <= SP_DM_TABM) n_lds++;
    };
    if (mode == DM_SEARCH) sort_items();
    SP_HIP(ctx, hipSetDevice(ctx->device));
    dm_elem *d_elems;
    dm_item *d_items = nullptr;
    dm_prof *d_profs;
    dm_frame *d_frames = nullptr;
    int64_t *d_boff = nullptr;
    int32_t *d_emis = nullptr, *d_trans = nullptr, *d_out = nullptr, *d_emis_n = nullptr, *d_trans_n = nullptr, *d_ssv = nullptr;
    uint8_t *d_res;
    sp_dm_hit *d_hits = nullptr;
    auto layout = [&](sp_carve &cv) {
        d_elems = cv.take<dm_elem>((size_t)n);
        if (search) d_items = cv.take<dm_item>(n_with + 1);
        d_profs = cv.take<dm_prof>((size_t)P);
        if (search) {
            d_hits = cv.take<sp_dm_hit>(entries * 6);
            d_emis = cv.take<int32_t>(nodes * SP_DM_COLS);
            d_trans = cv.take<int32_t>(nodes * 7);
            d_out = cv.take<int32_t>(entries * 6);
        }
        d_res = cv.take<uint8_t>((size_t)total + 64);
        if (ssv) {
            d_frames = cv.take<dm_frame>(frames.size() + 1);
            d_boff = cv.take<int64_t>((size_t)P + 1);
            d_emis_n = cv.take<int32_t>(nodes * SP_DM_COLS);
            d_trans_n = cv.take<int32_t>(nodes * 7);
            d_ssv = cv.take<int32_t>(entries * 6);
        }
    };
    sp_carve sizes;
    layout(sizes);
    sp_tmp<unsigned char> wsp;
    const hipError_t e = wsp.alloc(sizes.off);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "%s: %lld elements x %d profiles, %lld residues, %lld bytes, do not fit on the device (%s)",
                       who, (long long)n, P, (long long)total, (long long)sizes.off, hipGetErrorString(e));
    }
    sp_carve at(wsp.p);
    layout(at);
    SP_HIP(ctx, hipMemcpyAsync(d_elems, elems.data(), elems.size() * sizeof(dm_elem), hipMemcpyHostToDevice, ctx->stream));
    if (mode == DM_SEARCH && !items.empty())
        SP_HIP(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(dm_item), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_profs, profs.data(), profs.size() * sizeof(dm_prof), hipMemcpyHostToDevice, ctx->stream));
    if (search) {
        SP_HIP(ctx, hipMemcpyAsync(d_emis, emisT.data(), emisT.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(d_trans, transT.data(), transT.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        SP_HIP(ctx, hipMemsetAsync(d_hits, 0, entries * 6 * sizeof(sp_dm_hit), ctx->stream));      // k = 0: no hit
    }
    SP_LAUNCH(ctx, "dm_translate", dm_translate, dim3((unsigned)n), dim3(SP_DM_TTHREADS), 0, (const dm_elem *)d_elems, d_res);
    if (ssv) {
        SP_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)d_ssv, INT32_MIN, entries * 6, ctx->stream));      // no residues: no score
        if (!frames.empty()) {
            SP_HIP(ctx, hipMemcpyAsync(d_frames, frames.data(), frames.size() * sizeof(dm_frame), hipMemcpyHostToDevice, ctx->stream));
            SP_HIP(ctx, hipMemcpyAsync(d_boff, boff.data(), boff.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            SP_HIP(ctx, hipMemcpyAsync(d_emis_n, emis, nodes * SP_DM_COLS * 4, hipMemcpyHostToDevice, ctx->stream));
            SP_HIP(ctx, hipMemcpyAsync(d_trans_n, trans, nodes * 7 * 4, hipMemcpyHostToDevice, ctx->stream));
            SP_LAUNCH(ctx, "dm_ssv", dm_ssv, dim3((unsigned)boff[(size_t)P]), dim3(SP_DM_STHREADS), 0, (const dm_frame *)d_frames, (int64_t)frames.size(), total,
                      (const dm_prof *)d_profs, (const int64_t *)d_boff, P, (const int32_t *)d_emis_n, (const int32_t *)d_trans_n, (const uint8_t *)d_res, tile,
                      span, d_ssv);
        }
        if (mode == DM_SSV) {
            SP_HIP(ctx, hipMemcpyAsync(out, d_ssv, entries * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return SP_OK;
        }
        // the survivors, listed in the order DM_SEARCH lists every item
        std::vector<int32_t> score(entries * 6);
        SP_HIP(ctx, hipMemcpyAsync(score.data(), d_ssv, entries * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (const dm_frame &fr : frames) {
            const int64_t i = fr.ef / 6;
            const int f = fr.ef % 6;
            for (int p = 0; p < P; p++) {
                const int32_t slot = (int32_t)((i * P + p) * 6 + f);
                if (score[(size_t)slot] >= threshold) items.push_back(dm_item{fr.roff, fr.nres, p, slot, 0});
            }
        }
        sort_items();
        stats[0] = (int64_t)n_with;
        stats[1] = (int64_t)items.size();
        if (!items.empty()) SP_HIP(ctx, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(dm_item), hipMemcpyHostToDevice, ctx->stream));
    }
    const size_t cnt[2] = {n_lds, items.size() - n_lds};
    int runM[2] = {maxM[0], maxM[1]};      // the largest profile of each kind among the items that run
    if (mode == DM_PRE) {
        runM[0] = runM[1] = 0;
        for (const dm_item &it : items) {
            const int M = profs[(size_t)it.prof].M;
            runM[M > SP_DM_TABM] = std::max(runM[M > SP_DM_TABM], M);
        }
    }
    size_t lds_max = 0;
    for (int g = 0; g < 2; g++)
        if (cnt[g]) lds_max = std::max(lds_max, (size_t)6 * (size_t)(runM[g] + 1) * 8 + (g == 0 ? (size_t)29 * (size_t)runM[0] * 4 : 0));
    if (lds_max) SP_HIP(ctx, hipFuncSetAttribute((const void *)dm_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    for (int g = 0; g < 2; g++) {
        if (!cnt[g]) continue;
        const int cap = runM[g] + 1, tabM = g == 0 ? runM[0] : 0;
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
        return sp_fail(ctx, SP_ENOMEM, "%s: the host lists of %lld elements x %d profiles do not fit in memory", who, (long long)n, P);
    }
}

extern "C" {

int sp_dom_search(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P, const int32_t *moff,
                  const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t *out) {
    return dm_run(ctx, "sp_dom_search", DM_SEARCH, n, chrom, start, end, P, moff, emis, trans, entry, 0, out, nullptr);
}

int sp_dom_ssv(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P, const int32_t *moff,
               const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t *out) {
    return dm_run(ctx, "sp_dom_ssv", DM_SSV, n, chrom, start, end, P, moff, emis, trans, entry, 0, out, nullptr);
}

int sp_dom_search_pre(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P, const int32_t *moff,
                      const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t threshold, int32_t *out, int64_t *stats) {
    return dm_run(ctx, "sp_dom_search_pre", DM_PRE, n, chrom, start, end, P, moff, emis, trans, entry, threshold, out, stats);
}

int sp_dom_ssv_set_tile(sp_ctx *ctx, int nodes, int span) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_dom_ssv_set_tile: ctx is NULL");
    if (nodes < 0 || nodes > SP_DM_STILE || span < 0 || span > SP_DM_SSPAN)
        return sp_fail(ctx, SP_EINVAL, "sp_dom_ssv_set_tile: a tile of %d nodes, %d diagonals a workgroup (0 = the default; up to %d, %d)", nodes, span,
                       SP_DM_STILE, SP_DM_SSPAN);
    ctx->ds_tile = nodes;
    ctx->ds_span = span;
    return SP_OK;
}

}  // extern "C"
