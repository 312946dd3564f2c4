// sp_blocks.hip -- homoeologous blocks from shared single-copy k-mers (definition: sp_blocks.h).
//
// Per chromosome an INDEX: an open-addressing table over the sampled keys -- 64-bit key, 32-bit value (pos << 1 | fw,
// SP_BK_DUP once a second start of the key was seen).  bk_count sizes it (one and a half entries per sampled start, so it
// can never fill), bk_build fills it with one scan and 64-bit compare-and-swap, after that it is read-only.  Per ordered
// pair ONE kernel, bk_pair: a workgroup owns whole A-windows; it rescans the window's starts, looks every sampled key
// up in A's index (single copy?) and in B's (single copy?) and tallies the anchor's cell (wb, opp) in an LDS hash of
// `cells` entries.  A window with more distinct cells than that is tallied again by BAND passes: direct counters over
// `cells` consecutive cell numbers at a time, from the smallest to the largest cell the first pass saw -- any number of
// cells, no assumption about the LDS.  The anchors themselves are produced on request only (sp_blocks_anchors: count per
// 32-start unit, one-block scan, write), for tests and small inputs.  No library sort anywhere.
#include "sp_blocks.h"
#include "sp_common.h"
#include "sp_device.h"
#include "sp_internal.h"

#define SP_BK_EMPTY (~0ULL)            // keys are below 2^62
#define SP_BK_NONE 0xffffffffu
#define SP_BK_DUP 0xfffffffeu          // values are below 2^32 - 32 (SP_BK_MAXLEN)
#define SP_BK_THREADS 256
#define SP_BK_MAXCELLS 4096

struct sp_bk_index {
    unsigned long long *d_keys = nullptr;   // [cap], then the values: one allocation
    uint32_t *d_vals = nullptr;
    uint32_t cap = 0;
    int kb = 0, s = 0;
    int64_t n_sampled = 0, n_single = 0;
};
struct sp_blocks_state {
    std::vector<sp_bk_index> idx;
    int cells = SP_BK_MAXCELLS;
    int lastA = -1, lastB = -1;             // the pair sp_blocks_anchors answers for
    int64_t last_n = 0;
    sp_buf b_out, b_small;
};

struct bk_table {
    const unsigned long long *keys;
    const uint32_t *vals;
    uint32_t cap;
};

// value of `key` in a finished index: SP_BK_NONE when absent.  The table is at most two thirds full: the walk ends.
__device__ __forceinline__ uint32_t bk_lookup(const bk_table &t, uint64_t key, uint64_t mixed) {
    uint32_t h = sp_bk_home(mixed, t.cap);
    for (;;) {
        const unsigned long long k = t.keys[h];
        if (k == key) return t.vals[h];
        if (k == SP_BK_EMPTY) return SP_BK_NONE;
        h = (h + 1 == t.cap) ? 0u : h + 1;
    }
}

// ---------------------------------------------------------------- index
__global__ void __launch_bounds__(SP_BK_THREADS)
bk_count(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, int64_t n_units,
         sp_kparams kp, int s, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long n = 0;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x)
        sp_scan32_valid64(pk, pm, nm, u * 32, kp, [&](int64_t, uint64_t fwd, uint64_t rc) {
            n += sp_bk_sampled(fwd < rc ? fwd : rc, s) ? 1u : 0u;
        });
    const unsigned long long t = sp_block_sum_u64(n, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

__device__ __attribute__((noinline)) void bk_insert(unsigned long long *keys, uint32_t *vals, uint32_t cap, uint64_t key,
                                                    uint64_t mixed, uint32_t v, unsigned long long *flags) {
    uint32_t h = sp_bk_home(mixed, cap);
    for (uint32_t probes = 0; probes < cap; probes++) {
        const unsigned long long old = atomicCAS(&keys[h], SP_BK_EMPTY, (unsigned long long)key);
        if (old == SP_BK_EMPTY || old == key) {
            if (atomicCAS(&vals[h], SP_BK_NONE, v) != SP_BK_NONE) atomicExch(&vals[h], SP_BK_DUP);
            return;
        }
        h = (h + 1 == cap) ? 0u : h + 1;
    }
    atomicAdd(&flags[1], 1ULL);       // every entry taken by another key: the host reports it, nothing is dropped silently
}

__global__ void __launch_bounds__(SP_BK_THREADS)
bk_build(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, int64_t n_units,
         sp_kparams kp, int s, unsigned long long *keys, uint32_t *vals, uint32_t cap, unsigned long long *flags) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x)
        sp_scan32_valid64(pk, pm, nm, u * 32, kp, [&](int64_t pos, uint64_t fwd, uint64_t rc) {
            const bool fw = fwd < rc;
            const uint64_t key = fw ? fwd : rc, mixed = sp_bk_mix(key);
            if (sp_bk_sampled_mix(mixed, s)) bk_insert(keys, vals, cap, key, mixed, ((uint32_t)pos << 1) | (fw ? 1u : 0u), flags);
        });
}

__global__ void __launch_bounds__(SP_BK_THREADS)
bk_singles(const uint32_t *__restrict__ vals, uint32_t cap, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long n = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)cap; i += (int64_t)gridDim.x * blockDim.x)
        n += vals[i] < SP_BK_DUP ? 1u : 0u;
    const unsigned long long t = sp_block_sum_u64(n, red);
    if (threadIdx.x == 0 && t) atomicAdd(out + 2, t);
}

// ---------------------------------------------------------------- pair
struct bk_pair_args {
    const uint32_t *pk, *pm, *nm;
    int64_t lenA, bin;
    int32_t n_wa, n_wb;
    uint32_t bin32;            // min(bin, 2^31 - 1): positions are below that, the quotient is the same
    sp_kparams kp;
    int s, cells, cell_shift;  // cells = 1 << (32 - cell_shift)
    bk_table A, B;
};
// the anchor of a sampled start of A, if it is one: (posB << 1 | opp) or SP_BK_NONE
__device__ __forceinline__ uint32_t bk_anchor(const bk_table &A, const bk_table &B, uint64_t key, uint64_t mixed, bool fw) {
    if (bk_lookup(A, key, mixed) >= SP_BK_DUP) return SP_BK_NONE;      // (a single-copy key of A: this start is its record)
    const uint32_t vb = bk_lookup(B, key, mixed);
    if (vb >= SP_BK_DUP) return SP_BK_NONE;
    return (vb & ~1u) | (((vb & 1u) != 0) != fw ? 1u : 0u);
}

struct bk_lds {
    uint32_t ck[SP_BK_MAXCELLS], cc[SP_BK_MAXCELLS];
    unsigned long long best;
    uint32_t total, lo, hi, spilled;
};
// one per workgroup of bk_pair; named here so that bk_tally, which is not inlined into the 32 starts of a unit, reaches it
// with LDS instructions
__shared__ bk_lds L;

// band < 0: hash tally (the first pass); band >= 0: direct counters of the cells [band, band + cells)
__device__ __attribute__((noinline)) void bk_tally(const bk_pair_args &P, uint64_t key, uint64_t mixed, bool fw, int64_t band) {
    const uint32_t a = bk_anchor(P.A, P.B, key, mixed, fw);
    if (a == SP_BK_NONE) return;
    const uint32_t wb = (a >> 1) / P.bin32, opp = a & 1u;
    const uint32_t dense = opp * (uint32_t)P.n_wb + wb;                 // below 2^32: n_wb fits int32
    if (band >= 0) {
        const int64_t r = (int64_t)dense - band;
        if (r >= 0 && r < P.cells) atomicAdd(&L.cc[r], 1u);
        return;
    }
    atomicAdd(&L.total, 1u);
    atomicMin(&L.lo, dense);
    atomicMax(&L.hi, dense);
    const uint32_t cell = sp_bk_cell((int32_t)wb, (int)opp);
    uint32_t h = P.cell_shift >= 32 ? 0u : (cell * 2654435761u) >> P.cell_shift;
    for (int probes = 0; probes < P.cells; probes++) {
        const uint32_t old = atomicCAS(&L.ck[h], SP_BK_NONE, cell);
        if (old == SP_BK_NONE || old == cell) {
            atomicAdd(&L.cc[h], 1u);
            return;
        }
        h = (h + 1 == (uint32_t)P.cells) ? 0u : h + 1;
    }
    L.spilled = 1u;       // more distinct cells than the table holds: the band passes count this window again
}

__device__ __forceinline__ void bk_scan_window(const bk_pair_args &P, int64_t p0, int64_t p1, int64_t band) {
    const int64_t u0 = p0 >> 5, u1 = (p1 - 1) >> 5;
    for (int64_t u = u0 + threadIdx.x; u <= u1; u += blockDim.x)
        sp_scan32_valid64(P.pk, P.pm, P.nm, u * 32, P.kp, [&](int64_t pos, uint64_t fwd, uint64_t rc) {
            const bool fw = fwd < rc;
            const uint64_t key = fw ? fwd : rc, mixed = sp_bk_mix(key);
            if (sp_bk_sampled_mix(mixed, P.s) && pos >= p0 && pos < p1) bk_tally(P, key, mixed, fw, band);
        });
}

__global__ void __launch_bounds__(SP_BK_THREADS)
bk_pair(bk_pair_args P, int32_t *__restrict__ win_b, uint8_t *__restrict__ opp, int32_t *__restrict__ votes,
        int32_t *__restrict__ total, unsigned long long *__restrict__ flags) {
    unsigned long long n_anchors = 0, n_spilled = 0;      // thread 0's
    for (int32_t wa = blockIdx.x; wa < P.n_wa; wa += gridDim.x) {
        const int64_t p0 = (int64_t)wa * P.bin, p1 = (p0 + P.bin < P.lenA) ? p0 + P.bin : P.lenA;
        for (int i = threadIdx.x; i < P.cells; i += blockDim.x) {
            L.ck[i] = SP_BK_NONE;
            L.cc[i] = 0u;
        }
        if (threadIdx.x == 0) {
            L.best = 0ULL;
            L.total = 0u;
            L.lo = 0xffffffffu;
            L.hi = 0u;
            L.spilled = 0u;
        }
        __syncthreads();
        bk_scan_window(P, p0, p1, -1);
        __syncthreads();
        const bool spilled = L.spilled != 0u;
        if (!spilled) {
            unsigned long long b = 0ULL;
            for (int i = threadIdx.x; i < P.cells; i += blockDim.x)
                if (L.ck[i] != SP_BK_NONE) {
                    const unsigned long long v = sp_bk_vote_pack(L.cc[i], L.ck[i]);
                    b = v > b ? v : b;
                }
            if (b) atomicMax(&L.best, b);
        } else {
            const int64_t lo = L.lo, hi = L.hi;
            for (int64_t band = lo; band <= hi; band += P.cells) {
                __syncthreads();
                for (int i = threadIdx.x; i < P.cells; i += blockDim.x) L.cc[i] = 0u;
                __syncthreads();
                bk_scan_window(P, p0, p1, band);
                __syncthreads();
                unsigned long long b = 0ULL;
                for (int i = threadIdx.x; i < P.cells; i += blockDim.x)
                    if (L.cc[i]) {
                        const uint32_t dense = (uint32_t)(band + i), o = dense >= (uint32_t)P.n_wb ? 1u : 0u;
                        const unsigned long long v = sp_bk_vote_pack(L.cc[i], sp_bk_cell((int32_t)(dense - o * (uint32_t)P.n_wb), (int)o));
                        b = v > b ? v : b;
                    }
                if (b) atomicMax(&L.best, b);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            sp_bk_vote_out(L.best, (int32_t)L.total, &win_b[wa], &opp[wa], &votes[wa], &total[wa]);
            n_anchors += L.total;
            n_spilled += spilled ? 1u : 0u;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (n_anchors) atomicAdd(&flags[0], n_anchors);
        if (n_spilled) atomicAdd(&flags[3], n_spilled);
    }
}

// ---------------------------------------------------------------- anchors on request
// phase 0: cnt[u] = anchors among the starts of unit u; phase 1: write them at cnt[u] (after the exclusive scan)
__device__ __attribute__((noinline)) void bk_emit(const bk_pair_args &P, uint64_t key, uint64_t mixed, bool fw, int64_t pos,
                                                  unsigned long long &at, int32_t *posA, int32_t *posB, uint8_t *opp) {
    const uint32_t a = bk_anchor(P.A, P.B, key, mixed, fw);
    if (a == SP_BK_NONE) return;
    if (posA) {
        posA[at] = (int32_t)pos;
        posB[at] = (int32_t)(a >> 1);
        opp[at] = (uint8_t)(a & 1u);
    }
    at++;
}
__global__ void __launch_bounds__(SP_BK_THREADS)
bk_anchors(bk_pair_args P, int64_t n_units, unsigned long long *__restrict__ cnt, int32_t *__restrict__ posA,
           int32_t *__restrict__ posB, uint8_t *__restrict__ opp) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long at = posA ? cnt[u] : 0ULL;
        sp_scan32_valid64(P.pk, P.pm, P.nm, u * 32, P.kp, [&](int64_t pos, uint64_t fwd, uint64_t rc) {
            const bool fw = fwd < rc;
            const uint64_t key = fw ? fwd : rc, mixed = sp_bk_mix(key);
            if (sp_bk_sampled_mix(mixed, P.s)) bk_emit(P, key, mixed, fw, pos, at, posA, posB, opp);
        });
        if (!posA) cnt[u] = at;
    }
}

// ---------------------------------------------------------------- host
static sp_blocks_state *bk_state(sp_ctx *ctx) {
    if (!ctx->blocks) ctx->blocks = new sp_blocks_state();
    if (ctx->blocks->idx.size() != ctx->chroms.size()) ctx->blocks->idx.resize(ctx->chroms.size());
    return ctx->blocks;
}
static void bk_free_index(sp_bk_index &x) {
    if (x.d_keys) hipFree(x.d_keys);
    x = sp_bk_index();
}
void sp_blocks_drop(sp_ctx *ctx, int chrom) {
    sp_blocks_state *st = ctx->blocks;
    if (!st) return;
    for (size_t i = 0; i < st->idx.size(); i++)
        if (chrom < 0 || (int)i == chrom) bk_free_index(st->idx[i]);
    if (chrom < 0) st->idx.clear();
    st->lastA = st->lastB = -1;
}
void sp_blocks_destroy(sp_ctx *ctx) {
    if (!ctx->blocks) return;
    sp_blocks_drop(ctx, -1);
    sp_buf_free(ctx->blocks->b_out);
    sp_buf_free(ctx->blocks->b_small);
    delete ctx->blocks;
    ctx->blocks = nullptr;
}

static int bk_check_params(sp_ctx *ctx, const char *who, int kb, int s, int64_t bin) {
    switch (sp_bk_check(kb, s, bin)) {
    case 1: return sp_fail(ctx, SP_EINVAL, "%s: block_k = %d is not an odd number in %d..%d", who, kb, SP_BK_KMIN, SP_BK_KMAX);
    case 2: return sp_fail(ctx, SP_EINVAL, "%s: block_sample = %d is outside 0..%d", who, s, SP_BK_SMAX);
    case 3: return sp_fail(ctx, SP_EINVAL, "%s: block_bin = %lld is below 1", who, (long long)bin);
    }
    return SP_OK;
}
static unsigned bk_grid(sp_ctx *ctx, int64_t items) {
    int64_t g = (items + SP_BK_THREADS - 1) / SP_BK_THREADS;
    const int64_t most = 8LL * ctx->n_cu;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}
static int bk_small(sp_ctx *ctx, sp_blocks_state *st, unsigned long long **flags) {
    int rc = sp_buf_ensure(ctx, st->b_small, 4 * sizeof(unsigned long long));
    if (rc) return rc;
    *flags = (unsigned long long *)st->b_small.p;     // [0] a tally, [1] inserts that found no entry, [2] singles, [3] spilled windows
    SP_HIP(ctx, hipMemsetAsync(*flags, 0, 4 * sizeof(unsigned long long), ctx->stream));
    return SP_OK;
}

extern "C" {

int sp_blocks_index(sp_ctx *ctx, int chrom, int kb, int s, int64_t *n_sampled, int64_t *n_single) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_blocks_index: ctx is NULL");
    int rc = bk_check_params(ctx, "sp_blocks_index", kb, s, 1);
    if (rc) return rc;
    if (chrom < 0 || chrom >= (int)ctx->chroms.size())
        return sp_fail(ctx, SP_EINVAL, "sp_blocks_index: chromosome %d is outside the genome (0..%d)", chrom, (int)ctx->chroms.size() - 1);
    const sp_chrom &c = ctx->chroms[(size_t)chrom];
    if (!c.d_pk || !c.d_nm) return sp_fail(ctx, SP_EINVAL, "sp_blocks_index: chromosome %d has no packed sequence (sp_genome_add first)", chrom);
    if (c.len > SP_BK_MAXLEN)
        return sp_fail(ctx, SP_EUNSUP, "sp_blocks_index: chromosome %d has %lld bases, positions travel in 31 bits", chrom, (long long)c.len);
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_blocks_state *st = bk_state(ctx);
    sp_bk_index &x = st->idx[(size_t)chrom];
    if (!(x.d_keys && x.kb == kb && x.s == s)) {
        bk_free_index(x);
        if (st->lastA == chrom || st->lastB == chrom) st->lastA = st->lastB = -1;
        unsigned long long *flags = nullptr, h[4];
        if ((rc = bk_small(ctx, st, &flags))) return rc;
        const int64_t n_units = (c.len + 31) / 32;
        const sp_kparams kp = sp_make_kparams(kb);
        SP_LAUNCH(ctx, "bk_count", bk_count, dim3(bk_grid(ctx, n_units)), dim3(SP_BK_THREADS), 0, c.d_pk, c.d_pm, c.d_nm, n_units, kp, s, flags);
        SP_HIP(ctx, hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const int64_t n = (int64_t)h[0], cap = n + n / 2 + 64;      // distinct keys <= n: never more than two thirds full
        const size_t bytes = (size_t)cap * (sizeof(unsigned long long) + sizeof(uint32_t));
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();     // or the context's next launch check would report this allocation
            return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP,
                           "sp_blocks_index: an index of %lld bytes (%lld sampled k-mers of chromosome %d) does not fit on the device (%s)",
                           (long long)bytes, (long long)n, chrom, hipGetErrorString(e));
        }
        x.d_keys = (unsigned long long *)p;
        x.d_vals = (uint32_t *)(x.d_keys + cap);
        x.cap = (uint32_t)cap;
        x.kb = kb;
        x.s = s;
        rc = SP_OK;
        do {
            hipError_t e2 = hipMemsetAsync(p, 0xff, bytes, ctx->stream);
            if (e2 != hipSuccess) { rc = sp_fail(ctx, SP_EHIP, "sp_blocks_index: clearing the index failed: %s", hipGetErrorString(e2)); break; }
            sp_prof_begin(ctx, "bk_build", dim3(bk_grid(ctx, n_units)));
            hipLaunchKernelGGL(bk_build, dim3(bk_grid(ctx, n_units)), dim3(SP_BK_THREADS), 0, ctx->stream, c.d_pk, c.d_pm, c.d_nm, n_units, kp, s,
                               x.d_keys, x.d_vals, x.cap, flags);
            sp_prof_end(ctx);
            sp_prof_begin(ctx, "bk_singles", dim3(bk_grid(ctx, cap)));
            hipLaunchKernelGGL(bk_singles, dim3(bk_grid(ctx, cap)), dim3(SP_BK_THREADS), 0, ctx->stream, x.d_vals, x.cap, flags);
            sp_prof_end(ctx);
            e2 = hipGetLastError();
            if (e2 == hipSuccess) e2 = hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, ctx->stream);
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(ctx->stream);
            if (e2 != hipSuccess) { rc = sp_fail(ctx, SP_EHIP, "sp_blocks_index: building the index failed: %s", hipGetErrorString(e2)); break; }
            if (h[1])
                rc = sp_fail(ctx, SP_EHIP, "sp_blocks_index: the index of chromosome %d (%lld entries for %lld sampled k-mers) is full: %llu k-mers found no entry",
                             chrom, (long long)cap, (long long)n, h[1]);
        } while (0);
        if (rc) {
            bk_free_index(x);
            return rc;
        }
        x.n_sampled = n;
        x.n_single = (int64_t)h[2];
    }
    if (n_sampled) *n_sampled = x.n_sampled;
    if (n_single) *n_single = x.n_single;
    return SP_OK;
}

int sp_blocks_set_cells(sp_ctx *ctx, int cells) {
    if (!ctx || cells < 2 || cells > SP_BK_MAXCELLS || (cells & (cells - 1)))
        return sp_fail(ctx, SP_EINVAL, "sp_blocks_set_cells: %d is not a power of two in 2..%d", cells, SP_BK_MAXCELLS);
    bk_state(ctx)->cells = cells;
    return SP_OK;
}

static int bk_pair_setup(sp_ctx *ctx, const char *who, int a, int b, int kb, int s, int64_t bin, bk_pair_args &P) {
    int rc = bk_check_params(ctx, who, kb, s, bin);
    if (rc) return rc;
    const int C = (int)ctx->chroms.size();
    if (a < 0 || a >= C || b < 0 || b >= C) return sp_fail(ctx, SP_EINVAL, "%s: pair (%d, %d) is outside the genome (0..%d)", who, a, b, C - 1);
    if (a == b) return sp_fail(ctx, SP_EINVAL, "%s: a chromosome (%d) is not paired with itself", who, a);
    sp_blocks_state *st = bk_state(ctx);
    for (int ch : {a, b}) {
        const sp_bk_index &x = st->idx[(size_t)ch];
        if (!x.d_keys) return sp_fail(ctx, SP_EINVAL, "%s: chromosome %d has no index (sp_blocks_index first)", who, ch);
        if (x.kb != kb || x.s != s)
            return sp_fail(ctx, SP_EINVAL, "%s: the index of chromosome %d was built with block_k = %d, block_sample = %d, not %d, %d", who, ch, x.kb,
                           x.s, kb, s);
    }
    const sp_chrom &ca = ctx->chroms[(size_t)a], &cb = ctx->chroms[(size_t)b];
    const int64_t n_wa = sp_bk_nwin(ca.len, bin), n_wb = sp_bk_nwin(cb.len, bin);
    if (n_wa > 0x7fffffffLL || n_wb > 0x7fffffffLL)
        return sp_fail(ctx, SP_EINVAL, "%s: block_bin = %lld leaves %lld windows, more than 32 bits index", who, (long long)bin, (long long)(n_wa > n_wb ? n_wa : n_wb));
    P.pk = ca.d_pk;
    P.pm = ca.d_pm;
    P.nm = ca.d_nm;
    P.lenA = ca.len;
    P.bin = bin;
    P.n_wa = (int32_t)n_wa;
    P.n_wb = (int32_t)n_wb;
    P.bin32 = (uint32_t)(bin < 0x7fffffffLL ? bin : 0x7fffffffLL);
    P.kp = sp_make_kparams(kb);
    P.s = s;
    P.cells = st->cells;
    P.cell_shift = 32;
    for (int c = P.cells; c > 1; c >>= 1) P.cell_shift--;
    P.A = bk_table{st->idx[(size_t)a].d_keys, st->idx[(size_t)a].d_vals, st->idx[(size_t)a].cap};
    P.B = bk_table{st->idx[(size_t)b].d_keys, st->idx[(size_t)b].d_vals, st->idx[(size_t)b].cap};
    return SP_OK;
}

int sp_blocks_pair(sp_ctx *ctx, int a, int b, int kb, int s, int64_t bin, int32_t *win_b, uint8_t *opp, int32_t *votes,
                   int32_t *total, int64_t *n_anchors, int64_t *n_spilled) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_blocks_pair: ctx is NULL");
    bk_pair_args P;
    int rc = bk_pair_setup(ctx, "sp_blocks_pair", a, b, kb, s, bin, P);
    if (rc) return rc;
    if (P.n_wa > 0 && (!win_b || !opp || !votes || !total)) return sp_fail(ctx, SP_EINVAL, "sp_blocks_pair: an output array is NULL");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_blocks_state *st = ctx->blocks;
    st->lastA = st->lastB = -1;
    unsigned long long *flags = nullptr, h[4] = {0, 0, 0, 0};
    if ((rc = bk_small(ctx, st, &flags))) return rc;
    const size_t W = (size_t)P.n_wa;
    if (W) {
        rc = sp_buf_ensure(ctx, st->b_out, (int64_t)(W * 13 + 64));
        if (rc == SP_ENOMEM) {
            (void)hipGetLastError();
            return sp_fail(ctx, SP_ENOMEM, "sp_blocks_pair: the votes of %lld windows, %lld bytes, do not fit on the device", (long long)W, (long long)(W * 13 + 64));
        }
        if (rc) return rc;
        int32_t *d_wb = (int32_t *)st->b_out.p, *d_votes = d_wb + W, *d_total = d_votes + W;
        uint8_t *d_opp = (uint8_t *)(d_total + W);
        const unsigned grid = (unsigned)(W < (size_t)(16 * ctx->n_cu) ? W : (size_t)(16 * ctx->n_cu));
        SP_LAUNCH(ctx, "bk_pair", bk_pair, dim3(grid), dim3(SP_BK_THREADS), 0, P, d_wb, d_opp, d_votes, d_total, flags);
        SP_HIP(ctx, hipMemcpyAsync(win_b, d_wb, W * 4, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(votes, d_votes, W * 4, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(total, d_total, W * 4, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(opp, d_opp, W, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    st->lastA = a;
    st->lastB = b;
    st->last_n = (int64_t)h[0];
    if (n_anchors) *n_anchors = (int64_t)h[0];
    if (n_spilled) *n_spilled = (int64_t)h[3];
    return SP_OK;
}

int sp_blocks_anchors(sp_ctx *ctx, int32_t *pos_a, int32_t *pos_b, uint8_t *opp, int64_t n) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_blocks_anchors: ctx is NULL");
    sp_blocks_state *st = ctx->blocks;
    if (!st || st->lastA < 0) return sp_fail(ctx, SP_EINVAL, "sp_blocks_anchors: no pair to answer for (sp_blocks_pair first)");
    if (n != st->last_n) return sp_fail(ctx, SP_EINVAL, "sp_blocks_anchors: the last pair has %lld anchors, not %lld", (long long)st->last_n, (long long)n);
    if (n == 0) return SP_OK;
    if (!pos_a || !pos_b || !opp) return sp_fail(ctx, SP_EINVAL, "sp_blocks_anchors: an output array is NULL");
    const sp_bk_index &xa = st->idx[(size_t)st->lastA];
    bk_pair_args P;
    int rc = bk_pair_setup(ctx, "sp_blocks_anchors", st->lastA, st->lastB, xa.kb, xa.s, 1, P);
    if (rc) return rc;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n_units = (P.lenA + 31) / 32;
    const size_t need = (size_t)n_units * 8 + 8 + (size_t)n * 9 + 64;
    sp_tmp<unsigned char> w;
    const hipError_t e = w.alloc(need);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return sp_fail(ctx, e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP, "sp_blocks_anchors: %lld anchors and %lld unit counts, %lld bytes, do not fit on the device (%s)",
                       (long long)n, (long long)n_units, (long long)need, hipGetErrorString(e));
    }
    unsigned long long *cnt = (unsigned long long *)w.p, *tot = cnt + n_units;
    int32_t *d_pa = (int32_t *)(tot + 1), *d_pb = d_pa + n;
    uint8_t *d_opp = (uint8_t *)(d_pb + n);
    unsigned long long h_tot = 0;
    const unsigned grid = bk_grid(ctx, n_units);
    SP_LAUNCH(ctx, "bk_anchors", bk_anchors, dim3(grid), dim3(SP_BK_THREADS), 0, P, n_units, cnt, (int32_t *)nullptr, (int32_t *)nullptr, (uint8_t *)nullptr);
    SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, cnt, n_units, tot);
    SP_HIP(ctx, hipMemcpyAsync(&h_tot, tot, 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((int64_t)h_tot != n)      // (before anything is written through offsets that would not fit)
        return sp_fail(ctx, SP_EHIP, "sp_blocks_anchors: the units hold %llu anchors, the pair call counted %lld", h_tot, (long long)n);
    SP_LAUNCH(ctx, "bk_anchors", bk_anchors, dim3(grid), dim3(SP_BK_THREADS), 0, P, n_units, cnt, d_pa, d_pb, d_opp);
    SP_HIP(ctx, hipMemcpyAsync(pos_a, d_pa, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(pos_b, d_pb, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(opp, d_opp, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_blocks_release(sp_ctx *ctx, int chrom) {
    if (!ctx) return sp_fail(ctx, SP_EINVAL, "sp_blocks_release: ctx is NULL");
    if (chrom >= (int)ctx->chroms.size()) return sp_fail(ctx, SP_EINVAL, "sp_blocks_release: chromosome %d is outside the genome", chrom);
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sp_blocks_drop(ctx, chrom < 0 ? -1 : chrom);
    return SP_OK;
}

}  // extern "C"
