// sp_lists.h -- the per-chromosome sorted (key, count) lists: what the units that build them (sp_sparse.hip,
// sp_sparse2.hip) and the list filter (sp_listfilter.hip) share.
#pragma once
#include "sp_common.h"
#include "sp_listplan.h"     // SPS_MAXC

#define SPS_SENTINEL (~0ULL)

__device__ __forceinline__ uint64_t sps_mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

// ordered selections (sps_sel_*, sps_eval, sps_emit): a workgroup takes SEL_SPAN entries
#define SEL_PER_THREAD 16
#define SEL_BLOCK 256
#define SEL_SPAN (SEL_PER_THREAD * SEL_BLOCK)

struct sps_list {
    const unsigned long long *keys;
    const uint32_t *cnts;
    long long n;
};

// the lists the filter works on: the local chromosomes, or a caller-owned key-range view (sp_sparse_view)
static int sps_C(sp_ctx *ctx) { return ctx->sv_on ? (int)ctx->sv_keys.size() : (int)ctx->chroms.size(); }
static int64_t sps_n(sp_ctx *ctx, int c) { return ctx->sv_on ? ctx->sv_n[(size_t)c] : ctx->sparse[(size_t)c].n; }
static const unsigned long long *sps_keys(sp_ctx *ctx, int c) {
    return (const unsigned long long *)(ctx->sv_on ? ctx->sv_keys[(size_t)c] : ctx->sparse[(size_t)c].d_keys);
}
static const uint32_t *sps_cnts(sp_ctx *ctx, int c) {
    return ctx->sv_on ? ctx->sv_cnts[(size_t)c] : ctx->sparse[(size_t)c].d_cnts;
}
static int64_t sps_len(sp_ctx *ctx, int c) {
    return ctx->sv_on ? ctx->fv_lengths[(size_t)c] : ctx->chroms[(size_t)c].length_sum;
}
