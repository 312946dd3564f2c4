// sp_internal.h -- every host function and kernel that one translation unit defines and another one calls.  The unit
// that defines a function includes this header as its callers do, so a declaration cannot drift from its definition.
// (Kernels launched from another unit go through their host stubs: no relocatable device code.)
#pragma once
#include "sp_common.h"

struct c2_bdesc;         // sp_c2batch.h
struct sp_map_params;    // sp_map.h

// sp_ctx.hip
__global__ void k0_pack(const uint8_t *ascii, int64_t len, uint32_t *pk, uint32_t *pm, uint32_t *nm, int64_t n_mask_words);

// sp_count.hip
__global__ void scan_excl_u64(unsigned long long *a, int64_t n, unsigned long long *total);
int sp_ovf_finalize(sp_ctx *ctx, sp_chrom &c, const uint2 *tmp, const uint32_t *seg_base, const uint32_t *seg_cnt,
                    uint32_t *seg_off, int64_t n_buckets, unsigned long long *d_total);
int sp_ovf_finalize_split(sp_ctx *ctx, unsigned long long *keys, uint32_t *cnts, const uint2 *tmp, const uint32_t *seg_base,
                          const uint32_t *seg_cnt, uint32_t *seg_off, int64_t n_buckets, unsigned long long *d_total);
int sp_ovf_finalize_split_batch(sp_ctx *ctx, const c2_bdesc *d_desc, int n_chrom, int64_t n_buckets);
int sp_lanes_open(sp_ctx *ctx, int n);      // lanes 0 .. n - 1: stream and `done` event; the context's lane_go event
int sp_lanes_join(sp_ctx *ctx, int n);      // the context's stream waits for the lanes
void sp_lanes_drain(sp_ctx *ctx, int n);    // after an error: host wait for the lanes and the context's stream, ctx->err kept

// sp_count2.hip
bool sp_engine2_supported(int64_t nslots);
int sp_count_engine2(sp_ctx *ctx, sp_chrom &c, const sp_kparams &kp, int lower, unsigned long long *d_len4, bool exact,
                     sp_sparse_chrom *list);
int sp_count_engine3_batch(sp_ctx *ctx, const int *chrom_idx, int n, const sp_kparams &kp, int lower, unsigned long long *d_len);

// sp_sparse.hip: count engine 1 of k > 15, the label tables and the map kernels of k > 15
void sp_sparse_release(sp_ctx *ctx);
int sp_sparse_count(sp_ctx *ctx, int k, int lower);
int sp_sparse_dump(sp_ctx *ctx, int chrom, uint64_t *keys, uint32_t *counts);
int sp_sparse_labels_build(sp_ctx *ctx, const sp_label_plan &plan, const unsigned long long *d_keys, const uint8_t *d_sg,
                           int64_t n, unsigned long long *d_flags);
int sp_sparse_map_launch(sp_ctx *ctx, sp_chrom &c, const sp_map_params &P, int *d_counts, unsigned long long *d_n);
int sp_sparse_feat_launch(sp_ctx *ctx, const uint32_t *d_pk, const uint32_t *d_pm, const uint32_t *d_nm, int64_t n_units,
                          const int64_t *d_foff, int64_t n_feat, int S, unsigned long long *d_counts);
int sp_sparse_mask_launch(sp_ctx *ctx, sp_chrom &c, int64_t n_units, int S, const unsigned long long *d_cov,
                          unsigned long long *d_masks);
int sp_sparse_hit(sp_ctx *ctx, unsigned long long *d_n);

// sp_sparse2.hip
int sp_sparse_count3(sp_ctx *ctx, int k, int lower);

// sp_listfilter.hip
int sp_sparse_filter(sp_ctx *ctx, int n_sets, const int32_t *set_off, const int32_t *unit_off, const int32_t *unit_chrom,
                     const std::vector<double> &den, double min_fold, int baseline, double min_freq, double max_freq,
                     double ratio);
int sp_sparse_fetch(sp_ctx *ctx, bool hist, uint64_t *keys, uint32_t *counts, double *freqs, uint64_t *tot, bool async);

// sp_enrich.hip: pass 1 of the k-mer tests for wide groups (k7_ttest_wide_means): means[r][g] = np.mean of the group's
// list, top / second by the reference's order key.  sp_tw_means_plan builds the groups' summation programs on the host
// (SP_EUNSUP with `who` in the message when a group needs a deeper stack than the kernel has); the caller carves
// plan.poff.size() ints and plan.prog.size() bytes behind its own arrays, and sp_tw_means_launch uploads the programs
// and launches the kernel on the context's stream.  The plan is the source of asynchronous copies: it lives until the
// caller has waited for the stream.
struct sp_tw_plan {
    std::vector<int> poff;          // [n_groups + 1]: where a group's program starts
    std::vector<uint8_t> prog;
};
int sp_tw_means_plan(sp_ctx *ctx, const char *who, int n_groups, const int32_t *group_off, sp_tw_plan &plan);
int sp_tw_means_launch(sp_ctx *ctx, const sp_tw_plan &plan, int *d_poff, uint8_t *d_prog, const uint32_t *rows, int64_t M, int C,
                       const double *d_len, int n_groups, const int *d_goff, const int *d_gch, int *d_top, int *d_sec,
                       double *d_means);

// sp_blocks.hip: the indexes of a chromosome (chrom < 0: of all) go when its sequence does; everything at sp_ctx_destroy
void sp_blocks_drop(sp_ctx *ctx, int chrom);
void sp_blocks_destroy(sp_ctx *ctx);

// sp_ltrdetect.hip: everything at sp_ctx_destroy
void sp_ltrdetect_destroy(sp_ctx *ctx);

// sp_map.hip
int sp_map_filter_build(sp_ctx *ctx, const unsigned long long *d_keys, int64_t n);
