/*
 * subphaser_hip.h -- C-ABI of libsubphaser_hip.so: the MI355X (gfx950) native
 * implementation of SubPhaser's k-mer hot path.
 *
 * The reference has no FFI; its seam is five Python call sites in
 * Pipeline.run() (subphaser/__main__.py:403-404, 409-433, 484-486, 491,
 * 497-498).  Each entry point below names the reference interface it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SP_E* code on failure;
 *     the message is available from sp_last_error(ctx) (ctx may be NULL for
 *     errors raised before a context exists).  No C++ exception crosses.
 *   - pointers named d_* are DEVICE pointers (HIP), all others are host.
 *   - k-mers are uint64: 2 bits per base (A=0 C=1 G=2 T=3), first base in the
 *     most significant used bits, always the canonical orientation
 *     (min of the k-mer and its reverse complement).
 *   - the caller owns every output buffer; the library owns device memory
 *     inside the context; no caller pointer is retained after return.
 *   - one context per process per GPU; calls on a context are serialised by
 *     the caller.
 */
#ifndef SUBPHASER_HIP_H
#define SUBPHASER_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK 0
#define SP_EINVAL (-1)    /* bad argument / call order                     */
#define SP_EUNSUP (-2)    /* k outside the supported range                 */
#define SP_ENOMEM (-3)    /* hipMalloc failed                              */
#define SP_EHIP (-4)      /* any other HIP runtime error                   */
#define SP_ENODEV (-5)    /* no usable gfx950 device                       */
#define SP_ESTATE (-6)    /* reference-level precondition (message mirrors
                             the reference's ValueError text)              */
#define SP_EIO (-7)       /* write() to the caller's descriptor failed
                             (errno in sp_last_error(NULL))                */

typedef struct sp_ctx sp_ctx;

int sp_version(void);
const char *sp_last_error(const sp_ctx *ctx);

/* stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL
 * to let the library create its own. */
int sp_ctx_create(int device, void *stream, sp_ctx **out);
int sp_ctx_destroy(sp_ctx *ctx);
int sp_sync(sp_ctx *ctx);
/* the hipStream_t every kernel of this context is launched on */
void *sp_stream(sp_ctx *ctx);

/* ---- genome ingest (K0) -------------------------------------------------
 * Replaces the per-chromosome FASTA files written by Seqs.split_genomes
 * (Seqs.py:27-71) and read by jellyfish / chunk_chromfiles: the FASTA body of
 * chromosome `chrom` (newlines removed, any case, IUPAC allowed) is packed to
 * 2 bits/base + 1 validity bit/base in HBM.                                */
int sp_genome_reset(sp_ctx *ctx, int n_chrom);
int sp_genome_add(sp_ctx *ctx, int chrom, const uint8_t *ascii, int64_t len);
int sp_genome_add_device(sp_ctx *ctx, int chrom, const uint8_t *d_ascii, int64_t len);
int sp_genome_len(sp_ctx *ctx, int chrom, int64_t *len);
/* unpack back to upper-case ASCII ('N' for every invalid base) -- debugging / tests */
int sp_genome_unpack(sp_ctx *ctx, int chrom, uint8_t *ascii_out, int64_t len);

/* ---- k-mer counting (K1 + K2) -------------------------------------------
 * Replaces run_jellyfish_dumps (Jellyfish.py:671-704): for every chromosome,
 * canonical k-mer counts, kept when count >= lower_count (`jellyfish dump -L`).
 * engine: 0 = auto, 1 = global-atomic table, 2 = LDS radix-partition counter (byte tables), 3 = the same partition
 * chain ending in per-chromosome (slot, count) LISTS -- no byte tables; what auto picks for small genomes, where a
 * chromosome fills less than 1/3 of its dense table (k <= 15 with 2^17..2^31 slots, <= 64 chromosomes, whole-genome
 * sp_count calls only; sp_table_overflow / sp_filter_view / the table exchange are byte-table interfaces). */
int sp_count(sp_ctx *ctx, int k, int lower_count, int engine);
/* same for chromosomes [first, last) only (k <= 15): lets a multi-GPU caller ship the finished
 * table of chromosome i over xGMI while chromosome i+1 is being counted.          */
int sp_count_range(sp_ctx *ctx, int k, int lower_count, int engine, int first, int last);
/* Engine 2 sizes its partition buckets from a 1-in-16 sample of the chromosome and counts a chromosome again, with
 * exact sizes, when a bucket outgrows its region: *recounts = chromosomes counted twice since the context was
 * created (0 on ordinary genomes; results are identical either way -- this is a performance diagnostic). */
int sp_count_recounts(sp_ctx *ctx, int64_t *recounts);
/* number of slots of the dense count table for this k (2^(2k-1) for odd k, 4^k for even k) */
int sp_nslots(sp_ctx *ctx, int k, int64_t *nslots);
/* Count tables (k <= 15) are BYTE tables: one byte per dense slot holding the RAW count, saturated --
 * 0..254 = the count, 255 = "the count is >= 255: see the chromosome's overflow list" of
 * (uint32 slot, uint32 count) pairs, ascending slot.  lower_count (`jellyfish dump -L`,
 * Jellyfish.py:697) is applied wherever a table is read, so lengths, dumps and the matrix all see
 * m[key][c] = count if count >= lower_count else 0.  A byte table is also the multi-GPU wire format:
 * slot-range slices travel over xGMI as they are (a quarter of a u32 table).
 *   sp_tables_bind    use caller-owned device memory (nslots bytes, 16-byte aligned) as the table of
 *                     `chrom`, so that the caller (e.g. a torch tensor handed to RCCL) can exchange it;
 *                     NULL unbinds.  Call before sp_count.
 *   sp_table_overflow copy the overflow pairs of `chrom` into caller-owned DEVICE memory (capacity `cap`
 *                     pairs; d_pairs = NULL only queries *n_pairs); asynchronous on the context's stream. */
int sp_tables_bind(sp_ctx *ctx, int chrom, void *d_table);
int sp_table_overflow(sp_ctx *ctx, int chrom, void *d_pairs, int64_t cap, int64_t *n_pairs);
/* Multi-GPU, a chromosome counted in pieces by several ranks (the reference cuts chromosomes into 10-Mb
 * chunks with a k-1 overlap for the same purpose, Seqs.py:121-139): byte slices of the same slot range
 * [slot_base, slot_base + n) are added up exactly on the rank that filters that range.
 *   sp_table_merge    dst += src (device byte slices, dst may be read and written in place).  A slot whose sum
 *                     reaches 255 or whose summands were saturated becomes 255 and its exact sum (looked up in
 *                     the two overflow lists, absolute slots) goes to d_out_ovf -- a NEW list of the slots of this
 *                     range only, ascending (capacity `cap` pairs; SP_ENOMEM with *n_out = the number needed).
 *                     slot_base may be ANY non-negative slot (dist.py's ranges are 64-slot aligned, not aligned to
 *                     the 2^15-slot buckets the list is built in): the output list is ascending whatever the
 *                     alignment.  The input lists may cover the whole table or the range only; d_out_ovf must not
 *                     be one of them (a chain of merges alternates between two output buffers).
 *   sp_table_lengths  sum and number of the counts >= lower_count of a slice (the chromosome's contribution of this
 *                     slot range to `lengths`, Jellyfish.py:97,449, and to the dump size).                         */
int sp_table_merge(sp_ctx *ctx, void *d_dst_u8, const void *d_dst_ovf, int64_t n_dst_ovf, const void *d_src_u8,
                   const void *d_src_ovf, int64_t n_src_ovf, int64_t slot_base, int64_t n, void *d_out_ovf, int64_t cap,
                   int64_t *n_out);
int sp_table_lengths(sp_ctx *ctx, const void *d_tab_u8, const void *d_ovf, int64_t n_ovf, int64_t slot_base, int64_t n,
                     int lower_count, int64_t *sum, int64_t *n_dump);
/* lengths[c] = sum of the dumped counts of chromosome c (Jellyfish.py:97,449) */
int sp_lengths(sp_ctx *ctx, int64_t *lengths /*C*/);
/* jellyfish-dump equivalent of one chromosome.  Two calls: sp_dump_size then
 * sp_dump with buffers of that size.  Entries come in ascending order of the
 * internal dense slot (deterministic; jellyfish's own order is hash order);
 * the Python binding sorts them by canonical key.                           */
int sp_dump_size(sp_ctx *ctx, int chrom, int64_t *n);
int sp_dump(sp_ctx *ctx, int chrom, uint64_t *keys, uint32_t *counts, int64_t cap, int64_t *n);

/* ---- matrix + differential filter (K3) ----------------------------------
 * Replaces JellyfishDumps.to_matrix (Jellyfish.py:439-460) and .filter /
 * _filter_kmer (:462-512, :611-648).  Homoeologous sets in CSR form: set s
 * owns units [set_off[s], set_off[s+1]); unit u owns the chromosome indices
 * unit_chrom[unit_off[u] .. unit_off[u+1]).  min_freq / max_freq are the
 * already-resolved thresholds (min_prop/max_prop applied by the caller with
 * sp_lengths).  Outputs: n_union = len(d_mat), n_rows = differential k-mers,
 * n_hist = len(tot_freqs) (fold-passing k-mers, in or out of the freq range). */
/* Multi-GPU: make sp_filter / sp_filter_fetch work on a slot-range VIEW instead of the local
 * tables: C device pointers (16-byte aligned), each to the nslots_view table bytes of slots [slot_base,
 * slot_base + nslots_view) of one chromosome (all chromosomes of the genome, gathered from their
 * owner ranks), the chromosomes' overflow lists (d_ovf[c]: n_ovf[c] pairs with ABSOLUTE slots,
 * ascending; may cover more than the slot range; d_ovf = NULL: none) and the global `lengths`.
 * d_tabs = NULL returns to the local tables.                                                   */
int sp_filter_view(sp_ctx *ctx, int C, const void *const *d_tabs, int64_t slot_base,
                   int64_t nslots_view, const int64_t *lengths, int k, int lower_count,
                   const void *const *d_ovf, const int64_t *n_ovf);
int sp_filter(sp_ctx *ctx, int n_sets, const int32_t *set_off, const int32_t *unit_off,
              const int32_t *unit_chrom, double min_fold, int baseline, double min_freq,
              double max_freq, double ratio, int64_t *n_union, int64_t *n_rows, int64_t *n_hist);
/* rows in ascending dense-slot order (deterministic; the Python binding sorts by
 * canonical key); counts is row-major n_rows x C
 * (thresholded counts: 0 where count < lower_count); freqs = count/length in
 * fp64 exactly as Jellyfish.py:647 (may be NULL); tot = row sums (may be NULL) */
int sp_filter_fetch(sp_ctx *ctx, uint64_t *keys, uint32_t *counts, double *freqs, uint64_t *tot,
                    int64_t cap_rows);
/* the same rows, copied to PAGE-LOCKED host buffers (sp_host_alloc) by a copy stream while the calling stream is
 * free for the next stage; the buffers are valid after sp_filter_fetch_wait (k > 15: copies synchronously).
 * The emit buffers on the device are reused by the next sp_filter_fetch*: wait before calling it again.     */
int sp_filter_fetch_async(sp_ctx *ctx, uint64_t *keys, uint32_t *counts, uint64_t *tot, int64_t cap_rows);
int sp_filter_fetch_wait(sp_ctx *ctx);
/* same rows written to caller-owned DEVICE buffers (any may be NULL): multi-GPU callers gather
 * them over xGMI without a host round trip.  d_keys/d_tot: uint64 x n_rows, d_counts: uint32 x n_rows x C. */
int sp_filter_fetch_device(sp_ctx *ctx, void *d_keys, void *d_counts, void *d_tot, int64_t cap_rows);
/* tot of every fold-passing k-mer (the reference's tot_freqs histogram input) */
int sp_filter_hist(sp_ctx *ctx, uint64_t *tot, int64_t cap);

/* ---- subgenome-specific k-mer labels (K4) + bin mapping (K5) ------------
 * sp_labels_set replaces the d_kmers dict handed to Seqs.map_kmer3
 * (Cluster.py:174-175): canonical key -> subgenome index in [0, n_sg).
 * sp_map_bins replaces Seqs.map_kmer3 / map_kmer_each4 (Seqs.py:74-119,
 * 209-237) for one chromosome: counts by k-mer START position into
 *   slot(s) = s / bin_size + chunk(s)
 * where chunk(s) reproduces the reference's 10-Mb chunking (Seqs.py:121-139;
 * chunk_size = 0 disables it), so that a bin straddling a chunk boundary is
 * reported on two lines like the reference does.
 * slot_counts: nslots x n_sg int32 (overwritten).
 * A label set belongs to the k it was set at: after an sp_count with another k (or an sp_labels_set that failed)
 * the map entries and sp_labels_hit return SP_EINVAL until sp_labels_set succeeds again.  */
int sp_labels_set(sp_ctx *ctx, const uint64_t *keys, const uint8_t *sg, int64_t n, int n_sg);
/* the same with `keys` and `sg` already in DEVICE memory (e.g. the rows Cluster.output_kmers selected, kept where
 * sp_kmer_ttest tested them: Cluster.py:186-194 hands the reference's d_kmers dict to Seqs.map_kmer3 in memory too):
 * no host round trip; labels >= n_sg are detected on the device (SP_EINVAL)                                   */
int sp_labels_set_device(sp_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_sg, int64_t n, int n_sg);
int sp_map_nslots(sp_ctx *ctx, int chrom, int64_t bin_size, int64_t chunk_size, int64_t *nslots);
int sp_map_bins(sp_ctx *ctx, int chrom, int64_t bin_size, int64_t chunk_size, int32_t *slot_counts,
                int64_t nslots, int64_t *n_mapped);
/* every chromosome in one call: chromosome c owns slots [slot_off[c], slot_off[c+1]) of
 * slot_counts (total x n_sg int32), sized with sp_map_nslots; n_mapped: C int64 (may be NULL).
 * One launch per chromosome back to back, one device->host copy.               */
int sp_map_bins_all(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, const int64_t *slot_off,
                    int32_t *slot_counts, int64_t *n_mapped);
/* The three stack entries below read the table the last sp_map_bins_all left on the device.  The context
 * remembers what that table is: bin_size, chunk_size, slot_off (all C + 1 offsets), n_sg, k and the chromosome
 * count.  A stack entry whose bin_size, chunk_size or slot_off differ from those, or that is called after the
 * context's n_sg, k or chromosome count moved, returns SP_EINVAL with a message naming the mismatch, before
 * anything is launched.  The table stops being valid ("call sp_map_bins_all first") with the next sp_map_bins,
 * sp_labels_set / sp_labels_set_device, sp_genome_reset, sp_genome_add / sp_genome_add_device, sp_count /
 * sp_count_range.  (A sp_map_bins_all that is refused for its arguments leaves the previous table as it was.)
 *
 * window stack of the slot counts left on the device by the last sp_map_bins_all
 * (replaces Circos.stack_matrix, Circos.py:734-742, 831-842, without the text round trip):
 * window = (bin start) / window_size; chromosome c owns windows [win_off[c], win_off[c+1]),
 * at least len/window_size + 2 each; win_counts: total x n_sg int64 (overwritten).          */
int sp_stack_windows(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, int64_t window_size,
                     const int64_t *slot_off, const int64_t *win_off, int64_t *win_counts);
/* same into a caller-owned DEVICE table (total x n_sg uint64, ACCUMULATED: clear it first), for callers that
 * hold pieces of chromosomes: seg_start[i] = position of local chromosome i's base 0 inside the chromosome it is
 * a piece of (NULL = 0), win_off[i] = first window row of THAT chromosome.  Several ranks' tables add up
 * (all-reduce) to the whole-genome window table.                                                        */
int sp_stack_windows_dev(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, int64_t window_size,
                         const int64_t *slot_off, const int64_t *win_off, const int64_t *seg_start, void *d_win);
/* feature mode (map_kmer3(..., chunk=False), __main__.py:509-511): n_feat
 * sequences lying back to back in `ascii`, feature f = [off[f], off[f+1]).
 * Only k-mers that lie entirely inside one feature count (the kernel rejects
 * k-mers running across a boundary; no separator copy on the host).
 * counts: n_feat x n_sg int64 (whole-feature totals).                      */
int sp_map_features(sp_ctx *ctx, const uint8_t *ascii, const int64_t *off, int64_t n_feat,
                    int64_t *counts);
/* interval mode: BED-style features over the RESIDENT genome -- what `-custom_features` (__main__.py:509-517;
 * Seqs.map_kmer3(chunk=False), Seqs.py:228-244) computes from a FASTA of the feature sequences, without uploading
 * sequence that is already in HBM.  counts[i * n_sg + sg] = number of k-mer starts s with start[i] <= s and
 * s + k <= end[i] on chromosome chrom[i] whose canonical k-mer is labelled sg (0-based, half-open like BED).
 * Intervals may overlap or nest.  A labelled k-mer counts as "seen" (sp_labels_hit) only where some interval
 * contains it -- the same k-mers a FASTA of the features would contain.                                   */
int sp_map_intervals(sp_ctx *ctx, const int32_t *chrom, const int64_t *start, const int64_t *end, int64_t n,
                     int64_t *counts);
/* number of distinct labelled k-mers seen by sp_map_bins/sp_map_features since
 * sp_labels_set (the reference's "mapped kmers" log line, Seqs.py:109-117)  */
int sp_labels_hit(sp_ctx *ctx, int64_t *n_hit);

/* ---- per-window enrichment (K6) -----------------------------------------
 * Replaces Stats.enrich / _enrich / fisher_test / Pvalues.get_enriched
 * (Stats.py:14-31, 140-192).  counts: W x S int64 window rows (host).
 * Outputs (host): pvals W x S; argmin W; sig W; ratios W x S.              */
int sp_enrich(sp_ctx *ctx, const int64_t *counts, int64_t W, int S, double max_pval,
              double min_ratio, double *pvals, int32_t *argmin, uint8_t *sig, double *ratios);
/* counts in DEVICE memory (column totals are reduced on the device) */
int sp_enrich_dev(sp_ctx *ctx, const void *d_counts, int64_t W, int S, double max_pval, double min_ratio,
                  double *pvals, int32_t *argmin, uint8_t *sig, double *ratios);
/* sp_stack_windows + sp_enrich fused on the device (Circos.stack_matrix -> Stats.enrich without the text and
 * host round trips): every window row of win_off (empty rows included -- they change no total) is tested;
 * outputs are host arrays of win_off[C] rows.                                                            */
int sp_stack_enrich(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, int64_t window_size, const int64_t *slot_off,
                    const int64_t *win_off, double max_pval, double min_ratio, int64_t *win_counts, double *pvals,
                    int32_t *argmin, uint8_t *sig, double *ratios);

/* ---- subgenome-specific k-mer test ------------------------------------------
 * Replaces Cluster.output_kmers / _output_kmers for test_method = ttest_ind (Cluster.py:151-194): per
 * differential k-mer (row of `counts`, M x C thresholded counts as sp_filter_fetch returns them) the
 * frequencies count / lengths[c] are grouped by subgenome (group g owns the chromosome indices
 * group_chrom[group_off[g] .. group_off[g+1]), groups in sorted subgenome-name order), the groups are ordered
 * by mean (descending, ties in group order) and scipy.stats.ttest_ind(top, second) -- pooled variance,
 * two-sided -- gives pvals[row].  means: M x n_groups.  The caller keeps rows with !(p > max_pval).
 * `counts` may also be a device pointer (rows staged with sp_dev_copy_from_host earlier).                   */
int sp_kmer_ttest(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                  const int32_t *group_off, const int32_t *group_chrom, int32_t *top, int32_t *second,
                  double *pvals, double *means);
/* The same test for groups of 1 .. 65536 chromosomes (scaffold-level assemblies; SP_EUNSUP beyond, SP_ENOMEM with the
 * size when the workspace does not fit), same arguments, `counts` host or device.  Two definitions are the reference's
 * to the bit, for lists of any length:
 *   means[row][g]  np.mean of the group's list in list order (Cluster.py:181): numpy's pairwise sum / n;
 *   top, second    by the order key -sum(x) / len(x) (Cluster.py:183): the sum added strictly left to right,
 *                  ties in group order.  (sp_kmer_ttest orders by the pairwise mean; the two agree except where two
 *                  groups' keys meet in the last bits.)
 * The variances are numpy's (pairwise sums of squared deviations from the pairwise mean); the p-value's incomplete beta
 * keeps a relative 1e-10 up to df = 131070, where the prefactor sp_kmer_ttest uses does not.                     */
int sp_kmer_ttest_wide(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths, int n_groups,
                       const int32_t *group_off, const int32_t *group_chrom, int32_t *top, int32_t *second,
                       double *pvals, double *means);
/* The same stage for test_method = kruskal (method 0) and mannwhitneyu (method 1), Cluster.py:178-194: arguments as in
 * sp_kmer_ttest (`counts` a host or a device pointer: rows staged on this device are read in place), and means, top and
 * second are formed exactly as sp_kmer_ttest forms them, so one matrix gets the same pair of groups under every method.
 * The test runs between the values of the top group and those of the second; csrc/sp_ranktest.h states the arithmetic:
 * doubled midranks by counting comparisons (integers), the rank sums and the tie term from them, and
 *   kruskal       H with scipy's tie correction in scipy's order of operations, p = erfc(sqrt(H / 2)); all values
 *                 identical: p = 1, stat = NaN (scipy raises there and the reference's caller never sees a value);
 *   mannwhitneyu  scipy 1.15's two-sided test, use_continuity=True, method="auto": the exact null distribution (tables
 *                 built on the host per size pair in integers and uploaded with the call) when a row has no ties and one
 *                 of the two groups has at most 8 chromosomes, the normal approximation with the tie correction
 *                 otherwise; p clipped to [0, 1].
 * stat: M statistics (H, or U of the top group) -- bit-defined; may be NULL.  pvals differ from scipy's only through erfc.
 * One group alone: second = top, p = 1, stat = NaN.  k7_ranktest is one thread per row with the pooled values in LDS;
 * every loop is bounded by the 128 values a row can have.
 * SP_EINVAL: a NULL pointer, method outside 0..1, an empty group, a chromosome index outside [0, C), a length <= 0.
 * SP_EUNSUP: a group of more than 64 chromosomes (decided before any allocation).  SP_ENOMEM: the workspace does not fit
 * (the message carries its size).  M == 0: SP_OK without a launch.                                                  */
int sp_kmer_ranktest(sp_ctx *ctx, const uint32_t *counts /*host or device*/, int64_t M, int C, const int64_t *lengths,
                     int n_groups, const int32_t *group_off, const int32_t *group_chrom,
                     int method /*0 kruskal, 1 mannwhitneyu*/, int32_t *top, int32_t *second, double *pvals,
                     double *means /*M x n_groups*/, double *stat /*M, or NULL*/);
/* sp_kmer_ranktest for groups of 1 .. 4096 chromosomes (scaffold-level assemblies), same arguments, `counts` host or
 * device.  means, top and second are those of sp_kmer_ttest_wide -- np.mean of the list, the order key -sum(x) / len(x)
 * added left to right -- so a matrix gets the pair of groups the reference picks at any list length (sp_kmer_ranktest
 * orders by the pairwise mean; the two agree except where two groups' keys meet in the last bits).  The test is the one
 * of sp_kmer_ranktest; csrc/sp_rankwide.h states the arithmetic: the same doubled midranks, rank sums and tie term as
 * 64-bit integers, found by sorting each group's values and bounding every value in both sorted lists, and the same
 * statistics operation for operation -- at sizes both entries take, stat and p are the same bits.  The exact
 * Mann-Whitney null serves every row without ties whose smaller group has at most 8 chromosomes, whatever the larger
 * (tables built on the host in 128-bit integers per distinct size pair, every entry within 1 ulp of the exact fraction).
 * k7_ranktest_wide is one workgroup per row: a bitonic sort of the two groups in LDS, binary searches, integer sums.
 * SP_EINVAL: a NULL pointer, method outside 0..1, an empty group, a chromosome index outside [0, C), a length <= 0.
 * SP_EUNSUP: a group of more than 4096 chromosomes (decided before any allocation; the message carries the size).
 * SP_ENOMEM: the workspace does not fit (the message carries its size).  M == 0: SP_OK without a launch.          */
int sp_kmer_ranktest_wide(sp_ctx *ctx, const uint32_t *counts /*host or device*/, int64_t M, int C, const int64_t *lengths,
                          int n_groups, const int32_t *group_off, const int32_t *group_chrom,
                          int method /*0 kruskal, 1 mannwhitneyu*/, int32_t *top, int32_t *second, double *pvals,
                          double *means /*M x n_groups*/, double *stat /*M, or NULL*/);
/* The same stage for test_method = wilcoxon, Cluster.py:178-194: arguments as in sp_kmer_ranktest without `method`
 * (`counts` a host or a device pointer: rows staged on this device are read in place); means, top and second are formed
 * exactly as sp_kmer_ttest and sp_kmer_ranktest form them.  The test is paired: every group has the same number n of
 * chromosomes, 2 <= n <= 64, and pair j is (j-th chromosome of the top group, j-th of the second), both in list order.
 * csrc/sp_wilcoxon.h states the arithmetic -- d = a - b on the fp64 quotients count / length, zeros dropped, doubled
 * midranks of the nonzero |d| by counting comparisons (integers), stat = min(r_plus, r_minus) -- and the branch scipy
 * 1.13 .. 1.16 takes per row under method="auto", correction=False:
 *   exact        no zero, no tie, n <= 50: the null distribution of r_plus (one table for n, built on the host in
 *                integers and uploaded with the call);
 *   permutation  a zero or a tie, n <= 13: all 2^n sign assignments, counted in integers by a Gray-code walk -- p is
 *                bit-defined and equal to scipy's; all d zero: p = 1;
 *   asymptotic   otherwise: the normal approximation with the tie correction; all d zero: p = NaN, as scipy returns
 *                (the caller keeps NaN rows).
 * stat: M statistics -- bit-defined; may be NULL.  The exact and the asymptotic p differ from scipy's only in the last bits.
 * One group alone: second = top, p = 1, stat = NaN.  k7_wilcoxon is one thread per row with the pairs in LDS; every loop
 * is bounded by n^2 or by 2^13.
 * SP_EINVAL: a NULL pointer, an empty group, a chromosome index outside [0, C), a length <= 0.
 * SP_EUNSUP: groups that do not all have one size, a size of 1, a size above 64 (decided before any allocation; the
 * message carries the sizes).  SP_ENOMEM: the workspace does not fit (the message carries its size).  M == 0: SP_OK
 * without a launch.                                                                                                  */
int sp_kmer_wilcoxon(sp_ctx *ctx, const uint32_t *counts /*host or device*/, int64_t M, int C, const int64_t *lengths,
                     int n_groups, const int32_t *group_off, const int32_t *group_chrom, int32_t *top, int32_t *second,
                     double *pvals, double *means /*M x n_groups*/, double *stat /*M, or NULL*/);

/* ---- bootstrap support of the chromosome -> subgenome assignment -----------------------------
 * Replaces the loop of Cluster.bootstrap (Cluster.py:82-118): R k-means fits, replicate r on the n columns
 * cols[r * n .. r * n + n) of z (C x M row-major fp64, the Z-normalised matrix; every index in [0, M), checked before
 * anything is launched: SP_EINVAL).  One workgroup per replicate: it gathers its columns, accumulates the C x C Gram
 * matrix in draw order (bit-defined), and runs greedy k-means++ and Lloyd on it (csrc/sp_kboot.h states every order
 * and the counter-based RNG; `seed` selects the stream, the replicate index the substream).  The reference's fits are
 * unseeded, so its support column is a random variable; this draws from the same distribution.
 * labels: R x C raw cluster ids in [0, K) (the caller renumbers them by chromosome order); iters: Lloyd iterations per
 * replicate (at most 300); gram: R x C x C, filled when not NULL (for tests).
 * Limits: 1 <= K <= C and n >= 1 (SP_EINVAL otherwise); C <= 128 and K <= 32 (SP_EUNSUP beyond: the caller keeps
 * scikit-learn).  `z` may also be a device pointer (staged with sp_dev_copy_from_host earlier); a host matrix is
 * uploaded for the call and released after it (SP_ENOMEM with the size when it does not fit).                     */
int sp_kmeans_bootstrap(sp_ctx *ctx, const double *z /*C x M*/, int C, int64_t M, const int64_t *cols /*R x n*/, int R,
                        int n, int K, uint64_t seed, int32_t *labels /*R x C*/, int32_t *iters /*R*/,
                        double *gram /*R x C x C or NULL*/);

/* ---- PCA of the k-mer matrix (Cluster.pca, Cluster.py:48-75) -------------------------------------------------
 * sklearn's PCA of the C x M Z-score matrix, split where the work is: the two passes over the M rows run here, the
 * C x C eigen-decomposition between them on the host.  counts / lengths as in sp_kmer_ttest (counts a host or a device
 * pointer: rows staged on this device are read in place, host rows are uploaded for the call and released after it).
 * Z is never materialised; csrc/sp_kpca.h states every order of operations, and both results are bit-defined.
 * sp_kmer_pca_gram: kp_rowstats writes (mean, sd) of every row -- x = count / length, sums left to right, population
 * variance -- and counts the bad rows (sd == 0 or not finite) into *n_bad; kp_gram accumulates, per tile of chromosome
 * pairs and per chunk of SP_KP_ROWS = 1024 rows, the products z_a z_b of the good rows in row order; kp_gram_sum adds the
 * chunks in chunk order and mirrors the triangle into gram (C x C).  stats: M x 2 (mean, sd), filled when not NULL (for
 * tests).  Workspace: chunks x C (C + 1) / 2 x 8 + M x 16 bytes, checked before any launch (SP_ENOMEM with its size).
 * sp_kmer_pca_signs: for each of the n_comp columns of U (C x n_comp row-major, the eigenvectors) the good row with the
 * largest |v_j| = |sum_c U[c][j] z_c| (left to right), the lowest row on ties: rows[j] its index, vals[j] the signed
 * v_j; (-1, 0) when every row is bad.  It recomputes the row statistics: the call stands alone and does not depend on a
 * preceding sp_kmer_pca_gram.
 * SP_EINVAL: C < 2, M < 1, n_comp outside 1..32, a length <= 0.  SP_EUNSUP: C > 1024.                              */
int sp_kmer_pca_gram(sp_ctx *ctx, const uint32_t *counts /*M x C, host or device*/, int64_t M, int C,
                     const int64_t *lengths, double *gram /*C x C*/, int64_t *n_bad, double *stats /*M x 2 or NULL*/);
int sp_kmer_pca_signs(sp_ctx *ctx, const uint32_t *counts, int64_t M, int C, const int64_t *lengths,
                      const double *U /*C x n_comp*/, int n_comp, int64_t *rows /*n_comp*/, double *vals /*n_comp*/);

/* ---- complete-linkage clustering for the heatmap (Cluster.heatmap, Jellyfish.py:524-609) ----------------------
 * The dendrograms R's heatmap.2 draws over the sampled k-mers and over the chromosomes: Euclidean distances between the
 * P rows of pts (host, P x D fp64, all finite) and the nearest-neighbour chain for complete linkage on them.
 * csrc/sp_hclust.h states every order of operations and every tie rule, so merges is bit-defined: (P - 1) x 4 doubles,
 * (slot x, slot y, height, size) in merge order with x < y, raw slot ids, unsorted -- what scipy's linkage holds before it
 * sorts by height and relabels (subphaser_amd/heatmap.py: to_linkage).  hc_dist fills the P x P matrix in a device buffer
 * (tiles of 32 x 32 pairs, coordinates staged through LDS 32 at a time, sums left to right, no FMA); hc_chain is ONE
 * workgroup of 1024 threads that runs all P - 1 merges on it: no second workgroup, no cooperative launch, every loop
 * bounded.  dist: the matrix before the first merge, P x P, filled when not NULL (for tests).
 * SP_EINVAL: a NULL pointer, P < 2, D < 1, a coordinate that is not finite (checked on the host before any launch).
 * SP_EUNSUP: P > 16384 (SP_HC_MAXP; decided before any allocation).  SP_ENOMEM: the workspace, P x P x 8 bytes and the
 * points, does not fit.  SP_ESTATE: the chain passed 4 P scans or a point has no neighbour at a finite distance
 * (squared differences that overflow).                                                                            */
int sp_hclust_complete(sp_ctx *ctx, const double *pts /*host, P x D*/, int P, int D, double *merges /*(P-1) x 4*/,
                       double *dist /*P x P or NULL*/);

/* ---- multi-GPU, k > 15 ----------------------------------------------------------------------
 * Twin of sp_tables_bind / sp_filter_view for 64-bit keys ("for k > 16 the exchange
 * becomes key-partitioned").  After sp_count (k > 15) every local chromosome is a sorted list of
 * (canonical key, count >= lower_count) -- what jellyfish dump holds, Jellyfish.py:697-699.
 *   sp_sparse_sizes   n[c] = entries of local chromosome c.
 *   sp_sparse_sample  up to n_samples evenly spaced keys of one list (to choose common splitters).
 *   sp_sparse_split   bounds[0..n_split+1]: bounds[i+1] = first index whose key >= splitters[i];
 *                     bounds[0] = 0, bounds[n_split+1] = n.
 *   sp_sparse_export  copy entries [first, first+count) into caller-owned DEVICE buffers (uint64
 *                     keys, uint32 counts); asynchronous on the context's stream (sp_sync).
 *   sp_sparse_view    point sp_filter / sp_filter_fetch(_device) at caller-owned DEVICE lists, one per
 *                     chromosome of the whole genome (sorted keys of ONE key range, counts >= lower),
 *                     with the global `lengths` (Jellyfish.py:449); d_keys = NULL returns to the local
 *                     chromosomes.  to_matrix/filter semantics are unchanged (Jellyfish.py:439-512). */
int sp_sparse_sizes(sp_ctx *ctx, int64_t *n);
int sp_sparse_sample(sp_ctx *ctx, int chrom, int64_t n_samples, uint64_t *keys, int64_t *n_out);
int sp_sparse_split(sp_ctx *ctx, int chrom, const uint64_t *splitters, int n_split, int64_t *bounds);
int sp_sparse_export(sp_ctx *ctx, int chrom, int64_t first, int64_t count, void *d_keys, void *d_counts);
int sp_sparse_view(sp_ctx *ctx, int C, const void *const *d_keys, const void *const *d_counts, const int64_t *n,
                   const int64_t *lengths, int k, int lower_count);

/* ---- homoeologous blocks from shared single-copy k-mers --------------------
 * Replaces the aligner runs of step_blocks (__main__.py:699-713, Blocks.py:7-56: minimap2 / unimap on every pair of
 * homoeologous chromosomes) and the alignment filter of Circos.paf2blocks (Circos.py:654-682) by an anchor vote over
 * the packed genome; the definition -- k-mer, sampling, single copy, anchor, vote, all integers -- is in
 * csrc/sp_blocks.h.  block_k odd in 17..31, block_sample 0..16, bin >= 1, chromosomes below 2^31 - 16 bases.
 *   sp_blocks_index    builds the index of one chromosome (kept until sp_blocks_release, a new sequence for the
 *                      chromosome, sp_genome_reset or the end of the context; a second call with the same block_k and
 *                      block_sample returns the stored tallies): n_sampled = valid sampled starts, n_single =
 *                      single-copy keys
 *   sp_blocks_pair     the vote of the ordered pair (a, b), both indexed with these block_k / block_sample: win_b
 *                      (-1: no anchor), opp, votes, total of ceil(len(a) / bin) entries each, caller-owned;
 *                      n_anchors = sum of total; n_spilled (may be NULL) = windows with more distinct cells than
 *                      the LDS table holds, tallied again by band passes
 *   sp_blocks_anchors  the n = n_anchors anchors of the last pair in ascending pos_a (tests and small inputs: it scans
 *                      chromosome a twice more)
 *   sp_blocks_release  frees the index of `chrom`, or every index with chrom < 0
 *   sp_blocks_set_cells  cells of the per-window LDS table, a power of two in 2..4096 (default 4096); tests use small
 *                      values to reach the band passes on small inputs -- the results do not depend on it         */
int sp_blocks_index(sp_ctx *ctx, int chrom, int block_k, int block_sample, int64_t *n_sampled, int64_t *n_single);
int sp_blocks_pair(sp_ctx *ctx, int a, int b, int block_k, int block_sample, int64_t bin, int32_t *win_b, uint8_t *opp,
                   int32_t *votes, int32_t *total, int64_t *n_anchors, int64_t *n_spilled);
int sp_blocks_anchors(sp_ctx *ctx, int32_t *pos_a, int32_t *pos_b, uint8_t *opp, int64_t n);
int sp_blocks_release(sp_ctx *ctx, int chrom);
int sp_blocks_set_cells(sp_ctx *ctx, int cells);

/* ---- LTR-pair alignment on the resident genome -------------------------------
 * The similarity of an element's two LTRs, which the reference takes from whichever detector wrote the record
 * (LTR.py:680-686): a global, banded alignment with linear gap costs, all integers, no traceback; the definition --
 * band, column scores, tie order, the edge bit -- is in csrc/sp_ltralign.h.  Pair i is the left LTR
 * [a_start[i], a_start[i] + a_len[i]) and the right LTR [b_start[i], b_start[i] + b_len[i]) of chromosome chrom[i],
 * 0-based positions on the genome of sp_genome_add; `band` = w >= 0.  out: n x 6 int32, caller-owned: score, match,
 * mismatch, gap, skip, flags.  Flag bits: 1 = the chosen path touched the first or last diagonal of the band (the
 * result may be band-limited), 2 = the band |b_len - a_len| + 2 w + 1 is wider than SP_LA_MAXBAND = 1024, 4 = an LTR is
 * longer than SP_LA_MAXLEN = 8192; a pair with bit 2 or 4 is not aligned and its other five columns are zero.
 * SP_EINVAL: no genome loaded, a chromosome index out of range, a length below 1 or an interval off its chromosome,
 * band < 0.  n = 0 is fine.  Pairs are handed to the device longest first.                                        */
int sp_ltr_align(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *a_start, const int32_t *a_len,
                 const int64_t *b_start, const int32_t *b_len, int band, int32_t *out);

/* ---- de novo LTR-RT detection on the resident genome --------------------------
 * Exact seeds at a bounded distance and their gapless X-drop extensions on the forward strand of one chromosome; the
 * definition -- word, partners (at most 32 successors looked at, 8 kept), left-maximal seeds, extension, the HSP word --
 * is in csrc/sp_ltrdetect.h, the chaining of the HSPs into candidates in subphaser_amd/ltr.py.  Positions are 0-based.
 *   sp_ltr_seeds   detects on chromosome `chrom` and keeps the HSP list of this call: the distinct (p0, len, d),
 *                  ascending as tuples; *n_seeds = the seeds before extension, *n_hsps = the length of the list.  A
 *                  chromosome shorter than seed_len has none.  No seed is lost: the seed list is sized from the count
 *                  when it outgrows its capacity.  SP_ENOMEM names the size that did not fit.
 *   sp_ltr_hsps    the list of the last sp_ltr_seeds; n = its n_hsps
 *   sp_ltr_detect_set_chunk     starts a chunk of a chromosome owns (1 .. 2^24 - 32800; 0 = that default); tests use
 *                  small values so that small inputs span many chunks -- no result depends on it
 *   sp_ltr_detect_set_capacity  seeds the append list holds at first (0 = the default, 2^20); no result depends on it
 * SP_EINVAL: null arguments, a chromosome out of range or without a packed sequence, dmin < 1 or dmin > dmax, xdrop < 0,
 * maxlen < 1, an n that is not the last call's.  SP_EUNSUP: seed_len outside 12..20, dmax > 32767, maxlen > 8192
 * (SP_LA_MAXLEN), a chromosome above 2^31 - 16 bases.                                                              */
int sp_ltr_seeds(sp_ctx *ctx, int chrom, int seed_len, int xdrop, int64_t dmin, int64_t dmax, int32_t maxlen,
                 int64_t *n_seeds, int64_t *n_hsps);
int sp_ltr_hsps(sp_ctx *ctx, int32_t *p0, int32_t *len, int32_t *d, int64_t n);
int sp_ltr_detect_set_chunk(sp_ctx *ctx, int64_t body_bases);
int sp_ltr_detect_set_capacity(sp_ctx *ctx, int64_t seeds);

/* ---- LTR-RT tree: MinHash sketches, their pairwise comparison, neighbour joining ------
 * The tree of the LTR stage is defined by integer arithmetic (csrc/sp_ltrtree.h holds the definition: k-mer, hash, sketch,
 * pair, criterion, tie order, update, guard); the distance between (shared, denom) and the matrix is host arithmetic.
 *   sp_ltr_sketch        bottom-s sketches of n elements [start[i], end[i]) (0-based, half-open) of chromosome chrom[i] on
 *                        the genome of sp_genome_add: sketch n x s uint64 (ascending, unused entries UINT64_MAX) and len n
 *                        int32, caller-owned host memory.  k odd in 9..31, s in 16..4096, end - start <= 65536.  One
 *                        workgroup per element, longest first.  n = 0 is fine.
 *   sp_ltr_sketch_set_chunk  starts of an element that one chunk of the kernel holds (1..4096; 0 = the default, which
 *                        depends on s); tests use small values so that short elements span many chunks -- no result depends
 *                        on it
 *   sp_ltr_sketch_pairs  (shared, denom) of all n x n pairs of n sketches in host memory (hand-made ones are fine: rows
 *                        ascending and distinct in their first len[i] entries); both matrices n x n int32, written in full:
 *                        symmetric, the diagonal is (len, len).  At most 32 MiB of sketches (n * s * 8 bytes) go up.
 *   sp_nj_tree           neighbour joining on the N x N int64 matrix `dist` (host): merges (N - 1) x 5 int64 =
 *                        (i, j, D(i, j), R_i, R_j) per join and (i, j, D(i, j), 0, 0) for the last two slots.  2 <= N <= 4096.
 *   sp_nj_set_mode       which driver runs the joins: 0 = chosen by N (the default), 1 = one workgroup that loops, 2 = one
 *                        row-minimum launch and one join launch per join.  No result depends on it.
 *   sp_nj_set_guard      the magnitude at which a derived distance stops the run with SP_ESTATE: 1 .. 2^40, 0 = the
 *                        default 2^40.  For tests: no matrix inside the input contract is known to reach 2^40, so a small
 *                        value is how the guard's path is reached.  A limit that is not reached changes no result.
 * SP_EINVAL: a NULL pointer; no genome; a chromosome out of range; an interval off its chromosome or with end <= start; k
 * or s out of range; len[i] outside 0..s; N < 2; a matrix that is asymmetric, has a non-zero diagonal or an entry outside
 * [0, 2^31) -- all checked on the host before any launch.  SP_EUNSUP: an element above 65536 bases, more than 32 MiB of
 * sketches, N > 4096 -- decided before any allocation.  SP_ENOMEM: the workspace does not fit.  SP_ESTATE: a derived
 * distance reached the guard (2^40, sp_ltrtree.h; sp_nj_set_guard) in magnitude; `merges` is then undefined.                          */
int sp_ltr_sketch(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int k, int s,
                  uint64_t *sketch, int32_t *len);
int sp_ltr_sketch_set_chunk(sp_ctx *ctx, int starts);
int sp_ltr_sketch_pairs(sp_ctx *ctx, int n, int s, const uint64_t *sketch, const int32_t *len, int32_t *shared,
                        int32_t *denom);
int sp_nj_tree(sp_ctx *ctx, const int64_t *dist, int N, int64_t *merges);
int sp_nj_set_mode(sp_ctx *ctx, int mode);
int sp_nj_set_guard(sp_ctx *ctx, int64_t limit);

/* ---- LTR-RT classification: profile-HMM domains in the six-frame translation of the inner sequences ------
 * The search is defined by integer arithmetic (csrc/sp_domains.h holds the definition: frames, genetic code, the pair
 * order, the recurrence, the hit and its tie order, the ranges); it is this build's own local Viterbi search, one hit per
 * (frame, profile), and is not hmmscan.  The step from a HMMER3 text file to the tables is host arithmetic
 * (subphaser_amd/domains.py: read_hmm).
 *   sp_dom_search   n intervals [start[i], end[i]) (0-based, half-open; empty is fine and means no hit) of chromosome
 *                   chrom[i] on the genome of sp_genome_add against P profiles.  Profile p has M_p = moff[p + 1] - moff[p]
 *                   nodes (moff[0] = 0); its match emissions are rows moff[p] .. of `emis` (22 columns: the residues A C D E
 *                   F G H I K L M N P Q R S T V W Y, a codon with an invalid base, a stop codon), its transitions rows
 *                   moff[p] .. of `trans` (7 columns: m->m, m->i, m->d, i->m, i->i, d->m, d->d), its local entry entry[p];
 *                   units of 1/256 bit.  The tables go up once per call.  out: n x P x 6 int32, caller-owned host memory,
 *                   per (element, profile) = score, frame (0..2 forward, 3..5 reverse complement), i_start, i_end (residues
 *                   of the frame, 0-based, inclusive), k_start, k_end (nodes, 1-based, inclusive); no residue in any
 *                   frame: INT32_MIN and zeros.  One wave per (element, frame, profile), longest first.  n = 0 is fine.
 *   sp_dom_ssv      the ungapped prefilter score (csrc/sp_domains.h: the search's recurrence restricted to the match
 *                   states; never above the score of the frame's hit) of every (element, profile, frame), arguments as
 *                   sp_dom_search: out n x P x 6 int32, one score per FRAME, INT32_MIN where the frame has no residue.
 *   sp_dom_search_pre  sp_dom_search behind the prefilter: only the (frame, profile) items with ssv >= threshold are
 *                   searched, a frame that does not pass has no hit, and an (element, profile) without a passing frame
 *                   is INT32_MIN and zeros.  A HEURISTIC: a domain whose best ungapped segment scores below the threshold
 *                   is lost.  threshold = INT32_MIN is sp_dom_search, byte for byte.  stats[0] = the items with
 *                   residues, stats[1] = those that passed.  The scores go to the host, which lists the survivors.
 *   sp_dom_ssv_set_tile  nodes a tile of the prefilter kernel holds (1..128) and diagonals a workgroup of it walks
 *                   (1..1024); 0 = the default, 128 and 1024; tests use small values -- no result depends on them
 * SP_EINVAL: a NULL pointer; no genome; a chromosome out of range; an interval off its chromosome or with end < start;
 * P < 1; offsets that do not ascend from 0 (an M < 1); a transition or entry outside [-2^20, 0] or an emission outside
 * [-2^20, 2^15]; a tile or span outside its range -- all checked on the host before any launch.  SP_EUNSUP: M > 2048,
 * an interval above 65536 bases, P > 4096, n x P > 2^24, more than 2^31 - 1 workgroups of the prefilter -- decided
 * before any allocation.  SP_ENOMEM: the workspace does not fit (the message has its size).  The three entries share
 * their checks: the same refusals, the same codes.                                                                         */
int sp_dom_search(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P,
                  const int32_t *moff, const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t *out);
int sp_dom_ssv(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P,
               const int32_t *moff, const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t *out);
int sp_dom_search_pre(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end, int P,
                      const int32_t *moff, const int32_t *emis, const int32_t *trans, const int32_t *entry,
                      int32_t threshold, int32_t *out, int64_t *stats);
int sp_dom_ssv_set_tile(sp_ctx *ctx, int nodes, int span);

/* ---- LTR-RT domain trees: profile alignment with traceback, peptides, pairwise comparison of aligned rows ------
 * The alignment is defined by integer arithmetic (csrc/sp_domalign.h holds the definition: the item, the back-pointer
 * order of the three cells, the trace, the outputs, the limits); it is the Viterbi path of sp_dom_search's local search
 * over a window of one frame, residues placed on the match nodes of one profile, and is not mafft or hmmalign.  Inserted
 * residues appear in no column.
 *   sp_dom_align     n items: interval [start[q], end[q]) of chromosome chrom[q] (as sp_dom_search takes them), frame[q]
 *                    (0..5), the residue window [i0[q], i1[q]] of that frame (0-based, inclusive, at most 8192 residues),
 *                    profile prof[q] of the P profiles (tables as sp_dom_search takes them; they go up once per call).
 *                    hit: n x 5 int32 = score, i_start, i_end, k_start, k_end (i indices of the FRAME, k 1-based, both
 *                    inclusive).  col: int32 at coff[q] .., coff[q + 1] - coff[q] = the nodes of profile prof[q] (coff[0]
 *                    = 0): the frame index of the residue in node k's match state, -1 for a node the path deletes or
 *                    does not reach.  Caller-owned host memory.  The items go in batches whose back-pointer planes (a
 *                    byte per cell) fit 1 GiB, a batch's items longest first; a batch is two or three launches: the fill
 *                    (one wave per item) and the trace.  n = 0 is fine.
 *   sp_dom_align_set_batch  the most items a batch takes (0 = the default: by the 1 GiB cap); tests use 1 and 3 -- no
 *                    result depends on it
 *   sp_dom_peptide   the residue codes of the windows of n items (0..19 = A C D E F G H I K L M N P Q R S T V W Y, 20 = a
 *                    codon with an invalid base, 21 = a stop codon): pep uint8 at poff[q] .., poff[q + 1] - poff[q] =
 *                    i1[q] - i0[q] + 1 (poff[0] = 0).  n = 0 is fine.
 *   sp_aln_pairs     N rows of C bytes in host memory: 0..19 are residues, anything else (20, 21, the gap 255) is "no
 *                    residue".  both[a][b] = the columns where both rows hold a residue, same[a][b] = those where the two
 *                    are equal.  Both N x N int32, written in full: symmetric, the diagonal is (own count, own count).
 *                    2 <= N <= 4096, 1 <= C <= 8192.  A workgroup owns a tile of 32 x 32 pairs and stages its rows in
 *                    LDS 1024 columns at a time (66048 bytes).
 * SP_EINVAL: a NULL pointer; no genome; a chromosome out of range; an interval off its chromosome or with end < start;
 * a frame outside 0..5; i0 < 0 or i0 > i1; i1 beyond the frame's residues; prof outside 0..P-1; P < 1; node offsets that
 * do not ascend from 0; coff / poff that do not start at 0 or do not leave an item its nodes / its window; a score
 * outside its range (as sp_dom_search); N < 2 or C < 1; a batch size below 0 -- all checked on the host before any
 * launch.  SP_EUNSUP: a window above 8192 residues, M > 2048, P > 4096, an interval above 65536 bases, N > 4096,
 * C > 8192 -- decided before any allocation.  SP_ENOMEM: the workspace does not fit (the message has its size).          */
int sp_dom_align(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end,
                 const int32_t *frame, const int32_t *i0, const int32_t *i1, const int32_t *prof, int P,
                 const int32_t *moff, const int32_t *emis, const int32_t *trans, const int32_t *entry, int32_t *hit,
                 const int64_t *coff, int32_t *col);
int sp_dom_align_set_batch(sp_ctx *ctx, int64_t items);
int sp_dom_peptide(sp_ctx *ctx, int64_t n, const int32_t *chrom, const int64_t *start, const int64_t *end,
                   const int32_t *frame, const int32_t *i0, const int32_t *i1, const int64_t *poff, uint8_t *pep);
int sp_aln_pairs(sp_ctx *ctx, int N, int C, const uint8_t *rows, int32_t *same, int32_t *both);

/* ---- profiling: per-kernel HIP-event timing on the context's stream ------ */
int sp_prof_enable(sp_ctx *ctx, int on);
int sp_prof_reset(sp_ctx *ctx);
/* writes a JSON object {"kernel": {"calls": n, "ms": total, "grid": g}, ...}; g: the largest grid (x * y * z
 * workgroups) launched under that name while profiling was on, since sp_prof_reset -- the counting lanes' launches
 * included */
int sp_prof_report(sp_ctx *ctx, char *buf, int64_t cap);

/* ---- bench support (not part of the reference's interface) --------------
 * Deterministic synthetic chromosome written as ASCII into a device buffer. */
int sp_synth_chrom(sp_ctx *ctx, uint8_t *d_out, int64_t len, uint64_t seed, int set_id,
                   int sg_id, int n_sg, int chrom_id, int exchange);
/* positions [start, start + n) of the same chromosome (every base is a pure function of its position) */
int sp_synth_chrom_range(sp_ctx *ctx, uint8_t *d_out, int64_t len, int64_t start, int64_t n, uint64_t seed, int set_id,
                         int sg_id, int n_sg, int chrom_id, int exchange);
/* page-locked host memory: device->host copies into it run at PCIe speed; plain
 * (pageable) buffers are accepted everywhere but copy several times slower.     */
int sp_host_alloc(sp_ctx *ctx, int64_t bytes, void **h_ptr);
int sp_host_free(sp_ctx *ctx, void *h_ptr);
/* page-lock memory the caller already owns (e.g. a POSIX shared-memory segment the ranks of one node
 * assemble the matrix in: every rank copies ITS rows over ITS PCIe link); undone by sp_host_unregister */
int sp_host_register(sp_ctx *ctx, void *h_ptr, int64_t bytes);
int sp_host_unregister(sp_ctx *ctx, void *h_ptr);
/* device memory helpers so a non-torch caller can stage buffers */
int sp_dev_alloc(sp_ctx *ctx, int64_t bytes, void **d_ptr);
int sp_dev_free(sp_ctx *ctx, void *d_ptr);
int sp_dev_copy_to_host(sp_ctx *ctx, void *dst, const void *d_src, int64_t bytes);
int sp_dev_copy_from_host(sp_ctx *ctx, void *d_dst, const void *src, int64_t bytes);


/* ---- host-side FASTA scanner (no GPU work; replaces the Bio.SeqIO record loops of Seqs.py:27-71, 121-153) ----
 * `data`/`n`: the file image (mmap or decompressed bytes), which must stay valid until sp_fasta_close.  A record
 * starts at a '>' that is the first byte of a line; bytes <= 0x20 are dropped from the sequence lines.
 * sp_fasta_fetch: hdr_start[r] .. hdr_end[r] = header text of record r (without '>' and the line break),
 * seq_off[r] .. seq_off[r + 1] = its bases inside `cat` (n_bases bytes, caller-owned, may be page-locked). */
typedef struct sp_fasta sp_fasta;
int sp_fasta_open(const void *data, int64_t n, int threads, sp_fasta **out);
int sp_fasta_counts(const sp_fasta *h, int64_t *n_records, int64_t *n_bases);
int sp_fasta_fetch(const sp_fasta *h, int64_t *hdr_start, int64_t *hdr_end, int64_t *seq_off, void *cat);
void sp_fasta_close(sp_fasta *h);


/* ---- host-side text writers (no GPU work) --------------------------------------------------------------------
 * Rows of `.kmer.mat` (Jellyfish.py:515-520) and `.sig.kmer-subgenome.tsv` (Cluster.py:165-176) formatted by
 * threads of the calling process and written to the open file descriptor `fd` in row order; floats are printed as
 * Python's repr() prints them.  The caller writes the header line (and flushes) first.  names: n_names
 * '\0'-separated strings.  sp_text_repr: repr of x[i] back to back in out (>= 40 bytes per value), off[n + 1]. */
int sp_text_kmer_matrix(const uint64_t *keys, int k, const double *freqs, int64_t M, int C, int threads, int fd,
                        int64_t *bytes);
int sp_text_sig_kmers(const uint64_t *keys, int k, const int32_t *top, const char *names, int n_names,
                      const double *pvals, const double *means, int G, int64_t M, int threads, int fd, int64_t *bytes);
int sp_text_repr(const double *x, int64_t n, char *out, int64_t *off);

/* Generic tab-separated rows for the feature-scale outputs: `.custom.enrich` / `.ltr.enrich` (Stats.py:59-70) and
 * the feature-mode `.bin.count` lines (Seqs.py:228-244).  Row i = the columns joined by '\t' + '\n'.
 *   SP_COL_STR   data = char blob, off[M + 1]: the string of row i is data[off[i] .. off[i + 1])
 *   SP_COL_I64   data = int64 [M x width], printed in decimal, joined by `join`
 *   SP_COL_F64   data = double [M x width], printed as Python's repr(), joined by `join`
 *   SP_COL_NAME  data = int32 [M] indices into `names` (`width` strings; string j = names[off[j] .. off[j + 1]))
 *   SP_COL_IVAL  data = int64 [M x 3] (name index, start, end), printed `name:start-end` (ids of BED intervals) */
#define SP_COL_STR 0
#define SP_COL_I64 1
#define SP_COL_F64 2
#define SP_COL_NAME 3
#define SP_COL_IVAL 4
typedef struct sp_text_col {
    int kind;
    int width;
    char join;
    const void *data;
    const int64_t *off;
    const char *names;
} sp_text_col;
int sp_text_table(const sp_text_col *cols, int n_cols, int64_t M, int threads, int fd, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
