// sp_s3plan.h -- the plan of the k = 16..32 count chain (sp_sparse2.hip) and the thresholds at which its finish kernels
// change path, as plain C++: no HIP types, so the host compiler alone builds it (tests/s3plan_host_check.cpp).  The
// kernels, their drivers and the hand-made test chromosomes (tests/s3_cases.py, through the host check's NAME value
// lines) all read the numbers from here.
#pragma once
#include <stdint.h>

#define S3_P1_UNIT 32
#ifndef S3_P1T32
#define S3_P1T32 512            // threads of an s3_part1 tile with 32-bit residuals (k <= 21): 512 x 32 = 16384 starts
#endif
#define S3_P1T64 256            // ... with 64-bit residuals (k >= 22): 256 x 32 = 8192 starts
#ifndef S3_P2_THREADS
#define S3_P2_THREADS 512
#endif
#ifndef S3_P2_PER
#define S3_P2_PER 16
#endif
#define S3_P2_KEYS (S3_P2_THREADS * S3_P2_PER)   // keys per part2 / hist2 tile
#define S3_SORT_THREADS 256
#ifndef S3_SORT_PER
#define S3_SORT_PER 8      // (16: s3_final 140 -> 131 ms per wheat-like pass at k = 21, but 11 -> 16 ms at k = 17 and more big-list buckets)
#endif
#define S3_SORT_CAP (S3_SORT_THREADS * S3_SORT_PER)   // keys one workgroup sorts

struct s3_plan {
    int T, B1, B2, R1, R2, F1, F2;
    bool wide1, wide2;   // residuals after level 1 / level 2 need 64 bits
};

static inline s3_plan s3_make_plan(int k) {
    s3_plan p;
    p.T = 2 * k;
    p.B1 = 10;   // k <= 21: the residual (2k - 10 bits) fits 32 bits
#ifndef S3_B2
#define S3_B2 9
#endif
    // Round 6: k = 16 / 17 split level 2 into 2^8 instead of 2^9: the bitmap finish takes 16-bit residuals anyway, and with
    // half as many fine buckets of twice the keys (2.6 K on a wheat-sized chromosome) s3_part2 writes runs of twice the
    // length and every per-bucket step of the finish -- seven barriers, two block scans -- is paid half as often:
    // wheat-like k = 17 pass 213.2 -> 195.5 ms (s3_part2 149 -> 115 ms of events).  k >= 18 (hash finish) stays at 2^9:
    // 2^8 sends its buckets past the table's capacity (k = 21: 429 ms), 2^10 is slower as well (228 against 220).
    p.B2 = k <= 17 ? 8 : S3_B2;
    p.R1 = p.T - p.B1;
    p.R2 = p.R1 - p.B2;
    p.F1 = 1 << p.B1;
    p.F2 = 1 << p.B2;
    p.wide1 = p.R1 > 32;
    p.wide2 = p.R2 > 32;
    return p;
}

#define S3_SAMPLE_MIN_LEN (1LL << 24)     // shorter chromosomes: exact level-1 histogram (and the key count with it)

// ---- s3_final
#define S3_SPLIT_BITS 8
#define S3_DIRECT_BITS 12

#define S3_SMALL_PER 8
#define S3_SMALL_CAP (S3_SORT_THREADS * S3_SMALL_PER)   // buckets up to this size take the light kernel

#define S3_HASH_SLOTS 2048                       // LDS hash table of the hot-key path
#define S3_HASH_MAX (S3_HASH_SLOTS * 3 / 4)      // distinct residuals it accepts

// (s3_final_hash's table -- described at the kernel -- is also what s3_final counts its pieces with)
#define S3H_COUNTERS 4096
#define S3H_SLOTS 2048
#define S3H_CAP 1536            // distinct residuals the table accepts
#define S3H_PER 8               // keys per thread held in registers: buckets up to 2048 keys are read once

// ---- s3_final_bitmap (k = 16, 17)
#define S3_BM_MAXBITS 16
#ifndef S3_BM_CAP
#define S3_BM_CAP 4096      // distinct residuals per bucket this kernel takes (cnt[] entries); beyond: s3_final
#endif
#define S3_BM_NMAX (1u << 22)   // keys per bucket it is willing to stream (hot buckets: few distinct, many copies)
#define S3_BM_PER 8             // keys per thread prefetched into registers (buckets up to 2048 keys never re-read)

// ---- oversized buckets by hash class
#define S3B_SPREAD 32
#define S3B_KCAP 4096
#define S3B_MAXBIG 1024         // more oversized buckets than this per chromosome: the library path

// s3_final splits a bucket of n > S3_SORT_CAP residuals of R2 bits on their top `sb` bits.  The rule is ONE text with two
// readers: s3_final expands S3_SPLIT_BITS_LOOP in place, and s3_split_bits wraps the same text for the host (the routing
// model of tests/s3_cases.py is checked against it).  s3_final does not call the function: through a call the compiler
// learns the range of the returned value (sb <= 8) and compiles the rest of s3_final differently -- the same registers and
// LDS, 43 instructions fewer with 64-bit residuals -- and a change of that kernel's code wants a measurement of its own.
#define S3_SPLIT_BITS_LOOP(sb, n, R2)                                                                              \
    int sb = 1; /* pieces of ~2 K residuals: a few sorts, not 2^10 tiny ones */                                    \
    while (sb < S3_SPLIT_BITS && ((n) >> sb) > S3_SORT_CAP / 2) sb++;                                              \
    if (sb > (R2)) sb = (R2)
static inline int s3_split_bits(uint32_t n, int R2) {
    S3_SPLIT_BITS_LOOP(sb, n, R2);
    return sb;
}
