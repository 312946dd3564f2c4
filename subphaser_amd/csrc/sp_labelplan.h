// sp_labelplan.h -- which table a label set lives in and how large it is, as plain C++: no HIP types, so the host compiler
// alone builds it (tests/labelplan_host_check.cpp).  sp_labels_set (sp_map.hip) reads the switches, makes the plan and
// executes it; the map entries dispatch on the plan's `kind`.
//
// The three switches, read on every sp_labels_set call (never cached: a caller may change them between two calls):
//   SP_MAP_ENGINE=1    one label per k-mer (label bytes / per-k-mer hash) whatever the number of subgenomes
//   SP_CTAB=0          never a bucket table (cross-check);  SP_CTAB=1: at k <= 15 the compact table whenever its tag fits
//   SP_CTAB_FACTOR=f   at least f x n buckets (default 2)
#pragma once
#include <stdint.h>
#include <stdlib.h>

#define MAP_PAIR_MAX_SG 7            // the pair tables keep labels in fields of 4 bits: 0 = none, 1..7, and a "seen" bit
#define MAP_CT_MAX_TAG_BITS 2        // compact table (sp_map.h): bits of mix(t) in the tag (next to side and e)
#define SQ_TAG_BITS 39               // quad-bucket table (sp_sparse.hip): bits of the tag, 5 of them side and e

enum sp_label_kind {
    SP_LABELS_DIRECT,        // k <= 15: 4^(k-1) words addressed by the (k-1)-mer
    SP_LABELS_COMPACT,       // k <= 15, S <= 3: 2^bb buckets of four tagged entries + overflow table (sp_map.h)
    SP_LABELS_LABEL_BYTES,   // k <= 15: one byte per dense slot (more than 7 subgenomes)
    SP_LABELS_QUAD,          // k > 15, S <= 3: 2^bb buckets of four tagged 64-bit entries + overflow table (sp_sparse.hip)
    SP_LABELS_PAIR_HASH,     // k > 15, S <= 7: open-addressing hash keyed by the (k-1)-mer
    SP_LABELS_KMER_HASH      // k > 15: open-addressing hash keyed by the k-mer
};

struct sp_label_env {
    bool per_kmer;           // SP_MAP_ENGINE=1
    int ctab;                // SP_CTAB: 0, 1, or -1 when unset
    int64_t factor;          // SP_CTAB_FACTOR (> 0), else 2
};

inline sp_label_env sp_label_env_read() {
    const char *eng = getenv("SP_MAP_ENGINE"), *ct = getenv("SP_CTAB"), *f = getenv("SP_CTAB_FACTOR");
    sp_label_env E;
    E.per_kmer = eng && eng[0] == '1';
    E.ctab = ct && ct[0] == '0' ? 0 : ct && ct[0] == '1' ? 1 : -1;
    E.factor = f && atoll(f) > 0 ? atoll(f) : 2;
    return E;
}

struct sp_label_plan {
    sp_label_kind kind;
    int bb;                  // COMPACT / QUAD: 2^bb buckets; else 0
    int64_t bucket_bytes;    // 16 (COMPACT) / 32 (QUAD) a bucket
    int64_t ovf_n;           // entries of the overflow table, a power of two >= max(4096, n / 2)
    int64_t ovf_bytes;       // 8 (COMPACT) / 16 (QUAD) an entry
    int64_t cap;             // k > 15: 16-byte entries of the hash table, a power of two (1024, unused, beside the quad table)
    int64_t entries;         // k <= 15: words of the direct table, 4^(k-1)
};

inline int64_t sp_label_pow2(int64_t from, int64_t least) {
    while (from < least) from <<= 1;
    return from;
}

// k: as counted; n: labelled k-mers; nslots: the dense table's slots (unused by the rules: the label bytes are sized by it)
inline sp_label_plan sp_label_plan_make(int k, int64_t n, int n_sg, int64_t nslots, const sp_label_env &E) {
    (void)nslots;
    sp_label_plan P = {SP_LABELS_DIRECT, 0, 0, 0, 0, 0, 0};
    const bool pairs = !(n_sg > MAP_PAIR_MAX_SG || E.per_kmer);
    const int sb = 2 * (k - 3);      // bits of the (k-3)-mer the bucket tables are addressed by
    // a labelled k-mer brings ~3.6 keys (two (k-1)-mers, each under two (k-3)-mers, shared with its neighbours in a run)
    int bb = 8;
    while (bb < 30 && ((int64_t)1 << bb) < E.factor * (n > 0 ? n : 1)) bb++;
    const int tag_bits = k <= 15 ? MAP_CT_MAX_TAG_BITS : SQ_TAG_BITS - 5;      // what the tag holds of the sb - bb other bits
    if (bb < sb - tag_bits) bb = sb - tag_bits;
    const bool fits = pairs && n_sg <= 3 && bb <= sb && bb <= 27;
    bool buckets;
    if (k <= 15) {
        // the compact table when the direct one is beyond every cache and at least four times larger, or on demand
        P.entries = (int64_t)1 << (2 * (k - 1));
        buckets = fits && k >= 5 && bb >= 1 && E.ctab != 0 &&
                  (E.ctab == 1 || (P.entries * 4 > ((int64_t)64 << 20) && ((int64_t)16 << bb) * 4 <= P.entries * 4));
        P.kind = buckets ? SP_LABELS_COMPACT : pairs ? SP_LABELS_DIRECT : SP_LABELS_LABEL_BYTES;
    } else {
        buckets = fits && E.ctab != 0;
        P.kind = buckets ? SP_LABELS_QUAD : pairs ? SP_LABELS_PAIR_HASH : SP_LABELS_KMER_HASH;
        P.cap = buckets ? 1024 : sp_label_pow2(1024, (pairs ? 4 : 2) * n + 16);
    }
    if (buckets) {
        P.bb = bb;
        P.bucket_bytes = ((int64_t)1 << bb) * (k <= 15 ? 16 : 32);
        P.ovf_n = sp_label_pow2(4096, n / 2);
        P.ovf_bytes = P.ovf_n * (k <= 15 ? 8 : 16);
    }
    return P;
}

// the overflow table of a bucket table filled up (adversarial key sets only): the table that takes over
inline sp_label_plan sp_label_plan_fallback(const sp_label_plan &Q, int64_t n) {
    sp_label_plan P = Q;
    P.bb = 0;
    P.bucket_bytes = P.ovf_n = P.ovf_bytes = 0;
    if (Q.kind == SP_LABELS_COMPACT) P.kind = SP_LABELS_DIRECT;
    if (Q.kind == SP_LABELS_QUAD) {
        P.kind = SP_LABELS_PAIR_HASH;
        P.cap = sp_label_pow2(1024, 4 * n + 16);
    }
    return P;
}
