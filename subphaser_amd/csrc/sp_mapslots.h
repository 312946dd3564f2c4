// sp_mapslots.h -- the integer rules of the map stage's three walk modes, shared by every kernel of sp_map.hip and
// sp_sparse.hip: which output slot (bin + chunk duplicates, Seqs.map_kmer3) a start counts in and where that slot ends, when
// a range's slots fit the LDS histogram, the chunk of a slot (window stack), which feature a start belongs to and which
// starts of a unit lie inside one, and the subgenome mask of three label planes.
// Everything here is plain integer arithmetic, __host__ __device__, so that tests/test_mapslots_host.py checks it with the
// host compiler alone (as sp_maphash.h and sp_labelplan.h are checked).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_MS_HD __host__ __device__ __forceinline__
#else
#define SP_MS_HD static inline
#endif

#ifndef SP_UNIT
#define SP_UNIT 64      // starts per unit: one bit of a 64-bit plane each (sp_device.h)
#endif
#ifndef MAP_BLOCK
#define MAP_BLOCK 512   // rounds 2-5 (one-phase walks): 256 -> 70.5 ms, 512 -> 68.3, 768 -> 66.2, 1024 -> 73.8.  Round 6 (two-phase walk,
                        // bound by waiting, not by instruction issue): 768 x 2 workgroups per CU (6 waves per SIMD) 34.5 ms,
                        // 512 x 4 (8 per SIMD, 64 VGPRs) 32.6, 256 x 8 33.0, 384 x 5 35.4, 1024 x 2 33.6
#endif
#define MAP_RANGE (MAP_BLOCK * SP_UNIT)  // starts per block iteration
#ifndef MAP_LDS_ENTRIES
#define MAP_LDS_ENTRIES 1024      // (4096 until round 6: the LDS went to the walk's candidate queue; a range of 49 152 starts needs
                                   // ~ 10 x S entries at 10-kb bins, 1024 cover bins down to ~150 bases at S = 3 -- below that: global atomics)
#endif

// ----------------------------------------------------------------- bins: output slots
struct sp_map_params {
    int64_t n_units;
    int64_t bin_size;
    int64_t chunk_size;
    int64_t nslots;
    int S;
    int use_lds;
};

SP_MS_HD int64_t map_slot(int64_t s, const sp_map_params &P, int k) {
    int64_t chunk = 0;
    if (P.chunk_size > 0 && s >= P.chunk_size - (k - 1)) chunk = (s + (k - 1)) / P.chunk_size;
    return s / P.bin_size + chunk;
}

// first start after `s` whose output slot differs from map_slot(s) (next bin or next chunk boundary)
SP_MS_HD int64_t map_slot_end(int64_t s, const sp_map_params &P, int k) {
    int64_t e = (s / P.bin_size + 1) * P.bin_size;
    if (P.chunk_size > 0) {
        const int64_t chunk = (s >= P.chunk_size - (k - 1)) ? (s + (k - 1)) / P.chunk_size : 0;
        const int64_t c = (chunk + 1) * P.chunk_size - (k - 1);
        e = c < e ? c : e;
    }
    return e;
}

SP_MS_HD int64_t map_nslots_host(int64_t len, int64_t bin_size, int64_t chunk_size, int k) {
    int64_t L = len > 0 ? len : 1;
    int64_t nb = (L + bin_size - 1) / bin_size;
    int64_t nch = chunk_size > 0 ? (L + (k - 1)) / chunk_size + 1 : 1;
    return nb + nch;
}

// the parameters of a bins walk; its LDS histogram serves when the slots a range of MAP_RANGE starts touches fit it
SP_MS_HD sp_map_params map_params_of(int64_t len, int64_t bin_size, int64_t chunk_size, int64_t nslots, int S) {
    sp_map_params P;
    P.n_units = (len + SP_UNIT - 1) / SP_UNIT;
    P.bin_size = bin_size;
    P.chunk_size = chunk_size;
    P.nslots = nslots;
    P.S = S;
    const int64_t local = MAP_RANGE / bin_size + 3 + (chunk_size > 0 ? MAP_RANGE / chunk_size + 2 : 0);
    P.use_lds = (local * S <= MAP_LDS_ENTRIES) ? 1 : 0;
    return P;
}

// the chunk a slot belongs to (map_slot inverted; chunk_size > 0).  First slot of chunk j >= 1: (j*W - (k-1)) / b + j;
// chunk(slot) = #{j : first(j) <= slot}
SP_MS_HD int64_t map_chunk_of_slot(int64_t slot, int64_t bin_size, int64_t chunk_size, int k) {
    int64_t chunk = slot * bin_size / (chunk_size + bin_size);
    while ((((chunk + 1) * chunk_size - (k - 1)) / bin_size + (chunk + 1)) <= slot) chunk++;
    while (chunk > 0 && ((chunk * chunk_size - (k - 1)) / bin_size + chunk) > slot) chunk--;
    return chunk;
}

// bits [a, b) of a unit, 0 <= a, b <= 64
SP_MS_HD unsigned long long map_span(int64_t a, int64_t b) {
    if (b <= a) return 0ULL;
    return (b >= 64 ? ~0ULL : ((1ULL << b) - 1ULL)) & ~((1ULL << a) - 1ULL);
}

// the starts of a unit that carry label l = 1 + subgenome (1 .. 7), from the three planes of the label's bits
SP_MS_HD unsigned long long map_plane_mask(const unsigned long long lab[3], int sg) {
    const int l = sg + 1;
    return ((l & 1) ? lab[0] : ~lab[0]) & ((l & 2) ? lab[1] : ~lab[1]) & ((l & 4) ? lab[2] : ~lab[2]);
}

// ----------------------------------------------------------------- features
// feature mode: per-feature totals.  The features lie back to back in one packed sequence (no
// separators): a k-mer belongs to feature f iff it lies entirely inside [foff[f], foff[f+1]).  The
// feature of a unit's first hit is found by binary search, later hits of the unit walk forward.
struct map_feat_cursor {
    int64_t f, next;   // current feature and foff[f + 1]; f < 0: not located yet
};
SP_MS_HD bool map_feat_locate(map_feat_cursor &c, int64_t start, int k, const int64_t *__restrict__ foff, int64_t n_feat) {
    if (c.f < 0) {
        int64_t lo = 0, hi = n_feat;   // last f with foff[f] <= start
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (foff[mid] <= start) lo = mid;
            else hi = mid;
        }
        c.f = lo;
        c.next = foff[lo + 1];
    }
    while (start >= c.next && c.f + 1 < n_feat) {
        c.f++;
        c.next = foff[c.f + 1];
    }
    return start + k <= c.next;        // false: the k-mer runs into the next feature
}

// The unit of 64 starts at s0: the feature it starts in (`first`: last f with foff[f] <= s0) and, returned, the starts whose
// k-mer crosses no feature boundary.  A boundary at `e` = foff[f + 1] disqualifies the starts (e - k, e): their k-mers run
// into the next feature.
SP_MS_HD unsigned long long map_unit_fit(const int64_t *__restrict__ foff, int64_t n_feat, int64_t s0, int k, int64_t &first) {
    int64_t lo = 0, hi = n_feat;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (foff[mid] <= s0) lo = mid;
        else hi = mid;
    }
    first = lo;
    unsigned long long fit = ~0ULL;
    for (int64_t f = lo; f < n_feat; f++) {
        const int64_t e = foff[f + 1];
        if (e - k + 1 >= s0 + SP_UNIT) break;
        fit &= ~map_span((e - k + 1 > s0 ? e - k + 1 : s0) - s0, (e < s0 + SP_UNIT ? e : s0 + SP_UNIT) - s0);
        if (e >= s0 + SP_UNIT) break;
    }
    return fit;
}
