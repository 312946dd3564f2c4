// sp_map.h -- what the dense (sp_map.hip) and the sparse (sp_sparse.hip) map stages share: the pair
// filter, the pair-table field layout, the walkers' interface and the one consumer per walk mode (bins, features, intervals).
// The integer rules of the modes (output slots of Seqs.map_kmer3's chunks and bins, feature cursor, plane masks): sp_mapslots.h.
#pragma once
#include "sp_device.h"
#include "sp_maphash.h"
#include "sp_mapslots.h"

#ifndef MAP_BLOOM_MAX_BITS
#define MAP_BLOOM_MAX_BITS 25
#endif
#ifndef MAP_BLOOM_MIN_BITS
#define MAP_BLOOM_MIN_BITS 12
#endif
#ifndef MAP_FILL_MAX
#define MAP_FILL_MAX 0.40
#endif
// Blocked Bloom filter: one 32-bit word per key (ONE memory access per probe), three bits in it.
//
// Round 6 -- WHICH word.  The map stage is bound by the number of these probes: one scattered 4-byte gather per pair of starts,
// priced per ACTIVE lane (tools/ubench_gather.hip: two gathers per quad issued by 2/3 of the lanes each cost 2/3).  Until now the
// word was the hashed (k-1)-mer x itself, so neighbouring pairs never met in a word.  A (k-1)-mer has two (k-3)-mer CORES, its
// first and its last k-3 bases, and the pairs along a scan form a chain: the last core of the pair at s is the first core of the
// pair at s + 2.  With MAP_BLOOM_CORE the word of x is addressed by the core of x with the SMALLER hash (canonical cores, so
// both strands agree): a core that beats both of its neighbours in the chain answers BOTH of its pairs with one gather, and a
// lane needs a fresh word for 2/3 of its pairs -- a third of the probes gone, with ONE insertion per (k-1)-mer: the filter keeps
// its size (2 MiB for the wheat-like label set: it must stay inside an XCD's L2 next to the table lines streaming through) and
// its false-positive rate.  (The alternative of the round-5 review -- an 8-byte block addressed by the core two pairs of a quad
// share, every (k-1)-mer under both cores -- halves the gathers but doubles the entries: 34 % false-positive quads at 2 MiB, and
// at 4 MiB the filter falls out of the L2 and the gain is gone: profiles/r06_notes.md, section 3.)  The minimum of two uniform
// hashes is not uniform (density 2 (1 - u)); 1 - (1 - u)^2 is, and that is what indexes the words, so the fill stays even.
// The three bits inside the word still come from the hashed (k-1)-mer.  k < 5 (cores of fewer than two bases): the old addressing.
// (MAP_BLOOM_CORE, the flag in the `nbits` argument of everything below, and the hash functions themselves: sp_maphash.h.
// That is the family of k > 15; at k <= 15 the mirror image -- the LARGER hash and u^2 -- addresses the word and the three
// bits come from the two core hashes: the same design on cheaper arithmetic, profiles/map_hash_notes.md.)
// Runs (profiles/map_runs_notes.md).  Labelled k-mers come in runs -- inside a repeat copy every quad of a lane is a candidate --
// and a candidate quad goes to the exact table whatever the filter says, so the two-phase walk of k <= 15 (map_unit_scan64)
// does not ASK the filter inside a run: a lane whose last MAP_RUNS_R probed quads passed on both pairs enqueues the next quad
// unprobed, both pair flags set, for at most MAP_RUNS_P quads in a row; then it probes again.  The table is exact and the
// filter only ever said "maybe": a predicted pair that is not labelled finds no tag and sets nothing.  The price is one
// bucket look-up for a predicted quad that lies just past a run's end.  SP_MAP_RUNS=0 clears the flag (cross-check: the walk
// then probes every quad).  The k > 15 twin (map_unit_scan64_h) probes every quad: there the rule measured slower.
#define MAP_RUNS 0x200                // flag in `nbits`, next to MAP_BLOOM_CORE
#ifndef MAP_RUNS_R
#define MAP_RUNS_R 2
#endif
#ifndef MAP_RUNS_P
#define MAP_RUNS_P 3
#endif
__device__ __forceinline__ bool map_bloom_test(const uint32_t *__restrict__ bloom, int nbits, int k, uint64_t x) {
    const map_bloom_probe p = map_bloom(x, k, nbits);
    return (bloom[p.word] & p.bits) == p.bits;
}

// Walk one unit and call hit(start, fwd, rc) for every VALID start whose pair passes the filter.
template <typename KeyT, typename KP, typename F>
__device__ __forceinline__ void map_pair_scan(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm,
                                              int64_t s0, const KP &kp, const uint32_t *__restrict__ bloom,
                                              int nbits, F &&hit) {
    bool pairhit = false;
    const KeyT m1mask = (KeyT)(kp.kmask >> 2);
    sp_scan_unit_all<SP_UNIT, KeyT>(pk, nm, s0, kp, [&](int64_t start, KeyT fwd, KeyT rc, bool valid_k, bool valid_k1) {
        if (!(start & 1)) {   // first of the pair: screen both members through their shared (k-1)-mer
            pairhit = false;
            if (valid_k1) {
                const KeyT mf = fwd & m1mask, mr = rc >> 2;
                pairhit = map_bloom_test(bloom, nbits, kp.k, (uint64_t)(mf < mr ? mf : mr));
            }
        }
        if (pairhit && valid_k) hit(start, fwd, rc);
    });
}

struct map_pair_loc {
    uint32_t idx;   // canonical (k-1)-mer
    int field;
};
// where the k-mer `o` (any orientation; k >= 1) lives when it is looked up through its prefix / suffix (k-1)-mer
__host__ __device__ __forceinline__ map_pair_loc map_pair_loc_prefix(uint64_t o, int k) {
    map_pair_loc r;
    const uint32_t b = (uint32_t)(o & 3ULL);
    if (k == 1) { r.idx = 0; r.field = 4 + (int)b; return r; }
    const uint64_t p = o >> 2, pc = sp_revcomp(p, k - 1);
    if (p <= pc) { r.idx = (uint32_t)p; r.field = 4 + (int)b; }       // x + b
    else { r.idx = (uint32_t)pc; r.field = 3 - (int)b; }              // rc: comp(b) + rc(x)
    return r;
}
__host__ __device__ __forceinline__ map_pair_loc map_pair_loc_suffix(uint64_t o, int k) {
    map_pair_loc r;
    const uint32_t b = (uint32_t)(o >> (2 * (k - 1))) & 3u;
    if (k == 1) { r.idx = 0; r.field = (int)b; return r; }
    const uint64_t m1mask = (1ULL << (2 * (k - 1))) - 1ULL;
    const uint64_t x = o & m1mask, xc = sp_revcomp(x, k - 1);
    if (x <= xc) { r.idx = (uint32_t)x; r.field = (int)b; }           // b + x
    else { r.idx = (uint32_t)xc; r.field = 7 - (int)b; }              // rc: rc(x) + comp(b)
    return r;
}

// ----------------------------------------------------------------- compact exact pair table (S <= 3; round 5: QUAD buckets)
// The direct pair table is 4^(k-1) words (1 GiB at k = 15) for a few million used entries, and every gather from it
// leaves the chip's caches (54 G/s).  Round 4 put the entries into 2^23 buckets of two tagged words behind a bijective
// mix of the (k-1)-mer (64 MB, served by the Infinity Cache: one 8-byte load per candidate PAIR, 51 -> 46 ms per
// wheat-like pass).  What is left of the map stage after the filter probes is exactly those look-ups (1.4 G per pass at
// 12.8 ns per G), and labelled k-mers come in runs: the two pairs of a QUAD of starts 4g .. 4g+3 are almost always
// candidates together.  Their (k-1)-mers x1 (at 4g+1) and x2 (at 4g+3) overlap in the (k-3)-mer s = suffix of x1 =
// prefix of x2, so the table is now addressed by s: bucket = top bits of a bijective mix of the CANONICAL t = min(s,
// rc(s)), FOUR tagged 32-bit entries per 16-byte bucket, and ONE 16-byte load answers all four starts of the quad.
// An entry belongs to a (k-1)-mer y read in the orientation in which its (k-3)-mer at one end is canonical:
//     side 0 ("L"):  y = e + t      side 1 ("R"):  y = t + e        e = the two bases beyond t (4 bits)
// and holds the labels of the eight k-mers b + y and y + b in THAT orientation (field b / 4 + b, as in the direct
// table).  Every (k-1)-mer of a labelled k-mer is entered twice -- under its prefix and under its suffix (k-3)-mer --
// because which of the two a genome position shares with its neighbour pair depends on the position modulo 4.
// Entry: tag << 25 | overflow flag << 24 | eight 3-bit fields (label 1..3, "seen" in the third bit); tag = the low tb
// <= 2 bits of mix(t) << 5 | side << 4 | e; bucket + tag determine (t, side, e): a tag match is an exact match.
// 0 = empty.  A key that finds its bucket full goes to a small open-addressing overflow table of {key id + 1, fields}
// words and raises the flag in the bucket's first entry.
#define MAP_CT_FIELD 3
#define MAP_CT_ANY 0x6DB6DBu          // the label bits of all eight fields
#define MAP_CT_PAYLOAD 0xFFFFFFu
#define MAP_CT_OVF (1u << 24)
// (MAP_CT_MAX_TAG_BITS, the bits of mix(t) in the tag next to side and e: sp_labelplan.h, the sizing needs it)
struct map_ptab {
    uint32_t *direct;                 // 4^(k-1) words, 4-bit fields (S <= 7), or NULL
    uint4 *buckets;                   // compact table: four entries per bucket
    unsigned long long *ovf;          // overflow table: (key id + 1) << 32 | fields, 0 = empty
    uint32_t ovf_mask;                // its size - 1
    int sb, tb;                       // bits of the shared (k-3)-mer 2(k-3), bits of mix(t) kept in the tag
};
__host__ __device__ __forceinline__ uint32_t map_ct_ovf_home(uint32_t x) { return (x * 0xC2B2AE35u) >> 7; }
struct map_ct_key {
    uint32_t bucket, tag, kid;        // kid: (t, side, e) packed, the overflow table's key
};
__host__ __device__ __forceinline__ map_ct_key map_ct_key_of(const map_ptab &T, uint32_t t, uint32_t side, uint32_t e) {
    const uint32_t h = map_ct_mix24(t, T.sb);      // (a map_ptab exists at k <= 15 only: sb <= 24 -- sp_maphash.h)
    map_ct_key r;
    r.bucket = h >> T.tb;
    r.tag = ((h & ((1u << T.tb) - 1u)) << 5) | (side << 4) | e;
    r.kid = (t << 5) | (side << 4) | e;
    return r;
}
// the eight fields of a key (0: absent) and where they live (for the "seen" mark): bucket * 4 + entry, or
// 0x80000000 | overflow slot.  `B` = the key's bucket, already loaded.
struct map_ct_hit {
    uint32_t fields, loc;
};
__device__ __forceinline__ map_ct_hit map_ct_find(const map_ptab &T, const uint4 &B, const map_ct_key &q) {
    map_ct_hit r;
    const uint32_t w[4] = {B.x, B.y, B.z, B.w};
    r.fields = 0;
    r.loc = 4u * q.bucket;
#pragma unroll
    for (int i = 3; i >= 0; i--)
        if ((w[i] >> 25) == q.tag && (w[i] & MAP_CT_PAYLOAD)) {
            r.fields = w[i] & MAP_CT_PAYLOAD;
            r.loc = 4u * q.bucket + (uint32_t)i;
        }
    if (!r.fields && (B.x & MAP_CT_OVF)) {         // rare: the bucket overflowed and the key is in none of its entries
        uint32_t i = map_ct_ovf_home(q.kid) & T.ovf_mask;
        // bounded like map_ct_insert's loop: a table that ended exactly full has no empty slot to stop an absent key
        // (advisor r04; sp_labels_set also keeps the table at most half full)
        for (uint32_t probes = 0; probes <= T.ovf_mask; probes++) {
            const unsigned long long o = T.ovf[i];
            if (o == 0ULL) break;
            if ((uint32_t)(o >> 32) == q.kid + 1u) {
                r.fields = (uint32_t)o & MAP_CT_PAYLOAD;
                r.loc = 0x80000000u | i;
                break;
            }
            i = (i + 1u) & T.ovf_mask;
        }
    }
    return r;
}
__device__ __forceinline__ void map_ct_mark(const map_ptab &T, uint32_t loc, uint32_t bits) {
    if (loc & 0x80000000u) atomicOr(&T.ovf[loc & 0x7fffffffu], (unsigned long long)bits);
    else atomicOr(reinterpret_cast<uint32_t *>(T.buckets) + loc, bits);
}
// The (up to four) table keys under which the k-mer `o` (ONE orientation, as given) is entered / found: its prefix and
// its suffix (k-1)-mer, each under its prefix and its suffix (k-3)-mer -- but only where that (k-3)-mer is canonical AS
// READ in this orientation (u <= rc(u)); the other orientation of the k-mer supplies the rest, and a palindromic
// (k-3)-mer is entered from both (the scan meets it with either flank on either side).  k >= 4.
struct map_ct_site {
    uint32_t t, side, e;
    int field;
};
__host__ __device__ __forceinline__ int map_ct_sites(uint64_t o, int k, map_ct_site out[4]) {
    const int sb = 2 * (k - 3);
    const uint64_t m1mask = (1ULL << (2 * (k - 1))) - 1ULL, smask = (1ULL << sb) - 1ULL;
    const uint64_t x[2] = {o >> 2, o & m1mask};                                  // prefix / suffix (k-1)-mer
    const int field[2] = {4 + (int)(o & 3ULL), (int)((o >> (2 * (k - 1))) & 3ULL)};      // o = x + b  /  o = b + x
    int n = 0;
    for (int i = 0; i < 2; i++) {
        const uint64_t u1 = x[i] >> 4, u2 = x[i] & smask;
        if (u1 <= sp_revcomp(u1, k - 3)) {       // x = u1 + e: side R
            out[n].t = (uint32_t)u1; out[n].side = 1u; out[n].e = (uint32_t)(x[i] & 15ULL); out[n].field = field[i];
            n++;
        }
        if (u2 <= sp_revcomp(u2, k - 3)) {       // x = e + u2: side L
            out[n].t = (uint32_t)u2; out[n].side = 0u; out[n].e = (uint32_t)(x[i] >> sb); out[n].field = field[i];
            n++;
        }
    }
    return n;
}

// ----------------------------------------------------------------- K5
// One block-iteration covers MAP_UNITS_PER_BLOCK units of 64 starts.  Hits are
// accumulated in an LDS histogram over the (few) output slots the range
// touches and flushed with one global atomic per non-zero entry.
#ifndef MAP_GRID_MULT
#define MAP_GRID_MULT 16
#endif
// the grid of every map walk, k <= 15 and k > 15: a workgroup per range of MAP_BLOCK units, MAP_GRID_MULT per compute unit at most
inline int64_t map_grid(const sp_ctx *ctx, int64_t n_ranges) {
    const int64_t cap = (int64_t)ctx->n_cu * MAP_GRID_MULT;
    return n_ranges < cap ? n_ranges : cap;
}
// ---- LDS of the two-phase walks over a unit (map_unit_scan64 in sp_map.hip, map_unit_scan64_h in sp_sparse.hip)
#ifndef MAP2_P2
#define MAP2_P2 1      // queue entries per lane and iteration of the candidate phase (2: 34.5 against 34.3 ms -- the wait is not per wave)
#endif
struct map_unit_lds {
    uint32_t *words;                 // [5 + 2 or 6 + 2][MAP_BLOCK]: the unit's packed words (LSB-first; the MSB-first twin is derived), then its countable starts
    unsigned long long *planes;      // [2 or 3][MAP_BLOCK]: the label planes of every thread's unit
    uint16_t *queue;                 // [MAP_BLOCK / 64][MAP_QCAP]: the wave's candidate quads
};
#ifndef MAP2_ROUND_W
#define MAP2_ROUND_W 2      // 16-start words of every lane per round of the two phases (compact table; 4 = the whole unit: one
                            // partly filled iteration fewer per unit, but the queue's LDS then allows three workgroups per CU, not four)
#endif
#define MAP_QCAP(TABLE) ((TABLE) ? 256 * MAP2_ROUND_W : 512)      // the whole unit / two of the four 16-start words of every lane per round
#define MAP_UNIT_LDS_DECL(TABLE, WORDS)                                                   \
    __shared__ uint32_t s_uw[(WORDS) * MAP_BLOCK];                                        \
    __shared__ unsigned long long s_up[((TABLE) ? 2 : 3) * MAP_BLOCK];                    \
    __shared__ uint16_t s_uq[(MAP_BLOCK / 64) * MAP_QCAP(TABLE)];                         \
    const map_unit_lds ulds = {s_uw, s_up, s_uq}

// ----------------------------------------------------------------- walkers and consumers
// A map kernel pairs a WALKER -- how a unit of 64 starts is answered from the label table -- with a CONSUMER -- what its walk
// mode does with the answer.  Two flavours of answer:
//   planes  walk(s0, lab, U, cm): three 64-bit label planes of the unit, bit j = the label bits of start s0 + j; only the starts
//           in `cm` are counted and marked "seen" (the two-phase walks: map_walk_pair in sp_map.hip, sps_walk_pair in sp_sparse.hip);
//   hits    walk.scan(s0, each): each(start, key) for every valid start that passes the filter, and walk.look(key, counted):
//           the subgenome of `key` or -1.  `counted` is asked at most once, and the k-mer is marked "seen" only where it
//           holds: a walker that can look before it marks asks it after the look-up, one whose look-up marks asks it first
//           (map_walk_bytes in sp_map.hip, sps_walk_kmer in sp_sparse.hip).
// Every consumer below exists once; everything is inlined into the twelve kernels.  Walkers and the bins accumulator hold
// the kernel's by-value arguments (k-mer parameters, table, map parameters) by reference: they never outlive its frame.
struct map_always {
    __device__ __forceinline__ bool operator()() const { return true; }
};

// ---- bins: counts[slot][sg] of one chromosome.  One accumulator per thread; a workgroup takes ranges of MAP_BLOCK units
// through begin() / end() (block-uniform calls: they hold barriers), a range's hits go to the LDS histogram over the few
// output slots it touches (P.use_lds: map_params_of) and from there to the table with one atomic per non-zero entry.
// (the histogram's pointer keeps its address space in its type: as a generic pointer the compiler merges the LDS atomic with
// the global one of the other branch into one flat atomic on a selected address)
typedef __attribute__((address_space(3))) int map_lds_int;
struct map_bins_acc {
    map_lds_int *hist;              // [MAP_LDS_ENTRIES]
    const sp_map_params &P;         // the kernel's argument: the accumulator lives inside one kernel's frame, as the walkers do
    int k;
    int *counts = nullptr;          // [nslots x S]: the table of the range's chromosome
    int64_t nslots = 0;
    int64_t slot_lo = 0;            // the range's first output slot
    bool one_slot = false;          // ... is its only one (uniform; found once per range, not per hit)
    unsigned long long mapped = 0;  // hits this thread has counted

    __device__ __forceinline__ map_bins_acc(int *hist_, const sp_map_params &P_, int k_) : hist((map_lds_int *)hist_), P(P_), k(k_) {}
    __device__ __forceinline__ void begin(int64_t r, int *counts_, int64_t nslots_) {
        counts = counts_;
        nslots = nslots_;
        slot_lo = map_slot(r * MAP_RANGE, P, k);
        one_slot = map_slot_end(r * MAP_RANGE, P, k) >= (r + 1) * MAP_RANGE;
        if (P.use_lds) {
            for (int i = threadIdx.x; i < MAP_LDS_ENTRIES; i += MAP_BLOCK) hist[i] = 0;
            __syncthreads();
        }
    }
    __device__ __forceinline__ void end() {
        if (P.use_lds) {
            __syncthreads();
            for (int i = threadIdx.x; i < MAP_LDS_ENTRIES; i += MAP_BLOCK) {
                int v = hist[i];
                if (v) {
                    int64_t os = slot_lo + i / P.S;
                    if (os < nslots) atomicAdd(&counts[os * P.S + (i % P.S)], v);
                }
            }
            __syncthreads();
        }
    }
    __device__ __forceinline__ void add(int64_t os, int sg, int v) {
        if (P.use_lds) atomicAdd((int *)&hist[(int)(os - slot_lo) * P.S + sg], v);
        else if (os < nslots) atomicAdd(&counts[os * P.S + sg], v);
        mapped += v;
    }
    // hits: every labelled start a hits walker finds in the unit at s0
    template <typename Walk>
    __device__ __forceinline__ void add_hits(const Walk &walk, int64_t s0) {
        walk.scan(s0, [&](int64_t start, auto key) {
            const int sg = walk.look(key, map_always());
            if (sg >= 0) add(map_slot(start, P, k), sg, 1);
        });
    }
    // the hits of the unit at s0 among the starts `within` -> slot os
    __device__ __forceinline__ void add_within(int64_t os, const unsigned long long lab[3], unsigned long long within) {
        for (int sg = 0; sg < P.S; sg++) {
            const int v = __popcll(map_plane_mask(lab, sg) & within);
            if (v) add(os, sg, v);
        }
    }
    __device__ __forceinline__ void add_planes(int64_t s0, const unsigned long long lab[3]) {
        if (!(lab[0] | lab[1] | lab[2])) return;
        if (one_slot) {
            add_within(slot_lo, lab, ~0ULL);
            return;
        }
        int64_t p = s0;
        while (p < s0 + SP_UNIT) {
            int64_t e = map_slot_end(p, P, k);
            if (e > s0 + SP_UNIT) e = s0 + SP_UNIT;
            const unsigned long long within = map_span(p - s0, e - s0);      // starts [p, e) of the unit
            if ((lab[0] | lab[1] | lab[2]) & within) add_within(map_slot(p, P, k), lab, within);
            p = e;
        }
    }
};

// the bins of ONE chromosome per launch (all but k5_map2): unit(s0) answers the unit at s0 into the accumulator
template <typename Unit>
__device__ __forceinline__ void map_bins_chrom(map_bins_acc &acc, unsigned long long *red /* [16], LDS */, int *counts,
                                               unsigned long long *n_mapped, Unit &&unit) {
    const int64_t n_ranges = (acc.P.n_units + MAP_BLOCK - 1) / MAP_BLOCK;
    for (int64_t r = blockIdx.x; r < n_ranges; r += gridDim.x) {
        const int64_t u = r * MAP_BLOCK + threadIdx.x;
        acc.begin(r, counts, acc.P.nslots);
        if (u < acc.P.n_units) unit(u * SP_UNIT);
        acc.end();
    }
    const unsigned long long t = sp_block_sum_u64(acc.mapped, red);
    if (threadIdx.x == 0 && t) atomicAdd(n_mapped, t);
}

// ---- features: counts[f][sg].  Planes, per unit: (1) the starts whose k-mer crosses no feature boundary (`fit`) -- only those
// are scanned, counted and marked "seen", exactly the k-mers a FASTA of the features holds; (2) the label planes of the unit;
// (3) one walk over the features that overlap the unit: popcounts of the planes inside the feature.
template <typename Walk>
__device__ __forceinline__ void map_feat_planes(const Walk &walk, const map_unit_lds &U, int k, int64_t n_units,
                                                const int64_t *__restrict__ foff, int64_t n_feat, int S,
                                                unsigned long long *__restrict__ counts) {
    int64_t u = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * MAP_BLOCK;
    for (; u < n_units; u += stride) {
        const int64_t s0 = u * SP_UNIT;
        int64_t lo;                            // the feature the unit starts in
        const unsigned long long fit = map_unit_fit(foff, n_feat, s0, k, lo);
        unsigned long long lab[3] = {0ULL, 0ULL, 0ULL};
        walk(s0, lab, U, fit);
        if (!(lab[0] | lab[1] | lab[2])) continue;
        // (3) (a start beyond the last feature's end is padding: never valid)
        for (int64_t f = lo; f < n_feat; f++) {
            const int64_t a = foff[f], e = foff[f + 1];
            if (a >= s0 + SP_UNIT) break;
            const unsigned long long within = map_span((a > s0 ? a : s0) - s0, (e < s0 + SP_UNIT ? e : s0 + SP_UNIT) - s0) & fit;
            if (!((lab[0] | lab[1] | lab[2]) & within)) continue;
            for (int sg = 0; sg < S; sg++) {
                const unsigned long long m = map_plane_mask(lab, sg) & within;
                if (m) atomicAdd(&counts[f * S + sg], (unsigned long long)__popcll(m));
            }
        }
    }
}
// hits: a cursor over the features, per unit; a start counts where the cursor finds its whole k-mer inside one feature
template <typename Walk>
__device__ __forceinline__ void map_feat_hits(const Walk &walk, int k, int64_t n_units, const int64_t *__restrict__ foff,
                                              int64_t n_feat, int S, unsigned long long *__restrict__ counts) {
    int64_t u = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * MAP_BLOCK;
    for (; u < n_units; u += stride) {
        map_feat_cursor cur;
        cur.f = -1;
        cur.next = 0;
        walk.scan(u * SP_UNIT, [&](int64_t start, auto key) {
            const int sg = walk.look(key, [&]() { return map_feat_locate(cur, start, k, foff, n_feat); });
            if (sg >= 0) atomicAdd(&counts[cur.f * S + sg], 1ULL);
        });
    }
}

// ---- intervals: masks[u][sg], bit j = the covered start 64 u + j carries a k-mer of subgenome sg (`cov`: kv_cover in
// sp_map.hip).  Planes: the label planes of a unit, restricted to the covered starts, ARE its masks.
template <typename Walk>
__device__ __forceinline__ void map_mask_planes(const Walk &walk, const map_unit_lds &U, int64_t n_units, int S,
                                                const unsigned long long *__restrict__ cov, unsigned long long *__restrict__ masks) {
    int64_t u = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * MAP_BLOCK;
    for (; u < n_units; u += stride) {
        const unsigned long long cv = cov[u];
        if (__all(cv == 0ULL)) continue;         // nothing of this wave's 4096 starts lies in a feature
        unsigned long long lab[3] = {0ULL, 0ULL, 0ULL};
        walk(u * SP_UNIT, lab, U, cv);
        for (int sg = 0; sg < S; sg++) masks[u * S + sg] = map_plane_mask(lab, sg) & cv;
    }
}
template <typename Walk>
__device__ __forceinline__ void map_mask_hits(const Walk &walk, int64_t n_units, int S, const unsigned long long *__restrict__ cov,
                                              unsigned long long *__restrict__ masks) {
    int64_t u = (int64_t)blockIdx.x * MAP_BLOCK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * MAP_BLOCK;
    for (; u < n_units; u += stride) {
        const unsigned long long cv = cov[u];
        if (__all(cv == 0ULL)) continue;
        walk.scan(u * SP_UNIT, [&](int64_t start, auto key) {
            const unsigned long long bit = 1ULL << (start & 63);
            if (!(cv & bit)) return;             // not covered: not looked up, so never marked
            const int sg = walk.look(key, map_always());
            if (sg >= 0) atomicOr(&masks[u * S + sg], bit);
        });
    }
}

// ---- host: the walker of a label-table kind, as a type.  Each file has ONE switch from ctx->labels.kind to these
// (map_with_walker in sp_map.hip, sps_with_walker in sp_sparse.hip); a mode's launcher is a generic lambda over them.
template <int TABLE>
struct map_planes_of {              // a two-phase walk; TABLE as in map_unit_scan64 / map_unit_scan64_h
    static constexpr bool planes = true;
    static constexpr int table = TABLE;
};
struct map_hits_of {                // map_pair_scan + a look-up per candidate start
    static constexpr bool planes = false;
};
