// sp_sparse.hip -- the k = 16..32 engine ("sparse": 64-bit keys, sorted (key, count) lists instead of dense
// tables; BASELINE.json config 5 sweeps k = 17 / 21), less its counting lanes (sp_sparse2.hip, same translation
// unit) and its filter (sp_listfilter.hip, a unit of its own, which k <= 15 list mode shares).  This file holds:
//
//   count  : engine 1 -- 64-bit scan -> canonical key per start position (sentinel where the window is broken)
//            -> radix sort -> run-length encode -> keep count >= lower_count   (per chromosome), and the dump
//   labels : labelled k-mers in an open-addressing hash table, the pair-keyed table and the quad-bucket table
//            (+ the L2-resident pre-filter)
//   map    : the k > 15 walkers (sps_walk_pair: map_unit_scan64_h; sps_walk_kmer: sps_lookup) and the six kernels that pair them
//            with the consumers of sp_map.h: k5_map_sparse2, k5_map_feat_sparse2, k5_map_mask_sparse2 (planes) and
//            k5_map_sparse_lab, k5_map_feat_sparse_lab, k5_map_mask_sparse_lab (hits); one dispatch (sps_with_walker)
//   lists  : the multi-GPU exports of the per-chromosome lists (sp_sparse_sizes / _sample / _split / _export / _view)
//
// The sort and the run-length encode are rocPRIM device primitives (plain library ops on this secondary path);
// everything specific to the problem is hand-written.
#include <algorithm>
#include <cstring>
#include <utility>
#include <rocprim/rocprim.hpp>

#include "sp_device.h"
#include "sp_internal.h"
#include "sp_lists.h"
#include "sp_map.h"

// ------------------------------------------------------------------ count
__global__ void __launch_bounds__(256)
sps_keygen(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, int64_t n_units, sp_kparams kp,
           unsigned long long *__restrict__ keys /* pre-filled with the sentinel */,
           unsigned long long *__restrict__ n_valid) {
    __shared__ unsigned long long red[16];
    unsigned long long nv = 0;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units;
         u += (int64_t)gridDim.x * blockDim.x) {
        sp_scan_unit64<SP_UNIT>(pk, nm, u * SP_UNIT, kp, [&](int64_t start, uint64_t fwd, uint64_t rc) {
            keys[start] = fwd < rc ? fwd : rc;
            nv++;
        });
    }
    unsigned long long t = sp_block_sum_u64(nv, red);
    if (threadIdx.x == 0 && t) atomicAdd(n_valid, t);
}

// runs with count >= lower: per-block tally (+ sum of those counts = `lengths`)
__global__ void __launch_bounds__(SEL_BLOCK)
sps_sel_count(const uint32_t *__restrict__ counts, int64_t n, uint32_t lower, unsigned long long *__restrict__ blk,
              unsigned long long *__restrict__ sum_out) {
    __shared__ unsigned long long red[16];
    const int64_t base = (int64_t)blockIdx.x * SEL_SPAN;
    unsigned long long c = 0, s = 0;
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        int64_t i = base + (int64_t)j * SEL_BLOCK + threadIdx.x;
        if (i < n && counts[i] >= lower) {
            c++;
            s += counts[i];
        }
    }
    unsigned long long tc = sp_block_sum_u64(c, red);
    unsigned long long ts = sp_block_sum_u64(s, red);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = tc;
        if (ts) atomicAdd(sum_out, ts);
    }
}

__global__ void __launch_bounds__(SEL_BLOCK)
sps_sel_write(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts, int64_t n,
              uint32_t lower, const unsigned long long *__restrict__ blk, unsigned long long *__restrict__ out_keys,
              uint32_t *__restrict__ out_counts) {
    __shared__ uint32_t lds[16];
    const int64_t base = (int64_t)blockIdx.x * SEL_SPAN;
    unsigned long long off = blk[blockIdx.x];
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        int64_t i = base + (int64_t)j * SEL_BLOCK + threadIdx.x;
        uint32_t c = (i < n) ? counts[i] : 0u;
        bool p = (i < n) && c >= lower;
        uint32_t tot;
        uint32_t my = sp_block_excl_count(p, lds, tot);
        if (p) {
            out_keys[off + my] = keys[i];
            out_counts[off + my] = c;
        }
        off += tot;
    }
}

// ------------------------------------------------------------------ labels + map
// Open-addressing table of 16-byte entries {key, label}: a hit costs ONE cache line (key and label
// used to live in two arrays = two L2 misses per mapped position).  label: 0 none, 1+sg, bit 7 = seen.
__global__ void __launch_bounds__(256)
sps_hash_insert(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ sg, int64_t n,
                unsigned long long *__restrict__ htab, uint64_t mask) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    uint64_t h = sps_mix(key) & mask;
    for (;;) {
        unsigned long long prev = atomicCAS(&htab[2 * h], SPS_SENTINEL, key);
        if (prev == SPS_SENTINEL || prev == key) break;
        h = (h + 1) & mask;
    }
    htab[2 * h + 1] = (unsigned long long)(1u + sg[i]);
}

__device__ __forceinline__ int sps_lookup(uint64_t key, unsigned long long *__restrict__ htab, uint64_t mask) {
    uint64_t h = sps_mix(key) & mask;
    for (;;) {
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(htab + 2 * h);
        if (e.x == key) {
            const uint32_t l = (uint32_t)e.y;
            if (!(l & 0x80u)) htab[2 * h + 1] = (unsigned long long)(l | 0x80u);   // idempotent "seen" mark
            return (int)(l & 0x7fu) - 1;
        }
        if (e.x == SPS_SENTINEL) return -1;
        h = (h + 1) & mask;
    }
}

// ------------------------------------------------------------------ pair-keyed label table (k > 15, <= 7 subgenomes)
// The k <= 15 pair table, hashed: an entry is keyed by the canonical (k-1)-mer x that two neighbouring starts share
// and its payload holds the same eight 4-bit fields (label of b + x and of x + b for the four bases b, seen flag in
// bit 3), so ONE 16-byte look-up answers BOTH starts of a candidate pair -- the per-k-mer table above costs one L2
// miss per candidate start, and those misses are what k5_map_sparse waits for.
struct sps_pair_loc {
    uint64_t idx;   // canonical (k-1)-mer
    int field;
};
__host__ __device__ __forceinline__ sps_pair_loc sps_loc_prefix(uint64_t o, int k) {     // o = x + b
    sps_pair_loc r;
    const uint32_t b = (uint32_t)(o & 3ULL);
    const uint64_t p = o >> 2, pc = sp_revcomp(p, k - 1);
    if (p <= pc) { r.idx = p; r.field = 4 + (int)b; }
    else { r.idx = pc; r.field = 3 - (int)b; }              // rc: comp(b) + rc(x)
    return r;
}
__host__ __device__ __forceinline__ sps_pair_loc sps_loc_suffix(uint64_t o, int k) {     // o = b + x
    sps_pair_loc r;
    const uint32_t b = (uint32_t)(o >> (2 * (k - 1))) & 3u;
    const uint64_t m1mask = (1ULL << (2 * (k - 1))) - 1ULL;
    const uint64_t x = o & m1mask, xc = sp_revcomp(x, k - 1);
    if (x <= xc) { r.idx = x; r.field = (int)b; }
    else { r.idx = xc; r.field = 7 - (int)b; }              // rc: rc(x) + comp(b)
    return r;
}
__global__ void __launch_bounds__(256)
sps_pair_init(unsigned long long *__restrict__ htab, int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
        htab[2 * i] = SPS_SENTINEL;
        htab[2 * i + 1] = 0ULL;
    }
}
__device__ __forceinline__ void sps_pair_put(unsigned long long *__restrict__ htab, uint64_t mask, sps_pair_loc a, uint32_t l) {
    uint64_t h = sps_mix(a.idx) & mask;
    for (;;) {
        const unsigned long long prev = atomicCAS(&htab[2 * h], SPS_SENTINEL, (unsigned long long)a.idx);
        if (prev == SPS_SENTINEL || prev == a.idx) break;
        h = (h + 1) & mask;
    }
    atomicOr(&htab[2 * h + 1], (unsigned long long)l << (4 * a.field));
}
__global__ void __launch_bounds__(256)
sps_pair_insert(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ sg, int64_t n, int k,
                unsigned long long *__restrict__ htab, uint64_t mask) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i], r = sp_revcomp(key, k);
    const uint32_t l = 1u + sg[i];
    sps_pair_put(htab, mask, sps_loc_prefix(key, k), l);
    sps_pair_put(htab, mask, sps_loc_suffix(key, k), l);
    sps_pair_put(htab, mask, sps_loc_prefix(r, k), l);      // (the same two entries and fields; kept for symmetry
    sps_pair_put(htab, mask, sps_loc_suffix(r, k), l);      //  with k4_pair_table: the OR is idempotent)
}
// entry of the canonical (k-1)-mer `x`: payload (0 when absent) and its slot
__device__ __forceinline__ uint32_t sps_pair_get(uint64_t x, const unsigned long long *__restrict__ htab, uint64_t mask,
                                                 uint64_t &slot) {
    uint64_t h = sps_mix(x) & mask;
    for (;;) {
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(htab + 2 * h);
        if (e.x == x) {
            slot = h;
            return (uint32_t)e.y;
        }
        if (e.x == SPS_SENTINEL) return 0u;
        h = (h + 1) & mask;
    }
}
__global__ void __launch_bounds__(256)
sps_pair_seen(const unsigned long long *__restrict__ keys, int64_t n, int k, const unsigned long long *__restrict__ htab,
              uint64_t mask, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i], r = sp_revcomp(key, k);
        const sps_pair_loc L[4] = {sps_loc_prefix(key, k), sps_loc_suffix(key, k), sps_loc_prefix(r, k), sps_loc_suffix(r, k)};
        uint32_t seen = 0;
        for (int q = 0; q < 4; q++) {
            uint64_t slot;
            seen |= (sps_pair_get(L[q].idx, htab, mask, slot) >> (4 * L[q].field)) & 8u;
        }
        c += seen ? 1 : 0;
    }
    unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

// The hits walker of k > 15 (sp_map.h), per-k-mer table (SP_LABELS_KMER_HASH: more than 7 subgenomes, or on demand --
// sp_labelplan.h): the rolling scan, one filter probe per pair of starts, one 16-byte look-up per candidate start.
// sps_lookup marks "seen" as it finds, so `counted` is asked before the look-up.  (`kp` refers to the kernel's argument:
// a walker lives inside one kernel's frame.)
struct sps_walk_kmer {
    const uint32_t *pk, *nm;
    const sp_kparams &kp;
    unsigned long long *htab;
    uint64_t mask;
    const uint32_t *bloom;
    int nbits;
    template <typename F>
    __device__ __forceinline__ void scan(int64_t s0, F &&each) const {
        map_pair_scan<uint64_t>(pk, nm, s0, kp, bloom, nbits,
                                [&](int64_t start, uint64_t fwd, uint64_t rc) { each(start, fwd < rc ? fwd : rc); });
    }
    template <typename C>
    __device__ __forceinline__ int look(uint64_t key, C &&counted) const {
        return counted() ? sps_lookup(key, htab, mask) : -1;
    }
};

// K5 for k > 15 on that walker: bins, then features and intervals.  (The pair-keyed tables take k5_map_sparse2 below; the
// unrolled pair kernel of rounds 1-4 -- 532 KB of machine code -- was removed in round 6.)
__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_sparse_lab(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, sp_kparams kp, sp_map_params P,
                  unsigned long long *__restrict__ htab, uint64_t mask,
                  const uint32_t *__restrict__ bloom, int bloom_bits, int *__restrict__ slot_counts,
                  unsigned long long *__restrict__ n_mapped) {
    __shared__ int hist[MAP_LDS_ENTRIES];
    __shared__ unsigned long long red[16];
    const sps_walk_kmer walk{pk, nm, kp, htab, mask, bloom, bloom_bits};
    map_bins_acc acc(hist, P, kp.k);
    map_bins_chrom(acc, red, slot_counts, n_mapped, [&](int64_t s0) { acc.add_hits(walk, s0); });
}
__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_feat_sparse_lab(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, sp_kparams kp, int64_t n_units,
                       const int64_t *__restrict__ foff, int64_t n_feat, int S,
                       unsigned long long *__restrict__ htab, uint64_t mask,
                       const uint32_t *__restrict__ bloom, int bloom_bits, unsigned long long *__restrict__ counts) {
    map_feat_hits(sps_walk_kmer{pk, nm, kp, htab, mask, bloom, bloom_bits}, kp.k, n_units, foff, n_feat, S, counts);
}
__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_mask_sparse_lab(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, sp_kparams kp, int64_t n_units, int S,
                       unsigned long long *__restrict__ htab, uint64_t mask, const uint32_t *__restrict__ bloom, int bloom_bits,
                       const unsigned long long *__restrict__ cov, unsigned long long *__restrict__ masks) {
    map_mask_hits(sps_walk_kmer{pk, nm, kp, htab, mask, bloom, bloom_bits}, n_units, S, cov, masks);
}

// ------------------------------------------------------------------ quad-bucket label table for k > 15 (round 6)
// The k <= 15 compact table (sp_map.h) with 64-bit entries: the two pairs of a QUAD of starts share the (k-3)-mer core t =
// last k-3 bases of x1 = first k-3 bases of x2, the table is addressed by the canonical core -- bucket = top bb bits of a
// bijective mix of t -- and ONE 32-byte bucket of four tagged entries answers all four starts, where the pair-keyed hash table
// above costs one 16-byte look-up per candidate PAIR (1.5 G against 0.96 G per wheat-like pass; the look-ups are what the
// kernel waits for).  An entry belongs to a (k-1)-mer y read in the orientation in which its core at one end is canonical:
// side 0 ("L") y = e + t, side 1 ("R") y = t + e, e = the two bases beyond t; it holds the labels of the eight k-mers b + y,
// y + b in THAT orientation (eight 3-bit fields: label 1..3, "seen" in the third bit).  Entry = tag << 25 | overflow flag << 24 |
// fields; tag = the tb = 2 (k - 3) - bb low bits of mix(t) << 5 | side << 4 | e: bucket + tag determine (t, side, e), a tag
// match is exact; tb + 5 <= 39 bits (else -- k = 31 / 32 with a small label set -- the hash table stays).  0 = empty.  A key
// that finds its bucket full goes to an open-addressing overflow table of {key id + 1, fields} pairs.  S <= 3.
#define SQ_FIELD 3
#define SQ_ANY 0x6DB6DBULL
#define SQ_PAYLOAD 0xFFFFFFULL
#define SQ_OVF (1ULL << 24)
// (SQ_TAG_BITS = 39: sp_labelplan.h, the sizing needs it)
struct sq_tab {
    unsigned long long *buckets;      // 4 entries (32 bytes) per bucket, or NULL: the pair-keyed hash table is in use
    unsigned long long *ovf;          // overflow table: {key id + 1, fields} pairs, 0 = empty
    uint64_t ovf_mask;                // its pairs - 1
    int sb, tb;                       // bits of the core 2 (k - 3); bits of mix(t) kept in the tag
};
__host__ __device__ __forceinline__ uint64_t sq_mix(uint64_t x, int kb) {      // a bijection of the kb-bit values (kb <= 58)
    const uint64_t m = (1ULL << kb) - 1ULL;
    x = (x * 0x9E3779B97F4A7C15ULL) & m;
    x ^= x >> ((kb + 1) / 2);
    x = (x * 0xD6E8FEB86659FD93ULL) & m;
    x ^= x >> ((kb + 1) / 2);
    return x;
}
struct sq_key {
    uint64_t bucket, tag, kid;
};
__host__ __device__ __forceinline__ sq_key sq_key_of(const sq_tab &T, uint64_t t, uint32_t side, uint32_t e) {
    const uint64_t h = sq_mix(t, T.sb);
    sq_key r;
    r.bucket = h >> T.tb;
    r.tag = ((h & ((1ULL << T.tb) - 1ULL)) << 5) | ((uint64_t)side << 4) | e;
    r.kid = (t << 5) | ((uint64_t)side << 4) | e;
    return r;
}
__device__ __forceinline__ void sq_insert(const sq_tab &T, const sq_key &q, uint64_t bits, unsigned long long *fail) {
    unsigned long long *e = T.buckets + 4 * q.bucket;
    const unsigned long long fresh = (q.tag << 25) | bits;
    for (int j = 0; j < 4; j++) {
        const int i = (int)((q.tag + (uint64_t)j) & 3ULL);      // (every key starts at the entry its own tag names)
        const unsigned long long old = atomicCAS(&e[i], 0ULL, fresh);
        if (old == 0ULL) return;
        if ((old >> 25) == q.tag && (old & SQ_PAYLOAD)) {
            atomicOr(&e[i], (unsigned long long)bits);
            return;
        }
    }
    atomicOr(&e[0], (unsigned long long)SQ_OVF);
    uint64_t i = (sps_mix(q.kid) >> 7) & T.ovf_mask;
    for (uint64_t probes = 0; probes <= T.ovf_mask; probes++) {
        const unsigned long long old = atomicCAS(&T.ovf[2 * i], 0ULL, (unsigned long long)(q.kid + 1ULL));
        if (old == 0ULL) atomicAdd(fail + 1, 1ULL);      // (statistics: keys in the overflow table)
        if (old == 0ULL || old == q.kid + 1ULL) {
            atomicOr(&T.ovf[2 * i + 1], (unsigned long long)bits);
            return;
        }
        i = (i + 1ULL) & T.ovf_mask;
    }
    atomicAdd(fail, 1ULL);      // the overflow table is full: the host falls back to the hash table
}
struct sq_hit {
    uint32_t fields, loc;             // loc: 4 * bucket + entry, or 0x80000000 | overflow pair: where the "seen" bits go
};
__device__ __forceinline__ sq_hit sq_find(const sq_tab &T, const ulonglong2 &B0, const ulonglong2 &B1, uint64_t bucket, uint64_t tag,
                                          uint64_t t, uint32_t side_e /* side << 4 | e */) {
    sq_hit r;
    const unsigned long long w[4] = {B0.x, B0.y, B1.x, B1.y};
    r.fields = 0;
    r.loc = (uint32_t)(4ULL * bucket);
#pragma unroll
    for (int i = 3; i >= 0; i--)
        if ((w[i] >> 25) == tag && (w[i] & SQ_PAYLOAD)) {
            r.fields = (uint32_t)(w[i] & SQ_PAYLOAD);
            r.loc = (uint32_t)(4ULL * bucket) + (uint32_t)i;
        }
    if (!r.fields && (B0.x & SQ_OVF)) {         // rare: the bucket overflowed and the key is in none of its entries
        const uint64_t kid = (t << 5) | side_e;
        uint64_t i = (sps_mix(kid) >> 7) & T.ovf_mask;
        for (uint64_t probes = 0; probes <= T.ovf_mask; probes++) {      // (bounded: a full table has no empty slot to stop at)
            const unsigned long long o = T.ovf[2 * i];
            if (o == 0ULL) break;
            if (o == kid + 1ULL) {
                r.fields = (uint32_t)(T.ovf[2 * i + 1] & SQ_PAYLOAD);
                r.loc = 0x80000000u | (uint32_t)i;
                break;
            }
            i = (i + 1ULL) & T.ovf_mask;
        }
    }
    return r;
}
__device__ __forceinline__ void sq_mark(const sq_tab &T, uint32_t loc, uint32_t bits) {
    if (loc & 0x80000000u) atomicOr(&T.ovf[2 * (size_t)(loc & 0x7fffffffu) + 1], (unsigned long long)bits);
    else atomicOr(&T.buckets[loc], (unsigned long long)bits);
}
// The (up to four) table keys under which the k-mer `o` (ONE orientation, as given) is entered / found: its prefix and its
// suffix (k-1)-mer, each under its first and its last (k-3)-mer -- but only where that core is canonical AS READ in this
// orientation; the other orientation of the k-mer supplies the rest (a palindromic core is entered from both).  k >= 16.
struct sq_site {
    uint64_t t;
    uint32_t side, e;
    int field;
};
__host__ __device__ __forceinline__ int sq_sites(uint64_t o, int k, sq_site out[4]) {
    const int sb = 2 * (k - 3);
    const uint64_t m1mask = (1ULL << (2 * (k - 1))) - 1ULL, smask = (1ULL << sb) - 1ULL;
    const uint64_t x[2] = {o >> 2, o & m1mask};                                          // prefix / suffix (k-1)-mer
    const int field[2] = {4 + (int)(o & 3ULL), (int)((o >> (2 * (k - 1))) & 3ULL)};      // o = x + b  /  o = b + x
    int n = 0;
    for (int i = 0; i < 2; i++) {
        const uint64_t u1 = x[i] >> 4, u2 = x[i] & smask;
        if (u1 <= sp_revcomp(u1, k - 3)) {       // x = u1 + e: side R
            out[n].t = u1; out[n].side = 1u; out[n].e = (uint32_t)(x[i] & 15ULL); out[n].field = field[i];
            n++;
        }
        if (u2 <= sp_revcomp(u2, k - 3)) {       // x = e + u2: side L
            out[n].t = u2; out[n].side = 0u; out[n].e = (uint32_t)(x[i] >> sb); out[n].field = field[i];
            n++;
        }
    }
    return n;
}
__global__ void __launch_bounds__(256)
sq_build(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ sg, int64_t n, int k, sq_tab T,
         unsigned long long *__restrict__ fail) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o2[2] = {keys[i], sp_revcomp(keys[i], k)};
    const uint64_t l = 1ULL + sg[i];
    for (int r = 0; r < 2; r++) {
        sq_site st[4];
        const int ns = sq_sites(o2[r], k, st);
        for (int j = 0; j < ns; j++) sq_insert(T, sq_key_of(T, st[j].t, st[j].side, st[j].e), l << (SQ_FIELD * st[j].field), fail);
    }
}
__global__ void __launch_bounds__(256)
sq_seen(const unsigned long long *__restrict__ keys, int64_t n, int k, sq_tab T, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t o2[2] = {keys[i], sp_revcomp(keys[i], k)};
        uint32_t seen = 0;
        for (int r = 0; r < 2; r++) {
            sq_site st[4];
            const int ns = sq_sites(o2[r], k, st);
            for (int j = 0; j < ns; j++) {
                const sq_key q = sq_key_of(T, st[j].t, st[j].side, st[j].e);
                const ulonglong2 *bp = reinterpret_cast<const ulonglong2 *>(T.buckets + 4 * q.bucket);
                seen |= (sq_find(T, bp[0], bp[1], q.bucket, q.tag, st[j].t, (st[j].side << 4) | st[j].e).fields >> (SQ_FIELD * st[j].field)) & 4u;
            }
        }
        c += seen ? 1 : 0;
    }
    const unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

// ------------------------------------------------------------------ k5_map_sparse2 (round 5)
// The pair kernel of rounds 1-4 was 532 KB of machine code -- the rolling scan unrolled over 95 bases with the hit path inlined
// at every start -- against 64 KB of instruction cache, and it kept ONE probe in flight per lane.  This is the k5_map2 walk
// (sp_map.hip) for 64-bit keys: the loop over the pairs of a unit stays rolled (32-base windows by run-time shifts out
// of three rotating registers per stream), two pairs travel together (their filter probes, then their table look-ups),
// a hit is a bit in three label planes and a unit's hits are settled once, by popcounts.  Pair-keyed table only
// (S <= 7); the per-k-mer table takes k5_map_sparse_lab above.  TABLE: 0 = the pair-keyed hash table (one look-up per candidate
// pair, S <= 7), 1 = the quad buckets above (one per candidate quad, S <= 3; `htab` / `hmask` unused).
// Round 6: two phases, as map_unit_scan64 (sp_map.hip): the filter leaves the wave's candidate quads in an LDS queue, the
// look-ups are dealt out to all lanes (a lane rebuilds the windows of the quad it was dealt from the owner's six packed words
// in LDS and ORs the labels it finds into the owner's planes).
struct map_pair_win {
    uint64_t xf, xr;       // the shared (k-1)-mer of a pair of starts, forward / reverse complement
    uint32_t b0, b1;       // the base in front of it / behind it
};
// the pair whose first start is base rr (0 .. 14) of the word la: the 32-base window lies in la, lb, lc
__device__ __forceinline__ map_pair_win map_pair_window(uint32_t la, uint32_t lb, uint32_t lc, uint32_t ma, uint32_t mb, uint32_t mc,
                                                        int rr, int k, int sh, uint64_t m1mask) {
    map_pair_win q;
    const uint64_t W = (uint64_t)__builtin_amdgcn_alignbit(lb, la, 2 * rr) | ((uint64_t)__builtin_amdgcn_alignbit(lc, lb, 2 * rr) << 32);
    const unsigned long long mA = ((unsigned long long)ma << 32) | mb, mB = ((unsigned long long)mb << 32) | mc;
    const uint64_t V = (((mA << (2 * rr)) >> 32) << 32) | ((mB << (2 * rr)) >> 32);
    q.b0 = (uint32_t)(V >> 62);            // the base in front of x (first base of the pair's first k-mer)
    q.xf = (V >> sh) & m1mask;             // x forward (the k-mer at the pair's first start without its first base)
    q.xr = (~W >> 2) & m1mask;             // its reverse complement
    // the base behind x (last base of the pair's second k-mer): position rr + k of the words, 16 <= k <= 32: in lb or lc
    const int pb = rr + k;
    q.b1 = (((pb >> 4) == 1 ? lb : lc) >> (2 * (pb & 15))) & 3u;
    return q;
}
template <int TABLE>
__device__ __forceinline__ void map_unit_scan64_h(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm,
                                                  const uint32_t *__restrict__ nm, int64_t s0, const sp_kparams &kp,
                                                  const uint32_t *__restrict__ bloom, int nbits,
                                                  unsigned long long *__restrict__ htab, uint64_t hmask, const sq_tab &T,
                                                  unsigned long long lab[3], const map_unit_lds &U,
                                                  unsigned long long cm = ~0ULL /* starts that count */) {
    constexpr int FW = TABLE ? SQ_FIELD : 4;
    constexpr uint32_t LBL = TABLE ? 3u : 7u, SEEN = TABLE ? 4u : 8u, FMASK = TABLE ? 7u : 15u;
    constexpr uint32_t ANY = TABLE ? (uint32_t)SQ_ANY : 0x77777777u;
    constexpr int NP = TABLE ? 2 : 3, ROUND_W = TABLE ? MAP2_ROUND_W : 2;
    unsigned long long ok_k, ok_x;      // k-mer at s0+j valid; shared (k-1)-mer at s0+j+1 valid
    {
        const uint64_t badA = sp_bad_starts64(nm, s0, kp.k - 1), badB = sp_bad_starts64(nm, s0 + 32, kp.k - 1);
        const uint64_t invA = (uint64_t)nm[s0 >> 5] | ((uint64_t)nm[(s0 >> 5) + 1] << 32);
        const uint64_t invB = (uint64_t)nm[(s0 >> 5) + 1] | ((uint64_t)nm[(s0 >> 5) + 2] << 32);
        const uint32_t kA = ~(uint32_t)(badA | (invA >> (kp.k - 1))), kB = ~(uint32_t)(badB | (invB >> (kp.k - 1)));
        const uint32_t xA = ~(uint32_t)(badA >> 1), xB = ~(uint32_t)(badB >> 1);
        ok_k = ((unsigned long long)kA | ((unsigned long long)kB << 32)) & cm;      // (not covered: neither counted nor marked seen)
        ok_x = (unsigned long long)xA | ((unsigned long long)xB << 32);
    }
    if (__all((ok_x & 0x5555555555555555ULL) == 0)) return;
    // the lanes of the wave that are here (a range's last wave, a grid-stride loop's last round): they share the candidates
    const unsigned long long here = __ballot(1);
    const int n_here = __popcll(here);
    const int me = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(here >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)here, 0u));
    const int tid = (int)threadIdx.x, lane = tid & 63, wave0 = tid & ~63;
    uint32_t *sw = U.words + tid;
    uint16_t *queue = U.queue + (tid >> 6) * MAP_QCAP(TABLE);
    const int64_t w0 = s0 >> 4;   // a multiple of 4: 16-byte aligned
    const uint4 la = *reinterpret_cast<const uint4 *>(pk + w0);
    uint32_t l0 = la.x, l1 = la.y, l2 = la.z, l3 = la.w, l4 = pk[w0 + 4], l5 = pk[w0 + 5];
#if SP_DERIVE_PM
    (void)pm;
    uint32_t m0 = sp_msb_of_lsb(l0), m1 = sp_msb_of_lsb(l1), m2 = sp_msb_of_lsb(l2), m3 = sp_msb_of_lsb(l3), m4 = sp_msb_of_lsb(l4),
             m5 = sp_msb_of_lsb(l5);
#else
    const uint4 ma = *reinterpret_cast<const uint4 *>(pm + w0);
    uint32_t m0 = ma.x, m1 = ma.y, m2 = ma.z, m3 = ma.w, m4 = pm[w0 + 4], m5 = pm[w0 + 5];
#endif
    sw[0 * MAP_BLOCK] = l0; sw[1 * MAP_BLOCK] = l1; sw[2 * MAP_BLOCK] = l2; sw[3 * MAP_BLOCK] = l3; sw[4 * MAP_BLOCK] = l4; sw[5 * MAP_BLOCK] = l5;
    sw[6 * MAP_BLOCK] = (uint32_t)ok_k; sw[7 * MAP_BLOCK] = (uint32_t)(ok_k >> 32);
#pragma unroll
    for (int bit = 0; bit < NP; bit++) U.planes[bit * MAP_BLOCK + tid] = 0ULL;
    const int sh = 64 - 2 * kp.k;
    const uint64_t m1mask = kp.kmask >> 2;
    const bool core = (nbits & MAP_BLOOM_CORE) != 0;                   // (uniform; k >= 16 here)
    const uint64_t cmask = (1ULL << (2 * (kp.k - 3))) - 1ULL;
    const int wsh = 32 - (MAP_BLOOM_NBITS(nbits) - 5);
    uint32_t last_wi = 0xFFFFFFFFu, last_w = 0u;                       // the word this lane fetched last (index, content)
    uint32_t h_carry = 0u;                                              // hash of the core the previous two pairs ended with
#pragma unroll 1
    for (int wr = 0; wr < 4; wr += ROUND_W) {
        // ---- phase 1: the filter over ROUND_W words of sixteen starts
        uint32_t qn = 0;                                                // (uniform)
#pragma unroll 1
        for (int w = wr; w < wr + ROUND_W; w++) {
#pragma unroll 1
            for (int r = 0; r < 16; r += 4) {
                const int j = 16 * w + r;           // two pairs: x1 at j + 1 (starts j, j + 1), x2 at j + 3 (starts j + 2, j + 3)
                const map_pair_win A = map_pair_window(l0, l1, l2, m0, m1, m2, r, kp.k, sh, m1mask);
                const map_pair_win B = map_pair_window(l0, l1, l2, m0, m1, m2, r + 2, kp.k, sh, m1mask);
                uint32_t hx1, hx2;
                const uint32_t bt1 = map_bloom_bits3(A.xf < A.xr ? A.xf : A.xr, hx1), bt2 = map_bloom_bits3(B.xf < B.xr ? B.xf : B.xr, hx2);
                // the filter words of x1 and x2 (sp_map.h): by the smaller-hashed core of the chain a - x1 - b - x2 - c, or by
                // the (k-1)-mer itself; a word the lane fetched for the previous pair is not fetched again
                uint32_t wi1, wi2;
                if (core) {
                    const uint64_t tb_f = A.xf & cmask, tb_r = A.xr >> 4, tc_f = B.xf & cmask, tc_r = B.xr >> 4;
                    uint32_t ha = h_carry;              // (this iteration's a IS the previous one's c: the same bases)
                    if (j == 0) {                       // (uniform: the unit's first two pairs)
                        const uint64_t ta_f = A.xf >> 4, ta_r = A.xr & cmask;
                        ha = map_core_hash(ta_f < ta_r ? ta_f : ta_r);
                    }
                    const uint32_t hb = map_core_hash(tb_f < tb_r ? tb_f : tb_r), hc = map_core_hash(tc_f < tc_r ? tc_f : tc_r);
                    h_carry = hc;
                    wi1 = map_core_word(ha < hb ? ha : hb, nbits);
                    wi2 = map_core_word(hb < hc ? hb : hc, nbits);
                } else {
                    wi1 = hx1 >> wsh;
                    wi2 = hx2 >> wsh;
                }
                const bool v1 = (ok_x >> j) & 1ULL, v2 = (ok_x >> (j + 2)) & 1ULL;
                const bool need1 = v1 && wi1 != last_wi;
                const bool need2 = v2 && wi2 != (v1 ? wi1 : last_wi);
                uint32_t f1 = 0, f2 = 0;
                if (need1) f1 = bloom[wi1];
                if (need2) f2 = bloom[wi2];
                const uint32_t wd1 = v1 ? (need1 ? f1 : last_w) : 0u;
                const uint32_t wd2 = v2 ? (need2 ? f2 : (v1 ? wd1 : last_w)) : 0u;
                if (v2) { last_wi = wi2; last_w = wd2; }
                else if (v1) { last_wi = wi1; last_w = wd1; }
                const bool cand1 = (wd1 & bt1) == bt1, cand2 = (wd2 & bt2) == bt2;      // (an invalid pair's word is 0)
                const unsigned long long bal = __ballot(cand1 || cand2);
                if (cand1 || cand2)
                    queue[qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] =
                        (uint16_t)((uint32_t)lane | ((uint32_t)(j >> 2) << 6) | (cand1 ? 0x400u : 0u) | (cand2 ? 0x800u : 0u));
                qn += (uint32_t)__popcll(bal);
            }
            l0 = l1; l1 = l2; l2 = l3; l3 = l4; l4 = l5;
            m0 = m1; m1 = m2; m2 = m3; m3 = m4; m4 = m5;
        }
        // ---- phase 2: the queue, dealt out to the lanes that are here (LDS operations of a wave complete in program order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t e0 = (uint32_t)me; e0 < qn; e0 += (uint32_t)n_here) {
            const uint32_t ent = queue[e0];
            const int owner = wave0 + (int)(ent & 63u), qi = (int)((ent >> 6) & 15u), j = 4 * qi, w = qi >> 2, r = j & 15;
            const bool cand[2] = {(ent & 0x400u) != 0u, (ent & 0x800u) != 0u};
            const uint32_t *ow = U.words + owner;
            const uint32_t oa = ow[w * MAP_BLOCK], ob = ow[(w + 1) * MAP_BLOCK], oc = ow[(w + 2) * MAP_BLOCK];
            const uint32_t okq = ow[(6 + (w >> 1)) * MAP_BLOCK] >> (j & 31);       // countable starts j .. j + 3 of the owner's unit
            const uint32_t pa = sp_msb_of_lsb(oa), pb_ = sp_msb_of_lsb(ob), pc = sp_msb_of_lsb(oc);
            const map_pair_win Pw[2] = {map_pair_window(oa, ob, oc, pa, pb_, pc, r, kp.k, sh, m1mask),
                                        map_pair_window(oa, ob, oc, pa, pb_, pc, r + 2, kp.k, sh, m1mask)};
            uint32_t e[2] = {0u, 0u};
            uint32_t loc[2] = {0u, 0u};                               // TABLE: where a hit's "seen" bits go (sq_mark)
            uint64_t slot[2] = {0, 0};                                // hash table: the pair's slot
            bool fwd_[2] = {Pw[0].xf <= Pw[0].xr, Pw[1].xf <= Pw[1].xr};          // orientation the fields are laid out in
            if (TABLE) {
                // the core the two pairs share: last k-3 bases of x1 = first k-3 bases of x2 (a candidate's (k-1)-mer is valid, so it is)
                const uint64_t s_f = cand[0] ? (Pw[0].xf & cmask) : (Pw[1].xf >> 4), s_r = cand[0] ? (Pw[0].xr >> 4) : (Pw[1].xr & cmask);
                const bool sfw = s_f <= s_r;
                const uint64_t t = sfw ? s_f : s_r;
                const uint64_t hm = sq_mix(t, T.sb);
                const uint64_t bucket = hm >> T.tb, tagb = (hm & ((1ULL << T.tb) - 1ULL)) << 5;
                // x1 = e + s: side L read forward, side R (e reverse-complemented) read backward; x2 = s + e: the mirror image
                const uint32_t se1 = (sfw ? 0u : 16u) | (uint32_t)(sfw ? (Pw[0].xf >> T.sb) : (Pw[0].xr & 15ULL));
                const uint32_t se2 = (sfw ? 16u : 0u) | (uint32_t)(sfw ? (Pw[1].xf & 15ULL) : (Pw[1].xr >> T.sb));
                const ulonglong2 *bp = reinterpret_cast<const ulonglong2 *>(T.buckets + 4 * bucket);
                const ulonglong2 B0 = bp[0], B1 = bp[1];
                if (cand[0]) {
                    const sq_hit hh = sq_find(T, B0, B1, bucket, tagb | se1, t, se1);
                    e[0] = hh.fields;
                    loc[0] = hh.loc;
                }
                if (cand[1]) {
                    const sq_hit hh = sq_find(T, B0, B1, bucket, tagb | se2, t, se2);
                    e[1] = hh.fields;
                    loc[1] = hh.loc;
                }
                fwd_[0] = fwd_[1] = sfw;      // the fields are laid out in the orientation in which t is canonical
            } else {
#pragma unroll
                for (int h = 0; h < 2; h++)
                    if (cand[h]) e[h] = sps_pair_get(Pw[h].xf < Pw[h].xr ? Pw[h].xf : Pw[h].xr, htab, hmask, slot[h]);
            }
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (!(e[h] & ANY)) continue;
                const bool fw = fwd_[h];
                const int f0 = fw ? (int)Pw[h].b0 : 7 - (int)Pw[h].b0, f1 = fw ? 4 + (int)Pw[h].b1 : 3 - (int)Pw[h].b1;
                const uint32_t okk = okq >> (2 * h);
                const uint32_t v0 = (okk & 1u) ? (e[h] >> (FW * f0)) & FMASK : 0u;
                const uint32_t v1 = (okk & 2u) ? (e[h] >> (FW * f1)) & FMASK : 0u;
                const uint32_t two = (v0 & LBL) | ((v1 & LBL) << 8);
                if (!two) continue;
#pragma unroll
                for (int bit = 0; bit < NP; bit++) {
                    const unsigned long long b2 = (unsigned long long)(((two >> bit) & 1u) | (((two >> (8 + bit)) & 1u) << 1));
                    if (b2) atomicOr(&U.planes[bit * MAP_BLOCK + owner], b2 << (j + 2 * h));
                }
                uint32_t mark = 0;       // "seen": first touch only
                if ((v0 & LBL) && !(v0 & SEEN)) mark |= SEEN << (FW * f0);
                if ((v1 & LBL) && !(v1 & SEEN)) mark |= SEEN << (FW * f1);
                if (mark) {
                    if (TABLE) sq_mark(T, loc[h], mark);
                    else atomicOr(&htab[2 * slot[h] + 1], (unsigned long long)mark);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#pragma unroll
    for (int bit = 0; bit < NP; bit++) lab[bit] = U.planes[bit * MAP_BLOCK + tid];
}

// the planes walker of k > 15 (sp_map.h): the two-phase walk over the pair-keyed hash table (TABLE 0) or the quad buckets (1)
// (`kp` and `T` refer to the kernel's arguments: a walker lives inside one kernel's frame)
template <int TABLE>
struct sps_walk_pair {
    const uint32_t *pk, *pm, *nm;
    const sp_kparams &kp;
    unsigned long long *htab;
    uint64_t hmask;
    const sq_tab &T;
    const uint32_t *bloom;
    int nbits;
    __device__ __forceinline__ void operator()(int64_t s0, unsigned long long lab[3], const map_unit_lds &U,
                                               unsigned long long cm = ~0ULL) const {
        map_unit_scan64_h<TABLE>(pk, pm, nm, s0, kp, bloom, nbits, htab, hmask, T, lab, U, cm);
    }
};

// (the bound: six waves per SIMD, that is three workgroups of MAP_BLOCK = 512 threads per CU, leave a wave 80 VGPRs, and the
// walk needs every one of them.  What a register too many costs was measured in round 6, with workgroups of 768: at 82 VGPRs
// the kernel ran one workgroup per CU instead of two, 52.6 -> 66.6 ms)
template <int TABLE>
__global__ void __launch_bounds__(MAP_BLOCK, 6)
k5_map_sparse2(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, sp_kparams kp,
               sp_map_params P, unsigned long long *__restrict__ htab, uint64_t hmask, sq_tab T, const uint32_t *__restrict__ bloom,
               int bloom_bits, int *__restrict__ slot_counts, unsigned long long *__restrict__ n_mapped) {
    __shared__ int hist[MAP_LDS_ENTRIES];
    __shared__ unsigned long long red[16];
    MAP_UNIT_LDS_DECL(TABLE, 8);
    const sps_walk_pair<TABLE> walk{pk, pm, nm, kp, htab, hmask, T, bloom, bloom_bits};
    map_bins_acc acc(hist, P, kp.k);
    map_bins_chrom(acc, red, slot_counts, n_mapped, [&](int64_t s0) {
        unsigned long long lab[3] = {0ULL, 0ULL, 0ULL};
        walk(s0, lab, ulds);
        acc.add_planes(s0, lab);
    });
}
// feature mode and interval mode on the same walker (the consumers: sp_map.h)
template <int TABLE>
__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_feat_sparse2(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, sp_kparams kp,
                    int64_t n_units, const int64_t *__restrict__ foff, int64_t n_feat, int S,
                    unsigned long long *__restrict__ htab, uint64_t hmask, sq_tab T,
                    const uint32_t *__restrict__ bloom, int bloom_bits, unsigned long long *__restrict__ counts) {
    MAP_UNIT_LDS_DECL(TABLE, 8);
    map_feat_planes(sps_walk_pair<TABLE>{pk, pm, nm, kp, htab, hmask, T, bloom, bloom_bits}, ulds, kp.k, n_units, foff, n_feat, S,
                    counts);
}
template <int TABLE>
__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_mask_sparse2(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, sp_kparams kp,
                    int64_t n_units, int S, unsigned long long *__restrict__ htab, uint64_t hmask, sq_tab T, const uint32_t *__restrict__ bloom,
                    int bloom_bits, const unsigned long long *__restrict__ cov, unsigned long long *__restrict__ masks) {
    MAP_UNIT_LDS_DECL(TABLE, 8);
    map_mask_planes(sps_walk_pair<TABLE>{pk, pm, nm, kp, htab, hmask, T, bloom, bloom_bits}, ulds, n_units, S, cov, masks);
}

__global__ void __launch_bounds__(256)
sps_count_seen(const unsigned long long *__restrict__ htab, int64_t n, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        c += (htab[2 * i] != SPS_SENTINEL) ? ((htab[2 * i + 1] >> 7) & 1u) : 0u;   // empty entries are all ones
    unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

// ================================================================== host side
static void sps_free_chrom(sp_sparse_chrom &c) {
    if (c.d_keys) hipFree(c.d_keys);
    if (c.d_cnts) hipFree(c.d_cnts);
    c = sp_sparse_chrom();
}

void sp_sparse_release(sp_ctx *ctx) {
    for (auto &c : ctx->sparse) sps_free_chrom(c);
    ctx->sparse.clear();
    if (ctx->d_hkeys) hipFree(ctx->d_hkeys);
    ctx->d_hkeys = nullptr;
    ctx->hcap = 0;
    sp_buf_free(ctx->b_sp_a);
    sp_buf_free(ctx->b_sp_b);
    sp_buf_free(ctx->b_sp_c);
    sp_buf_free(ctx->b_sp_tmp);
    sp_buf_free(ctx->b_s3_small);
    for (auto &ln : ctx->lanes) {       // the k > 15 counting lanes' workspaces (sp_sparse2.hip)
        sp_buf_free(ln.b_sp_a);
        sp_buf_free(ln.b_sp_b);
        sp_buf_free(ln.b_sp_c);
        sp_buf_free(ln.b_sp_tmp);
        sp_buf_free(ln.b_s3_small);
    }
    sp_buf_free(ctx->b_sf_keys);
    sp_buf_free(ctx->b_sf_counts);
    sp_buf_free(ctx->b_sf_tot);
    sp_buf_free(ctx->b_sf_hist);
}

static int sps_ordered_select(sp_ctx *ctx, const unsigned long long *d_keys, const uint32_t *d_counts, int64_t n,
                              uint32_t lower, sp_sparse_chrom &out, unsigned long long *d_small /*>= 4 u64*/) {
    // d_small[0] = sum of kept counts, d_small[1] = kept runs
    const int64_t nblk = (n + SEL_SPAN - 1) / SEL_SPAN;
    int rc = sp_buf_ensure(ctx, ctx->b_sp_tmp, (nblk + 2) * 8);
    if (rc) return rc;
    unsigned long long *d_blk = (unsigned long long *)ctx->b_sp_tmp.p;
    SP_HIP(ctx, hipMemsetAsync(d_small, 0, 32, ctx->stream));
    if (n == 0) {
        out.n = 0;
        return SP_OK;
    }
    SP_LAUNCH(ctx, "sps_sel_count", sps_sel_count, dim3((unsigned)nblk), dim3(SEL_BLOCK), 0, d_counts, n, lower, d_blk,
              d_small);
    SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, d_blk, nblk, d_small + 1);
    unsigned long long h[2] = {0, 0};
    SP_HIP(ctx, hipMemcpyAsync(h, d_small, 16, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t keep = (int64_t)h[1];
    if (keep > out.cap) {
        if (out.d_keys) hipFree(out.d_keys);
        if (out.d_cnts) hipFree(out.d_cnts);
        out.d_keys = nullptr;
        out.d_cnts = nullptr;
        out.cap = 0;
        SP_HIP(ctx, hipMalloc(&out.d_keys, (size_t)(keep + 1) * 8));
        SP_HIP(ctx, hipMalloc(&out.d_cnts, (size_t)(keep + 1) * 4));
        out.cap = keep;
    }
    out.n = keep;
    out.length_sum = (int64_t)h[0];
    if (keep)
        SP_LAUNCH(ctx, "sps_sel_write", sps_sel_write, dim3((unsigned)nblk), dim3(SEL_BLOCK), 0, d_keys, d_counts, n,
                  lower, d_blk, (unsigned long long *)out.d_keys, out.d_cnts);
    return SP_OK;
}

int sp_sparse_count(sp_ctx *ctx, int k, int lower) {
    const size_t C = ctx->chroms.size();
    if (ctx->sparse.size() != C) {
        for (auto &c : ctx->sparse) sps_free_chrom(c);
        ctx->sparse.assign(C, sp_sparse_chrom());
    }
    const sp_kparams kp = sp_make_kparams(k);
    const unsigned end_bit = (2 * k + 1 > 64) ? 64u : (unsigned)(2 * k + 1);
    void *scr = nullptr;
    int rc = sp_scratch(ctx, 256, &scr);
    if (rc) return rc;
    unsigned long long *d_small = (unsigned long long *)scr;
    for (size_t ci = 0; ci < C; ci++) {
        sp_chrom &c = ctx->chroms[ci];
        sp_sparse_chrom &o = ctx->sparse[ci];
        const int64_t n = c.len;
        o.n = 0;
        o.length_sum = 0;
        c.length_sum = 0;
        c.n_dump = 0;
        if (n <= 0) continue;
        rc = sp_buf_ensure(ctx, ctx->b_sp_a, n * 8);
        if (rc) return rc;
        rc = sp_buf_ensure(ctx, ctx->b_sp_b, n * 8);
        if (rc) return rc;
        rc = sp_buf_ensure(ctx, ctx->b_sp_c, n * 4 + 64);
        if (rc) return rc;
        unsigned long long *A = (unsigned long long *)ctx->b_sp_a.p, *B = (unsigned long long *)ctx->b_sp_b.p;
        uint32_t *Cn = (uint32_t *)ctx->b_sp_c.p;
        SP_HIP(ctx, hipMemsetAsync(A, 0xff, (size_t)n * 8, ctx->stream));
        SP_HIP(ctx, hipMemsetAsync(d_small, 0, 64, ctx->stream));
        const int64_t n_units = (n + SP_UNIT - 1) / SP_UNIT;
        int64_t grid = (n_units + 255) / 256;
        if (grid > (int64_t)ctx->n_cu * 16) grid = (int64_t)ctx->n_cu * 16;
        SP_LAUNCH(ctx, "sps_keygen", sps_keygen, dim3((unsigned)grid), dim3(256), 0, c.d_pk, c.d_nm, n_units, kp, A,
                  d_small + 4);
        unsigned long long nv = 0;
        SP_HIP(ctx, hipMemcpyAsync(&nv, d_small + 4, 8, hipMemcpyDeviceToHost, ctx->stream));
        // sort (sentinels, having bit 2k set, end up last)
        size_t tmp_bytes = 0;
        SP_HIP(ctx, rocprim::radix_sort_keys(nullptr, tmp_bytes, A, B, (size_t)n, 0u, end_bit, ctx->stream));
        rc = sp_buf_ensure(ctx, ctx->b_sp_tmp, (int64_t)tmp_bytes + 256);
        if (rc) return rc;
        SP_HIP(ctx, rocprim::radix_sort_keys(ctx->b_sp_tmp.p, tmp_bytes, A, B, (size_t)n, 0u, end_bit, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (nv == 0) continue;
        if (nv >= (1ULL << 32)) return sp_fail(ctx, SP_EUNSUP, "k > 15: chromosomes of 2^32 or more k-mers are not supported");
        // run-length encode the valid prefix: unique keys -> A, counts -> Cn, number of runs -> d_small[5]
        tmp_bytes = 0;
        SP_HIP(ctx, rocprim::run_length_encode(nullptr, tmp_bytes, B, (unsigned int)nv, A, Cn, d_small + 5, ctx->stream));
        rc = sp_buf_ensure(ctx, ctx->b_sp_tmp, (int64_t)tmp_bytes + 256);
        if (rc) return rc;
        SP_HIP(ctx, rocprim::run_length_encode(ctx->b_sp_tmp.p, tmp_bytes, B, (unsigned int)nv, A, Cn, d_small + 5,
                                               ctx->stream));
        unsigned long long nruns = 0;
        SP_HIP(ctx, hipMemcpyAsync(&nruns, d_small + 5, 8, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        rc = sps_ordered_select(ctx, A, Cn, (int64_t)nruns, (uint32_t)lower, o, d_small);
        if (rc) return rc;
        c.length_sum = o.length_sum;
        c.n_dump = o.n;
    }
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_sparse_dump(sp_ctx *ctx, int chrom, uint64_t *keys, uint32_t *counts) {
    sp_sparse_chrom &o = ctx->sparse[(size_t)chrom];
    if (o.n == 0) return SP_OK;
    SP_HIP(ctx, hipMemcpyAsync(keys, o.d_keys, (size_t)o.n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(counts, o.d_cnts, (size_t)o.n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->list_mode) {
        // engine 3 keeps dense SLOTS (ascending); a dump is canonical k-mers in ascending order: convert and sort
        // here, on the host -- the dump is the compatibility export (jellyfish-format files, tests), not the hot path
        const sp_kparams kp = sp_make_kparams(ctx->k);
        try {
            std::vector<std::pair<uint64_t, uint32_t>> v((size_t)o.n);
            for (int64_t i = 0; i < o.n; i++) v[(size_t)i] = {sp_key_of_slot(keys[i], kp), counts[i]};
            std::sort(v.begin(), v.end());
            for (int64_t i = 0; i < o.n; i++) {
                keys[i] = v[(size_t)i].first;
                counts[i] = v[(size_t)i].second;
            }
        } catch (const std::bad_alloc &) {
            return sp_fail(ctx, SP_ENOMEM, "sp_dump: out of host memory sorting %lld k-mers", (long long)o.n);
        }
    }
    return SP_OK;
}


// the quad-bucket table the current k > 15 label set lives in (buckets = NULL: the pair-keyed / per-k-mer hash table)
static sq_tab sq_tab_of(const sp_ctx *ctx) {
    const bool quad = ctx->labels.kind == SP_LABELS_QUAD;
    sq_tab T;
    T.buckets = quad ? (unsigned long long *)ctx->b_ctab.p : nullptr;
    T.ovf = (unsigned long long *)ctx->b_covf.p;
    T.ovf_mask = ctx->labels.ovf_mask;
    T.sb = 2 * (ctx->k - 3);
    T.tb = quad ? T.sb - ctx->labels.bb : 0;
    return T;
}

// the hash table of the k > 15 kinds: `cap` 16-byte entries (1024 unused ones beside the quad-bucket table: every map
// kernel takes the pointer)
static int sps_hash_ensure(sp_ctx *ctx, int64_t cap) {
    if (cap == ctx->hcap) return SP_OK;
    if (ctx->d_hkeys) hipFree(ctx->d_hkeys);
    ctx->d_hkeys = nullptr;
    ctx->hcap = 0;
    SP_HIP(ctx, hipMalloc(&ctx->d_hkeys, (size_t)cap * 16));
    ctx->hcap = cap;
    return SP_OK;
}

// sp_labels_set at k > 15 (the driver: sp_map.hip): the planned table, already the context's label state, from the staged keys
int sp_sparse_labels_build(sp_ctx *ctx, const sp_label_plan &plan, const unsigned long long *d_keys, const uint8_t *d_sg,
                           int64_t n, unsigned long long *d_flags) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    int rc = sps_hash_ensure(ctx, plan.cap);
    if (rc) return rc;
    unsigned long long *htab = (unsigned long long *)ctx->d_hkeys;
    switch (plan.kind) {
    case SP_LABELS_QUAD:
        if ((rc = sp_buf_ensure(ctx, ctx->b_ctab, plan.bucket_bytes))) return rc;
        if ((rc = sp_buf_ensure(ctx, ctx->b_covf, plan.ovf_bytes))) return rc;
        SP_HIP(ctx, hipMemsetAsync(ctx->b_ctab.p, 0, (size_t)plan.bucket_bytes, ctx->stream));
        SP_HIP(ctx, hipMemsetAsync(ctx->b_covf.p, 0, (size_t)plan.ovf_bytes, ctx->stream));
        if (n > 0)      // d_flags[2] = overflow table full, [3] = keys in the overflow table
            SP_LAUNCH(ctx, "sq_build", sq_build, dim3(grid), dim3(256), 0, d_keys, d_sg, n, ctx->k, sq_tab_of(ctx), d_flags + 2);
        return SP_OK;
    case SP_LABELS_PAIR_HASH:
        SP_LAUNCH(ctx, "sps_pair_init", sps_pair_init, dim3((unsigned)(ctx->n_cu * 8)), dim3(256), 0, htab, plan.cap);
        if (n > 0)
            SP_LAUNCH(ctx, "sps_pair_insert", sps_pair_insert, dim3(grid), dim3(256), 0, d_keys, d_sg, n, ctx->k, htab,
                      (uint64_t)(plan.cap - 1));
        return SP_OK;
    default:      // SP_LABELS_KMER_HASH
        // {key = sentinel (all ones), label = 0}: 0xff everywhere, then the label words are written on insert
        // and read only after a key match, so they need no clearing
        SP_HIP(ctx, hipMemsetAsync(htab, 0xff, (size_t)plan.cap * 16, ctx->stream));
        if (n > 0)
            SP_LAUNCH(ctx, "sps_hash_insert", sps_hash_insert, dim3(grid), dim3(256), 0, d_keys, d_sg, n, htab,
                      (uint64_t)(plan.cap - 1));
        return SP_OK;
    }
}

// The ONE place that turns the kind of a k > 15 label table into its walker (sp_map.h): `launch` is a mode's launcher, a
// generic lambda over the walker that is also handed the hash table every k > 15 kernel takes.
template <typename F>
static int sps_with_walker(sp_ctx *ctx, F &&launch) {
    unsigned long long *htab = (unsigned long long *)ctx->d_hkeys;
    const uint64_t hmask = (uint64_t)(ctx->hcap - 1);
    switch (ctx->labels.kind) {
    case SP_LABELS_QUAD: return launch(map_planes_of<1>{}, htab, hmask);
    case SP_LABELS_PAIR_HASH: return launch(map_planes_of<0>{}, htab, hmask);
    default: return launch(map_hits_of{}, htab, hmask);      // SP_LABELS_KMER_HASH
    }
}

// the k > 15 halves of the three mode launchers of sp_map.hip.  Bins: one launch per chromosome.
int sp_sparse_map_launch(sp_ctx *ctx, sp_chrom &c, const sp_map_params &P, int *d_counts, unsigned long long *d_n) {
    if (P.n_units == 0) return SP_OK;
    const sp_kparams kp = sp_make_kparams(ctx->k);
    const int64_t grid = map_grid(ctx, (P.n_units + MAP_BLOCK - 1) / MAP_BLOCK);
    return sps_with_walker(ctx, [&](auto w, unsigned long long *htab, uint64_t hmask) -> int {
        if constexpr (decltype(w)::planes)
            SP_LAUNCH(ctx, "k5_map_sparse", k5_map_sparse2<decltype(w)::table>, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, c.d_pk, c.d_pm,
                      c.d_nm, kp, P, htab, hmask, sq_tab_of(ctx), ctx->d_bloom, ctx->bloom_bits, d_counts, d_n);
        else
            SP_LAUNCH(ctx, "k5_map_sparse_lab", k5_map_sparse_lab, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, c.d_pk, c.d_nm, kp, P,
                      htab, hmask, ctx->d_bloom, ctx->bloom_bits, d_counts, d_n);
        return SP_OK;
    });
}

int sp_sparse_feat_launch(sp_ctx *ctx, const uint32_t *d_pk, const uint32_t *d_pm, const uint32_t *d_nm, int64_t n_units,
                          const int64_t *d_foff, int64_t n_feat, int S, unsigned long long *d_counts) {
    const sp_kparams kp = sp_make_kparams(ctx->k);
    const int64_t grid = map_grid(ctx, (n_units + MAP_BLOCK - 1) / MAP_BLOCK);
    return sps_with_walker(ctx, [&](auto w, unsigned long long *htab, uint64_t hmask) -> int {
        if constexpr (decltype(w)::planes)
            SP_LAUNCH(ctx, "k5_map_feat_sparse", k5_map_feat_sparse2<decltype(w)::table>, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, d_pk,
                      d_pm, d_nm, kp, n_units, d_foff, n_feat, S, htab, hmask, sq_tab_of(ctx), ctx->d_bloom, ctx->bloom_bits, d_counts);
        else
            SP_LAUNCH(ctx, "k5_map_feat_sparse_lab", k5_map_feat_sparse_lab, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, d_pk, d_nm, kp,
                      n_units, d_foff, n_feat, S, htab, hmask, ctx->d_bloom, ctx->bloom_bits, d_counts);
        return SP_OK;
    });
}

// interval mode (sp_map.hip: kv_cover / kv_count): the k > 15 scan that fills the per-unit subgenome masks
int sp_sparse_mask_launch(sp_ctx *ctx, sp_chrom &c, int64_t n_units, int S, const unsigned long long *d_cov,
                          unsigned long long *d_masks) {
    const sp_kparams kp = sp_make_kparams(ctx->k);
    const int64_t grid = map_grid(ctx, (n_units + MAP_BLOCK - 1) / MAP_BLOCK);
    return sps_with_walker(ctx, [&](auto w, unsigned long long *htab, uint64_t hmask) -> int {
        if constexpr (decltype(w)::planes)
            SP_LAUNCH(ctx, "k5_map_mask_sparse", k5_map_mask_sparse2<decltype(w)::table>, dim3((unsigned)grid), dim3(MAP_BLOCK), 0,
                      c.d_pk, c.d_pm, c.d_nm, kp, n_units, S, htab, hmask, sq_tab_of(ctx), ctx->d_bloom, ctx->bloom_bits, d_cov, d_masks);
        else
            SP_LAUNCH(ctx, "k5_map_mask_sparse_lab", k5_map_mask_sparse_lab, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, c.d_pk, c.d_nm,
                      kp, n_units, S, htab, hmask, ctx->d_bloom, ctx->bloom_bits, d_cov, d_masks);
        return SP_OK;
    });
}

int sp_sparse_hit(sp_ctx *ctx, unsigned long long *d_n) {
    const unsigned long long *d_keys = (const unsigned long long *)ctx->b_labkeys.p;
    switch (ctx->labels.kind) {
    case SP_LABELS_QUAD:
        if (ctx->n_labels > 0)
            SP_LAUNCH(ctx, "sq_seen", sq_seen, dim3((unsigned)(ctx->n_cu * 4)), dim3(256), 0, d_keys, ctx->n_labels, ctx->k,
                      sq_tab_of(ctx), d_n);
        return SP_OK;
    case SP_LABELS_PAIR_HASH:
        if (ctx->n_labels > 0)
            SP_LAUNCH(ctx, "sps_pair_seen", sps_pair_seen, dim3((unsigned)(ctx->n_cu * 4)), dim3(256), 0, d_keys, ctx->n_labels,
                      ctx->k, (const unsigned long long *)ctx->d_hkeys, (uint64_t)(ctx->hcap - 1), d_n);
        return SP_OK;
    default:
        SP_LAUNCH(ctx, "sps_count_seen", sps_count_seen, dim3((unsigned)(ctx->n_cu * 4)), dim3(256), 0,
                  (const unsigned long long *)ctx->d_hkeys, ctx->hcap, d_n);
        return SP_OK;
    }
}

// ------------------------------------------------------------------ multi-GPU support (k > 15)
// The dense path exchanges slot-range slices of the count tables; with 64-bit keys the same exchange
// is a KEY-RANGE partition of every chromosome's sorted (key, count >= lower) list: the owner cuts its
// lists at common splitters (sp_sparse_split), copies the pieces into the buffers handed to RCCL
// (sp_sparse_export), and the receiver filters its key range of all chromosomes (sp_sparse_view).
__global__ void sps_lower_bound(const unsigned long long *__restrict__ keys, int64_t n,
                                const unsigned long long *__restrict__ q, int nq, long long *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const unsigned long long x = q[i];
    int64_t lo = 0, hi = n;   // first index with keys[idx] >= x
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    out[i] = lo;
}

extern "C" {

int sp_sparse_sizes(sp_ctx *ctx, int64_t *n) {
    if (!ctx || !n) return sp_fail(ctx, SP_EINVAL, "sp_sparse_sizes: bad arguments");
    if (!ctx->sparse_mode || !ctx->counted) return sp_fail(ctx, SP_EINVAL, "sp_sparse_sizes: call sp_count with k > 15 first");
    for (size_t c = 0; c < ctx->sparse.size(); c++) n[c] = ctx->sparse[c].n;
    return SP_OK;
}

int sp_sparse_sample(sp_ctx *ctx, int chrom, int64_t n_samples, uint64_t *keys, int64_t *n_out) {
    if (!ctx || !keys || !n_out || n_samples < 1 || chrom < 0 || chrom >= (int)ctx->sparse.size())
        return sp_fail(ctx, SP_EINVAL, "sp_sparse_sample: bad arguments");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const sp_sparse_chrom &o = ctx->sparse[(size_t)chrom];
    const int64_t stride = o.n / n_samples;
    if (stride < 1) {   // short list: all of it
        if (o.n) SP_HIP(ctx, hipMemcpyAsync(keys, o.d_keys, (size_t)o.n * 8, hipMemcpyDeviceToHost, ctx->stream));
        *n_out = o.n;
    } else {            // every stride-th key of the sorted list
        SP_HIP(ctx, hipMemcpy2DAsync(keys, 8, o.d_keys, (size_t)stride * 8, 8, (size_t)n_samples, hipMemcpyDeviceToHost,
                                     ctx->stream));
        *n_out = n_samples;
    }
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_sparse_split(sp_ctx *ctx, int chrom, const uint64_t *splitters, int n_split, int64_t *bounds) {
    if (!ctx || !bounds || n_split < 0 || (n_split > 0 && !splitters) || n_split > 4096 || chrom < 0 ||
        chrom >= (int)ctx->sparse.size())
        return sp_fail(ctx, SP_EINVAL, "sp_sparse_split: bad arguments");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const sp_sparse_chrom &o = ctx->sparse[(size_t)chrom];
    bounds[0] = 0;
    bounds[n_split + 1] = o.n;
    if (n_split == 0) return SP_OK;
    void *scr = nullptr;
    int rc = sp_scratch(ctx, (int64_t)n_split * 16 + 256, &scr);
    if (rc) return rc;
    unsigned long long *d_q = (unsigned long long *)scr;
    long long *d_out = (long long *)(d_q + n_split);
    SP_HIP(ctx, hipMemcpyAsync(d_q, splitters, (size_t)n_split * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_LAUNCH(ctx, "sps_lower_bound", sps_lower_bound, dim3((unsigned)((n_split + 63) / 64)), dim3(64), 0,
              (const unsigned long long *)o.d_keys, o.n, (const unsigned long long *)d_q, n_split, d_out);
    SP_HIP(ctx, hipMemcpyAsync(bounds + 1, d_out, (size_t)n_split * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_sparse_export(sp_ctx *ctx, int chrom, int64_t first, int64_t count, void *d_keys, void *d_counts) {
    if (!ctx || chrom < 0 || chrom >= (int)ctx->sparse.size() || first < 0 || count < 0)
        return sp_fail(ctx, SP_EINVAL, "sp_sparse_export: bad arguments");
    const sp_sparse_chrom &o = ctx->sparse[(size_t)chrom];
    if (first + count > o.n) return sp_fail(ctx, SP_EINVAL, "sp_sparse_export: range exceeds the list (%lld)", (long long)o.n);
    if (count == 0) return SP_OK;
    if (!d_keys || !d_counts) return sp_fail(ctx, SP_EINVAL, "sp_sparse_export: NULL destination");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    SP_HIP(ctx, hipMemcpyAsync(d_keys, o.d_keys + first, (size_t)count * 8, hipMemcpyDeviceToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_counts, o.d_cnts + first, (size_t)count * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return SP_OK;   // asynchronous on the context's stream: sp_sync before another stream reads the buffers
}

int sp_sparse_view(sp_ctx *ctx, int C, const void *const *d_keys, const void *const *d_counts, const int64_t *n,
                   const int64_t *lengths, int k, int lower_count) {
    if (!ctx) return SP_EINVAL;
    if (!d_keys) {   // back to the local chromosomes
        ctx->sv_on = false;
        ctx->sv_keys.clear();
        ctx->sv_cnts.clear();
        ctx->sv_n.clear();
        ctx->fv_lengths.clear();
        ctx->filtered = false;
        return SP_OK;
    }
    if (C <= 0 || !d_counts || !n || !lengths || k < 16 || k > 32)
        return sp_fail(ctx, SP_EINVAL, "sp_sparse_view: bad arguments (k = 16..32)");
    if (C > SP_LIST_MAXC)
        return sp_fail(ctx, SP_EUNSUP, "sp_sparse_view: a view takes at most %d chromosomes (got %d); more chromosomes are "
                                       "filtered on one GPU", SP_LIST_MAXC, C);
    if (ctx->fv_on) return sp_fail(ctx, SP_EINVAL, "sp_sparse_view: a dense filter view is active");
    if (ctx->k != 0 && ctx->k != k) return sp_fail(ctx, SP_EINVAL, "sp_sparse_view: k=%d but the context counted with k=%d", k, ctx->k);
    for (int i = 0; i < C; i++)
        if (n[i] < 0 || (n[i] > 0 && (!d_keys[i] || !d_counts[i])))
            return sp_fail(ctx, SP_EINVAL, "sp_sparse_view: list %d is NULL", i);
    ctx->sv_keys.assign((size_t)C, nullptr);
    ctx->sv_cnts.assign((size_t)C, nullptr);
    ctx->sv_n.assign((size_t)C, 0);
    ctx->fv_lengths.assign((size_t)C, 0);
    for (int i = 0; i < C; i++) {
        ctx->sv_keys[(size_t)i] = (const uint64_t *)d_keys[i];
        ctx->sv_cnts[(size_t)i] = (const uint32_t *)d_counts[i];
        ctx->sv_n[(size_t)i] = n[i];
        ctx->fv_lengths[(size_t)i] = lengths[i];
    }
    if (ctx->k == 0) {   // a rank that owns no chromosome still filters its key range
        ctx->k = k;
        ctx->sparse_mode = true;
    }
    ctx->lower = lower_count < 1 ? 1 : lower_count;
    ctx->sv_on = true;
    ctx->filtered = false;
    return SP_OK;
}

}  // extern "C"
