// sp_map.hip -- K4 (label table) + K5 (fused scan + label lookup + bin reduce).
//
// Replaces Seqs.map_kmer3 / chunk_chromfiles / map_kmer_each4
// (reference: subphaser/Seqs.py:74-153, 209-244): every k-mer START position
// whose canonical k-mer is subgenome-specific adds 1 to (bin of start, SG).
//
// The K5 kernels of this file pair a walker of k <= 15 with a consumer of sp_map.h: k5_map2, k5_map_feat2, k5_map_mask2
// (map_walk_pair: map_unit_scan64 over the direct or the compact pair table, label planes) and k5_map_lab, k5_map_feat_lab,
// k5_map_mask_lab (map_walk_bytes: map_pair_scan + the byte table, hits).  Their k > 15 twins are in sp_sparse.hip.  One
// switch (map_with_walker) turns the label table's kind into the walker; a mode's launcher is a generic lambda over it.
#include "sp_device.h"
#include "sp_internal.h"
#include "sp_map.h"

// ----------------------------------------------------------------- K4
// Two-level label lookup.  A random 1-byte gather from the 512-MiB label table
// runs at ~54 G lookups/s on MI355X while a gather from an L2-resident structure
// runs at ~250 G/s (profiles/r01_ubench_mi355x.txt).  Most genome positions do
// not carry a subgenome-specific k-mer, so positions are first screened by a
// blocked Bloom filter that fits each XCD's 4-MiB L2 and only positions that
// pass it touch the exact table.
//
// The filter is keyed on the (k-1)-mer that two neighbouring k-mers (starts
// 2i and 2i+1) SHARE, so ONE L2 probe screens two start positions (7 G probes
// instead of 14 G on the wheat-like genome; K5 106 -> 84 ms at 2^25 bits, 70 ms
// at 2^24 bits).  Every labelled k-mer inserts its prefix and its suffix
// (k-1)-mer in canonical form: if the k-mer at s is labelled, its suffix is in
// the filter; if the k-mer at s+1 is labelled, its prefix -- the same (k-1)-mer
// -- is.  Size: the smallest power of two whose measured fill stays below
// MAP_FILL_MAX, at most 2^25 bits (a 2-MiB filter leaves half of the L2 to the
// genome stream and the table lines; 2^26 bits does not fit and is slower than
// no growth).
// pair filter: prefix and suffix (k-1)-mers of every labelled canonical k-mer
__global__ void __launch_bounds__(256)
k4_pair_filter(const unsigned long long *__restrict__ keys, int64_t n, int k, uint32_t *__restrict__ bloom, int nbits) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    uint64_t pre = 0, suf = 0;          // k = 1: the shared 0-mer is the constant 0
    if (k > 1) {
        const uint64_t m1mask = (k - 1 >= 32) ? ~0ULL : ((1ULL << (2 * (k - 1))) - 1ULL);
        pre = key >> 2;
        suf = key & m1mask;
        const uint64_t rpre = sp_revcomp(pre, k - 1), rsuf = sp_revcomp(suf, k - 1);
        pre = pre < rpre ? pre : rpre;
        suf = suf < rsuf ? suf : rsuf;
    }
    const map_bloom_probe p = map_bloom(pre, k, nbits);
    atomicOr(&bloom[p.word], p.bits);
    const map_bloom_probe q = map_bloom(suf, k, nbits);
    atomicOr(&bloom[q.word], q.bits);
}

__global__ void __launch_bounds__(256)
k4_filter_fill(const uint32_t *__restrict__ bloom, int64_t n_words, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x)
        c += __popc(bloom[i]);
    unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

__global__ void __launch_bounds__(256)
k4_labels(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ sg, int64_t n,
          sp_kparams kp, uint8_t *__restrict__ label) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    label[sp_slot_of_key(keys[i], kp)] = (uint8_t)(1u + sg[i]);
}

// ----------------------------------------------------------------- K4b: exact PAIR table
// The exact lookup that follows the filter used to be one random byte gather per candidate START from
// the 2^(2k-1)-byte label table -- an L2 miss each (54 G/s on this chip), 2.7 G of them on the wheat-like
// genome.  The pair table is keyed like the filter, on the canonical (k-1)-mer x two neighbouring starts
// share, and its 32-bit entry answers BOTH of them: eight 4-bit fields
//     field b     (b = 0..3)  label of the k-mer  b + x   ("L": x extended to the left by base b)
//     field 4 + b             label of the k-mer  x + b   ("R")
// in the orientation in which x is canonical; a field is (1 + SG) in its low three bits (0 = not a
// subgenome-specific k-mer) and a "seen" flag in bit 3.  One gather per candidate PAIR instead of one per
// candidate start: labelled k-mers come in runs (repeat copies), so almost every candidate pair carries
// two hits.  4^(k-1) entries (1 GiB at k = 15); S <= 7 (the label-table path below stays for S > 7).
__global__ void __launch_bounds__(256)
k4_pair_table(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ sg, int64_t n, int k,
              uint32_t *__restrict__ ptab) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const uint32_t l = 1u + sg[i];
    // a strand pair has ONE prefix location and ONE suffix location (both orientations lead to the same
    // two fields); palindromic x is handled by the <= in map_pair_loc_* and the same <= in the lookup
    const map_pair_loc a = map_pair_loc_prefix(key, k), b = map_pair_loc_suffix(key, k);
    atomicOr(&ptab[a.idx], l << (4 * a.field));
    atomicOr(&ptab[b.idx], l << (4 * b.field));
    const uint64_t r = sp_revcomp(key, k);
    const map_pair_loc c = map_pair_loc_prefix(r, k), d = map_pair_loc_suffix(r, k);
    atomicOr(&ptab[c.idx], l << (4 * c.field));
    atomicOr(&ptab[d.idx], l << (4 * d.field));
}

// un-build: zero the (at most four) entries every key of the PREVIOUS label set touched.  The table is 4^(k-1)
// words (1 GiB at k = 15) of which a label set writes a few million: clearing it with a memset cost 3.4 ms per
// sp_labels_set call, this costs what k4_pair_table costs.
__global__ void __launch_bounds__(256)
k4_pair_clear(const unsigned long long *__restrict__ keys, int64_t n, int k, uint32_t *__restrict__ ptab) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i], r = sp_revcomp(key, k);
    ptab[map_pair_loc_prefix(key, k).idx] = 0u;
    ptab[map_pair_loc_suffix(key, k).idx] = 0u;
    ptab[map_pair_loc_prefix(r, k).idx] = 0u;
    ptab[map_pair_loc_suffix(r, k).idx] = 0u;
}

__global__ void __launch_bounds__(256)
k4_pair_seen(const unsigned long long *__restrict__ keys, int64_t n, int k, const uint32_t *__restrict__ ptab,
             unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i], r = sp_revcomp(key, k);
        const map_pair_loc a = map_pair_loc_prefix(key, k), b = map_pair_loc_suffix(key, k);
        const map_pair_loc e = map_pair_loc_prefix(r, k), f = map_pair_loc_suffix(r, k);
        const uint32_t seen = ((ptab[a.idx] >> (4 * a.field)) | (ptab[b.idx] >> (4 * b.field)) |
                               (ptab[e.idx] >> (4 * e.field)) | (ptab[f.idx] >> (4 * f.field))) & 8u;
        c += seen ? 1 : 0;
    }
    unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

// ----------------------------------------------------------------- K4c: compact pair table (sp_map.h), S <= 3
// insert-or-find a key, then OR the field in.  The four entries of a bucket are tried in order and never freed, so two
// threads that insert the same key meet in the same entry; a bucket with four foreign entries raises its overflow flag
// and the key goes to the overflow table (linear probing; *fail is set when that table is full -- the host then falls
// back to the direct table).
__device__ __forceinline__ void map_ct_insert(const map_ptab &T, const map_ct_key &q, uint32_t bits, unsigned long long *fail) {
    uint32_t *e = reinterpret_cast<uint32_t *>(T.buckets + q.bucket);
    const uint32_t fresh = (q.tag << 25) | bits;
    // (the keys that share a (k-3)-mer share the bucket by design -- x1 and x2 of a run -- so every key starts at the
    // entry its own tag names instead of all of them queueing at entry 0: fewer failed compare-and-swaps beyond L2)
    for (int j = 0; j < 4; j++) {
        const int i = (int)((q.tag + (uint32_t)j) & 3u);
        const uint32_t old = atomicCAS(&e[i], 0u, fresh);
        if (old == 0u) return;
        if ((old >> 25) == q.tag && (old & MAP_CT_PAYLOAD)) {
            atomicOr(&e[i], bits);
            return;
        }
    }
    atomicOr(&e[0], MAP_CT_OVF);
    const unsigned long long mine = ((unsigned long long)(q.kid + 1u) << 32) | bits;
    uint32_t i = map_ct_ovf_home(q.kid) & T.ovf_mask;
    for (uint32_t probes = 0; probes <= T.ovf_mask; probes++) {
        const unsigned long long old = atomicCAS(&T.ovf[i], 0ULL, mine);
        if (old == 0ULL) {
            atomicAdd(fail + 1, 1ULL);      // (statistics: keys in the overflow table)
            return;
        }
        if ((uint32_t)(old >> 32) == q.kid + 1u) {
            atomicOr(&T.ovf[i], (unsigned long long)bits);
            return;
        }
        i = (i + 1u) & T.ovf_mask;
    }
    atomicAdd(fail, 1ULL);
}
__global__ void __launch_bounds__(256)
k4_ctab_build(const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ sg, int64_t n, int k, map_ptab T,
              unsigned long long *__restrict__ fail) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o2[2] = {keys[i], sp_revcomp(keys[i], k)};
    const uint32_t l = 1u + sg[i];
    // each (k-1)-mer / (k-3)-mer combination is canonical-as-read in exactly one of the two orientations (in both for a
    // palindromic (k-3)-mer; a palindromic k-mer, even k, enters the same fields twice: idempotent)
    for (int r = 0; r < 2; r++) {
        map_ct_site st[4];
        const int ns = map_ct_sites(o2[r], k, st);
        for (int j = 0; j < ns; j++)
            map_ct_insert(T, map_ct_key_of(T, st[j].t, st[j].side, st[j].e), l << (MAP_CT_FIELD * st[j].field), fail);
    }
}
__global__ void __launch_bounds__(256)
k4_ctab_seen(const unsigned long long *__restrict__ keys, int64_t n, int k, map_ptab T, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t o2[2] = {keys[i], sp_revcomp(keys[i], k)};
        uint32_t seen = 0;
        for (int r = 0; r < 2; r++) {
            map_ct_site st[4];
            const int ns = map_ct_sites(o2[r], k, st);
            for (int j = 0; j < ns; j++) {
                const map_ct_key q = map_ct_key_of(T, st[j].t, st[j].side, st[j].e);
                const uint4 B = T.buckets[q.bucket];
                seen |= (map_ct_find(T, B, q).fields >> (MAP_CT_FIELD * st[j].field)) & 4u;
            }
        }
        c += seen ? 1 : 0;
    }
    unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

// K5, pair-table engine (S <= 7): one block-iteration covers MAP_BLOCK units of 64 starts.  ONE launch maps every
// chromosome of the call: ranges are numbered through the whole genome (desc[c].range0 = first range of chromosome
// c) and dealt to the blocks round-robin, so the tail of the launch is one range per block instead of one partly
// filled round of blocks per chromosome (21 launches of 3.3 rounds each on the wheat-like genome).
struct map_chrom_desc {
    const uint32_t *pk, *pm, *nm;
    int64_t n_units;       // units of 64 starts
    int64_t nslots;        // output slots (bins + chunk duplicates) of this chromosome
    int64_t range0;        // number of ranges of the chromosomes before it
    int *counts;           // [nslots x S]
    unsigned long long *n_mapped;
};

#ifndef MAP_MIN_WAVES
#define MAP_MIN_WAVES 8     // waves per SIMD the register allocation must leave room for (four 512-thread workgroups per CU)
#endif
// ----------------------------------------------------------------- K5: the rolled walk (round 5)
// Rounds 2-4 unrolled the walk over a unit completely: 258 KB of machine code (the k > 15 twin: 532 KB) -- sixteen
// copies of the quad walk, each with four inlined copies of the hit path (64-bit divisions for the output slot, an LDS
// flush loop, the overflow probe loop) -- against 64 KB of instruction cache: every wave streamed the whole kernel from
// the L2 once per 64 starts, ~14 G instruction-line requests per wheat-like pass next to the 7 G filter probes the
// kernel was believed to be bound by, and the reason why no change to its memory accesses ever moved it (quad buckets:
// 1.55 G -> 0.96 G look-ups, same 45.9 ms; more loads in flight per lane: slower).  Those kernels were removed in round
// 6.  k5_map2 keeps the loop over the quads of a
// unit ROLLED (windows by run-time shifts out of a rotating pair of registers per stream), records a hit as a bit in
// three 64-bit label planes instead of calling into the slot arithmetic, and settles a unit's hits once: popcounts
// into the range's LDS histogram when the whole range lies in one output slot run (the common case; the boundaries
// are found once per range), the general walk otherwise.  TABLE: 1 = compact quad buckets (S <= 3), 0 = direct pair
// table (S <= 7).
// Round 6, second half: the walk over a unit has TWO phases, and the second is shared out over the wave.  PMC counters put
// k5_map2 at 70 % VALU utilisation (15.9 G wave instructions per wheat-like pass = 289 per quad and lane), half of them in the
// candidate path -- bucket key, tag compares, label fields, planes -- which every wave executed for every quad, because SOME lane
// of 64 is a candidate (27 % each; inside a repeat copy all sixteen quads of a lane are, so compacting per lane gains nothing:
// measured, same instruction count).  Phase 1 is the filter alone: it leaves the candidate quads of the WAVE in an LDS queue
// (lane, quad, which pairs).  Phase 2 deals the queue out to all lanes: ~280 candidates per 1024 quads are 4-5 iterations of the
// candidate path per unit instead of 16.  A lane rebuilds the windows of the quad it was dealt from the owner's ten packed words,
// parked in LDS (one column per thread), and ORs the labels it finds into the owner's planes there.
#ifndef MAP2_QI
#define MAP2_QI 1      // quads per iteration of the filter phase
#endif
struct map_quad_win {
    uint32_t V1, V2, xf1, xr1, xf2, xr2;       // 16-base windows at j / j + 2 (MSB-first), x1 / x2 forward and reverse complement
};
__device__ __forceinline__ map_quad_win map_quad_windows(uint32_t l0, uint32_t l1, uint32_t m0, uint32_t m1, int r /* 0, 4, 8, 12 */,
                                                         int sh, uint32_t m1mask) {
    map_quad_win q;
    const uint32_t W1 = __builtin_amdgcn_alignbit(l1, l0, 2 * r), W2 = __builtin_amdgcn_alignbit(l1, l0, 2 * r + 4);
    const unsigned long long mm = ((unsigned long long)m0 << 32) | m1;
    q.V1 = (uint32_t)((mm << (2 * r)) >> 32);
    q.V2 = (uint32_t)((mm << (2 * r + 4)) >> 32);
    q.xf1 = (q.V1 >> sh) & m1mask;       // x1 forward / reverse complement, key order
    q.xr1 = (~W1 >> 2) & m1mask;
    q.xf2 = (q.V2 >> sh) & m1mask;
    q.xr2 = (~W2 >> 2) & m1mask;
    return q;
}
template <int TABLE>
__device__ __forceinline__ void map_unit_scan64(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm,
                                                const uint32_t *__restrict__ nm, int64_t s0, const sp_kparams32 &kp,
                                                const uint32_t *__restrict__ bloom, int nbits, const map_ptab &T,
                                                unsigned long long lab[3], const map_unit_lds &U,
                                                unsigned long long cm = ~0ULL /* starts that count */) {
    constexpr int FW = TABLE ? MAP_CT_FIELD : 4;
    constexpr uint32_t LBL = TABLE ? 3u : 7u, SEEN = TABLE ? 4u : 8u, FMASK = TABLE ? 7u : 15u;
    constexpr uint32_t ANY = TABLE ? MAP_CT_ANY : 0x77777777u;
    constexpr int NP = TABLE ? 2 : 3, ROUND_W = TABLE ? MAP2_ROUND_W : 2;
    // validity of the 64 starts: k-mer at s0+j, shared (k-1)-mer at s0+j+1
    unsigned long long ok_k, ok_x;
    {
        const uint64_t badA = sp_bad_starts64(nm, s0, kp.k - 1), badB = sp_bad_starts64(nm, s0 + 32, kp.k - 1);
        const uint64_t invA = (uint64_t)nm[s0 >> 5] | ((uint64_t)nm[(s0 >> 5) + 1] << 32);
        const uint64_t invB = (uint64_t)nm[(s0 >> 5) + 1] | ((uint64_t)nm[(s0 >> 5) + 2] << 32);
        const uint32_t kA = ~(uint32_t)(badA | (invA >> (kp.k - 1))), kB = ~(uint32_t)(badB | (invB >> (kp.k - 1)));
        const uint32_t xA = ~(uint32_t)(badA >> 1), xB = ~(uint32_t)(badB >> 1);
        ok_k = (unsigned long long)kA | ((unsigned long long)kB << 32);
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
    uint32_t l0 = la.x, l1 = la.y, l2 = la.z, l3 = la.w, l4 = pk[w0 + 4];
#if SP_DERIVE_PM
    (void)pm;
    uint32_t m0 = sp_msb_of_lsb(l0), m1 = sp_msb_of_lsb(l1), m2 = sp_msb_of_lsb(l2), m3 = sp_msb_of_lsb(l3), m4 = sp_msb_of_lsb(l4);
#else
    const uint4 ma = *reinterpret_cast<const uint4 *>(pm + w0);
    uint32_t m0 = ma.x, m1 = ma.y, m2 = ma.z, m3 = ma.w, m4 = pm[w0 + 4];
#endif
    {
        const unsigned long long okc = ok_k & cm;      // (a start outside `cm` -- interval mode: not covered by a feature -- is neither counted nor marked seen)
        sw[0 * MAP_BLOCK] = l0; sw[1 * MAP_BLOCK] = l1; sw[2 * MAP_BLOCK] = l2; sw[3 * MAP_BLOCK] = l3; sw[4 * MAP_BLOCK] = l4;
        sw[5 * MAP_BLOCK] = (uint32_t)okc; sw[6 * MAP_BLOCK] = (uint32_t)(okc >> 32);
#pragma unroll
        for (int bit = 0; bit < NP; bit++) U.planes[bit * MAP_BLOCK + tid] = 0ULL;
    }
    const int sh = 32 - 2 * kp.k, sh1 = 30 - 2 * kp.k;
    const uint32_t m1mask = kp.kmask >> 2;
    const int sb = T.sb;
    const uint32_t smask = TABLE ? ((1u << sb) - 1u) : 0u;
    // the filter's addressing (sp_map.h): by the smaller-hashed core of the (k-1)-mer, or by the (k-1)-mer itself
    const bool core = (nbits & MAP_BLOOM_CORE) && kp.k >= 5;      // (uniform)
    const uint32_t cmask = kp.k >= 5 ? ((1u << (2 * (kp.k - 3))) - 1u) : 0u;
    const int wsh = 32 - (MAP_BLOOM_NBITS(nbits) - 5);
    uint32_t last_wi = 0xFFFFFFFFu, last_w = 0u;                  // the word this lane fetched last (index, content)
    // hash of the core the previous quad ended with, which is the core the next one begins with; the unit's first quad has
    // no predecessor: its first core is hashed here, once, and not behind a test in the loop
    uint32_t h_carry = 0u;
    if (core) {
        const map_quad_win Q0 = map_quad_windows(l0, l1, m0, m1, 0, sh, m1mask);
        h_carry = map_chain_start24(Q0.xf1, Q0.xr1, cmask);
    }
    // runs (sp_map.h), one counter per lane: below MAP_RUNS_R it is the lane's probed quads that passed on both pairs, in a
    // row; from there on, MAP_RUNS_R + the quads it has predicted since.  Per unit: 0 here, carried over the rounds.
    static_assert(MAP2_QI == 1, "the runs rule decides a quad from the filter's answer for the quad before it");
    const bool runs = (nbits & MAP_RUNS) != 0;                     // (uniform)
    uint32_t run = 0u;
#pragma unroll 1
    for (int wr = 0; wr < 4; wr += ROUND_W) {
        // ---- phase 1: the filter over ROUND_W words of sixteen starts; the wave's candidate quads go to its queue
        uint32_t qn = 0;                                           // (uniform)
#pragma unroll 1
        for (int w = wr; w < wr + ROUND_W; w++) {
#pragma unroll 1
            for (int r0 = 0; r0 < 16; r0 += 4 * MAP2_QI) {
                // MAP2_QI quads per iteration: their filter words are requested together (the word a pair re-uses is known from the
                // indices alone), then looked at
                uint32_t bt1[MAP2_QI], bt2[MAP2_QI], wi1[MAP2_QI], wi2[MAP2_QI], f1[MAP2_QI], f2[MAP2_QI];
                bool v1[MAP2_QI], v2[MAP2_QI], need1[MAP2_QI], need2[MAP2_QI], guess[MAP2_QI];
                uint32_t lw = last_wi;
#pragma unroll
                for (int q = 0; q < MAP2_QI; q++) {
                    const int r = r0 + 4 * q, j = 16 * w + r;     // the quad's first start; its pairs share x1 (at j + 1) and x2 (at j + 3)
                    const map_quad_win Q = map_quad_windows(l0, l1, m0, m1, r, sh, m1mask);
                    const uint32_t okx = (uint32_t)(ok_x >> j);
                    v1[q] = okx & 1u;
                    v2[q] = okx & 4u;
                    // word and bits of x1 and x2: the 24-bit family of sp_maphash.h (k <= 15 here: no choice per quad)
                    if (core) {
                        map_bloom_probe p1, p2;
                        map_quad_probes24(Q.xf1, Q.xr1, Q.xf2, Q.xr2, cmask, nbits, h_carry, p1, p2);
                        wi1[q] = p1.word; bt1[q] = p1.bits;
                        wi2[q] = p2.word; bt2[q] = p2.bits;
                    } else {
                        uint32_t h1, h2;
                        bt1[q] = map_bloom_bits3_24(Q.xf1 < Q.xr1 ? Q.xf1 : Q.xr1, h1);
                        bt2[q] = map_bloom_bits3_24(Q.xf2 < Q.xr2 ? Q.xf2 : Q.xr2, h2);
                        wi1[q] = h1 >> wsh;
                        wi2[q] = h2 >> wsh;
                    }
                    // a word this lane holds already (the previous pair's) is not fetched again: with the core addressing that
                    // is the case for a third of the pairs -- and a gather is priced per active lane
                    // inside a run the quad is not probed at all: it is a candidate on both of its (valid) pairs, and the word the
                    // lane holds stays the one it fetched last
                    guess[q] = runs && v1[q] && v2[q] && run - (uint32_t)MAP_RUNS_R < (uint32_t)MAP_RUNS_P;
                    need1[q] = !guess[q] && v1[q] && wi1[q] != lw;
                    need2[q] = !guess[q] && v2[q] && wi2[q] != (v1[q] ? wi1[q] : lw);
                    f1[q] = f2[q] = 0;
                    if (need1[q]) f1[q] = bloom[wi1[q]];
                    if (need2[q]) f2[q] = bloom[wi2[q]];
                    if (!guess[q]) {
                        if (v2[q]) lw = wi2[q];
                        else if (v1[q]) lw = wi1[q];
                    }
                }
                last_wi = lw;
#pragma unroll
                for (int q = 0; q < MAP2_QI; q++) {
                    const int j = 16 * w + r0 + 4 * q;
                    const uint32_t wd1 = v1[q] ? (need1[q] ? f1[q] : last_w) : 0u;
                    const uint32_t wd2 = v2[q] ? (need2[q] ? f2[q] : (v1[q] ? wd1 : last_w)) : 0u;
                    if (!guess[q]) {
                        if (v2[q]) last_w = wd2;
                        else if (v1[q]) last_w = wd1;
                    }
                    const bool cand1 = guess[q] || (wd1 & bt1[q]) == bt1[q], cand2 = guess[q] || (wd2 & bt2[q]) == bt2[q];       // (an invalid pair's word is 0: never a candidate)
                    // (a probed quad that passes keeps a run going: back to MAP_RUNS_R, the next MAP_RUNS_P quads are predicted)
                    run = guess[q] ? run + 1u : (cand1 && cand2) ? (run < (uint32_t)MAP_RUNS_R ? run + 1u : (uint32_t)MAP_RUNS_R) : 0u;
                    const unsigned long long bal = __ballot(cand1 || cand2);
                    if (cand1 || cand2)
                        queue[qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] =
                            (uint16_t)((uint32_t)lane | ((uint32_t)(j >> 2) << 6) | (cand1 ? 0x400u : 0u) | (cand2 ? 0x800u : 0u));
                    qn += (uint32_t)__popcll(bal);
                }
            }
            l0 = l1; l1 = l2; l2 = l3; l3 = l4;
            m0 = m1; m1 = m2; m2 = m3; m3 = m4;
        }
        // ---- phase 2: the queue, dealt out to the lanes that are here (LDS operations of a wave complete in program order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t e0 = (uint32_t)me; e0 < qn; e0 += (uint32_t)(MAP2_P2 * n_here)) {
            // MAP2_P2 entries per lane and iteration: their bucket loads (Infinity Cache: the longest wait of the kernel) travel together
            bool live[MAP2_P2], cand1[MAP2_P2], cand2[MAP2_P2], sfw[MAP2_P2];
            int owner[MAP2_P2], jj[MAP2_P2];
            map_quad_win Q[MAP2_P2];
            uint32_t okk[MAP2_P2], e1[MAP2_P2], e2[MAP2_P2];
            map_ct_key k1[MAP2_P2], k2[MAP2_P2];
            uint4 B[MAP2_P2];
#pragma unroll
            for (int p = 0; p < MAP2_P2; p++) {
                const uint32_t e = e0 + (uint32_t)(p * n_here);
                live[p] = e < qn;
                const uint32_t ent = live[p] ? (uint32_t)queue[e] : 0u;
                const int qi = (int)((ent >> 6) & 15u), w = qi >> 2;
                owner[p] = wave0 + (int)(ent & 63u);
                jj[p] = 4 * qi;
                cand1[p] = ent & 0x400u;
                cand2[p] = ent & 0x800u;
                const uint32_t *ow = U.words + owner[p];
                const uint32_t ola = ow[w * MAP_BLOCK], olb = ow[(w + 1) * MAP_BLOCK];
                Q[p] = map_quad_windows(ola, olb, sp_msb_of_lsb(ola), sp_msb_of_lsb(olb), jj[p] & 15, sh, m1mask);
                okk[p] = ow[(5 + (w >> 1)) * MAP_BLOCK] >> (jj[p] & 31);      // countable starts j .. j + 3 of the owner's unit
                e1[p] = e2[p] = 0;
                sfw[p] = false;
                B[p] = make_uint4(0u, 0u, 0u, 0u);
                if (TABLE) {
                    // s = the last k-3 bases of x1 = the first k-3 bases of x2 (a candidate's (k-1)-mer is valid, so s is)
                    const uint32_t s_f = cand1[p] ? (Q[p].xf1 & smask) : (Q[p].xf2 >> 4), s_r = cand1[p] ? (Q[p].xr1 >> 4) : (Q[p].xr2 & smask);
                    sfw[p] = s_f <= s_r;
                    const uint32_t t = sfw[p] ? s_f : s_r;
                    // x1 = e + s: side L read forward, side R (e reverse-complemented) read backward; x2 = s + e: the mirror image
                    k1[p] = map_ct_key_of(T, t, sfw[p] ? 0u : 1u, sfw[p] ? (Q[p].xf1 >> sb) : (Q[p].xr1 & 15u));
                    k2[p] = map_ct_key_of(T, t, sfw[p] ? 1u : 0u, sfw[p] ? (Q[p].xf2 & 15u) : (Q[p].xr2 >> sb));
                    if (live[p]) B[p] = T.buckets[k1[p].bucket];
                } else {
                    if (cand1[p]) e1[p] = T.direct[Q[p].xf1 < Q[p].xr1 ? Q[p].xf1 : Q[p].xr1];
                    if (cand2[p]) e2[p] = T.direct[Q[p].xf2 < Q[p].xr2 ? Q[p].xf2 : Q[p].xr2];
                }
            }
#pragma unroll
            for (int p = 0; p < MAP2_P2; p++) {
                if (!live[p]) continue;
                const int j = jj[p];
                uint32_t loc1 = Q[p].xf1 < Q[p].xr1 ? Q[p].xf1 : Q[p].xr1, loc2 = Q[p].xf2 < Q[p].xr2 ? Q[p].xf2 : Q[p].xr2;
                bool fw1 = Q[p].xf1 <= Q[p].xr1, fw2 = Q[p].xf2 <= Q[p].xr2;
                if (TABLE) {
                    if (cand1[p]) {
                        const map_ct_hit h = map_ct_find(T, B[p], k1[p]);
                        e1[p] = h.fields;
                        loc1 = h.loc;
                    }
                    if (cand2[p]) {
                        const map_ct_hit h = map_ct_find(T, B[p], k2[p]);
                        e2[p] = h.fields;
                        loc2 = h.loc;
                    }
                    fw1 = fw2 = sfw[p];       // the fields are laid out in the orientation in which t is canonical
                }
                // the (up to four) labelled starts of the quad: start j + 2h = b0 + x, start j + 2h + 1 = x + b1
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t ee = h ? e2[p] : e1[p];
                    if (!(ee & ANY)) continue;
                    const uint32_t V = h ? Q[p].V2 : Q[p].V1;
                    const bool fw = h ? fw2 : fw1;
                    const uint32_t b0 = V >> 30, b1 = (V >> sh1) & 3u;
                    const int f0 = fw ? (int)b0 : 7 - (int)b0, f1 = fw ? 4 + (int)b1 : 3 - (int)b1;
                    const uint32_t cnt2 = okk[p] >> (2 * h);
                    const uint32_t v0 = (cnt2 & 1u) ? (ee >> (FW * f0)) & FMASK : 0u;
                    const uint32_t v1 = (cnt2 & 2u) ? (ee >> (FW * f1)) & FMASK : 0u;
                    const uint32_t two = (v0 & LBL) | ((v1 & LBL) << 8);      // labels of the two starts
                    if (!two) continue;
#pragma unroll
                    for (int bit = 0; bit < NP; bit++) {
                        const unsigned long long b2 = (unsigned long long)(((two >> bit) & 1u) | (((two >> (8 + bit)) & 1u) << 1));
                        if (b2) atomicOr(&U.planes[bit * MAP_BLOCK + owner[p]], b2 << (j + 2 * h));
                    }
                    uint32_t mark = 0;       // "seen": first touch only
                    if ((v0 & LBL) && !(v0 & SEEN)) mark |= SEEN << (FW * f0);
                    if ((v1 & LBL) && !(v1 & SEEN)) mark |= SEEN << (FW * f1);
                    if (mark) {
                        if (TABLE) map_ct_mark(T, h ? loc2 : loc1, mark);
                        else atomicOr(&T.direct[h ? loc2 : loc1], mark);
                    }
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

// the planes walker of k <= 15 (sp_map.h): the two-phase walk over the direct (TABLE 0) or the compact (1) pair table
template <int TABLE>
struct map_walk_pair {
    const uint32_t *pk, *pm, *nm;
    const sp_kparams32 &kp;
    const map_ptab &T;
    const uint32_t *bloom;
    int nbits;
    __device__ __forceinline__ void operator()(int64_t s0, unsigned long long lab[3], const map_unit_lds &U,
                                               unsigned long long cm = ~0ULL) const {
        map_unit_scan64<TABLE>(pk, pm, nm, s0, kp, bloom, nbits, T, lab, U, cm);
    }
};

template <int TABLE>
__global__ void __launch_bounds__(MAP_BLOCK, MAP_MIN_WAVES)
k5_map2(const map_chrom_desc *__restrict__ desc, int n_chrom, int64_t n_ranges, sp_kparams32 kp, sp_map_params P,
        map_ptab ptab, const uint32_t *__restrict__ bloom, int bloom_bits) {
    __shared__ int hist[MAP_LDS_ENTRIES];
    __shared__ unsigned long long red[16];
    MAP_UNIT_LDS_DECL(TABLE, 7);
    map_bins_acc acc(hist, P, kp.k);
    int cur = -1;          // chromosome the block is accumulating `acc.mapped` for
    auto flush_mapped = [&]() {     // block-uniform control flow
        if (cur < 0) return;
        const unsigned long long t = sp_block_sum_u64(acc.mapped, red);
        if (threadIdx.x == 0 && t) atomicAdd(desc[cur].n_mapped, t);
        acc.mapped = 0;
    };
    for (int64_t rg = blockIdx.x; rg < n_ranges; rg += gridDim.x) {
        int lo = 0, hi = n_chrom;              // last chromosome with range0 <= rg (uniform: scalar loads)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (desc[mid].range0 <= rg) lo = mid;
            else hi = mid;
        }
        if (lo != cur) {
            flush_mapped();
            cur = lo;
        }
        const map_chrom_desc D = desc[lo];
        const int64_t r = rg - D.range0;
        const int64_t u = r * MAP_BLOCK + threadIdx.x;
        acc.begin(r, D.counts, D.nslots);
        if (u < D.n_units) {
            unsigned long long lab[3] = {0ULL, 0ULL, 0ULL};
            map_walk_pair<TABLE>{D.pk, D.pm, D.nm, kp, ptab, bloom, bloom_bits}(u * SP_UNIT, lab, ulds);
            acc.add_planes(u * SP_UNIT, lab);
        }
        acc.end();
    }
    flush_mapped();
}

template <int TABLE>
__global__ void __launch_bounds__(MAP_BLOCK, MAP_MIN_WAVES)
k5_map_mask2(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm, sp_kparams32 kp,
             int64_t n_units, int S, map_ptab ptab, const uint32_t *__restrict__ bloom, int bloom_bits,
             const unsigned long long *__restrict__ cov, unsigned long long *__restrict__ masks /* n_units x S */) {
    MAP_UNIT_LDS_DECL(TABLE, 7);
    map_mask_planes(map_walk_pair<TABLE>{pk, pm, nm, kp, ptab, bloom, bloom_bits}, ulds, n_units, S, cov, masks);
}

// the exact pair table the current label set lives in (SP_LABELS_DIRECT or SP_LABELS_COMPACT)
static map_ptab map_ptab_of(const sp_ctx *ctx) {
    const bool compact = ctx->labels.kind == SP_LABELS_COMPACT;
    map_ptab T;
    T.direct = compact ? nullptr : (uint32_t *)ctx->b_ptab.p;
    T.buckets = compact ? (uint4 *)ctx->b_ctab.p : nullptr;
    T.ovf = (unsigned long long *)ctx->b_covf.p;
    T.ovf_mask = (uint32_t)ctx->labels.ovf_mask;
    T.sb = 2 * (ctx->k - 3);
    T.tb = compact ? T.sb - ctx->labels.bb : 0;
    return T;
}

// the one readiness test of the map entries (sp_label_state in sp_common.h says when `ready` holds)
static int map_need_labels(sp_ctx *ctx, const char *entry) {
    if (ctx->labels.ready) return SP_OK;
    return sp_fail(ctx, SP_EINVAL, "%s: call sp_labels_set first", entry);
}

// the hits walker of k <= 15 (sp_map.h), any S <= 126: the rolling scan + one byte gather per candidate start from the label
// table; bit 7 of a label byte is its "seen" mark
struct map_walk_bytes {
    const uint32_t *pk, *nm;
    const sp_kparams32 &kp;
    uint8_t *label;
    const uint32_t *bloom;
    int nbits;
    template <typename F>
    __device__ __forceinline__ void scan(int64_t s0, F &&each) const {
        map_pair_scan<uint32_t>(pk, nm, s0, kp, bloom, nbits,
                                [&](int64_t start, uint32_t fwd, uint32_t rc) { each(start, sp_slot_of32(fwd, rc, kp)); });
    }
    template <typename C>
    __device__ __forceinline__ int look(uint32_t slot, C &&counted) const {
        const uint32_t l = label[slot];
        if (!l || !counted()) return -1;
        if (!(l & 0x80u)) label[slot] = (uint8_t)(l | 0x80u);  // idempotent "seen" mark
        return (int)(l & 0x7fu) - 1;
    }
};

__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_lab(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, sp_kparams32 kp,
       sp_map_params P, uint8_t *__restrict__ label, const uint32_t *__restrict__ bloom, int bloom_bits,
       int *__restrict__ slot_counts, unsigned long long *__restrict__ n_mapped) {
    __shared__ int hist[MAP_LDS_ENTRIES];
    __shared__ unsigned long long red[16];
    const map_walk_bytes walk{pk, nm, kp, label, bloom, bloom_bits};
    map_bins_acc acc(hist, P, kp.k);
    map_bins_chrom(acc, red, slot_counts, n_mapped, [&](int64_t s0) { acc.add_hits(walk, s0); });
}

// Window stack on the device (Circos.stack_matrix semantics, Circos.py:734-742): the window of a
// slot is (bin start) / window_size, bin = slot - chunk(slot); the two slots of a chunk-boundary bin
// land in the same window.
__global__ void __launch_bounds__(256)
k5_stack(const int *__restrict__ slot_counts, int64_t total_slots, int S, int C,
         const long long *__restrict__ slot_off, const long long *__restrict__ win_off,
         const long long *__restrict__ seg_start /* position of local base 0 inside its chromosome, or NULL */,
         int64_t bin_size, int64_t chunk_size, int64_t window_size, int k, unsigned long long *__restrict__ win_counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_slots * S) return;
    const int v = slot_counts[i];
    if (!v) return;
    const int64_t gslot = i / S;
    const int sg = (int)(i - gslot * S);
    int lo = 0, hi = C;  // chromosome of the slot
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (slot_off[mid] <= gslot) lo = mid;
        else hi = mid;
    }
    const int64_t slot = gslot - slot_off[lo];
    const int64_t chunk = chunk_size > 0 ? map_chunk_of_slot(slot, bin_size, chunk_size, k) : 0;
    const int64_t win = ((seg_start ? seg_start[lo] : 0) + (slot - chunk) * bin_size) / window_size;
    atomicAdd(&win_counts[(win_off[lo] + win) * S + sg], (unsigned long long)v);
}

// Feature mode (the consumers: map_feat_planes / map_feat_hits, sp_map.h).  The features lie back to back in one packed
// sequence; a k-mer belongs to feature f iff it lies entirely inside [foff[f], foff[f + 1]).
template <int TABLE>
__global__ void __launch_bounds__(MAP_BLOCK, MAP_MIN_WAVES)
k5_map_feat2(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ pm, const uint32_t *__restrict__ nm,
             sp_kparams32 kp, int64_t n_units, const int64_t *__restrict__ foff, int64_t n_feat, int S,
             map_ptab ptab, const uint32_t *__restrict__ bloom, int bloom_bits,
             unsigned long long *__restrict__ counts) {
    MAP_UNIT_LDS_DECL(TABLE, 7);
    map_feat_planes(map_walk_pair<TABLE>{pk, pm, nm, kp, ptab, bloom, bloom_bits}, ulds, kp.k, n_units, foff, n_feat, S, counts);
}

__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_feat_lab(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, sp_kparams32 kp,
            int64_t n_units, const int64_t *__restrict__ foff, int64_t n_feat, int S,
            uint8_t *__restrict__ label, const uint32_t *__restrict__ bloom, int bloom_bits,
            unsigned long long *__restrict__ counts) {
    map_feat_hits(map_walk_bytes{pk, nm, kp, label, bloom, bloom_bits}, kp.k, n_units, foff, n_feat, S, counts);
}

// ----------------------------------------------------------------- interval mode (BED features over the resident genome)
// The reference maps `-custom_features` as a FASTA of feature sequences (__main__.py:509-517, Seqs.py:228-244): at
// wheat scale that is 10 Gb of sequence that is already resident in HBM as the genome.  Intervals need no upload:
//   kv_cover    marks every k-mer start that lies, with its whole k-mer, inside at least one interval (1 bit per start);
//   k5_map_mask the usual scan, restricted to covered starts: one 64-bit mask per (unit of 64 starts, subgenome) --
//               bit j = start 64 u + j carries a k-mer of that subgenome; labelled k-mers are marked "seen" only at
//               covered starts, exactly the k-mers a feature FASTA would contain;
//   kv_count    one wave per interval: popcounts of the masks over its units (edge units masked) -> counts[i][sg].
// Overlapping and nested intervals cost nothing extra, every interval reads only its own units.
__global__ void __launch_bounds__(256)
kv_cover(const int32_t *__restrict__ chrom, const int64_t *__restrict__ start, const int64_t *__restrict__ end, int64_t n,
         int k, const int64_t *__restrict__ ubase /* first unit of every chromosome */, unsigned long long *__restrict__ cov) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wv; i < n; i += nw) {
        const int64_t a = start[i], b = end[i] - k + 1;     // starts [a, b)
        if (b <= a) continue;
        unsigned long long *cw = cov + ubase[chrom[i]];
        const int64_t u0 = a >> 6, u1 = (b - 1) >> 6;
        for (int64_t u = u0 + lane; u <= u1; u += 64) {
            unsigned long long m = ~0ULL;
            if (u == u0) m &= ~0ULL << (a & 63);
            if (u == u1 && (b & 63)) m &= (1ULL << (b & 63)) - 1ULL;
            if (m == ~0ULL) {
                if (cw[u] != ~0ULL) cw[u] = ~0ULL;     // (plain store of all ones: idempotent, races are benign)
            } else {
                atomicOr(&cw[u], m);
            }
        }
    }
}

// (label-table engine, more than 7 subgenomes; the pair-table engines take k5_map_mask2 above)
__global__ void __launch_bounds__(MAP_BLOCK)
k5_map_mask_lab(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ nm, sp_kparams32 kp, int64_t n_units, int S,
                uint8_t *__restrict__ label, const uint32_t *__restrict__ bloom, int bloom_bits,
                const unsigned long long *__restrict__ cov, unsigned long long *__restrict__ masks /* n_units x S */) {
    map_mask_hits(map_walk_bytes{pk, nm, kp, label, bloom, bloom_bits}, n_units, S, cov, masks);
}

__global__ void __launch_bounds__(256)
kv_count(const int32_t *__restrict__ chrom, const int64_t *__restrict__ start, const int64_t *__restrict__ end, int64_t n,
         int k, int S, const int64_t *__restrict__ ubase, const unsigned long long *__restrict__ masks,
         unsigned long long *__restrict__ counts /* n x S */) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wv; i < n; i += nw) {
        const int64_t a = start[i], b = end[i] - k + 1;
        const int64_t u0 = a >> 6, u1 = b > a ? (b - 1) >> 6 : u0 - 1;
        const unsigned long long *mk = masks + ubase[chrom[i]] * S;
        for (int sg = 0; sg < S; sg++) {
            unsigned long long c = 0;
            for (int64_t u = u0 + lane; u <= u1; u += 64) {
                unsigned long long m = mk[u * S + sg];
                if (u == u0) m &= ~0ULL << (a & 63);
                if (u == u1 && (b & 63)) m &= (1ULL << (b & 63)) - 1ULL;
                c += __popcll(m);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0) counts[i * S + sg] = c;
        }
    }
}

__global__ void __launch_bounds__(256)
k4_count_seen(const uint8_t *__restrict__ label, int64_t nslots, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long n = 0;
    const int64_t n16 = nslots >> 4;
    const uint4 *l4 = reinterpret_cast<const uint4 *>(label);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint4 v = l4[i];
        n += __popc(v.x & 0x80808080u) + __popc(v.y & 0x80808080u) + __popc(v.z & 0x80808080u) +
             __popc(v.w & 0x80808080u);
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n16 << 4) + threadIdx.x; i < nslots; i += blockDim.x) n += (label[i] >> 7) & 1u;
    unsigned long long t = sp_block_sum_u64(n, red);
    if (threadIdx.x == 0 && t) atomicAdd(out, t);
}

// the flags of one sp_labels_set call -> page-locked host memory the kernel writes directly: a hipMemcpy of 32 bytes
// would queue on the copy engine behind the matrix rows that are still travelling to the host (2 ms per pass)
__global__ void k4_flags_out(const unsigned long long *__restrict__ d_flags, unsigned long long *__restrict__ h_flags) {
    if (threadIdx.x < 4) h_flags[threadIdx.x] = d_flags[threadIdx.x];
}

// labels handed over in device memory: the largest one, for the `label < n_sg` check the host does on host arrays
__global__ void __launch_bounds__(256)
k4_label_max(const uint8_t *__restrict__ sg, int64_t n, unsigned int *__restrict__ out) {
    unsigned int m = 0;
    // (16 labels per load where the array allows it: byte by byte this took 0.25 ms for 2.2 M labels)
    const int64_t head = ((16 - (int64_t)((uintptr_t)sg & 15)) & 15) < n ? ((16 - (int64_t)((uintptr_t)sg & 15)) & 15) : n;
    const int64_t n16 = (n - head) / 16;
    const uint4 *v4 = reinterpret_cast<const uint4 *>(sg + head);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 v = v4[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned int x = (w[q] >> (8 * b)) & 255u;
                m = x > m ? x : m;
            }
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (i < head || i >= head + 16 * n16) m = sg[i] > m ? sg[i] : m;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int x = __shfl_down(m, o, 64);
        m = x > m ? x : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// Build the pair filter over the labelled keys (device array, canonical 2-bit keys) at the smallest
// size whose fill stays below MAP_FILL_MAX.  Shared by the dense and the sparse label paths.
int sp_map_filter_build(sp_ctx *ctx, const unsigned long long *d_keys, int64_t n) {
    if (!ctx->d_bloom) SP_HIP(ctx, hipMalloc(&ctx->d_bloom, ((size_t)1 << MAP_BLOOM_MAX_BITS) / 8 + 64));   // + fill counter
    int bits = MAP_BLOOM_MIN_BITS;
    while (bits < MAP_BLOOM_MAX_BITS - 1 && ((int64_t)1 << bits) < 6 * n) bits++;
    // The size is a speed heuristic (fill <= MAP_FILL_MAX), never a matter of correctness: a label set of the size of
    // the previous one (the same set, pass after pass, in a pipeline that re-maps) takes the size chosen then without
    // measuring the fill again -- the measurement is a device -> host round trip per candidate size.
    const bool cached = n > 0 && n == ctx->bloom_last_n && ctx->k == ctx->bloom_last_k && ctx->bloom_last_bits >= bits;
    if (cached) bits = ctx->bloom_last_bits;
    unsigned long long *d_small = (unsigned long long *)((char *)ctx->d_bloom + ((size_t)1 << MAP_BLOOM_MAX_BITS) / 8);
    // round 6: words addressed by the smaller-hashed core of the (k-1)-mer (sp_map.h); SP_MAP_FILTER=x keeps the round-1
    // addressing by the (k-1)-mer itself (cross-check).  ctx->bloom_bits carries the flag to every kernel that probes.
    const char *env_mf = getenv("SP_MAP_FILTER");
    const char *env_runs = getenv("SP_MAP_RUNS");       // SP_MAP_RUNS=0: the k <= 15 walk probes every quad (cross-check of the runs rule, sp_map.h)
    const int mode = ((env_mf && env_mf[0] == 'x') ? 0 : MAP_BLOOM_CORE) | ((env_runs && env_runs[0] == '0') ? 0 : MAP_RUNS);
    for (;;) {
        const size_t bytes = ((size_t)1 << bits) / 8;
        SP_HIP(ctx, hipMemsetAsync(ctx->d_bloom, 0, bytes, ctx->stream));
        ctx->bloom_bits = bits | mode;
        if (n == 0) break;
        SP_LAUNCH(ctx, "k4_pair_filter", k4_pair_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_keys, n,
                  ctx->k, ctx->d_bloom, bits | mode);
        if (bits >= MAP_BLOOM_MAX_BITS || cached) break;
        SP_HIP(ctx, hipMemsetAsync(d_small, 0, 8, ctx->stream));
        SP_LAUNCH(ctx, "k4_filter_fill", k4_filter_fill, dim3(256), dim3(256), 0, (const uint32_t *)ctx->d_bloom,
                  (int64_t)(bytes / 4), d_small);
        unsigned long long set = 0;
        SP_HIP(ctx, hipMemcpyAsync(&set, d_small, 8, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double fill = (double)set / (double)((int64_t)1 << bits);
        if (getenv("SP_DEBUG_FILTER")) fprintf(stderr, "[sp] pair filter: 2^%d bits, fill %.3f (n=%lld)\n", bits, fill, (long long)n);
        if (fill <= MAP_FILL_MAX) break;
        bits++;
    }
    ctx->bloom_last_n = n;
    ctx->bloom_last_bits = bits;
    ctx->bloom_last_k = ctx->k;
    return SP_OK;
}

// ----------------------------------------------------------------- dispatch
// The ONE place that turns the kind of a k <= 15 label table into its walker (map_planes_of<TABLE> / map_hits_of, sp_map.h):
// `dense` is a mode's launcher, a generic lambda over the walker; the k > 15 kinds go on to `sparse`, the same mode's
// launcher in sp_sparse.hip, beside their kernels.
template <typename F, typename G>
static int map_with_walker(sp_ctx *ctx, F &&dense, G &&sparse) {
    switch (ctx->labels.kind) {
    case SP_LABELS_COMPACT: return dense(map_planes_of<1>{});
    case SP_LABELS_DIRECT: return dense(map_planes_of<0>{});
    case SP_LABELS_LABEL_BYTES: return dense(map_hits_of{});
    default: return sparse();
    }
}

// bins mode, one chromosome: the planes walkers queue it in `hd` (every chromosome in ONE launch: map_bins_flush), the
// other kinds launch here
static int map_bins_launch(sp_ctx *ctx, sp_chrom &c, const sp_map_params &P, int *d_counts, unsigned long long *d_n,
                           std::vector<map_chrom_desc> &hd, int64_t &hd_ranges) {
    if (P.n_units == 0) return SP_OK;
    const int64_t n_ranges = (P.n_units + MAP_BLOCK - 1) / MAP_BLOCK;
    return map_with_walker(ctx, [&](auto w) -> int {
        if constexpr (decltype(w)::planes) {
            hd.push_back(map_chrom_desc{c.d_pk, c.d_pm, c.d_nm, P.n_units, P.nslots, hd_ranges, d_counts, d_n});
            hd_ranges += n_ranges;
        } else {
            SP_LAUNCH(ctx, "k5_map_lab", k5_map_lab, dim3((unsigned)map_grid(ctx, n_ranges)), dim3(MAP_BLOCK), 0, c.d_pk, c.d_nm,
                      sp_make_kparams32(ctx->k), P, ctx->d_label, ctx->d_bloom, ctx->bloom_bits, d_counts, d_n);
        }
        return SP_OK;
    }, [&] { return sp_sparse_map_launch(ctx, c, P, d_counts, d_n); });
}

// the descriptors of the queued chromosomes -> device, then the one launch
static int map_bins_flush(sp_ctx *ctx, const std::vector<map_chrom_desc> &hd, int64_t n_ranges, const sp_map_params &P) {
    if (n_ranges <= 0) return SP_OK;      // (nothing queued: no planes walker, or no units)
    int rcb = sp_buf_ensure(ctx, ctx->b_mapdesc, (int64_t)(hd.size() * sizeof(map_chrom_desc)));
    if (rcb) return rcb;
    // (pageable source: hipMemcpyAsync returns once the runtime has staged it, `hd` may die afterwards)
    SP_HIP(ctx, hipMemcpyAsync(ctx->b_mapdesc.p, hd.data(), hd.size() * sizeof(map_chrom_desc), hipMemcpyHostToDevice,
                              ctx->stream));
    return map_with_walker(ctx, [&](auto w) -> int {
        if constexpr (decltype(w)::planes)      // (only the planes walkers queue anything)
            SP_LAUNCH(ctx, "k5_map", k5_map2<decltype(w)::table>, dim3((unsigned)map_grid(ctx, n_ranges)), dim3(MAP_BLOCK), 0,
                      (const map_chrom_desc *)ctx->b_mapdesc.p, (int)hd.size(), n_ranges, sp_make_kparams32(ctx->k), P, map_ptab_of(ctx),
                      (const uint32_t *)ctx->d_bloom, ctx->bloom_bits);
        return SP_OK;
    }, [] { return SP_OK; });
}

// feature mode: one packed sequence of features
static int map_feat_launch(sp_ctx *ctx, const uint32_t *d_pk, const uint32_t *d_pm, const uint32_t *d_nm, int64_t n_units,
                           const int64_t *d_foff, int64_t n_feat, int S, unsigned long long *d_counts) {
    const sp_kparams32 kp = sp_make_kparams32(ctx->k);
    const int64_t grid = map_grid(ctx, (n_units + MAP_BLOCK - 1) / MAP_BLOCK);
    return map_with_walker(ctx, [&](auto w) -> int {
        if constexpr (decltype(w)::planes)
            SP_LAUNCH(ctx, "k5_map_feat", k5_map_feat2<decltype(w)::table>, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, d_pk, d_pm, d_nm,
                      kp, n_units, d_foff, n_feat, S, map_ptab_of(ctx), (const uint32_t *)ctx->d_bloom, ctx->bloom_bits, d_counts);
        else
            SP_LAUNCH(ctx, "k5_map_feat_lab", k5_map_feat_lab, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, d_pk, d_nm, kp, n_units,
                      d_foff, n_feat, S, ctx->d_label, (const uint32_t *)ctx->d_bloom, ctx->bloom_bits, d_counts);
        return SP_OK;
    }, [&] { return sp_sparse_feat_launch(ctx, d_pk, d_pm, d_nm, n_units, d_foff, n_feat, S, d_counts); });
}

// interval mode: the per-unit subgenome masks of one chromosome
static int map_mask_launch(sp_ctx *ctx, sp_chrom &c, int64_t n_units, int S, const unsigned long long *d_cov,
                           unsigned long long *d_masks) {
    const sp_kparams32 kp = sp_make_kparams32(ctx->k);
    const int64_t grid = map_grid(ctx, (n_units + MAP_BLOCK - 1) / MAP_BLOCK);
    return map_with_walker(ctx, [&](auto w) -> int {
        if constexpr (decltype(w)::planes)
            SP_LAUNCH(ctx, "k5_map_mask", k5_map_mask2<decltype(w)::table>, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, c.d_pk, c.d_pm,
                      c.d_nm, kp, n_units, S, map_ptab_of(ctx), (const uint32_t *)ctx->d_bloom, ctx->bloom_bits, d_cov, d_masks);
        else
            SP_LAUNCH(ctx, "k5_map_mask_lab", k5_map_mask_lab, dim3((unsigned)grid), dim3(MAP_BLOCK), 0, c.d_pk, c.d_nm, kp, n_units,
                      S, ctx->d_label, (const uint32_t *)ctx->d_bloom, ctx->bloom_bits, d_cov, d_masks);
        return SP_OK;
    }, [&] { return sp_sparse_mask_launch(ctx, c, n_units, S, d_cov, d_masks); });
}

// the labelled k-mers a walk has marked "seen"
static int map_hit_launch(sp_ctx *ctx, unsigned long long *d_n) {
    const unsigned long long *d_keys = (const unsigned long long *)ctx->b_labkeys.p;
    switch (ctx->labels.kind) {
    case SP_LABELS_COMPACT:
        if (ctx->n_labels > 0)
            SP_LAUNCH(ctx, "k4_ctab_seen", k4_ctab_seen, dim3((unsigned)(ctx->n_cu * 4)), dim3(256), 0, d_keys, ctx->n_labels,
                      ctx->k, map_ptab_of(ctx), d_n);
        return SP_OK;
    case SP_LABELS_DIRECT:
        if (ctx->n_labels > 0)
            SP_LAUNCH(ctx, "k4_pair_seen", k4_pair_seen, dim3((unsigned)(ctx->n_cu * 4)), dim3(256), 0, d_keys, ctx->n_labels,
                      ctx->k, (const uint32_t *)ctx->b_ptab.p, d_n);
        return SP_OK;
    case SP_LABELS_LABEL_BYTES:
        SP_LAUNCH(ctx, "k4_count_seen", k4_count_seen, dim3((unsigned)(ctx->n_cu * 8)), dim3(256), 0,
                  (const uint8_t *)ctx->d_label, ctx->nslots, d_n);
        return SP_OK;
    default:
        return sp_sparse_hit(ctx, d_n);
    }
}

// ----------------------------------------------------------------- sp_labels_set
// k <= 15: the planned table from the staged keys.  `table_clean`: the direct table holds nothing (its previous set was
// un-built key by key).
static int labels_build_dense(sp_ctx *ctx, const sp_label_plan &plan, const unsigned long long *d_keys, const uint8_t *d_sg,
                              int64_t n, bool table_clean, unsigned long long *d_flags) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    int rc;
    switch (plan.kind) {
    case SP_LABELS_COMPACT:
        if ((rc = sp_buf_ensure(ctx, ctx->b_ctab, plan.bucket_bytes))) return rc;
        if ((rc = sp_buf_ensure(ctx, ctx->b_covf, plan.ovf_bytes))) return rc;
        SP_HIP(ctx, hipMemsetAsync(ctx->b_ctab.p, 0, (size_t)plan.bucket_bytes, ctx->stream));
        SP_HIP(ctx, hipMemsetAsync(ctx->b_covf.p, 0, (size_t)plan.ovf_bytes, ctx->stream));
        if (n > 0)      // d_flags[2] = overflow table full, [3] = keys in the overflow table
            SP_LAUNCH(ctx, "k4_ctab_build", k4_ctab_build, dim3(grid), dim3(256), 0, d_keys, d_sg, n, ctx->k, map_ptab_of(ctx),
                      d_flags + 2);
        return SP_OK;
    case SP_LABELS_DIRECT:
        if ((rc = sp_buf_ensure(ctx, ctx->b_ptab, plan.entries * 4))) return rc;
        if (!table_clean) SP_HIP(ctx, hipMemsetAsync(ctx->b_ptab.p, 0, (size_t)plan.entries * 4, ctx->stream));
        if (n > 0)
            SP_LAUNCH(ctx, "k4_pair_table", k4_pair_table, dim3(grid), dim3(256), 0, d_keys, d_sg, n, ctx->k,
                      (uint32_t *)ctx->b_ptab.p);
        ctx->ptab_k = ctx->k;
        ctx->ptab_n = n;
        return SP_OK;
    default:      // SP_LABELS_LABEL_BYTES
        if (!ctx->d_label) SP_HIP(ctx, hipMalloc(&ctx->d_label, (size_t)ctx->nslots));
        SP_HIP(ctx, hipMemsetAsync(ctx->d_label, 0, (size_t)ctx->nslots, ctx->stream));
        if (n > 0)
            SP_LAUNCH(ctx, "k4_labels", k4_labels, dim3(grid), dim3(256), 0, d_keys, d_sg, n, sp_make_kparams(ctx->k), ctx->d_label);
        return SP_OK;
    }
}

// the plan becomes the context's label state (not ready yet), then its table is built
static int labels_build(sp_ctx *ctx, const sp_label_plan &plan, const unsigned long long *d_keys, const uint8_t *d_sg, int64_t n,
                        bool table_clean, unsigned long long *d_flags) {
    ctx->labels.kind = plan.kind;
    ctx->labels.bb = plan.bb;
    ctx->labels.ovf_mask = plan.ovf_n ? (uint64_t)(plan.ovf_n - 1) : 0;
    return ctx->sparse_mode ? sp_sparse_labels_build(ctx, plan, d_keys, d_sg, n, d_flags)
                            : labels_build_dense(ctx, plan, d_keys, d_sg, n, table_clean, d_flags);
}

extern "C" {

static int labels_set_impl(sp_ctx *ctx, const uint64_t *keys, const uint8_t *sg, int64_t n, int n_sg, bool on_device) {
    if (!ctx || n < 0 || (n > 0 && (!keys || !sg)) || n_sg < 1 || n_sg > 126)
        return sp_fail(ctx, SP_EINVAL, "sp_labels_set: bad arguments");
    if (ctx->k <= 0 || (ctx->nslots <= 0 && !ctx->sparse_mode))
        return sp_fail(ctx, SP_EINVAL, "sp_labels_set: call sp_count first (it fixes k)");
    SP_HIP(ctx, hipSetDevice(ctx->device));
    // device flags of this call: [0] largest label (device hand-over), [2] bucket table: overflow table full,
    // [3] keys in the overflow table.  They reach the host through k4_flags_out.
    int rc = sp_buf_ensure(ctx, ctx->b_lflags, 64);
    if (rc) return rc;
    unsigned long long *d_flags = (unsigned long long *)ctx->b_lflags.p;
    if (!ctx->h_lflags) SP_HIP(ctx, hipHostMalloc((void **)&ctx->h_lflags, 64, hipHostMallocDefault));
    SP_HIP(ctx, hipMemsetAsync(d_flags, 0, 64, ctx->stream));
    auto flags_out = [&]() -> int {
        SP_LAUNCH(ctx, "k4_flags_out", k4_flags_out, dim3(1), dim3(64), 0, (const unsigned long long *)d_flags, ctx->h_lflags);
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (on_device && n > 0 && (int)(unsigned int)ctx->h_lflags[0] >= n_sg)
            return sp_fail(ctx, SP_EINVAL, "sp_labels_set: label %d >= n_sg %d", (int)(unsigned int)ctx->h_lflags[0], n_sg);
        return SP_OK;
    };
    // the largest label is checked BEFORE any table is touched: a bad set must leave the previous one intact -- and must
    // not leave labels >= n_sg in the hashed tables of k > 15.  Labels handed over in device memory cost one more round
    // trip of the 64-byte flag block for that (~20 us).
    if (on_device && n > 0) {
        SP_LAUNCH(ctx, "k4_label_max", k4_label_max, dim3((unsigned)(n < 65536 ? 1 : ctx->n_cu)), dim3(256), 0, sg, n, (unsigned int *)d_flags);
        if ((rc = flags_out())) return rc;
    } else {
        uint8_t mx = 0;     // (a reduction the compiler vectorises; an early-exit loop over 2 M labels took 1 ms)
        for (int64_t i = 0; i < n; i++) mx = sg[i] > mx ? sg[i] : mx;
        if (n > 0 && mx >= n_sg) return sp_fail(ctx, SP_EINVAL, "sp_labels_set: label %d >= n_sg %d", (int)mx, n_sg);
    }
    sp_label_plan plan = sp_label_plan_make(ctx->k, n, n_sg, ctx->nslots, sp_label_env_read());
    ctx->labels.ready = false;
    sp_map_table_drop(ctx);      // the columns of sp_map_bins_all's table were the previous set's subgenomes
    ctx->n_sg = n_sg;
    ctx->n_labels = n;
    // direct table: the previous label set (same k, same buffer) is un-built key by key instead of memset -- while its
    // keys are still in b_labkeys
    bool table_clean = false;
    if (plan.kind == SP_LABELS_DIRECT && ctx->ptab_k == ctx->k && ctx->b_ptab.p && ctx->b_ptab.cap >= plan.entries * 4) {
        if (ctx->ptab_n > 0)
            SP_LAUNCH(ctx, "k4_pair_clear", k4_pair_clear, dim3((unsigned)((ctx->ptab_n + 255) / 256)), dim3(256), 0,
                      (const unsigned long long *)ctx->b_labkeys.p, ctx->ptab_n, ctx->k, (uint32_t *)ctx->b_ptab.p);
        table_clean = true;
    }
    ctx->ptab_k = 0;      // (from here on the direct table is in an unknown state unless it is rebuilt below)
    ctx->ptab_n = 0;
    // the labelled keys stay on the device: the filter is built from them, sp_labels_hit walks them, the next call un-builds
    // the direct table with them
    const int64_t n1 = n > 0 ? n : 1;
    if ((rc = sp_buf_ensure(ctx, ctx->b_labkeys, n1 * 9 + 64))) return rc;
    unsigned long long *d_keys = (unsigned long long *)ctx->b_labkeys.p;
    uint8_t *d_sg = (uint8_t *)(d_keys + n1);
    if (n > 0 && (const void *)keys != (const void *)d_keys) {
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        SP_HIP(ctx, hipMemcpyAsync(d_keys, keys, (size_t)n * 8, kind, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(d_sg, sg, (size_t)n, kind, ctx->stream));
    }
    if ((rc = labels_build(ctx, plan, d_keys, d_sg, n, table_clean, d_flags))) return rc;
    if ((rc = sp_map_filter_build(ctx, n > 0 ? d_keys : nullptr, n))) return rc;
    if ((rc = flags_out())) return rc;
    if (plan.bb && n > 0) {
        if (getenv("SP_DEBUG_FILTER") && plan.kind == SP_LABELS_COMPACT)
            fprintf(stderr, "[sp] compact pair table: 2^%d buckets, %llu entries in the overflow table (%lld labelled k-mers)\n",
                    plan.bb, ctx->h_lflags[3], (long long)n);
        if (getenv("SP_DEBUG_FILTER") && plan.kind == SP_LABELS_QUAD)
            fprintf(stderr, "[sp] quad-bucket table (k > 15): 2^%d buckets, %llu entries in the overflow table (%lld labelled k-mers)\n",
                    plan.bb, ctx->h_lflags[3], (long long)n);
        if (ctx->h_lflags[2]) {          // overflow table full (adversarial key sets only): the plain table takes over
            plan = sp_label_plan_fallback(plan, n);
            if ((rc = labels_build(ctx, plan, d_keys, d_sg, n, false, d_flags))) return rc;
            SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    ctx->labels.ready = true;
    return SP_OK;
}

int sp_labels_set(sp_ctx *ctx, const uint64_t *keys, const uint8_t *sg, int64_t n, int n_sg) {
    return labels_set_impl(ctx, keys, sg, n, n_sg, false);
}

int sp_labels_set_device(sp_ctx *ctx, const uint64_t *d_keys, const uint8_t *d_sg, int64_t n, int n_sg) {
    return labels_set_impl(ctx, d_keys, d_sg, n, n_sg, true);
}

int sp_map_nslots(sp_ctx *ctx, int chrom, int64_t bin_size, int64_t chunk_size, int64_t *nslots) {
    if (!ctx || !nslots || chrom < 0 || chrom >= (int)ctx->chroms.size() || bin_size < 1 || chunk_size < 0)
        return sp_fail(ctx, SP_EINVAL, "sp_map_nslots: bad arguments");
    *nslots = map_nslots_host(ctx->chroms[(size_t)chrom].len, bin_size, chunk_size, ctx->k);
    return SP_OK;
}

int sp_map_bins(sp_ctx *ctx, int chrom, int64_t bin_size, int64_t chunk_size, int32_t *slot_counts,
                int64_t nslots, int64_t *n_mapped) {
    if (!ctx || !slot_counts || chrom < 0 || chrom >= (int)ctx->chroms.size() || bin_size < 1 ||
        chunk_size < 0)
        return sp_fail(ctx, SP_EINVAL, "sp_map_bins: bad arguments");
    if (map_need_labels(ctx, "sp_map_bins")) return SP_EINVAL;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_chrom &c = ctx->chroms[(size_t)chrom];
    const int S = ctx->n_sg;
    int64_t need = map_nslots_host(c.len, bin_size, chunk_size, ctx->k);
    if (nslots < need) return sp_fail(ctx, SP_EINVAL, "sp_map_bins: nslots %lld < %lld", (long long)nslots, (long long)need);
    const size_t bytes = (size_t)nslots * S * sizeof(int);
    const size_t bytes8 = (bytes + 7) & ~(size_t)7;
    sp_map_table_drop(ctx);      // b_map is re-used
    int rcb = sp_buf_ensure(ctx, ctx->b_map, (int64_t)bytes8 + 8);
    if (rcb) return rcb;
    int *d_counts = (int *)ctx->b_map.p;
    unsigned long long *d_n = (unsigned long long *)((char *)d_counts + bytes8);
    SP_HIP(ctx, hipMemsetAsync(d_counts, 0, bytes8 + 8, ctx->stream));
    const sp_map_params P = map_params_of(c.len, bin_size, chunk_size, nslots, S);
    std::vector<map_chrom_desc> hd;
    int64_t hd_ranges = 0;
    int rcl = map_bins_launch(ctx, c, P, d_counts, d_n, hd, hd_ranges);
    if (!rcl) rcl = map_bins_flush(ctx, hd, hd_ranges, P);
    if (rcl) return rcl;
    unsigned long long hn = 0;
    SP_HIP(ctx, hipMemcpyAsync(slot_counts, d_counts, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(&hn, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_mapped) *n_mapped = (int64_t)hn;
    return SP_OK;
}

int sp_map_bins_all(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, const int64_t *slot_off,
                    int32_t *slot_counts, int64_t *n_mapped) {
    if (!ctx || !slot_off || !slot_counts || bin_size < 1 || chunk_size < 0)
        return sp_fail(ctx, SP_EINVAL, "sp_map_bins_all: bad arguments");
    if (map_need_labels(ctx, "sp_map_bins_all")) return SP_EINVAL;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const int C = (int)ctx->chroms.size();
    const int S = ctx->n_sg;
    for (int i = 0; i < C; i++) {
        int64_t need = map_nslots_host(ctx->chroms[(size_t)i].len, bin_size, chunk_size, ctx->k);
        if (slot_off[i + 1] - slot_off[i] < need)
            return sp_fail(ctx, SP_EINVAL, "sp_map_bins_all: chromosome %d needs %lld slots", i, (long long)need);
    }
    const int64_t total = slot_off[C];
    const size_t bytes = (size_t)total * S * sizeof(int);
    const size_t bytes8 = (bytes + 7) & ~(size_t)7;
    sp_map_table_drop(ctx);
    int rcb = sp_buf_ensure(ctx, ctx->b_map, (int64_t)(bytes8 + 8 * (size_t)C));
    if (rcb) return rcb;
    int *d_counts = (int *)ctx->b_map.p;
    unsigned long long *d_n = (unsigned long long *)((char *)d_counts + bytes8);
    SP_HIP(ctx, hipMemsetAsync(d_counts, 0, bytes8 + 8 * (size_t)C, ctx->stream));
    std::vector<map_chrom_desc> hd;     // pair-table kinds: every chromosome in ONE launch
    int64_t hd_ranges = 0;
    for (int i = 0; i < C; i++) {
        const sp_map_params P = map_params_of(ctx->chroms[(size_t)i].len, bin_size, chunk_size, slot_off[i + 1] - slot_off[i], S);
        int rcl = map_bins_launch(ctx, ctx->chroms[(size_t)i], P, d_counts + slot_off[i] * S, d_n + i, hd, hd_ranges);
        if (rcl) return rcl;
    }
    int rcl = map_bins_flush(ctx, hd, hd_ranges, map_params_of(0, bin_size, chunk_size, 0, S));
    if (rcl) return rcl;
    SP_HIP(ctx, hipMemcpyAsync(slot_counts, d_counts, bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<unsigned long long> hn((size_t)C, 0);
    SP_HIP(ctx, hipMemcpyAsync(hn.data(), d_n, 8 * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_mapped)
        for (int i = 0; i < C; i++) n_mapped[i] = (int64_t)hn[(size_t)i];
    // b_map holds the slot counts of every chromosome: what the stack entries must be told again
    ctx->map_table.bin_size = bin_size;
    ctx->map_table.chunk_size = chunk_size;
    ctx->map_table.n_sg = S;
    ctx->map_table.k = ctx->k;
    ctx->map_table.slot_off.assign(slot_off, slot_off + C + 1);
    ctx->map_table.valid = true;
    return SP_OK;
}

// The stack entries read the table sp_map_bins_all left in b_map, with the caller's description of it: a description
// that differs from the one the table was made with is refused before anything is launched (a larger bin_size alone
// would put windows behind the caller's table).
static int stack_need_table(sp_ctx *ctx, const char *entry, int64_t bin_size, int64_t chunk_size, const int64_t *slot_off) {
    const sp_ctx::map_table_t &T = ctx->map_table;
    if (!T.valid) return sp_fail(ctx, SP_EINVAL, "%s: call sp_map_bins_all first", entry);
    const int C = (int)ctx->chroms.size();
    if ((size_t)C + 1 != T.slot_off.size())
        return sp_fail(ctx, SP_EINVAL, "%s: %d chromosomes, sp_map_bins_all mapped %d", entry, C, (int)T.slot_off.size() - 1);
    if (ctx->n_sg != T.n_sg || ctx->k != T.k)
        return sp_fail(ctx, SP_EINVAL, "%s: n_sg %d, k %d, sp_map_bins_all mapped with n_sg %d, k %d", entry, ctx->n_sg, ctx->k,
                       T.n_sg, T.k);
    if (bin_size != T.bin_size)
        return sp_fail(ctx, SP_EINVAL, "%s: bin_size %lld, sp_map_bins_all mapped with %lld", entry, (long long)bin_size,
                       (long long)T.bin_size);
    if (chunk_size != T.chunk_size)
        return sp_fail(ctx, SP_EINVAL, "%s: chunk_size %lld, sp_map_bins_all mapped with %lld", entry, (long long)chunk_size,
                       (long long)T.chunk_size);
    for (int i = 0; i <= C; i++)
        if (slot_off[i] != T.slot_off[(size_t)i])
            return sp_fail(ctx, SP_EINVAL, "%s: slot_off[%d] = %lld, sp_map_bins_all mapped with %lld", entry, i,
                           (long long)slot_off[i], (long long)T.slot_off[(size_t)i]);
    return SP_OK;
}

// window stack into a DEVICE table (accumulated: the caller clears it).  Entry i of slot_off / win_off /
// seg_start describes local chromosome (or chromosome segment) i: its slots in the table sp_map_bins_all left
// behind, the first window row of the chromosome it belongs to, and where its base 0 lies in that chromosome.
int sp_stack_windows_dev(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, int64_t window_size, const int64_t *slot_off,
                         const int64_t *win_off, const int64_t *seg_start, void *d_win) {
    if (!ctx || !slot_off || !win_off || !d_win || bin_size < 1 || chunk_size < 0 || window_size < 1)
        return sp_fail(ctx, SP_EINVAL, "sp_stack_windows_dev: bad arguments");
    if (stack_need_table(ctx, "sp_stack_windows_dev", bin_size, chunk_size, slot_off)) return SP_EINVAL;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    const int C = (int)ctx->chroms.size();
    const int S = ctx->n_sg;
    const int64_t total_slots = slot_off[C];
    int rcb = sp_buf_ensure(ctx, ctx->b_win, (int64_t)(24 * (size_t)(C + 1)));
    if (rcb) return rcb;
    long long *d_soff = (long long *)ctx->b_win.p;
    long long *d_woff = d_soff + (C + 1), *d_seg = d_woff + (C + 1);
    SP_HIP(ctx, hipMemcpyAsync(d_soff, slot_off, 8 * (size_t)(C + 1), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_woff, win_off, 8 * (size_t)C, hipMemcpyHostToDevice, ctx->stream));
    if (seg_start) SP_HIP(ctx, hipMemcpyAsync(d_seg, seg_start, 8 * (size_t)C, hipMemcpyHostToDevice, ctx->stream));
    if (total_slots > 0)
        SP_LAUNCH(ctx, "k5_stack", k5_stack, dim3((unsigned)((total_slots * S + 255) / 256)), dim3(256), 0,
                  (const int *)ctx->b_map.p, total_slots, S, C, d_soff, d_woff, seg_start ? d_seg : (long long *)nullptr,
                  bin_size, chunk_size, window_size, ctx->k, (unsigned long long *)d_win);
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // slot_off / win_off are the caller's
    return SP_OK;
}

static int stack_check(sp_ctx *ctx, int64_t window_size, const int64_t *win_off) {
    const int C = (int)ctx->chroms.size();
    for (int i = 0; i < C; i++) {
        int64_t need = (ctx->chroms[(size_t)i].len + window_size - 1) / window_size + 1;
        if (win_off[i + 1] - win_off[i] < need)
            return sp_fail(ctx, SP_EINVAL, "sp_stack_windows: chromosome %d needs %lld windows", i, (long long)need);
    }
    return SP_OK;
}

int sp_stack_windows(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, int64_t window_size,
                     const int64_t *slot_off, const int64_t *win_off, int64_t *win_counts) {
    if (!ctx || !slot_off || !win_off || !win_counts || bin_size < 1 || chunk_size < 0 || window_size < 1)
        return sp_fail(ctx, SP_EINVAL, "sp_stack_windows: bad arguments");
    if (stack_need_table(ctx, "sp_stack_windows", bin_size, chunk_size, slot_off)) return SP_EINVAL;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = stack_check(ctx, window_size, win_off);
    if (rc) return rc;
    const int C = (int)ctx->chroms.size();
    const size_t wbytes = (size_t)win_off[C] * ctx->n_sg * 8;
    rc = sp_buf_ensure(ctx, ctx->b_wtab, (int64_t)wbytes + 64);
    if (rc) return rc;
    SP_HIP(ctx, hipMemsetAsync(ctx->b_wtab.p, 0, wbytes, ctx->stream));
    rc = sp_stack_windows_dev(ctx, bin_size, chunk_size, window_size, slot_off, win_off, nullptr, ctx->b_wtab.p);
    if (rc) return rc;
    SP_HIP(ctx, hipMemcpyAsync(win_counts, ctx->b_wtab.p, wbytes, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

// map -> stack -> enrich without leaving the device: the window table is built in HBM, the column totals are
// reduced there, every window row (empty ones included: they change no total) is tested, and the table and the
// decisions come back in one go.  The caller keeps the rows that have any count (Circos.py:734-742).
int sp_stack_enrich(sp_ctx *ctx, int64_t bin_size, int64_t chunk_size, int64_t window_size, const int64_t *slot_off,
                    const int64_t *win_off, double max_pval, double min_ratio, int64_t *win_counts, double *pvals,
                    int32_t *argmin, uint8_t *sig, double *ratios) {
    if (!ctx || !slot_off || !win_off || !win_counts || !pvals || !argmin || !sig || !ratios || bin_size < 1 ||
        chunk_size < 0 || window_size < 1)
        return sp_fail(ctx, SP_EINVAL, "sp_stack_enrich: bad arguments");
    if (stack_need_table(ctx, "sp_stack_enrich", bin_size, chunk_size, slot_off)) return SP_EINVAL;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = stack_check(ctx, window_size, win_off);
    if (rc) return rc;
    const int C = (int)ctx->chroms.size();
    const int64_t W = win_off[C];
    const size_t wbytes = (size_t)W * ctx->n_sg * 8;
    rc = sp_buf_ensure(ctx, ctx->b_wtab, (int64_t)wbytes + 64);
    if (rc) return rc;
    SP_HIP(ctx, hipMemsetAsync(ctx->b_wtab.p, 0, wbytes, ctx->stream));
    rc = sp_stack_windows_dev(ctx, bin_size, chunk_size, window_size, slot_off, win_off, nullptr, ctx->b_wtab.p);
    if (rc) return rc;
    SP_HIP(ctx, hipMemcpyAsync(win_counts, ctx->b_wtab.p, wbytes, hipMemcpyDeviceToHost, ctx->stream));
    return sp_enrich_dev(ctx, ctx->b_wtab.p, W, ctx->n_sg, max_pval, min_ratio, pvals, argmin, sig, ratios);
}

int sp_map_features(sp_ctx *ctx, const uint8_t *ascii, const int64_t *off, int64_t n_feat,
                    int64_t *counts) {
    if (!ctx || !off || !counts || n_feat < 0 || (n_feat > 0 && off[n_feat] > 0 && !ascii))
        return sp_fail(ctx, SP_EINVAL, "sp_map_features: bad arguments");
    if (map_need_labels(ctx, "sp_map_features")) return SP_EINVAL;
    const int S = ctx->n_sg;
    memset(counts, 0, (size_t)n_feat * S * sizeof(int64_t));
    if (n_feat == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    // the features are uploaded as they lie in the caller's buffer (back to back); the kernel rejects
    // k-mers that run across a feature boundary, so no separator copy is needed on the host
    const int64_t base = off[0], total = off[n_feat] - off[0];
    std::vector<int64_t> foff((size_t)n_feat + 1);
    for (int64_t f = 0; f <= n_feat; f++) {
        if (f > 0 && off[f] < off[f - 1]) return sp_fail(ctx, SP_EINVAL, "sp_map_features: offsets must be non-decreasing");
        foff[(size_t)f] = off[f] - base;
    }
    if (total == 0) return SP_OK;
    sp_tmp<uint8_t> d_ascii;
    sp_tmp<uint32_t> d_pk, d_nm;
    sp_tmp<int64_t> d_foff;
    sp_tmp<unsigned long long> d_counts;
    int64_t nmw = (total + 31) / 32 + SP_PAD_WORDS;
    SP_HIP(ctx, d_ascii.alloc((size_t)total));
    SP_HIP(ctx, d_pk.alloc((size_t)(4 * nmw)));   // LSB-first | MSB-first
    SP_HIP(ctx, d_nm.alloc((size_t)nmw));
    SP_HIP(ctx, d_foff.alloc((size_t)(n_feat + 1)));
    SP_HIP(ctx, d_counts.alloc((size_t)n_feat * S));
    SP_HIP(ctx, hipMemcpyAsync(d_ascii, ascii + base, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_foff, foff.data(), (size_t)(n_feat + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)n_feat * S * 8, ctx->stream));
    int64_t blocks = (nmw + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    SP_LAUNCH(ctx, "k0_pack", k0_pack, dim3((unsigned)blocks), dim3(256), 0, (const uint8_t *)d_ascii.p, total, d_pk.p,
              d_pk.p + 2 * nmw, d_nm.p, nmw);
    int64_t n_units = (total + SP_UNIT - 1) / SP_UNIT;
    int rcl = map_feat_launch(ctx, d_pk.p, d_pk.p + 2 * nmw, d_nm.p, n_units, d_foff.p, n_feat, S, d_counts.p);
    if (rcl) return rcl;
    SP_HIP(ctx, hipMemcpyAsync(counts, d_counts, (size_t)n_feat * S * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_map_intervals(sp_ctx *ctx, const int32_t *chrom, const int64_t *start, const int64_t *end, int64_t n,
                     int64_t *counts) {
    if (!ctx || n < 0 || (n > 0 && (!chrom || !start || !end || !counts)))
        return sp_fail(ctx, SP_EINVAL, "sp_map_intervals: bad arguments");
    if (map_need_labels(ctx, "sp_map_intervals")) return SP_EINVAL;
    const int C = (int)ctx->chroms.size(), S = ctx->n_sg, k = ctx->k;
    for (int64_t i = 0; i < n; i++) {
        if (chrom[i] < 0 || chrom[i] >= C) return sp_fail(ctx, SP_EINVAL, "sp_map_intervals: interval %lld: chromosome %d out of range", (long long)i, chrom[i]);
        if (start[i] < 0 || end[i] < start[i] || end[i] > ctx->chroms[(size_t)chrom[i]].len)
            return sp_fail(ctx, SP_EINVAL, "sp_map_intervals: interval %lld = [%lld, %lld) outside chromosome %d (%lld bases)",
                           (long long)i, (long long)start[i], (long long)end[i], chrom[i], (long long)ctx->chroms[(size_t)chrom[i]].len);
    }
    if (n == 0) return SP_OK;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int64_t> ubase((size_t)C + 1, 0);
    for (int c = 0; c < C; c++) ubase[(size_t)c + 1] = ubase[(size_t)c] + (ctx->chroms[(size_t)c].len + SP_UNIT - 1) / SP_UNIT + 1;
    const int64_t total_units = ubase[(size_t)C];
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_cov = 0, o_masks = al((size_t)total_units * 8), o_ub = o_masks + al((size_t)total_units * S * 8),
                 o_ch = o_ub + al((size_t)(C + 1) * 8), o_st = o_ch + al((size_t)n * 4), o_en = o_st + al((size_t)n * 8),
                 o_cnt = o_en + al((size_t)n * 8), bytes = o_cnt + al((size_t)n * S * 8);
    int rc = sp_buf_ensure(ctx, ctx->b_ival, (int64_t)bytes);
    if (rc) return rc;
    char *B = (char *)ctx->b_ival.p;
    unsigned long long *d_cov = (unsigned long long *)(B + o_cov), *d_masks = (unsigned long long *)(B + o_masks),
                       *d_counts = (unsigned long long *)(B + o_cnt);
    int64_t *d_ub = (int64_t *)(B + o_ub), *d_st = (int64_t *)(B + o_st), *d_en = (int64_t *)(B + o_en);
    int32_t *d_ch = (int32_t *)(B + o_ch);
    SP_HIP(ctx, hipMemsetAsync(B, 0, o_ub, ctx->stream));      // coverage + masks
    SP_HIP(ctx, hipMemcpyAsync(d_ub, ubase.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_ch, chrom, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_st, start, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_en, end, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    int64_t gw = (n + 3) / 4;       // four intervals (waves) per block
    if (gw > (int64_t)ctx->n_cu * 32) gw = (int64_t)ctx->n_cu * 32;
    SP_LAUNCH(ctx, "kv_cover", kv_cover, dim3((unsigned)gw), dim3(256), 0, (const int32_t *)d_ch, (const int64_t *)d_st,
              (const int64_t *)d_en, n, k, (const int64_t *)d_ub, d_cov);
    for (int c = 0; c < C; c++) {
        sp_chrom &ch = ctx->chroms[(size_t)c];
        const int64_t n_units = (ch.len + SP_UNIT - 1) / SP_UNIT;
        if (n_units == 0) continue;
        int rcl = map_mask_launch(ctx, ch, n_units, S, d_cov + ubase[(size_t)c], d_masks + ubase[(size_t)c] * S);
        if (rcl) return rcl;
    }
    SP_LAUNCH(ctx, "kv_count", kv_count, dim3((unsigned)gw), dim3(256), 0, (const int32_t *)d_ch, (const int64_t *)d_st,
              (const int64_t *)d_en, n, k, S, (const int64_t *)d_ub, (const unsigned long long *)d_masks, d_counts);
    SP_HIP(ctx, hipMemcpyAsync(counts, d_counts, (size_t)n * S * 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SP_OK;
}

int sp_labels_hit(sp_ctx *ctx, int64_t *n_hit) {
    if (!ctx || !n_hit) return sp_fail(ctx, SP_EINVAL, "sp_labels_hit: bad arguments");
    if (map_need_labels(ctx, "sp_labels_hit")) return SP_EINVAL;
    SP_HIP(ctx, hipSetDevice(ctx->device));
    sp_tmp<unsigned long long> d_n;
    unsigned long long h = 0;
    SP_HIP(ctx, d_n.alloc(1));
    SP_HIP(ctx, hipMemsetAsync(d_n.p, 0, 8, ctx->stream));
    int rcl = map_hit_launch(ctx, d_n.p);
    if (rcl) return rcl;
    SP_HIP(ctx, hipMemcpyAsync(&h, d_n.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_hit = (int64_t)h;
    return SP_OK;
}
}  // extern "C"
