// sp_listfilter.hip -- the list filter: the differential filter over per-chromosome sorted (key, count) lists.  It
// is the filter of k = 16..32, of every engine-3 count at k <= 15 (the keys are dense slots then), of genomes beyond the
// byte-table filter's chromosome limit and of their passenger path.
//
//   sps_filter_join        the C-way hash join: sps_bounds -> sps_join_blk (up to SPS_MAXC lists) / sps_join_wide ->
//                          sps_tally_* -> sps_place_*; its host planning is sp_listplan.h
//   sps_filter_passengers  k <= 15 above SP_LIST_MAXC chromosomes: the join over the set chromosomes, then bitmap
//                          passes over the slot space (sps_sg_*)
//   sps_filter_sort        SP_LIST_FILTER=sort, the cross-check: concatenate -> library radix sort -> sps_eval ->
//                          sps_emit (the one use of rocPRIM here)
//   sp_sparse_filter / sp_sparse_fetch   what sp_filter.hip calls
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "sp_device.h"
#include "sp_filter.h"
#include "sp_internal.h"
#include "sp_lists.h"
#include "sp_listplan.h"

// ------------------------------------------------------------------ filter
__global__ void __launch_bounds__(256)
sps_concat(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts, int64_t n, int chrom,
           unsigned long long *__restrict__ out_keys, unsigned long long *__restrict__ out_vals) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_keys[i] = keys[i];
    out_vals[i] = ((unsigned long long)chrom << 32) | counts[i];
}

struct sps_filter_args {
    int C;
    sp_fsets F;
};

// flags per entry: bit0 = differential row, bit1 = fold-passing (hist), bit2 = head of a run (union)
__global__ void __launch_bounds__(SEL_BLOCK)
sps_eval(const unsigned long long *__restrict__ K, const unsigned long long *__restrict__ V, int64_t n,
         sps_filter_args A, uint8_t *__restrict__ flags, unsigned long long *__restrict__ blk_row,
         unsigned long long *__restrict__ blk_hist, unsigned long long *__restrict__ n_union) {
    __shared__ unsigned long long red[16];
    const int64_t base = (int64_t)blockIdx.x * SEL_SPAN;
    unsigned long long nrow = 0, nhist = 0, nuni = 0;
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        const int64_t i = base + (int64_t)j * SEL_BLOCK + threadIdx.x;
        if (i >= n) continue;
        uint8_t fl = 0;
        const unsigned long long key = K[i];
        if (i == 0 || K[i - 1] != key) {
            uint32_t row[SPS_MAXC];
            for (int c = 0; c < A.C; c++) row[c] = 0;
            unsigned long long tot = 0;
            for (int64_t q = i; q < n && K[q] == key; q++) {
                const unsigned long long v = V[q];
                row[(int)(v >> 32)] = (uint32_t)v;
                tot += (uint32_t)v;
            }
            bool is_row, is_hist;
            sp_filter_decide([&](int c) -> uint32_t { return row[c]; }, tot, A.F, is_row, is_hist);
            fl = 4 | (is_row ? 1 : 0) | (is_hist ? 2 : 0);
            nuni++;
            nrow += is_row;
            nhist += is_hist;
        }
        flags[i] = fl;
    }
    unsigned long long t_row = sp_block_sum_u64(nrow, red);
    unsigned long long t_hist = sp_block_sum_u64(nhist, red);
    unsigned long long t_uni = sp_block_sum_u64(nuni, red);
    if (threadIdx.x == 0) {
        blk_row[blockIdx.x] = t_row;
        blk_hist[blockIdx.x] = t_hist;
        if (t_uni) atomicAdd(n_union, t_uni);
    }
}

__global__ void __launch_bounds__(SEL_BLOCK)
sps_emit(const unsigned long long *__restrict__ K, const unsigned long long *__restrict__ V, int64_t n, int C,
         const uint8_t *__restrict__ flags, uint8_t bit, const unsigned long long *__restrict__ blk,
         unsigned long long *__restrict__ out_keys, uint32_t *__restrict__ out_counts,
         unsigned long long *__restrict__ out_tot) {
    __shared__ uint32_t lds[16];
    const int64_t base = (int64_t)blockIdx.x * SEL_SPAN;
    unsigned long long off = blk[blockIdx.x];
    for (int j = 0; j < SEL_PER_THREAD; j++) {
        const int64_t i = base + (int64_t)j * SEL_BLOCK + threadIdx.x;
        const bool p = (i < n) && (flags[i] & bit);
        uint32_t tot_blk;
        const uint32_t my = sp_block_excl_count(p, lds, tot_blk);
        if (p) {
            const unsigned long long r = off + my, key = K[i];
            unsigned long long tot = 0;
            if (out_counts)
                for (int c = 0; c < C; c++) out_counts[r * C + c] = 0;
            for (int64_t q = i; q < n && K[q] == key; q++) {
                const unsigned long long v = V[q];
                if (out_counts) out_counts[r * C + (int)(v >> 32)] = (uint32_t)v;
                tot += (uint32_t)v;
            }
            if (out_keys) out_keys[r] = key;
            if (out_tot) out_tot[r] = tot;
        }
        off += tot_blk;
    }
}

// engine 3: the rows the list filter emitted carry dense slots; the API speaks canonical k-mers
__global__ void __launch_bounds__(256)
sps_slots_to_keys(unsigned long long *__restrict__ keys, int64_t n, sp_kparams kp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = sp_key_of_slot(keys[i], kp);
}

// ------------------------------------------------------------------ list filter: C-way hash join (round 3)
// The first list filter concatenated the C sorted lists, sorted the concatenation by key with a device-wide library
// radix sort and evaluated runs of equal keys: ~220 bytes of HBM traffic per list entry (27 ms per wheat-like pass at
// k = 17, the worst stage of that line).  The lists are sorted already, so the join needs no global sort:
//   sps_bounds   cuts the key space into 2^rb equal ranges and records where every list crosses every range edge;
//   sps_join     one workgroup per range: the C segments (a few hundred entries together) go to LDS, an LDS hash
//                table groups the entries of equal keys (chain per key, owner = the entry of the lowest chromosome),
//                the owner rebuilds the row and takes the decision (the shared sp_filter_decide).  Fold-passing
//                totals go to a staging array at the position the range has in the virtual concatenation (closed
//                form, no atomics); differential rows -- rare -- go to a row staging area handed out in chunks, each
//                with its rank inside the range (ascending key).  A range with more than BJ_T entries is worked
//                off in rounds of key sub-ranges (pivot = the smallest of the lists' (BJ_T / C)-th pending keys).
//   sps_place_*  scan of the per-range tallies, then rows / totals move to their final, key-ordered places.
// The lists are read once (12 B per entry) plus once for the range edges (8 B).

__global__ void __launch_bounds__(256)
sps_bounds(const sps_list *__restrict__ lists, int shift, long long R, uint32_t *__restrict__ bnd /* C x (R + 1) */) {
    const sps_list L = lists[blockIdx.y];
    uint32_t *b = bnd + (size_t)blockIdx.y * (size_t)(R + 1);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < L.n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = (long long)(L.keys[i] >> shift);
        const long long rp = i ? (long long)(L.keys[i - 1] >> shift) : -1;
        for (long long x = rp + 1; x <= r; x++) b[x] = (uint32_t)i;      // first entry at or beyond the edge of range x
        if (i == L.n - 1)
            for (long long x = r + 1; x <= R; x++) b[x] = (uint32_t)L.n;
    }
}

struct sps_join_args {
    int C, shift;
    long long R;
    sp_fsets F;
    const sps_list *lists;
    const uint32_t *bnd;
    uint32_t *n_rows, *n_hist;            // per range
    unsigned long long *hist_stage;       // [total]: fold-passing totals of range r from the range's first entry on
    unsigned long long *row_cursor;       // rows handed out so far (may exceed row_cap: the surplus is not written)
    unsigned long long row_cap;
    unsigned long long *row_keys, *row_tot;   // row staging: key (all ones = unused), tot, rank inside the range, counts
    uint32_t *row_rank, *row_counts;
    unsigned long long *n_union;
    const unsigned long long *chrom_sets;     // per chromosome: bit s set if it belongs to non-singleton set number s
    int screen;                               // the bit masks are usable (<= 64 non-singleton sets)
    int fast;                                 // every non-singleton set uses baseline 1 or -1 and has no empty unit: the
                                              // uniform fp32 walk of sps_join_blk applies (k3_eval's P.fast)
    const int32_t *rd;                        // its row descriptors: chromosome | JD_UNIT_END | JD_SET_END | JD_BI1, the
    const float *rinv;                        // non-singleton sets in config order; 1 / (unit length) at unit ends, fp32
    int n_rd;
};

// wave-level helpers of the join (wave 0 of a workgroup runs the cursor logic: lane c owns list c)
template <typename T>
__device__ __forceinline__ T jw_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long jw_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o, 64);
        v = x < v ? x : v;
    }
    return v;
}

// ------------------------------------------------------------------ sps_join_blk (round 5): the join, one WORKGROUP per range
// (Rounds 3-4 ran one WAVE per ~100-entry range; that kernel was the `SP_LIST_FILTER=wave` cross-check until round 6 and is gone:
// the independent check of the list filter is `SP_LIST_FILTER=sort`, the device-wide sort + run evaluation.)
// The wave-per-range join read ~90 bytes per list entry for 12 useful ones (PMC, round 4): a range of ~100 entries is
// 21 list segments of ~5 entries -- one or two 64-byte lines of keys and one of counts per segment, used to a tenth --
// plus two strided range-edge words per list and range.  With ranges of ~BJ_T / 1.5 entries (a segment is ~35 entries:
// four lines of keys, used in full) the fixed costs -- edges, cursors, hash clear, the tallies -- are paid once per ~700
// entries instead of once per ~100.  A workgroup of BJ_THREADS takes a range: wave 0 runs the cursor logic of the
// wave kernel (lane c owns list c: pivot, share, offsets by shuffles) and publishes it through LDS, every thread loads
// and hash-inserts BJ_T / BJ_THREADS entries.  Same outputs, same staging protocol (hist totals at the range's
// closed-form position, rows in chunks with their rank inside the range), so sps_tally_* / sps_place_* are unchanged.
//
// Nothing after the hash build walks a chain (second half of round 5).  The first version kept the wave kernel's
// per-key chains: the owner of a key walked them for the screen (set mask, total), again to rebuild its row for the
// decision, again to write a kept row -- dependent LDS reads, ~20 deep for exactly the k-mers that pass the screen, one
// lane busy while 63 wait.  Bound experiments on the peanut-like genome (5.2 ms): no decisions 2.3 ms, nothing after the
// hash build 1.2 ms.  Now every ENTRY works for its owner, all in parallel: it adds its set bit and count to the owner's
// tallies (two LDS atomics), writes its count into the owner's row when the owner is up for a decision or kept, and the
// decision itself is k3_eval's uniform row walk over a descriptor list (chromosome | unit end | set end, reciprocal
// lengths) -- the same instructions in every lane, independent LDS reads.
#define BJ_H (2 * BJ_T)   // hash slots
#ifndef BJ_THREADS
#define BJ_THREADS 256
#endif
#define BJ_WAVES (BJ_THREADS / 64)
#define BJ_Q (BJ_T / BJ_THREADS)
#define BJ_ROWS 16        // rows a wave decides at a time
#define BJ_NR (BJ_WAVES * BJ_ROWS)
// LDS of a workgroup: 31.6 KB + the rows (32-bit residuals) -- FOUR workgroups per CU.  The kernel's time follows its occupancy
// (two / three workgroups per CU: 3.61 / 2.70 ms on the peanut-like genome, 15.3 / 10.9 at wheat-like k = 21), so two tables share
// their space with the two that are dead by the time they are needed: the per-owner totals live where the hash keys were (no key
// is compared after the last insert), the per-owner set masks / queue places / ranks where the slot owners were (every entry
// copies its owner's index into Sl[] first).
template <typename RT>
struct bj_lds {
    alignas(8) RT Hk[BJ_H];               // hash keys; after the inserts: Et[BJ_T], per owner entry the sum of the key's counts
    uint32_t Hmin[BJ_H];                  // per slot: (chromosome << 16 | entry) of the owner; after the owner pass: Es[BJ_T], per
                                          // owner entry the set mask -> place in the decision queue -> rank among the kept rows
    RT Kk[BJ_T];
    uint32_t Vv[BJ_T];
    uint16_t Sl[BJ_T], PQ[BJ_T];          // Sl: hash slot, then the owner's entry; PQ: decision queue, then the list of kept rows
    uint8_t Ch[BJ_T];                     // chromosome (6 bits) | kept row << 6 | fold-passing << 7 (owners, after the decision)
    int32_t rd[BJ_FC];
    float rinv[BJ_FC];
    uint32_t seg_off[SPS_MAXC + 2], cur[SPS_MAXC];
    const unsigned long long *keys[SPS_MAXC];
    const uint32_t *cnts[SPS_MAXC];
    uint32_t T, more, n_hist, n_row, n_pend;
    unsigned long long hist_pos, chunk_pos;
};
static_assert(sizeof(unsigned long long) * BJ_T <= sizeof(uint32_t) * BJ_H, "Et fits where the 32-bit hash keys were");
static_assert(SPS_MAXC <= 64, "six bits of Ch[] hold the chromosome");

template <typename RT>
__global__ void __launch_bounds__(BJ_THREADS)
sps_join_blk(sps_join_args A) {
    __shared__ bj_lds<RT> L;
    unsigned long long *const Et = reinterpret_cast<unsigned long long *>(L.Hk);
    uint32_t *const Es = L.Hmin;
    extern __shared__ uint32_t jw_rows[];      // [BJ_NR][C | 1]: rows being decided / written
    __shared__ uint32_t s_csets[SPS_MAXC];
    const int C = A.C, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int Cs = C | 1;                      // row stride in words (odd: consecutive rows start in different banks)
    const sp_fsets F = A.F;                    // (global memory: only the generic decision reads it)
    {
        for (int i = threadIdx.x; i < A.n_rd; i += blockDim.x) {
            L.rd[i] = A.rd[i];
            L.rinv[i] = A.rinv[i];
        }
        for (int i = threadIdx.x; i < C; i += blockDim.x) {
            s_csets[i] = (uint32_t)A.chrom_sets[i];
            L.keys[i] = A.lists[i].keys;
            L.cnts[i] = A.lists[i].cnts;
        }
        __syncthreads();
    }
    const RT EMPTY = (RT)~(RT)0;
    const unsigned long long rmask = A.shift >= 64 ? ~0ULL : ((1ULL << A.shift) - 1ULL);
    const unsigned long long *my_keys = nullptr;      // wave 0, lane c: list c
    if (w == 0 && lane < C) my_keys = A.lists[lane].keys;
    unsigned long long uni = 0;
    unsigned long long chunk_pos = 0, chunk_end = 0;   // block-uniform (every thread keeps the same copy)
    const uint32_t per = BJ_T / (uint32_t)C;
    const float fold32 = (float)F.min_fold;
    // the edges of the NEXT range of this workgroup travel while the current one is joined (unconditional, clamped)
    uint32_t n_cur = 0, n_endp = 0;
    auto edges = [&](long long r) {
        if (w == 0 && lane < C) {
            const long long rc = r < A.R ? r : A.R - 1;
            n_cur = A.bnd[(size_t)lane * (size_t)(A.R + 1) + (size_t)rc];
            n_endp = A.bnd[(size_t)lane * (size_t)(A.R + 1) + (size_t)rc + 1];
        }
    };
    // rows [0, n) of jw_rows <- the counts of the entries whose owner's Es lies in [first, first + n)
    auto build_rows = [&](uint32_t T, uint32_t first, uint32_t n) {
        for (uint32_t i = threadIdx.x; i < n * (uint32_t)Cs; i += BJ_THREADS) jw_rows[i] = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < BJ_Q; q++) {
            const uint32_t e = threadIdx.x + BJ_THREADS * q;
            if (e < T) {
                const uint32_t ri = Es[L.Sl[e]] - first;
                if (ri < n) jw_rows[ri * (uint32_t)Cs + (L.Ch[e] & 63u)] = L.Vv[e];
            }
        }
        __syncthreads();
    };
    edges(blockIdx.x);
    for (long long r = blockIdx.x; r < A.R; r += gridDim.x) {
        uint32_t cur = n_cur, endp = n_endp;           // wave 0 only
        edges(r + gridDim.x);
        if (w == 0) {
            const unsigned long long hp = jw_sum((unsigned long long)cur);   // the range's place in the virtual concatenation
            if (lane == 0) L.hist_pos = hp;
        }
        const unsigned long long hi_bits = A.shift >= 64 ? 0ULL : ((unsigned long long)r << A.shift);
        uint32_t rows_before = 0, hist_before = 0;     // block-uniform
        for (;;) {
            uint32_t take = 0;
            if (w == 0) {
                // ---- the round's share of every list: everything, or everything below the pivot key
                const uint32_t left = endp - cur;
                unsigned long long pivot = SPS_SENTINEL;
                if (jw_sum(left) > BJ_T) pivot = jw_min((lane < C && left > per) ? my_keys[cur + per] : SPS_SENTINEL);
                take = left;
                if (pivot != SPS_SENTINEL && lane < C) {     // entries below the pivot: at most `per` (the per-th is >= pivot)
                    const unsigned long long *kk = my_keys + cur;
                    uint32_t lo = 0, hi = left < per ? left : per;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (kk[mid] < pivot) lo = mid + 1;
                        else hi = mid;
                    }
                    take = lo;
                }
                uint32_t incl = take;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t x = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += x;
                }
                const uint32_t T0 = __shfl(incl, 63, 64);                 // <= BJ_T by construction
                const bool more0 = __any(cur + take < endp);
                if (lane <= C) L.seg_off[lane] = lane < C ? incl - take : T0;
                if (lane < C) L.cur[lane] = cur;
                if (lane == 0) {
                    L.T = T0;
                    L.more = more0 ? 1u : 0u;
                    L.n_hist = 0;
                    L.n_row = 0;
                    L.n_pend = 0;
                }
            }
            for (uint32_t i = threadIdx.x; i < BJ_H; i += BJ_THREADS) {
                L.Hk[i] = EMPTY;
                L.Hmin[i] = 0xFFFFFFFFu;
            }
            __syncthreads();
            const uint32_t T = L.T;
            const bool more = L.more != 0;
            uint32_t Hn = 64;
            while (Hn < 2 * T) Hn <<= 1;
            // ---- load + hash-insert (owner of a key = its entry of the lowest chromosome)
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) {
                const uint32_t e = threadIdx.x + BJ_THREADS * q;
                if (e < T) {
                    int lo = 0, hi = C;       // list of entry e: last c with seg_off[c] <= e
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (L.seg_off[mid] <= e) lo = mid;
                        else hi = mid;
                    }
                    const int c = lo;
                    const size_t i = (size_t)L.cur[c] + (e - L.seg_off[c]);
                    const RT res = (RT)(L.keys[c][i] & rmask);
                    L.Kk[e] = res;
                    L.Vv[e] = L.cnts[c][i];
                    L.Ch[e] = (uint8_t)c;
                    uint32_t h = (uint32_t)sps_mix((uint64_t)res) & (Hn - 1);
                    for (;;) {
                        const RT prev = atomicCAS(&L.Hk[h], EMPTY, res);
                        if (prev == EMPTY || prev == res) break;
                        h = (h + 1) & (Hn - 1);
                    }
                    L.Sl[e] = (uint16_t)h;
                    atomicMin(&L.Hmin[h], ((uint32_t)c << 16) | e);
                }
            }
            __syncthreads();
            // ---- every entry learns its owner (Sl: slot -> owner's entry); the totals' space is dead hash keys by now
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) {
                const uint32_t e = threadIdx.x + BJ_THREADS * q;
                if (e < T) L.Sl[e] = (uint16_t)(L.Hmin[L.Sl[e]] & 0xFFFFu);
                Et[e] = 0;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) Es[threadIdx.x + BJ_THREADS * q] = 0;      // (where the slot owners were)
            __syncthreads();
            // ---- every entry adds itself to its owner's tallies
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) {
                const uint32_t e = threadIdx.x + BJ_THREADS * q;
                if (e < T) {
                    const uint32_t o = L.Sl[e];
                    if (A.screen) atomicOr(&Es[o], s_csets[L.Ch[e]]);
                    atomicAdd(&Et[o], (unsigned long long)L.Vv[e]);
                }
            }
            __syncthreads();
            // ---- owners: the union tally, the screen; the ones that pass queue up for the full decision
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) {
                const uint32_t e = threadIdx.x + BJ_THREADS * q;
                bool pending = false;
                if (e < T && L.Sl[e] == e) {
                    uni++;
                    pending = !A.screen || !((double)__popc(Es[e]) / (double)F.n_multi < F.ratio);
                    Es[e] = 0xFFFFFFFFu;     // (no row)
                }
                const unsigned long long pb = __ballot(pending);
                if (pb) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&L.n_pend, (uint32_t)__popcll(pb));
                    base = __shfl(base, 0, 64);
                    if (pending) {
                        const uint32_t p = base + __popcll(pb & ((1ULL << lane) - 1ULL));
                        L.PQ[p] = (uint16_t)e;
                        Es[e] = p;
                    }
                }
            }
            __syncthreads();
            // ---- decisions, BJ_NR rows at a time
            const uint32_t n_p = L.n_pend;
            for (uint32_t p0 = 0; p0 < n_p; p0 += BJ_NR) {
                const uint32_t n = n_p - p0 < BJ_NR ? n_p - p0 : BJ_NR;
                build_rows(T, p0, n);
                const uint32_t ri = (uint32_t)lane * BJ_WAVES + (uint32_t)w;     // the rows spread evenly over the waves
                if (lane < BJ_ROWS && ri < n) {
                    const uint32_t e = L.PQ[p0 + ri];
                    const uint32_t *row = jw_rows + ri * (uint32_t)Cs;
                    const unsigned long long tot = Et[e];
                    bool r_ = false, h_ = false, generic = !A.fast;
                    if (A.fast) {
                        // _filter_kmer (Jellyfish.py:611-648) for baseline 1 / -1, as in k3_eval: running max, second max
                        // and min of the unit frequencies in fp32 on reciprocal products; a k-mer with a set inside the
                        // 1e-5 band around the threshold takes the generic code (fp64 quotients, the reference's order)
                        int include = 0;
                        unsigned long long num = 0;
                        float m1 = -1.0f, m2 = -1.0f, mn = 3e38f;
                        for (int j = 0; j < A.n_rd; j++) {     // (A.n_rd <= BJ_FC: host)
                            const int d = L.rd[j];                   // (uniform)
                            num += row[d & JD_CHROM_MASK];
                            if (d & JD_UNIT_END) {
                                const float x = (float)num * L.rinv[j];
                                m2 = fmaxf(m2, fminf(m1, x));
                                m1 = fmaxf(m1, x);
                                mn = fminf(mn, x);
                                num = 0;
                            }
                            if (d & JD_SET_END) {
                                const float thr = fold32 * (((d & JD_BI1) ? m2 : mn) + 1e-20f);
                                const bool pass = m1 > thr * (1.0f + 1e-5f);
                                include += pass ? 1 : 0;
                                generic = generic || (!pass && !(m1 < thr * (1.0f - 1e-5f)));
                                m1 = -1.0f; m2 = -1.0f; mn = 3e38f;
                            }
                        }
                        if (!generic && !((double)include / (double)F.n_multi < F.ratio)) {   // :642-644
                            h_ = true;
                            const double t = (double)tot;
                            r_ = !(t < F.min_freq || t > F.max_freq);                          // :645-646
                        }
                    }
                    if (generic) sp_filter_decide([&](int c) -> uint32_t { return row[c]; }, tot, F, r_, h_);
                    L.Ch[e] = (uint8_t)(L.Ch[e] | (r_ ? 0x40 : 0) | (h_ ? 0x80 : 0));
                }
                __syncthreads();
            }
            // ---- fold-passing totals out; kept rows listed
            bool is_row[BJ_Q];
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) {
                const uint32_t e = threadIdx.x + BJ_THREADS * q;
                const uint32_t fl = e < T ? (uint32_t)L.Ch[e] >> 6 : 0u;      // (set for owners only)
                is_row[q] = (fl & 1u) != 0;
                const bool is_hist = (fl & 2u) != 0;
                // fold-passing totals: range start + tally so far + a place of the wave's in this round (any order)
                const unsigned long long bh = __ballot(is_hist);
                if (bh) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&L.n_hist, (uint32_t)__popcll(bh));
                    base = __shfl(base, 0, 64);
                    if (is_hist)
                        A.hist_stage[L.hist_pos + hist_before + base + __popcll(bh & ((1ULL << lane) - 1ULL))] = Et[e];
                }
            }
            __syncthreads();       // (PQ is the decision queue no longer)
#pragma unroll
            for (int q = 0; q < BJ_Q; q++) {
                const uint32_t e = threadIdx.x + BJ_THREADS * q;
                const unsigned long long br = __ballot(is_row[q]);
                if (br) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&L.n_row, (uint32_t)__popcll(br));
                    base = __shfl(base, 0, 64);
                    if (is_row[q]) L.PQ[base + __popcll(br & ((1ULL << lane) - 1ULL))] = (uint16_t)e;
                }
            }
            __syncthreads();
            const uint32_t nrow = L.n_row, nh = L.n_hist;
            if (nrow) {       // rare: rows to the staging area, ranked by key inside the round
                if (chunk_pos + nrow > chunk_end) {      // block-uniform
                    const unsigned long long grab = nrow > JOIN_CHUNK ? nrow : JOIN_CHUNK;
                    if (threadIdx.x == 0) L.chunk_pos = atomicAdd(A.row_cursor, grab);
                    __syncthreads();
                    chunk_pos = L.chunk_pos;
                    chunk_end = chunk_pos + grab;
                }
                // Es: rank among the round's kept rows; every other owner out of the way (the ones that were decided still
                // hold their queue place)
#pragma unroll
                for (int q = 0; q < BJ_Q; q++) {
                    const uint32_t e = threadIdx.x + BJ_THREADS * q;
                    if (e < T && !is_row[q] && L.Sl[e] == e) Es[e] = 0xFFFFFFFFu;
                }
#pragma unroll
                for (int q = 0; q < BJ_Q; q++) {
                    if (!is_row[q]) continue;
                    const uint32_t e = threadIdx.x + BJ_THREADS * q;
                    const RT res = L.Kk[e];
                    uint32_t rank = 0;
                    for (uint32_t j = 0; j < nrow; j++) rank += L.Kk[L.PQ[j]] < res;
                    Es[e] = rank;
                    const unsigned long long pos = chunk_pos + rank;
                    if (pos < A.row_cap) {
                        A.row_keys[pos] = hi_bits | (unsigned long long)res;
                        A.row_tot[pos] = Et[e];
                        A.row_rank[pos] = rows_before + rank;
                    }
                }
                __syncthreads();
                for (uint32_t r0 = 0; r0 < nrow; r0 += BJ_NR) {
                    const uint32_t n = nrow - r0 < BJ_NR ? nrow - r0 : BJ_NR;
                    build_rows(T, r0, n);
                    for (uint32_t i = threadIdx.x; i < n * (uint32_t)C; i += BJ_THREADS) {
                        const uint32_t rr = i / (uint32_t)C, c = i - rr * (uint32_t)C;
                        const unsigned long long pos = chunk_pos + r0 + rr;
                        if (pos < A.row_cap) A.row_counts[pos * (size_t)C + c] = jw_rows[rr * (uint32_t)Cs + c];
                    }
                    __syncthreads();
                }
                chunk_pos += nrow;
                rows_before += nrow;
            }
            hist_before += nh;
            __syncthreads();      // the round's LDS state is rewritten by the next round / range
            if (!more) break;
            cur += take;
        }
        if (threadIdx.x == 0) {
            A.n_rows[r] = rows_before;
            A.n_hist[r] = hist_before;
        }
    }
    uni = jw_sum(uni);
    if (lane == 0 && uni) atomicAdd(A.n_union, uni);
}

// ------------------------------------------------------------------ sps_join_wide: the join for 64 < C <= SP_LIST_MAXC
// sps_join_blk's layout stops at 64 lists: lane c of wave 0 owns list c, Ch[] keeps the chromosome in six bits, the share of
// a round is BJ_T / C entries per list and every decided key gets a C-word row in LDS (at C = 1024, 64 such rows alone are
// 256 KiB).  This kernel keeps its outputs and its staging protocol -- per-range tallies, fold-passing totals at the range's
// closed-form place, rows in JOIN_CHUNK chunks with their rank inside the range -- so sps_tally_* / sps_place_* and the
// row-cap retry of sps_filter_join serve both, and changes what depends on C:
//  * the cursor logic runs on the whole workgroup: thread t owns lists t, t + WJ_THREADS, ...; the range's place, the
//    round's pivot and the segment offsets are block reductions and scans.  A list's share of a round is proportional to
//    what it has left, one entry at least: the shares add up to WJ_T at most (WJ_T >= 2 * SP_LIST_MAXC), the pivot is the
//    smallest key just past a share, and the list it came from takes its whole share, so a round never overflows the hash
//    and always moves on;
//  * no rows in LDS.  sp_filter_decide only reads integer sums per unit, so the decision is taken set by set: the entry of
//    a key that holds the lowest chromosome of a non-singleton set among the key's entries decides that set
//    (sp_filter_set_pass; the other chromosomes' counts by binary search in their segments of the round, which are
//    sorted) and adds the result less the set's all-zero result to its owner's tally.  include = (sum of the all-zero
//    results) + tally, an integer in any order, and the ratio test is sp_filter_decide's.  SP_JOIN_GENERIC=1: the owner
//    runs sp_filter_decide itself on the same look-ups;
//  * kept rows are written by their entries straight into the row staging (rank * C + chromosome) after the workgroup
//    zero-fills them.
// LDS: 71.8 KB with 32-bit residuals (two workgroups per CU), 96.3 KB with 64-bit ones (one).
#define WJ_THREADS 256
#define WJ_T 2048             // entries per round
#define WJ_H (2 * WJ_T)       // hash slots
#define WJ_Q (WJ_T / WJ_THREADS)
#define WJ_LPT (SP_LIST_MAXC / WJ_THREADS)    // lists per thread
#define WJ_ROW 1u
#define WJ_HIST 2u
#define WJ_PEND 4u
static_assert(WJ_T >= 2 * SP_LIST_MAXC, "a list with entries left gets a share of one entry at least");
static_assert(SP_LIST_MAXC <= 65536 && WJ_T <= 65536, "Ch[] / Sl[] / PQ[] are 16 bits wide");

struct sps_wide_args {
    const int32_t *cset_off, *cset;   // per chromosome: the non-singleton sets it belongs to (CSR)
    int generic;                      // SP_JOIN_GENERIC=1: sp_filter_decide per owner
};

template <typename RT>
struct wj_lds {
    alignas(8) RT Hk[WJ_H];           // hash keys; after the inserts: Et[WJ_T], per owner entry the sum of the key's counts
    uint32_t Hmin[WJ_H];              // per slot: the owner entry (the lowest entry is the lowest chromosome); after the owner
                                      // pass: Es[WJ_T] set mask -> rank among the kept rows, Ei[WJ_T] the owner's set tally
    RT Kk[WJ_T];                      // residual keys, list by list (each segment ascending)
    uint32_t Vv[WJ_T];
    uint16_t Sl[WJ_T], Ch[WJ_T], PQ[WJ_T];   // Sl: hash slot, then the owner's entry; Ch: chromosome; PQ: kept rows
    uint8_t Fl[WJ_T];                 // owners: WJ_PEND, then WJ_ROW | WJ_HIST
    uint32_t seg_off[SP_LIST_MAXC + 1], cur[SP_LIST_MAXC];
    unsigned long long red[WJ_THREADS / 64];
    uint32_t scan[WJ_THREADS / 64];
    uint32_t n_hist, n_row;
    unsigned long long chunk_pos;
};
static_assert(sizeof(unsigned long long) * WJ_T <= sizeof(uint32_t) * WJ_H, "Et fits where the 32-bit hash keys were");

__device__ __forceinline__ unsigned long long wj_bsum(unsigned long long v, unsigned long long *red) {
    v = jw_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int i = 0; i < WJ_THREADS / 64; i++) t += red[i];
    __syncthreads();
    return t;
}
__device__ __forceinline__ unsigned long long wj_bmin(unsigned long long v, unsigned long long *red) {
    v = jw_min(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = ~0ULL;
#pragma unroll
    for (int i = 0; i < WJ_THREADS / 64; i++) t = red[i] < t ? red[i] : t;
    __syncthreads();
    return t;
}

template <typename RT>
__global__ void __launch_bounds__(WJ_THREADS)
sps_join_wide(sps_join_args A, sps_wide_args W) {
    __shared__ wj_lds<RT> L;
    unsigned long long *const Et = reinterpret_cast<unsigned long long *>(L.Hk);
    uint32_t *const Es = L.Hmin;
    int32_t *const Ei = reinterpret_cast<int32_t *>(L.Hmin + WJ_T);
    const int C = A.C, lane = threadIdx.x & 63;
    const sp_fsets F = A.F;
    const RT EMPTY = (RT)~(RT)0;
    const unsigned long long rmask = A.shift >= 64 ? ~0ULL : ((1ULL << A.shift) - 1ULL);
    // include of a key that touches no set, and whether the set screen holds (it assumes an untouched set fails)
    int zero_inc = 0;
    for (int s = threadIdx.x; s < F.n_sets; s += WJ_THREADS)
        if (F.set_off[s + 1] - F.set_off[s] > 1) zero_inc += sp_filter_set_pass([](int) -> uint32_t { return 0u; }, F, s);
    zero_inc = (int)wj_bsum((unsigned long long)zero_inc, L.red);
    const bool screen = A.screen && zero_inc == 0;
    // the count of residual `res` in chromosome c's segment of the round (0: absent)
    auto lookup = [&](int c, RT res) -> uint32_t {
        const uint32_t e1 = L.seg_off[c + 1];
        uint32_t lo = L.seg_off[c], hi = e1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (L.Kk[mid] < res) lo = mid + 1;
            else hi = mid;
        }
        return (lo < e1 && L.Kk[lo] == res) ? L.Vv[lo] : 0u;
    };
    unsigned long long uni = 0;
    unsigned long long chunk_pos = 0, chunk_end = 0;   // block-uniform
    for (long long r = blockIdx.x; r < A.R; r += gridDim.x) {
        uint32_t cur[WJ_LPT], endp[WJ_LPT];
        unsigned long long start = 0;
#pragma unroll
        for (int j = 0; j < WJ_LPT; j++) {
            const int c = threadIdx.x + WJ_THREADS * j;
            cur[j] = endp[j] = 0;
            if (c < C) {
                cur[j] = A.bnd[(size_t)c * (size_t)(A.R + 1) + (size_t)r];
                endp[j] = A.bnd[(size_t)c * (size_t)(A.R + 1) + (size_t)r + 1];
            }
            start += cur[j];
        }
        const unsigned long long hist_pos = wj_bsum(start, L.red);   // the range's place in the virtual concatenation
        const unsigned long long hi_bits = A.shift >= 64 ? 0ULL : ((unsigned long long)r << A.shift);
        uint32_t rows_before = 0, hist_before = 0;     // block-uniform
        for (;;) {
            // ---- the round's share of every list: everything, or everything below the pivot key
            uint32_t take[WJ_LPT];
            unsigned long long left_sum = 0;
#pragma unroll
            for (int j = 0; j < WJ_LPT; j++) {
                take[j] = endp[j] - cur[j];
                left_sum += take[j];
            }
            const unsigned long long S = wj_bsum(left_sum, L.red);
            const bool more = S > WJ_T;                  // the shares add up to WJ_T at most
            if (more) {
                uint32_t q[WJ_LPT];
                unsigned long long cand = SPS_SENTINEL;
#pragma unroll
                for (int j = 0; j < WJ_LPT; j++) {
                    const uint32_t left = take[j];
                    const uint32_t share = (uint32_t)((unsigned long long)left * (unsigned long long)(WJ_T - C) / S);
                    q[j] = left ? (share > 1u ? share : 1u) : 0u;
                    if (left > q[j]) {
                        const unsigned long long x = A.lists[threadIdx.x + WJ_THREADS * j].keys[(size_t)cur[j] + q[j]];
                        cand = x < cand ? x : cand;
                    }
                }
                const unsigned long long pivot = wj_bmin(cand, L.red);     // < SENTINEL: some list has more than its share
#pragma unroll
                for (int j = 0; j < WJ_LPT; j++) {
                    if (!take[j]) continue;
                    const unsigned long long *kk = A.lists[threadIdx.x + WJ_THREADS * j].keys + cur[j];
                    uint32_t lo = 0, hi = take[j] < q[j] ? take[j] : q[j];   // entries below the pivot lie in the share
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (kk[mid] < pivot) lo = mid + 1;
                        else hi = mid;
                    }
                    take[j] = lo;
                }
            }
            uint32_t T = 0;
#pragma unroll
            for (int j = 0; j < WJ_LPT; j++) {
                if (j * WJ_THREADS >= C) break;          // (block-uniform)
                uint32_t tot;
                const uint32_t ex = sp_block_excl_scan<uint32_t>(take[j], L.scan, tot);
                const int c = threadIdx.x + WJ_THREADS * j;
                if (c < C) {
                    L.seg_off[c] = T + ex;
                    L.cur[c] = cur[j];
                }
                T += tot;
            }
            if (threadIdx.x == 0) {
                L.seg_off[C] = T;
                L.n_hist = 0;
                L.n_row = 0;
            }
            for (uint32_t i = threadIdx.x; i < WJ_H; i += WJ_THREADS) {
                L.Hk[i] = EMPTY;
                L.Hmin[i] = 0xFFFFFFFFu;
            }
            __syncthreads();
            uint32_t Hn = 64;
            while (Hn < 2 * T) Hn <<= 1;
            // ---- load + hash-insert (owner of a key = its entry of the lowest chromosome = its lowest entry)
#pragma unroll
            for (int q = 0; q < WJ_Q; q++) {
                const uint32_t e = threadIdx.x + WJ_THREADS * q;
                if (e < T) {
                    int lo = 0, hi = C;       // list of entry e: last c with seg_off[c] <= e
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (L.seg_off[mid] <= e) lo = mid;
                        else hi = mid;
                    }
                    const int c = lo;
                    const size_t i = (size_t)L.cur[c] + (e - L.seg_off[c]);
                    const sps_list li = A.lists[c];
                    const RT res = (RT)(li.keys[i] & rmask);
                    L.Kk[e] = res;
                    L.Vv[e] = li.cnts[i];
                    L.Ch[e] = (uint16_t)c;
                    uint32_t h = (uint32_t)sps_mix((uint64_t)res) & (Hn - 1);
                    for (;;) {
                        const RT prev = atomicCAS(&L.Hk[h], EMPTY, res);
                        if (prev == EMPTY || prev == res) break;
                        h = (h + 1) & (Hn - 1);
                    }
                    L.Sl[e] = (uint16_t)h;
                    atomicMin(&L.Hmin[h], e);
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < WJ_Q; q++) {
                const uint32_t e = threadIdx.x + WJ_THREADS * q;
                if (e < T) L.Sl[e] = (uint16_t)L.Hmin[L.Sl[e]];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < WJ_Q; q++) {       // (the totals where the hash keys were, the tallies where the slot owners were)
                const uint32_t e = threadIdx.x + WJ_THREADS * q;
                Et[e] = 0;
                Es[e] = 0;
                Ei[e] = 0;
                L.Fl[e] = 0;
            }
            __syncthreads();
            // ---- every entry adds itself to its owner's tallies
#pragma unroll
            for (int q = 0; q < WJ_Q; q++) {
                const uint32_t e = threadIdx.x + WJ_THREADS * q;
                if (e < T) {
                    const uint32_t o = L.Sl[e];
                    if (screen) atomicOr(&Es[o], (uint32_t)A.chrom_sets[L.Ch[e]]);
                    atomicAdd(&Et[o], (unsigned long long)L.Vv[e]);
                }
            }
            __syncthreads();
            // ---- owners: the union tally, the screen; SP_JOIN_GENERIC: the whole decision here
#pragma unroll
            for (int q = 0; q < WJ_Q; q++) {
                const uint32_t e = threadIdx.x + WJ_THREADS * q;
                if (e < T && L.Sl[e] == e) {
                    uni++;
                    if (!screen || !((double)__popc(Es[e]) / (double)F.n_multi < F.ratio)) {
                        if (W.generic) {
                            const RT res = L.Kk[e];
                            bool r_ = false, h_ = false;
                            sp_filter_decide([&](int c) -> uint32_t { return lookup(c, res); }, Et[e], F, r_, h_);
                            L.Fl[e] = (uint8_t)((r_ ? WJ_ROW : 0u) | (h_ ? WJ_HIST : 0u));
                        } else {
                            L.Fl[e] = (uint8_t)WJ_PEND;
                        }
                    }
                }
            }
            __syncthreads();
            if (!W.generic) {
                // ---- every entry of a pending key decides the sets in which it holds the key's lowest chromosome
#pragma unroll
                for (int q = 0; q < WJ_Q; q++) {
                    const uint32_t e = threadIdx.x + WJ_THREADS * q;
                    if (e < T) {
                        const uint32_t o = L.Sl[e];
                        if (L.Fl[o] & WJ_PEND) {
                            const int c = L.Ch[e];
                            const RT res = L.Kk[e];
                            int d = 0;
                            for (int m = W.cset_off[c]; m < W.cset_off[c + 1]; m++) {
                                const int s = W.cset[m];
                                bool first = true;
                                for (int j = F.unit_off[F.set_off[s]]; first && j < F.unit_off[F.set_off[s + 1]]; j++) {
                                    const int c2 = F.unit_chrom[j];
                                    if (c2 < c && lookup(c2, res)) first = false;     // (list counts are >= 1)
                                }
                                if (first)
                                    d += sp_filter_set_pass([&](int c2) -> uint32_t { return lookup(c2, res); }, F, s) -
                                         sp_filter_set_pass([](int) -> uint32_t { return 0u; }, F, s);
                            }
                            if (d) atomicAdd(&Ei[o], d);
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < WJ_Q; q++) {
                    const uint32_t e = threadIdx.x + WJ_THREADS * q;
                    if (e < T && (L.Fl[e] & WJ_PEND)) {
                        const int include = zero_inc + Ei[e];
                        uint32_t fl = 0;
                        const double rr = 1.0 * (double)include / (double)F.n_multi;    // :642, as sp_filter_decide
                        if (!(rr < F.ratio)) {
                            fl = WJ_HIST;
                            const double t = (double)Et[e];
                            if (!(t < F.min_freq || t > F.max_freq)) fl |= WJ_ROW;          // :645-646
                        }
                        L.Fl[e] = (uint8_t)fl;
                    }
                }
                __syncthreads();
            }
            // ---- fold-passing totals out; kept rows listed
            bool is_row[WJ_Q];
#pragma unroll
            for (int q = 0; q < WJ_Q; q++) {
                const uint32_t e = threadIdx.x + WJ_THREADS * q;
                const uint32_t fl = e < T ? (uint32_t)L.Fl[e] : 0u;      // (set for owners only)
                is_row[q] = (fl & WJ_ROW) != 0;
                const bool is_hist = (fl & WJ_HIST) != 0;
                const unsigned long long bh = __ballot(is_hist);
                if (bh) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&L.n_hist, (uint32_t)__popcll(bh));
                    base = __shfl(base, 0, 64);
                    if (is_hist)
                        A.hist_stage[hist_pos + hist_before + base + __popcll(bh & ((1ULL << lane) - 1ULL))] = Et[e];
                }
                const unsigned long long br = __ballot(is_row[q]);
                if (br) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&L.n_row, (uint32_t)__popcll(br));
                    base = __shfl(base, 0, 64);
                    if (is_row[q]) L.PQ[base + __popcll(br & ((1ULL << lane) - 1ULL))] = (uint16_t)e;
                }
            }
            __syncthreads();
            const uint32_t nrow = L.n_row, nh = L.n_hist;
            if (nrow) {       // rows to the staging area, ranked by key inside the round
                if (chunk_pos + nrow > chunk_end) {      // block-uniform
                    const unsigned long long grab = nrow > JOIN_CHUNK ? nrow : JOIN_CHUNK;
                    if (threadIdx.x == 0) L.chunk_pos = atomicAdd(A.row_cursor, grab);
                    __syncthreads();
                    chunk_pos = L.chunk_pos;
                    chunk_end = chunk_pos + grab;
                }
#pragma unroll
                for (int q = 0; q < WJ_Q; q++) {
                    if (!is_row[q]) continue;
                    const uint32_t e = threadIdx.x + WJ_THREADS * q;
                    const RT res = L.Kk[e];
                    uint32_t rank = 0;
                    for (uint32_t j = 0; j < nrow; j++) rank += L.Kk[L.PQ[j]] < res;
                    Es[e] = rank;
                    const unsigned long long pos = chunk_pos + rank;
                    if (pos < A.row_cap) {
                        A.row_keys[pos] = hi_bits | (unsigned long long)res;
                        A.row_tot[pos] = Et[e];
                        A.row_rank[pos] = rows_before + rank;
                    }
                }
                for (unsigned long long i = threadIdx.x; i < (unsigned long long)nrow * (unsigned long long)C; i += WJ_THREADS)
                    if (chunk_pos + i / (unsigned long long)C < A.row_cap) A.row_counts[chunk_pos * (size_t)C + i] = 0u;
                __threadfence();      // the zeros are out before any entry writes its count over one of them
                __syncthreads();
#pragma unroll
                for (int q = 0; q < WJ_Q; q++) {
                    const uint32_t e = threadIdx.x + WJ_THREADS * q;
                    if (e < T) {
                        const uint32_t o = L.Sl[e];
                        if (L.Fl[o] & WJ_ROW) {
                            const unsigned long long pos = chunk_pos + Es[o];
                            if (pos < A.row_cap) A.row_counts[pos * (size_t)C + L.Ch[e]] = L.Vv[e];
                        }
                    }
                }
                chunk_pos += nrow;
                rows_before += nrow;
            }
            hist_before += nh;
            __syncthreads();      // the round's LDS state is rewritten by the next round / range
            if (!more) break;
#pragma unroll
            for (int j = 0; j < WJ_LPT; j++) cur[j] += take[j];
        }
        if (threadIdx.x == 0) {
            A.n_rows[r] = rows_before;
            A.n_hist[r] = hist_before;
        }
    }
    uni = wj_bsum(uni, L.red);
    if (threadIdx.x == 0 && uni) atomicAdd(A.n_union, uni);
}

// per-range tallies -> offsets: block sums, one-block scan of the sums, offsets inside every block
#define TALLY_CHUNK 4096
__global__ void __launch_bounds__(256)
sps_tally_sums(const uint32_t *__restrict__ a, long long n, unsigned long long *__restrict__ bsum) {
    __shared__ unsigned long long red[16];
    const long long lo = (long long)blockIdx.x * TALLY_CHUNK, hi = lo + TALLY_CHUNK < n ? lo + TALLY_CHUNK : n;
    unsigned long long v = 0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) v += a[i];
    const unsigned long long t = sp_block_sum_u64(v, red);
    if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}
__global__ void __launch_bounds__(256)
sps_tally_apply(const uint32_t *__restrict__ a, long long n, const unsigned long long *__restrict__ boff,
                const unsigned long long *__restrict__ total, unsigned long long *__restrict__ off /* n + 1 */) {
    __shared__ unsigned long long wsum[16];
    const long long lo = (long long)blockIdx.x * TALLY_CHUNK, hi = lo + TALLY_CHUNK < n ? lo + TALLY_CHUNK : n;
    constexpr int PER = TALLY_CHUNK / 256;
    const long long t0 = lo + (long long)threadIdx.x * PER;
    unsigned long long s = 0;
    for (int j = 0; j < PER; j++)
        if (t0 + j < hi) s += a[t0 + j];
    unsigned long long tot;
    unsigned long long run = boff[blockIdx.x] + sp_block_excl_scan(s, wsum, tot);
    for (int j = 0; j < PER; j++)
        if (t0 + j < hi) {
            off[t0 + j] = run;
            run += a[t0 + j];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[n] = *total;
}

// staged rows -> their final places: offset of the row's range + its rank inside the range (ascending key overall)
__global__ void __launch_bounds__(256)
sps_place_rows(const unsigned long long *__restrict__ row_keys, const unsigned long long *__restrict__ row_tot,
               const uint32_t *__restrict__ row_rank, const uint32_t *__restrict__ row_counts, unsigned long long n_staged,
               int C, int shift, const unsigned long long *__restrict__ row_off, unsigned long long *__restrict__ out_keys,
               uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ out_tot) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_staged) return;
    const unsigned long long key = row_keys[i];
    if (key == SPS_SENTINEL) return;      // the unused tail of a chunk
    const unsigned long long pos = row_off[key >> shift] + row_rank[i];
    out_keys[pos] = key;
    out_tot[pos] = row_tot[i];
    if (out_counts)      // (phase A of sps_filter_passengers keeps the keys only)
        for (int c = 0; c < C; c++) out_counts[pos * (size_t)C + c] = row_counts[i * (size_t)C + c];
}

// fold-passing totals of range r: hist_stage[start of the range ..) -> out[hist_off[r] ..)
__global__ void __launch_bounds__(256)
sps_place_hist(const unsigned long long *__restrict__ hist_stage, const uint32_t *__restrict__ bnd, int C, long long R,
               const uint32_t *__restrict__ n_hist, const unsigned long long *__restrict__ hist_off,
               unsigned long long *__restrict__ out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const uint32_t m = n_hist[r];
    if (!m) return;
    unsigned long long src = 0;
    for (int c = 0; c < C; c++) src += bnd[(size_t)c * (size_t)(R + 1) + (size_t)r];
    const unsigned long long dst = hist_off[r];
    for (uint32_t j = 0; j < m; j++) out[dst + j] = hist_stage[src + j];
}

// SP_ENOMEM naming the size when `bytes` do not fit what the device has free (the buffer's own bytes count as free)
static int sps_fits(sp_ctx *ctx, const sp_buf &b, int64_t bytes, const char *what) {
    if (bytes <= b.cap) return SP_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return SP_OK;     // (sp_buf_ensure reports a failed allocation)
    const double avail = (double)free_b + (double)b.cap;
    if ((double)bytes + (double)bytes / 8 + 4096 <= avail) return SP_OK;
    return sp_fail(ctx, SP_ENOMEM, "list filter: %s need %.2f GiB, the device has %.2f GiB free", what,
                   (double)bytes / (1 << 30), avail / (1 << 30));
}

static int sps_filter_sort(sp_ctx *ctx, int n_sets, const int32_t *set_off, const int32_t *unit_off,
                           const int32_t *unit_chrom, const std::vector<double> &den, double min_fold, int baseline,
                           double min_freq, double max_freq, double ratio) {
    const int C = sps_C(ctx);
    if (C > SPS_MAXC) return sp_fail(ctx, SP_EUNSUP, "list filter (k > 15, or engine 3): at most %d chromosomes supported (got %d)", SPS_MAXC, C);
    int64_t total = 0;
    for (int c = 0; c < C; c++) total += sps_n(ctx, c);
    ctx->sf_n = total;
    ctx->n_union = ctx->n_rows = ctx->n_hist = 0;
    if (total == 0) {
        ctx->filtered = true;
        return SP_OK;
    }
    int rc = sp_buf_ensure(ctx, ctx->b_sp_a, total * 16);   // keys | vals (unsorted)
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sp_b, total * 16);       // keys | vals (sorted)
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sp_c, total + 64);       // flags
    if (rc) return rc;
    unsigned long long *K0 = (unsigned long long *)ctx->b_sp_a.p, *V0 = K0 + total;
    unsigned long long *K1 = (unsigned long long *)ctx->b_sp_b.p, *V1 = K1 + total;
    uint8_t *flags = (uint8_t *)ctx->b_sp_c.p;
    int64_t off = 0;
    for (int c = 0; c < C; c++) {
        const int64_t n_c = sps_n(ctx, c);
        if (n_c)
            SP_LAUNCH(ctx, "sps_concat", sps_concat, dim3((unsigned)((n_c + 255) / 256)), dim3(256), 0,
                      sps_keys(ctx, c), sps_cnts(ctx, c), n_c, c, K0 + off, V0 + off);
        off += n_c;
    }
    const unsigned end_bit = (2 * ctx->k > 64) ? 64u : (unsigned)(2 * ctx->k);
    size_t tmp_bytes = 0;
    SP_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, K0, K1, V0, V1, (size_t)total, 0u, end_bit, ctx->stream));
    // b_sp_tmp: the rocprim temp storage | the set structure | block tallies (rows, hist) | [0] union [1] rows [2] hist
    const int n_units = set_off[n_sets], n_uc = unit_off[n_units];
    const int64_t nblk = (total + SEL_SPAN - 1) / SEL_SPAN;
    char *T = nullptr, *d_fs = nullptr;
    unsigned long long *blk_r = nullptr, *blk_h = nullptr, *small = nullptr;
    auto lay = [&](sp_carve cv) {
        T = cv.take<char>(tmp_bytes);
        d_fs = cv.take<char>(sp_fsets_bytes(n_sets, n_units, (size_t)n_uc + 1));
        blk_r = cv.take<unsigned long long>((size_t)nblk + 1);
        blk_h = cv.take<unsigned long long>((size_t)nblk + 1);
        small = cv.take<unsigned long long>(32);
        return cv.off;
    };
    rc = sp_buf_ensure(ctx, ctx->b_sp_tmp, (int64_t)lay(sp_carve()));
    if (rc) return rc;
    lay(sp_carve(ctx->b_sp_tmp.p));
    SP_HIP(ctx, rocprim::radix_sort_pairs(T, tmp_bytes, K0, K1, V0, V1, (size_t)total, 0u, end_bit, ctx->stream));
    sps_filter_args A;
    A.C = C;
    SP_HIP(ctx, sp_fsets_upload(ctx->stream, d_fs, n_sets, set_off, unit_off, unit_chrom, (size_t)n_uc + 1, den.data(), min_fold,
                                baseline, min_freq, max_freq, ratio, A.F));
    SP_HIP(ctx, hipMemsetAsync(small, 0, 256, ctx->stream));
    SP_LAUNCH(ctx, "sps_eval", sps_eval, dim3((unsigned)nblk), dim3(SEL_BLOCK), 0, K1, V1, total, A, flags, blk_r, blk_h,
              small);
    SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, blk_r, nblk, small + 1);
    SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, blk_h, nblk, small + 2);
    unsigned long long h[3] = {0, 0, 0};
    SP_HIP(ctx, hipMemcpyAsync(h, small, 24, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_union = (int64_t)h[0];
    ctx->n_rows = (int64_t)h[1];
    ctx->n_hist = (int64_t)h[2];
    // materialise the results now (the sort buffers are reused by the next call)
    const int64_t M = ctx->n_rows, H = ctx->n_hist;
    rc = sp_buf_ensure(ctx, ctx->b_sf_keys, (M + 1) * 8);
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sf_counts, (M + 1) * (int64_t)C * 4);
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sf_tot, (M + 1) * 8);
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sf_hist, (H + 1) * 8);
    if (rc) return rc;
    if (M)
        SP_LAUNCH(ctx, "sps_emit", sps_emit, dim3((unsigned)nblk), dim3(SEL_BLOCK), 0, K1, V1, total, C,
                  (const uint8_t *)flags, (uint8_t)1, (const unsigned long long *)blk_r,
                  (unsigned long long *)ctx->b_sf_keys.p, (uint32_t *)ctx->b_sf_counts.p,
                  (unsigned long long *)ctx->b_sf_tot.p);
    if (H)
        SP_LAUNCH(ctx, "sps_emit_hist", sps_emit, dim3((unsigned)nblk), dim3(SEL_BLOCK), 0, K1, V1, total, C,
                  (const uint8_t *)flags, (uint8_t)2, (const unsigned long long *)blk_h, (unsigned long long *)nullptr,
                  (uint32_t *)nullptr, (unsigned long long *)ctx->b_sf_hist.p);
    if (M && ctx->list_mode)
        SP_LAUNCH(ctx, "sps_slots_to_keys", sps_slots_to_keys, dim3((unsigned)((M + 255) / 256)), dim3(256), 0,
                  (unsigned long long *)ctx->b_sf_keys.p, M, sp_make_kparams(ctx->k));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->filtered = true;
    return SP_OK;
}

// the join kernel of either residual width (RT = uint32_t when the keys of a range differ in their low 32 bits only)
template <typename RT>
static int sps_join_launch(sp_ctx *ctx, const sps_join_args &A, const sps_wide_args *W) {
    int64_t grid = A.R;
    if (grid > (int64_t)ctx->n_cu * 16) grid = (int64_t)ctx->n_cu * 16;
    if (W) {
        SP_LAUNCH(ctx, "sps_join_wide", sps_join_wide<RT>, dim3((unsigned)grid), dim3(WJ_THREADS), 0, A, *W);
        return SP_OK;
    }
    const size_t row_lds = (size_t)BJ_NR * (size_t)(A.C | 1) * 4;     // <= 16.3 KiB
    // (static + dynamic LDS passes 64 KiB with many chromosomes and 64-bit residuals)
    SP_HIP(ctx, hipFuncSetAttribute((const void *)sps_join_blk<RT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)row_lds));
    SP_LAUNCH(ctx, "sps_join", sps_join_blk<RT>, dim3((unsigned)grid), dim3(BJ_THREADS), row_lds, A);
    return SP_OK;
}

// plan (sp_listplan.h) -> upload -> run (at most twice: the row staging is sized by a guess) -> place.
// pick: the chromosomes whose lists are joined, in list order (nullptr: all of them).  sps_filter_passengers' phase A
// joins the set chromosomes alone, with unit_chrom numbering the picked lists, and keeps its rows as dense slots without
// their counts.
static int sps_filter_join(sp_ctx *ctx, int n_sets, const int32_t *set_off, const int32_t *unit_off,
                           const int32_t *unit_chrom, const std::vector<double> &den, double min_fold, int baseline,
                           double min_freq, double max_freq, double ratio, const std::vector<int> *pick = nullptr) {
    const int C = pick ? (int)pick->size() : sps_C(ctx);
    if (C > SP_LIST_MAXC)
        return sp_fail(ctx, SP_EUNSUP, "list filter (k > 15, or engine 3): at most %d chromosomes supported (got %d)", SP_LIST_MAXC, C);
    int64_t total = 0, longest = 0;
    std::vector<sps_list> hl((size_t)C);
    for (int c = 0; c < C; c++) {
        const int cc = pick ? (*pick)[(size_t)c] : c;
        hl[(size_t)c] = sps_list{sps_keys(ctx, cc), sps_cnts(ctx, cc), (long long)sps_n(ctx, cc)};
        total += sps_n(ctx, cc);
        longest = sps_n(ctx, cc) > longest ? sps_n(ctx, cc) : longest;
    }
    ctx->sf_n = total;
    ctx->n_union = ctx->n_rows = ctx->n_hist = 0;
    if (total == 0) {
        ctx->filtered = true;
        return SP_OK;
    }
    if (longest >= (1LL << 32)) return sp_fail(ctx, SP_EUNSUP, "list filter: a list of 2^32 or more k-mers");
    // ---- plan
    const int n_units = set_off[n_sets], n_uc = unit_off[n_units];
    const bool generic = getenv("SP_JOIN_GENERIC") && atoi(getenv("SP_JOIN_GENERIC"));     // cross-check switch
    const sp_range_plan rp = sp_plan_ranges(total, C, ctx->k, ctx->list_mode ? ctx->nslots : 0);
    const long long R = rp.R;
    const sp_walk_plan walk = sp_plan_walk(n_sets, set_off, unit_off, unit_chrom, den.data() + n_units, baseline, generic);
    const sp_mask_plan masks = sp_plan_masks(C, n_sets, set_off, unit_off, unit_chrom, pick != nullptr, min_fold);
    std::vector<int32_t> h_cso, h_cs;
    if (rp.wide) sp_plan_wide_csr(C, n_sets, set_off, unit_off, unit_chrom, h_cso, h_cs);
    // ---- upload
    // b_sp_a: list descriptors | range edges | per-range tallies | offsets | the set structure | [0] union [1] row cursor
    //         [2] M [3] H | set masks | block sums of the tallies | walk descriptors (| the wide kernel's set CSR)
    // b_sp_b: staging of the totals
    const size_t n_bs = (size_t)(R / TALLY_CHUNK + 2);
    sps_list *d_lists = nullptr;
    uint32_t *bnd = nullptr, *n_rows = nullptr, *n_hist = nullptr;
    unsigned long long *row_off = nullptr, *hist_off = nullptr, *small = nullptr, *d_cs = nullptr, *bs_r = nullptr;
    char *d_fs = nullptr;
    int32_t *d_rd = nullptr, *d_cso = nullptr, *d_csl = nullptr;
    float *d_rinv = nullptr;
    auto lay = [&](sp_carve cv) {
        d_lists = cv.take<sps_list>((size_t)C);
        bnd = cv.take<uint32_t>((size_t)C * (size_t)(R + 1));
        n_rows = cv.take<uint32_t>((size_t)R);
        n_hist = cv.take<uint32_t>((size_t)R);
        row_off = cv.take<unsigned long long>((size_t)R + 1);
        hist_off = cv.take<unsigned long long>((size_t)R + 1);
        d_fs = cv.take<char>(sp_fsets_bytes(n_sets, n_units, (size_t)n_uc + 1));
        small = cv.take<unsigned long long>(32);
        d_cs = cv.take<unsigned long long>((size_t)C);
        bs_r = cv.take<unsigned long long>(n_bs);      // (bs_h follows bs_r at once; the second slot is its room)
        cv.take<unsigned long long>(n_bs);
        d_rd = cv.take<int32_t>(BJ_FC);
        d_rinv = cv.take<float>(BJ_FC);
        if (rp.wide) {
            d_cso = cv.take<int32_t>(h_cso.size());
            d_csl = cv.take<int32_t>(h_cs.size() + 1);
        }
        return cv.off;
    };
    int rc = sp_buf_ensure(ctx, ctx->b_sp_a, (int64_t)lay(sp_carve()));
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sp_b, total * 8 + 64);
    if (rc) return rc;
    lay(sp_carve(ctx->b_sp_a.p));
    unsigned long long *bs_h = bs_r + n_bs;
    sps_join_args A;
    SP_HIP(ctx, hipMemcpyAsync(d_lists, hl.data(), (size_t)C * sizeof(sps_list), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, sp_fsets_upload(ctx->stream, d_fs, n_sets, set_off, unit_off, unit_chrom, (size_t)n_uc + 1, den.data(), min_fold,
                                baseline, min_freq, max_freq, ratio, A.F));
    if (rp.wide) {
        SP_HIP(ctx, hipMemcpyAsync(d_cso, h_cso.data(), h_cso.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!h_cs.empty()) SP_HIP(ctx, hipMemcpyAsync(d_csl, h_cs.data(), h_cs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    SP_HIP(ctx, hipMemsetAsync(bnd, 0, (size_t)C * (size_t)(R + 1) * 4, ctx->stream));
    {
        int64_t gx = (longest + 255) / 256;
        if (gx > (int64_t)ctx->n_cu * 16) gx = (int64_t)ctx->n_cu * 16;
        SP_LAUNCH(ctx, "sps_bounds", sps_bounds, dim3((unsigned)(gx > 0 ? gx : 1), (unsigned)C), dim3(256), 0,
                  (const sps_list *)d_lists, rp.shift, R, bnd);
    }
    if (!walk.rd.empty()) {
        SP_HIP(ctx, hipMemcpyAsync(d_rd, walk.rd.data(), walk.rd.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        SP_HIP(ctx, hipMemcpyAsync(d_rinv, walk.rinv.data(), walk.rd.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    SP_HIP(ctx, hipMemcpyAsync(d_cs, masks.cs.data(), (size_t)C * 8, hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (the plan's host arrays are free to go from here on)
    A.C = C;
    A.shift = rp.shift;
    A.R = R;
    A.fast = walk.fast;
    A.n_rd = (int)walk.rd.size();
    A.rd = d_rd;
    A.rinv = d_rinv;
    A.screen = masks.screen;
    A.chrom_sets = d_cs;
    A.lists = d_lists;
    A.bnd = bnd;
    A.n_rows = n_rows;
    A.n_hist = n_hist;
    A.hist_stage = (unsigned long long *)ctx->b_sp_b.p;
    A.row_cursor = small + 1;
    A.n_union = small;
    sps_wide_args W;
    W.cset_off = d_cso;
    W.cset = d_csl;
    W.generic = generic ? 1 : 0;
    // ---- run
    unsigned long long row_cap = sp_plan_row_cap(total, ctx->n_cu);
    unsigned long long h[4] = {0, 0, 0, 0};
    for (int attempt = 0;; attempt++) {
        // b_sp_c, the row staging: keys | tot | rank inside the range | counts
        auto lay_rows = [&](sp_carve cv) {
            A.row_keys = cv.take<unsigned long long>(row_cap);
            A.row_tot = cv.take<unsigned long long>(row_cap);
            A.row_rank = cv.take<uint32_t>(row_cap);
            A.row_counts = cv.take<uint32_t>(row_cap * (size_t)C);
            return cv.off;
        };
        const int64_t stage_bytes = (int64_t)(lay_rows(sp_carve()) + 64);
        if (pick) {     // (phase A, frequency bounds open: with min_fold <= 0 every slot of the set chromosomes is a row)
            char what[160];
            snprintf(what, sizeof what, "the candidates of the set chromosomes (%llu rows x %d lists x 4 B staged)",
                     row_cap, C);
            if ((rc = sps_fits(ctx, ctx->b_sp_c, stage_bytes, what))) return rc;
        }
        rc = sp_buf_ensure(ctx, ctx->b_sp_c, stage_bytes);
        if (rc) return rc;
        lay_rows(sp_carve(ctx->b_sp_c.p));
        A.row_cap = row_cap;
        SP_HIP(ctx, hipMemsetAsync(A.row_keys, 0xff, row_cap * 8, ctx->stream));
        SP_HIP(ctx, hipMemsetAsync(small, 0, 64, ctx->stream));
        rc = rp.shift <= 31 ? sps_join_launch<uint32_t>(ctx, A, rp.wide ? &W : nullptr)
                            : sps_join_launch<unsigned long long>(ctx, A, rp.wide ? &W : nullptr);
        if (rc) return rc;
        const long long nb = (R + TALLY_CHUNK - 1) / TALLY_CHUNK;
        SP_LAUNCH(ctx, "sps_tally_sums", sps_tally_sums, dim3((unsigned)nb), dim3(256), 0, (const uint32_t *)n_rows, R, bs_r);
        SP_LAUNCH(ctx, "sps_tally_sums", sps_tally_sums, dim3((unsigned)nb), dim3(256), 0, (const uint32_t *)n_hist, R, bs_h);
        SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, bs_r, (int64_t)nb, small + 2);
        SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, bs_h, (int64_t)nb, small + 3);
        SP_LAUNCH(ctx, "sps_tally_apply", sps_tally_apply, dim3((unsigned)nb), dim3(256), 0, (const uint32_t *)n_rows, R,
                  (const unsigned long long *)bs_r, (const unsigned long long *)(small + 2), row_off);
        SP_LAUNCH(ctx, "sps_tally_apply", sps_tally_apply, dim3((unsigned)nb), dim3(256), 0, (const uint32_t *)n_hist, R,
                  (const unsigned long long *)bs_h, (const unsigned long long *)(small + 3), hist_off);
        SP_HIP(ctx, hipMemcpyAsync(h, small, 32, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h[1] <= row_cap) break;
        if (attempt) return sp_fail(ctx, SP_ESTATE, "list filter: row staging overran twice (%llu > %llu)", h[1], row_cap);
        row_cap = sp_plan_row_retry(h[1], ctx->n_cu);
    }
    // ---- place
    ctx->n_union = (int64_t)h[0];
    ctx->n_rows = (int64_t)h[2];
    ctx->n_hist = (int64_t)h[3];
    const int64_t M = ctx->n_rows, H = ctx->n_hist;
    rc = sp_buf_ensure(ctx, ctx->b_sf_keys, (M + 1) * 8);
    if (rc) return rc;
    if (!pick) {
        rc = sp_buf_ensure(ctx, ctx->b_sf_counts, (M + 1) * (int64_t)C * 4);
        if (rc) return rc;
    }
    rc = sp_buf_ensure(ctx, ctx->b_sf_tot, (M + 1) * 8);
    if (rc) return rc;
    rc = sp_buf_ensure(ctx, ctx->b_sf_hist, (H + 1) * 8);
    if (rc) return rc;
    if (M)
        SP_LAUNCH(ctx, "sps_place_rows", sps_place_rows, dim3((unsigned)((h[1] + 255) / 256)), dim3(256), 0,
                  (const unsigned long long *)A.row_keys, (const unsigned long long *)A.row_tot, (const uint32_t *)A.row_rank,
                  (const uint32_t *)A.row_counts, h[1], C, rp.shift, (const unsigned long long *)row_off,
                  (unsigned long long *)ctx->b_sf_keys.p, pick ? (uint32_t *)nullptr : (uint32_t *)ctx->b_sf_counts.p,
                  (unsigned long long *)ctx->b_sf_tot.p);
    if (H)
        SP_LAUNCH(ctx, "sps_place_hist", sps_place_hist, dim3((unsigned)((R + 255) / 256)), dim3(256), 0,
                  (const unsigned long long *)A.hist_stage, (const uint32_t *)bnd, C, R, (const uint32_t *)n_hist,
                  (const unsigned long long *)hist_off, (unsigned long long *)ctx->b_sf_hist.p);
    if (M && ctx->list_mode && !pick)
        SP_LAUNCH(ctx, "sps_slots_to_keys", sps_slots_to_keys, dim3((unsigned)((M + 255) / 256)), dim3(256), 0,
                  (unsigned long long *)ctx->b_sf_keys.p, M, sp_make_kparams(ctx->k));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->filtered = true;
    return SP_OK;
}

// ------------------------------------------------------------------ list filter with passengers (k <= 15, C > SP_LIST_MAXC)
// Set chromosomes (named by a set of two or more units) decide; every other chromosome -- a singleton config line, or
// through the C-ABI a chromosome in no set: a "passenger" -- only adds to a k-mer's tot and its row.
//   phase A  sps_filter_join over the set chromosomes' lists alone (sps_join_blk / sps_join_wide, frequency bounds open):
//            its rows are the slots that pass the fold and ratio tests, ascending.  Exact: sp_filter_decide reads the set
//            chromosomes only.  A slot that no set chromosome holds is decided like an all-zero row (sps_sg_zero).
//   phase B  bitmaps over the dense slot space (2^(2k-1) bits: 64 MiB at k = 15), a few streaming passes:
//     sps_sg_mark     every entry of every list -> union bits U (+ bits H of the set chromosomes' entries when an all-zero
//                     row passes); 32-bit atomic ORs, one per run of a thread's entries in the same 32-slot word
//     sps_sg_cand     phase A's slots -> candidate bits X
//     sps_sg_sums     X |= U & ~H (all-zero row passes); popcounts of X and U per block of words
//     sps_sg_dir      rank directory D[w] = candidates in the words before w; candidate index -> slot
//     sps_sg_tot      every entry on a candidate slot: tot[rank] += count (64-bit atomics; tot is the hist)
//     sps_sg_rows / sps_sg_place   row iff !(tot < min_freq || tot > max_freq) (:645-646), scan -> keys, tot, row index
//     sps_sg_scatter  every entry on a row slot -> counts[row][chromosome] (zeroed rows, plain stores)
#define SG_BLOCK 256
#define SG_PER 16                      // entries (bitmap words) per thread
#define SG_SPAN (SG_BLOCK * SG_PER)    // entries of one list per workgroup ("chunk"); 64-bit words per workgroup

__global__ void __launch_bounds__(64)
sps_sg_zero(sp_fsets F, int *__restrict__ out) {
    if (threadIdx.x) return;
    bool is_row, is_hist;
    sp_filter_decide([](int) -> uint32_t { return 0u; }, 0ULL, F, is_row, is_hist);
    out[0] = is_hist ? 1 : 0;
}

// a workgroup per chunk (list, first entry); a thread walks SG_PER consecutive entries of the sorted list
template <bool HELD>
__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_mark(const sps_list *__restrict__ lists, const uint2 *__restrict__ chunks, const uint8_t *__restrict__ is_set,
            uint32_t *__restrict__ U, uint32_t *__restrict__ H) {
    const uint2 ch = chunks[blockIdx.x];
    const sps_list L = lists[ch.x];
    const long long lo = (long long)ch.y + (long long)threadIdx.x * SG_PER;
    const long long hi = lo + SG_PER < L.n ? lo + SG_PER : L.n;
    const bool held = HELD && is_set[ch.x];
    uint32_t wp = 0, bits = 0;
    for (long long i = lo; i < hi; i++) {
        const uint32_t s = (uint32_t)L.keys[i], w = s >> 5;
        if (bits && w != wp) {
            atomicOr(&U[wp], bits);
            if (held) atomicOr(&H[wp], bits);
            bits = 0;
        }
        wp = w;
        bits |= 1u << (s & 31);
    }
    if (bits) {
        atomicOr(&U[wp], bits);
        if (held) atomicOr(&H[wp], bits);
    }
}

__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_cand(const unsigned long long *__restrict__ slots, int64_t n, uint32_t *__restrict__ X) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = (uint32_t)slots[i];
    atomicOr(&X[s >> 5], 1u << (s & 31));
}

__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_sums(const unsigned long long *__restrict__ U, const unsigned long long *__restrict__ H,
            unsigned long long *__restrict__ X, int64_t W, int zero_pass, unsigned long long *__restrict__ bsum_x,
            unsigned long long *__restrict__ bsum_u) {
    __shared__ unsigned long long red[16];
    const int64_t w0 = (int64_t)blockIdx.x * SG_SPAN;
    unsigned long long nx = 0, nu = 0;
    for (int j = 0; j < SG_PER; j++) {
        const int64_t w = w0 + (int64_t)j * SG_BLOCK + threadIdx.x;
        if (w >= W) break;
        const unsigned long long u = U[w];
        unsigned long long x = X[w];
        if (zero_pass) {
            x |= u & ~H[w];
            X[w] = x;
        }
        nx += (unsigned long long)__popcll(x);
        nu += (unsigned long long)__popcll(u);
    }
    const unsigned long long tx = sp_block_sum_u64(nx, red);
    const unsigned long long tu = sp_block_sum_u64(nu, red);
    if (threadIdx.x == 0) {
        bsum_x[blockIdx.x] = tx;
        bsum_u[blockIdx.x] = tu;
    }
}

// D[w] and the slots of the candidates; a thread owns SG_PER consecutive words (the order of the ranks)
__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_dir(const unsigned long long *__restrict__ X, int64_t W, const unsigned long long *__restrict__ boff,
           uint32_t *__restrict__ D, uint32_t *__restrict__ slot_of) {
    __shared__ unsigned long long wsum[16];
    const int64_t t0 = (int64_t)blockIdx.x * SG_SPAN + (int64_t)threadIdx.x * SG_PER;
    unsigned long long s = 0;
    for (int j = 0; j < SG_PER; j++)
        if (t0 + j < W) s += (unsigned long long)__popcll(X[t0 + j]);
    unsigned long long tot;
    unsigned long long run = boff[blockIdx.x] + sp_block_excl_scan(s, wsum, tot);
    for (int j = 0; j < SG_PER; j++) {
        const int64_t w = t0 + j;
        if (w >= W) break;
        D[w] = (uint32_t)run;
        for (unsigned long long x = X[w]; x; x &= x - 1) slot_of[run++] = (uint32_t)((w << 6) + __builtin_ctzll(x));
    }
}

// rank of slot s among the candidates, or -1
__device__ __forceinline__ long long sg_rank(const unsigned long long *__restrict__ X, const uint32_t *__restrict__ D,
                                             uint32_t s) {
    const unsigned long long x = X[s >> 6], b = 1ULL << (s & 63);
    return (x & b) ? (long long)D[s >> 6] + __popcll(x & (b - 1)) : -1LL;
}

__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_tot(const sps_list *__restrict__ lists, const uint2 *__restrict__ chunks, const unsigned long long *__restrict__ X,
           const uint32_t *__restrict__ D, unsigned long long *__restrict__ tot) {
    const uint2 ch = chunks[blockIdx.x];
    const sps_list L = lists[ch.x];
    const long long lo = (long long)ch.y + (long long)threadIdx.x * SG_PER;
    const long long hi = lo + SG_PER < L.n ? lo + SG_PER : L.n;
    for (long long i = lo; i < hi; i++) {
        const long long r = sg_rank(X, D, (uint32_t)L.keys[i]);
        if (r >= 0) atomicAdd(&tot[r], (unsigned long long)L.cnts[i]);
    }
}

__device__ __forceinline__ bool sg_is_row(unsigned long long tot, double min_freq, double max_freq) {
    const double t = (double)tot;
    return !(t < min_freq || t > max_freq);      // :645-646
}

__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_rows(const unsigned long long *__restrict__ tot, int64_t n, double min_freq, double max_freq,
            unsigned long long *__restrict__ bsum) {
    __shared__ unsigned long long red[16];
    const int64_t i0 = (int64_t)blockIdx.x * SG_SPAN;
    unsigned long long c = 0;
    for (int j = 0; j < SG_PER; j++) {
        const int64_t i = i0 + (int64_t)j * SG_BLOCK + threadIdx.x;
        if (i < n && sg_is_row(tot[i], min_freq, max_freq)) c++;
    }
    const unsigned long long t = sp_block_sum_u64(c, red);
    if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}

__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_place(const unsigned long long *__restrict__ tot, const uint32_t *__restrict__ slot_of, int64_t n, double min_freq,
             double max_freq, const unsigned long long *__restrict__ boff, uint32_t *__restrict__ row_of,
             unsigned long long *__restrict__ out_keys, unsigned long long *__restrict__ out_tot) {
    __shared__ uint32_t lds[16];
    const int64_t i0 = (int64_t)blockIdx.x * SG_SPAN;
    unsigned long long off = boff[blockIdx.x];
    for (int j = 0; j < SG_PER; j++) {
        const int64_t i = i0 + (int64_t)j * SG_BLOCK + threadIdx.x;
        const unsigned long long t = i < n ? tot[i] : 0ULL;
        const bool p = i < n && sg_is_row(t, min_freq, max_freq);
        uint32_t nblk;
        const uint32_t my = sp_block_excl_count(p, lds, nblk);
        if (i < n) row_of[i] = p ? (uint32_t)(off + my) : 0xffffffffu;
        if (p) {
            out_keys[off + my] = slot_of[i];
            out_tot[off + my] = t;
        }
        off += nblk;
    }
}

__global__ void __launch_bounds__(SG_BLOCK)
sps_sg_scatter(const sps_list *__restrict__ lists, const uint2 *__restrict__ chunks, const unsigned long long *__restrict__ X,
               const uint32_t *__restrict__ D, const uint32_t *__restrict__ row_of, int C, uint32_t *__restrict__ counts) {
    const uint2 ch = chunks[blockIdx.x];
    const sps_list L = lists[ch.x];
    const long long lo = (long long)ch.y + (long long)threadIdx.x * SG_PER;
    const long long hi = lo + SG_PER < L.n ? lo + SG_PER : L.n;
    for (long long i = lo; i < hi; i++) {
        const long long r = sg_rank(X, D, (uint32_t)L.keys[i]);
        if (r < 0) continue;
        const uint32_t row = row_of[r];
        if (row != 0xffffffffu) counts[(size_t)row * (size_t)C + ch.x] = L.cnts[i];
    }
}

static int sps_filter_passengers(sp_ctx *ctx, int n_sets, const int32_t *set_off, const int32_t *unit_off,
                                 const int32_t *unit_chrom, const std::vector<double> &den, double min_fold, int baseline,
                                 double min_freq, double max_freq, double ratio) {
    const int C = sps_C(ctx);
    const int n_units = set_off[n_sets];
    // ---- phase A: the set chromosomes, renumbered in ascending order; the sets of one unit left out
    const sp_passenger_plan pa = sp_plan_passengers(C, n_sets, set_off, unit_off, unit_chrom, den.data());
    if ((int)pa.pick.size() > SP_LIST_MAXC)
        return sp_fail(ctx, SP_EUNSUP, "list filter: at most %d set chromosomes (chromosomes named by a set of two or more "
                                       "units) supported (got %d of %d chromosomes)", SP_LIST_MAXC, (int)pa.pick.size(), C);
    int rc = sps_filter_join(ctx, (int)pa.a_so.size() - 1, pa.a_so.data(), pa.a_uo.data(), pa.a_uc.data(), pa.a_den, min_fold,
                             baseline, -1.0, HUGE_VAL, ratio, &pa.pick);
    if (rc) return rc;
    const int64_t n_a = ctx->n_rows;      // phase A's slots, ascending, in b_sf_keys
    // ---- phase B
    int64_t total = 0;
    std::vector<sps_list> hl((size_t)C);
    std::vector<uint2> hc;
    std::vector<uint8_t> hs((size_t)C, 0);
    for (int c = 0; c < C; c++) {
        const int64_t n = sps_n(ctx, c);
        hl[(size_t)c] = sps_list{sps_keys(ctx, c), sps_cnts(ctx, c), (long long)n};
        hs[(size_t)c] = pa.num[(size_t)c] >= 0;
        total += n;
        for (int64_t s = 0; s < n; s += SG_SPAN) hc.push_back(make_uint2((unsigned)c, (unsigned)s));
    }
    ctx->sf_n = total;
    ctx->n_union = ctx->n_rows = ctx->n_hist = 0;
    ctx->filtered = false;
    const int64_t W = (ctx->nslots + 63) / 64, nbw = (W + SG_SPAN - 1) / SG_SPAN;
    // b_sp_a: lists | chunks | set flags | set arrays of sps_sg_zero | block sums of the words (X, U) | small
    //         ([0] candidates [1] union [2] rows [3] the all-zero decision) | block sums of the candidates (room for
    //         every slot being one)
    const size_t nch = hc.size(), nuc = (size_t)unit_off[n_units];
    sps_list *d_l = nullptr;
    uint2 *d_ch = nullptr;
    uint8_t *d_is = nullptr;
    char *d_fs = nullptr;
    unsigned long long *bx = nullptr, *bu = nullptr, *small = nullptr, *br = nullptr;
    auto lay_a = [&](sp_carve cv) {
        d_l = cv.take<sps_list>((size_t)C);
        d_ch = cv.take<uint2>(nch + 1);
        d_is = cv.take<uint8_t>((size_t)C);
        d_fs = cv.take<char>(sp_fsets_bytes(n_sets, n_units, nuc + 1));
        bx = cv.take<unsigned long long>((size_t)nbw + 1);
        bu = cv.take<unsigned long long>((size_t)nbw + 1);
        small = cv.take<unsigned long long>(32);
        br = cv.take<unsigned long long>((size_t)(ctx->nslots / SG_SPAN + 2));
        return cv.off;
    };
    // b_sp_b: U | X | H | D
    unsigned long long *U = nullptr, *X = nullptr, *H = nullptr;
    uint32_t *D = nullptr;
    auto lay_b = [&](sp_carve cv) {
        U = cv.take<unsigned long long>((size_t)W);
        X = cv.take<unsigned long long>((size_t)W);
        H = cv.take<unsigned long long>((size_t)W);
        D = cv.take<uint32_t>((size_t)W);
        return cv.off;
    };
    const size_t b_bytes = lay_b(sp_carve());
    if ((rc = sps_fits(ctx, ctx->b_sp_b, (int64_t)b_bytes, "the slot bitmaps and their rank directory"))) return rc;
    if ((rc = sp_buf_ensure(ctx, ctx->b_sp_b, (int64_t)b_bytes))) return rc;
    if ((rc = sp_buf_ensure(ctx, ctx->b_sp_a, (int64_t)lay_a(sp_carve())))) return rc;
    lay_a(sp_carve(ctx->b_sp_a.p));
    lay_b(sp_carve(ctx->b_sp_b.p));
    SP_HIP(ctx, hipMemcpyAsync(d_l, hl.data(), (size_t)C * sizeof(sps_list), hipMemcpyHostToDevice, ctx->stream));
    if (nch) SP_HIP(ctx, hipMemcpyAsync(d_ch, hc.data(), nch * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
    SP_HIP(ctx, hipMemcpyAsync(d_is, hs.data(), (size_t)C, hipMemcpyHostToDevice, ctx->stream));
    sp_fsets F;
    SP_HIP(ctx, sp_fsets_upload(ctx->stream, d_fs, n_sets, set_off, unit_off, unit_chrom, nuc + 1, den.data(), min_fold, baseline,
                                min_freq, max_freq, ratio, F));
    SP_HIP(ctx, hipMemsetAsync(small, 0, 256, ctx->stream));
    SP_LAUNCH(ctx, "sps_sg_zero", sps_sg_zero, dim3(1), dim3(64), 0, F, (int *)(small + 3));
    unsigned long long h[4] = {0, 0, 0, 0};
    SP_HIP(ctx, hipMemcpyAsync(h, small, 32, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (the host vectors go out of scope)
    const int zero_pass = (int)(h[3] & 1);
    const char *clear_end = zero_pass ? (const char *)D : (const char *)H;     // U, X (, H)
    SP_HIP(ctx, hipMemsetAsync(U, 0, (size_t)(clear_end - (const char *)U), ctx->stream));
    if (nch) {
        if (zero_pass)
            SP_LAUNCH(ctx, "sps_sg_mark", sps_sg_mark<true>, dim3((unsigned)nch), dim3(SG_BLOCK), 0, (const sps_list *)d_l,
                      (const uint2 *)d_ch, (const uint8_t *)d_is, (uint32_t *)U, (uint32_t *)H);
        else
            SP_LAUNCH(ctx, "sps_sg_mark", sps_sg_mark<false>, dim3((unsigned)nch), dim3(SG_BLOCK), 0, (const sps_list *)d_l,
                      (const uint2 *)d_ch, (const uint8_t *)d_is, (uint32_t *)U, (uint32_t *)nullptr);
    }
    if (n_a)
        SP_LAUNCH(ctx, "sps_sg_cand", sps_sg_cand, dim3((unsigned)((n_a + SG_BLOCK - 1) / SG_BLOCK)), dim3(SG_BLOCK), 0,
                  (const unsigned long long *)ctx->b_sf_keys.p, n_a, (uint32_t *)X);
    SP_LAUNCH(ctx, "sps_sg_sums", sps_sg_sums, dim3((unsigned)nbw), dim3(SG_BLOCK), 0, (const unsigned long long *)U,
              (const unsigned long long *)H, X, W, zero_pass, bx, bu);
    SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, bx, nbw, small);
    SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, bu, nbw, small + 1);
    SP_HIP(ctx, hipMemcpyAsync(h, small, 16, hipMemcpyDeviceToHost, ctx->stream));
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t n_cand = (int64_t)h[0];
    ctx->n_union = (int64_t)h[1];
    // b_sp_c: slot of every candidate | row index of every candidate; b_sf_hist: the candidates' tot (= the hist)
    uint32_t *slot_of = nullptr, *row_of = nullptr;
    auto lay_c = [&](sp_carve cv) {
        slot_of = cv.take<uint32_t>((size_t)n_cand + 1);
        row_of = cv.take<uint32_t>((size_t)n_cand + 1);
        return cv.off;
    };
    const size_t c_bytes = lay_c(sp_carve());
    if ((rc = sps_fits(ctx, ctx->b_sp_c, (int64_t)c_bytes, "the candidates' slots and row indices"))) return rc;
    if ((rc = sp_buf_ensure(ctx, ctx->b_sp_c, (int64_t)c_bytes))) return rc;
    if ((rc = sps_fits(ctx, ctx->b_sf_hist, (n_cand + 1) * 8, "the candidates' totals"))) return rc;
    if ((rc = sp_buf_ensure(ctx, ctx->b_sf_hist, (n_cand + 1) * 8))) return rc;
    lay_c(sp_carve(ctx->b_sp_c.p));
    unsigned long long *tot = (unsigned long long *)ctx->b_sf_hist.p;
    SP_LAUNCH(ctx, "sps_sg_dir", sps_sg_dir, dim3((unsigned)nbw), dim3(SG_BLOCK), 0, (const unsigned long long *)X, W,
              (const unsigned long long *)bx, D, slot_of);
    int64_t M = 0;
    if (n_cand) {
        SP_HIP(ctx, hipMemsetAsync(tot, 0, (size_t)n_cand * 8, ctx->stream));
        SP_LAUNCH(ctx, "sps_sg_tot", sps_sg_tot, dim3((unsigned)nch), dim3(SG_BLOCK), 0, (const sps_list *)d_l, (const uint2 *)d_ch,
                  (const unsigned long long *)X, (const uint32_t *)D, tot);
        // rows: the candidates whose tot lies within the bounds, in slot order
        const int64_t nbc = (n_cand + SG_SPAN - 1) / SG_SPAN;      // <= nslots / SG_SPAN + 1
        SP_LAUNCH(ctx, "sps_sg_rows", sps_sg_rows, dim3((unsigned)nbc), dim3(SG_BLOCK), 0, (const unsigned long long *)tot,
                  n_cand, min_freq, max_freq, br);
        SP_LAUNCH(ctx, "scan_excl_u64", scan_excl_u64, dim3(1), dim3(1024), 0, br, nbc, small + 2);
        SP_HIP(ctx, hipMemcpyAsync(h + 2, small + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        M = (int64_t)h[2];
        const int64_t cnt_bytes = (M + 1) * (int64_t)C * 4;
        char what[128];
        snprintf(what, sizeof what, "the rows (%lld rows x %d chromosomes x 4 B)", (long long)M, C);
        if ((rc = sps_fits(ctx, ctx->b_sf_counts, cnt_bytes, what))) return rc;
        if ((rc = sp_buf_ensure(ctx, ctx->b_sf_keys, (M + 1) * 8))) return rc;
        if ((rc = sp_buf_ensure(ctx, ctx->b_sf_tot, (M + 1) * 8))) return rc;
        if ((rc = sp_buf_ensure(ctx, ctx->b_sf_counts, cnt_bytes))) return rc;
        SP_LAUNCH(ctx, "sps_sg_place", sps_sg_place, dim3((unsigned)nbc), dim3(SG_BLOCK), 0, (const unsigned long long *)tot,
                  (const uint32_t *)slot_of, n_cand, min_freq, max_freq, (const unsigned long long *)br, row_of,
                  (unsigned long long *)ctx->b_sf_keys.p, (unsigned long long *)ctx->b_sf_tot.p);
        if (M) {
            SP_HIP(ctx, hipMemsetAsync(ctx->b_sf_counts.p, 0, (size_t)M * (size_t)C * 4, ctx->stream));
            SP_LAUNCH(ctx, "sps_sg_scatter", sps_sg_scatter, dim3((unsigned)nch), dim3(SG_BLOCK), 0, (const sps_list *)d_l, (const uint2 *)d_ch,
                      (const unsigned long long *)X, (const uint32_t *)D, (const uint32_t *)row_of, C,
                      (uint32_t *)ctx->b_sf_counts.p);
            SP_LAUNCH(ctx, "sps_slots_to_keys", sps_slots_to_keys, dim3((unsigned)((M + 255) / 256)), dim3(256), 0,
                      (unsigned long long *)ctx->b_sf_keys.p, M, sp_make_kparams(ctx->k));
        }
    }
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_rows = M;
    ctx->n_hist = n_cand;
    ctx->filtered = true;
    return SP_OK;
}

// SP_LIST_FILTER=sort selects the first implementation (concatenate + library radix sort), kept as a cross-check; list
// mode (k <= 15) above SP_LIST_MAXC chromosomes filters in two phases (sps_filter_passengers)
int sp_sparse_filter(sp_ctx *ctx, int n_sets, const int32_t *set_off, const int32_t *unit_off,
                     const int32_t *unit_chrom, const std::vector<double> &den, double min_fold, int baseline,
                     double min_freq, double max_freq, double ratio) {
    const char *e = getenv("SP_LIST_FILTER");
    if (e && !strcmp(e, "sort"))
        return sps_filter_sort(ctx, n_sets, set_off, unit_off, unit_chrom, den, min_fold, baseline, min_freq, max_freq, ratio);
    if (ctx->list_mode && !ctx->sv_on && sps_C(ctx) > SP_LIST_MAXC)
        return sps_filter_passengers(ctx, n_sets, set_off, unit_off, unit_chrom, den, min_fold, baseline, min_freq, max_freq,
                                     ratio);
    return sps_filter_join(ctx, n_sets, set_off, unit_off, unit_chrom, den, min_fold, baseline, min_freq, max_freq, ratio);
}

int sp_sparse_fetch(sp_ctx *ctx, bool hist, uint64_t *keys, uint32_t *counts, double *freqs, uint64_t *tot, bool async) {
    const int C = sps_C(ctx);
    const int64_t M = hist ? ctx->n_hist : ctx->n_rows;
    if (M == 0) return SP_OK;
    if (hist) {
        SP_HIP(ctx, hipMemcpyAsync(tot, ctx->b_sf_hist.p, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
        SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return SP_OK;
    }
    std::vector<uint32_t> tmp;
    uint32_t *cdst = counts;
    if (!counts && freqs) {
        tmp.resize((size_t)M * C);
        cdst = tmp.data();
    }
    // async (sp_filter_fetch_async: no frequencies): the join left the rows in device buffers that nothing writes before the
    // next filter call -- a copy stream takes them to the (page-locked) host buffers while the compute stream goes on with the
    // map stage; sp_filter_fetch_wait joins the two (as the table engines do since round 4)
    hipStream_t cs = ctx->stream;
    async = async && !freqs;
    if (async) {
        if (!ctx->copy_stream) {
            SP_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
            SP_HIP(ctx, hipEventCreateWithFlags(&ctx->copy_event, hipEventDisableTiming));
        }
        SP_HIP(ctx, hipEventRecord(ctx->copy_event, ctx->stream));
        SP_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->copy_event, 0));
        cs = ctx->copy_stream;
    }
    if (keys) SP_HIP(ctx, hipMemcpyAsync(keys, ctx->b_sf_keys.p, (size_t)M * 8, hipMemcpyDeviceToHost, cs));
    if (tot) SP_HIP(ctx, hipMemcpyAsync(tot, ctx->b_sf_tot.p, (size_t)M * 8, hipMemcpyDeviceToHost, cs));
    if (cdst) SP_HIP(ctx, hipMemcpyAsync(cdst, ctx->b_sf_counts.p, (size_t)M * C * 4, hipMemcpyDeviceToHost, cs));
    if (async) return SP_OK;
    SP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (freqs)
        for (int64_t r = 0; r < M; r++)
            for (int c = 0; c < C; c++)   // count/length in fp64 (Jellyfish.py:647); IEEE division, same bits as the device path
                freqs[r * C + c] = (double)cdst[r * C + c] / (double)sps_len(ctx, c);
    return SP_OK;
}
