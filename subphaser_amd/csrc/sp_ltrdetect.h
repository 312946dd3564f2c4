// sp_ltrdetect.h -- the arithmetic of the de novo LTR-RT detection, compiled for the host and for the device.
//
// The reference finds LTR-RTs with ltr_finder and `gt ltrharvest` on 10-Mb chunks (LTR.py:33-42, :80-142); neither can be
// run or pinned here, so the detector is DEFINED by the integer arithmetic below: exact seeds at a bounded distance, a
// gapless X-drop extension, and (on the host, subphaser_amd/ltr.py) a chaining of the extended seeds.  Its parameters are
// the ones the reference passes to its detectors.  tests/ltrdetect_ref.py is the Python twin, written from the definition
// and compared with `==`.
//
//   positions  0-based on one chromosome of `len` < SP_BK_MAXLEN bases; a base is a code 0..3 or SP_LD_INVALID (whatever
//              the genome's validity mask marks: N, IUPAC, ...); the forward strand only -- LTRs are direct repeats
//   word       a start p is valid when none of its L bases is invalid (p + L <= len); its word is the 2L-bit number with
//              the first base most significant, SP_LD_LMIN <= L <= SP_LD_LMAX
//   partners   of a valid start p: the later valid starts q > p with the same word in ascending q -- no more than the first
//              SP_LD_SCAN of them are looked at, the walk stops at the first with q - p > dmax, those with q - p >= dmin
//              are partners and the first SP_LD_FANOUT of them are kept.  Low-complexity runs (a homopolymer, a short
//              tandem) lose seeds by this rule: their first SP_LD_SCAN successors are closer than dmin.  That is intended.
//   seed       a partner pair (p, q) that is left-maximal: p == 0, or base p - 1 or base q - 1 is invalid, or the two differ.
//              d = q - p, 1 <= dmin <= d <= dmax <= SP_LD_MAXDIST
//   extension  gapless, +2 for equal bases, -2 for different ones, cap = min(d, maxlen), maxlen <= SP_LD_MAXLEN.
//              right: e = L, s = best = 0, r = L; while e < cap, q + e < len and bases p + e, q + e are both valid: add the
//              column, e++, then s > best: best = s, r = e; else s < best - X: stop.
//              left: e = 0, s = best = 0, l = 0; while p - e - 1 >= 0, r + e < cap and bases p - e - 1, q - e - 1 are both
//              valid: the same step, giving l.
//   HSP        (p0 = p - l, n = r + l, d): n <= max(cap, L), so with d >= L the two copies never overlap.  One 64-bit word,
//              p0 high, n - 1 in 13 bits, d in 15 bits: its integer order is the order of the tuples.
//   HSP list   of a chromosome: the distinct HSPs, ascending
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SP_LD_HD __host__ __device__
#else
#define SP_LD_HD
#endif

#define SP_LD_LMIN 12
#define SP_LD_LMAX 20
#define SP_LD_SCAN 32
#define SP_LD_FANOUT 8
#define SP_LD_MAXDIST 32767            // d travels in 15 bits
#define SP_LD_MAXLEN 8192              // n - 1 travels in 13 bits; SP_LA_MAXLEN of sp_ltralign.h: every candidate is aligned
#define SP_LD_INVALID 4
#define SP_LD_MATCH 2
#define SP_LD_MISMATCH (-2)
#define SP_LD_POS_BITS 24              // a sorted element is (word << 24) | position in the chunk
#define SP_LD_POS_MASK 0xffffffULL
// starts a chunk owns by default: with the dmax + L bases a chunk holds behind them its positions stay below 2^24
#define SP_LD_BODY ((1 << SP_LD_POS_BITS) - 32768 - 32)
#define SP_LD_SEED_CAP (1 << 20)       // seeds the append buffer holds before it is sized from the count

// parameters: 0 when good; 1..3 are limits of this build (L, dmax, maxlen), 4..6 are never meaningful (dmin, X, maxlen)
SP_LD_HD inline int sp_ld_check(int L, int X, int64_t dmin, int64_t dmax, int64_t maxlen) {
    if (dmin < 1 || dmin > dmax) return 4;
    if (X < 0) return 5;
    if (maxlen < 1) return 6;
    if (L < SP_LD_LMIN || L > SP_LD_LMAX) return 1;
    if (dmax > SP_LD_MAXDIST) return 2;
    if (maxlen > SP_LD_MAXLEN) return 3;
    return 0;
}

// the word of start p, or false when the start is not valid.  B: int operator()(int64_t pos) const, 0 <= pos < len
template <typename B>
SP_LD_HD inline bool sp_ld_word(const B &base, int64_t len, int64_t p, int L, uint64_t *word) {
    if (p < 0 || p + L > len) return false;
    uint64_t w = 0;
    for (int j = 0; j < L; j++) {
        const int c = base(p + j);
        if (c >= SP_LD_INVALID) return false;
        w = (w << 2) | (uint64_t)c;
    }
    *word = w;
    return true;
}

SP_LD_HD inline uint64_t sp_ld_key(uint64_t word, uint32_t pos) { return (word << SP_LD_POS_BITS) | pos; }

// The partners of element i of `keys` -- the (word, position) elements of the valid starts, ascending: f(position) for
// each in ascending order; returns how many.
template <typename F>
SP_LD_HD inline int sp_ld_partners_each(const unsigned long long *keys, int64_t n, int64_t i, int64_t dmin, int64_t dmax, F &&f) {
    const uint64_t k = keys[i], w = k >> SP_LD_POS_BITS;
    const int64_t p = (int64_t)(k & SP_LD_POS_MASK);
    int kept = 0;
    for (int t = 1; t <= SP_LD_SCAN && i + t < n; t++) {
        const uint64_t k2 = keys[i + t];
        if ((k2 >> SP_LD_POS_BITS) != w) break;
        const int64_t d = (int64_t)(k2 & SP_LD_POS_MASK) - p;
        if (d > dmax) break;
        if (d >= dmin) {
            f((uint32_t)(k2 & SP_LD_POS_MASK));
            if (++kept == SP_LD_FANOUT) break;
        }
    }
    return kept;
}
// the same into out[SP_LD_FANOUT]
SP_LD_HD inline int sp_ld_partners(const unsigned long long *keys, int64_t n, int64_t i, int64_t dmin, int64_t dmax, uint32_t *out) {
    int at = 0;
    return sp_ld_partners_each(keys, n, i, dmin, dmax, [&](uint32_t q) { out[at++] = q; });
}

// is the partner pair (p, q) left-maximal?
template <typename B>
SP_LD_HD inline bool sp_ld_is_seed(const B &base, int64_t p, int64_t q) {
    if (p == 0) return true;
    const int x = base(p - 1), y = base(q - 1);
    return x >= SP_LD_INVALID || y >= SP_LD_INVALID || x != y;
}

// one column of an extension: false when it stops
SP_LD_HD inline bool sp_ld_step(bool equal, int X, int &s, int &best, int &e, int &at) {
    s += equal ? SP_LD_MATCH : SP_LD_MISMATCH;
    e++;
    if (s > best) {
        best = s;
        at = e;
    } else if (s < best - X) {
        return false;
    }
    return true;
}

// the HSP of the seed (p, q): its first base and its length
template <typename B>
SP_LD_HD inline void sp_ld_extend(const B &base, int64_t len, int64_t p, int64_t q, int L, int X, int64_t maxlen, int64_t *p0, int32_t *n) {
    const int64_t d = q - p;
    const int cap = (int)(d < maxlen ? d : maxlen);
    int e = L, s = 0, best = 0, r = L;
    while (e < cap && q + e < len) {
        const int x = base(p + e), y = base(q + e);
        if (x >= SP_LD_INVALID || y >= SP_LD_INVALID) break;
        if (!sp_ld_step(x == y, X, s, best, e, r)) break;
    }
    int l = 0;
    e = 0, s = 0, best = 0;
    while (p - e - 1 >= 0 && r + e < cap) {
        const int x = base(p - e - 1), y = base(q - e - 1);
        if (x >= SP_LD_INVALID || y >= SP_LD_INVALID) break;
        if (!sp_ld_step(x == y, X, s, best, e, l)) break;
    }
    *p0 = p - l;
    *n = r + l;
}

SP_LD_HD inline uint64_t sp_ld_hsp_pack(int64_t p0, int32_t n, int64_t d) {
    return ((uint64_t)p0 << 28) | ((uint64_t)(uint32_t)(n - 1) << 15) | (uint64_t)d;
}
SP_LD_HD inline void sp_ld_hsp_unpack(uint64_t h, int32_t *p0, int32_t *n, int32_t *d) {
    *p0 = (int32_t)(h >> 28);
    *n = (int32_t)((h >> 15) & 0x1fff) + 1;
    *d = (int32_t)(h & 0x7fff);
}
