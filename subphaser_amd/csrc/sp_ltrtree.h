// sp_ltrtree.h -- the arithmetic of the LTR-RT tree, compiled for the host and for the device.
//
// The reference builds its trees (LTR.LTRtree, __main__.py:622-638) from TEsorter's domain peptides with mafft, trimal and
// iqtree or FastTree.  None of these exists here, and neither do the HMM databases, so the tree of this build is DEFINED
// by the integer arithmetic below on the packed genome: bottom-s MinHash sketches of the elements' canonical k-mers, a
// pairwise comparison of the sketches, and neighbour joining on a fixed-point distance matrix.  tests/ltrtree_ref.py is the
// plain Python twin, written from this definition and compared with `==`.  The step from (shared, denom) to a distance is
// host arithmetic (subphaser_amd/ltrtree.py: mash_units).
//
// Sketch of an element (chrom, start, end), 0-based and half-open, end - start <= SP_LT_MAXLEN:
//   k-mer    a start p in [start, end - k] is valid when none of its k bases is invalid (the rule of sp_blocks.h);
//            key = min(fwd, rc) in key order (first base most significant, A = 0 .. T = 3); k is odd, SP_LT_KMIN..SP_LT_KMAX
//   hash     h = sp_bk_mix(key): a bijection of the 64-bit words.  The one word it sends to UINT64_MAX is
//            0xcf9a04affa6badc0, which is no key (keys are below 2^62), so UINT64_MAX is free to mean "unused"
//   sketch   the s smallest DISTINCT h of the element's valid starts, ascending; len <= s of them exist; entries len .. s - 1
//            are UINT64_MAX.  SP_LT_SMIN <= s <= SP_LT_SMAX, any integer.  "The s smallest of a set" is associative: the
//            sketch of a union of chunks is the bottom s of the chunks' bottom-s lists, whatever the chunks.
// Pair (A, B): walk the merge of the two ascending lists and count DISTINCT union values until denom = min(s, |A u B|) of
//   them are consumed; shared = how many of those are in both lists.  Two empty sketches: (0, 0).  pair(A, A) = (len, len).
// Neighbour joining on a symmetric int64 matrix D with zero diagonal and 0 <= D < 2^31 on input, slots 0 .. N - 1 all
//   live, 2 <= N <= SP_LT_MAXN.  R_i = sum of D(i, k) over the live k.  While n, the number of live slots, is above 2:
//   - the live pair i < j with the smallest Q = (n - 2) D(i, j) - R_i - R_j is joined, ties to the lowest i, then the
//     lowest j: the minimum of the triple (Q, i, j), which no order of comparison changes -- a reduction may find it;
//   - the record is (i, j, D(i, j), R_i, R_j);
//   - for every other live k:  D(i, k) = D(k, i) = floor((D(i, k) + D(j, k) - D(i, j)) / 2), floor toward minus infinity;
//   - slot j dies, slot i is the new node, and the sums are those of the new matrix (integers: updating R_k by the change
//     of its row and recomputing it give the same number).
//   The last record is (i, j, D(i, j), 0, 0) of the two slots left.  Output: (N - 1) x 5 int64; N = 2: that record alone.
//   Derived distances may be negative.
//   Guard: an updated |D| >= 2^40 (SP_LT_DMAX) stops the run with SP_LT_GUARD; the records are then undefined.  (The drivers
//   take the limit as an argument, 1 .. SP_LT_DMAX, so that tests can reach the guard with small matrices; a limit that is
//   not reached changes nothing.)  With every
//   |D| < 2^40 and n <= 4096 = 2^12:  |R| <= (n - 1) 2^40 < 2^52,  |(n - 2) D| < 2^52,  |Q| < 3 * 2^52 < 2^54, and the
//   numerator of an update is below 3 * 2^40: everything stays far inside 64 bits.
#pragma once
#include <stdint.h>
#include <string.h>

#include "sp_blocks.h"

#if defined(__HIPCC__)
#define SP_LT_HD __host__ __device__
#else
#define SP_LT_HD
#endif

#define SP_LT_KMIN 9
#define SP_LT_KMAX 31
#define SP_LT_SMIN 16
#define SP_LT_SMAX 4096
#define SP_LT_MAXLEN 65536
#define SP_LT_MAXN 4096
#define SP_LT_DIN (1LL << 31)        // input distances are below this
#define SP_LT_DMAX (1LL << 40)       // the guard
#define SP_LT_NONE (~0ULL)           // UINT64_MAX: an unused sketch entry
#define SP_LT_INVALID 4              // a base code that is no A, C, G, T (host drivers)

// status of a neighbour-joining run
#define SP_LT_OK 0
#define SP_LT_GUARD 1

// parameters: 0 when good, else the number of the first bad one (1 = k, 2 = s)
SP_LT_HD inline int sp_lt_check(int k, int s) {
    if (k < SP_LT_KMIN || k > SP_LT_KMAX || !(k & 1)) return 1;
    if (s < SP_LT_SMIN || s > SP_LT_SMAX) return 2;
    return 0;
}

// the 32 two-bit codes of a word in the opposite order
SP_LT_HD inline uint64_t sp_lt_rev2(uint64_t x) {
    x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0fULL) | ((x & 0x0f0f0f0f0f0f0f0fULL) << 4);
    x = ((x >> 8) & 0x00ff00ff00ff00ffULL) | ((x & 0x00ff00ff00ff00ffULL) << 8);
    x = ((x >> 16) & 0x0000ffff0000ffffULL) | ((x & 0x0000ffff0000ffffULL) << 16);
    return (x >> 32) | (x << 32);
}
// hash of the k-mer whose bases lie LSB-first in w (base t at bits 2t; bits from 2k on are ignored)
SP_LT_HD inline uint64_t sp_lt_hash(uint64_t w, int k) {
    const uint64_t kmask = (1ULL << (2 * k)) - 1ULL;
    const uint64_t fwd = sp_lt_rev2(w & kmask) >> (64 - 2 * k), rc = ~w & kmask;
    return sp_bk_mix(fwd < rc ? fwd : rc);
}

// one pair of sketches
SP_LT_HD inline void sp_lt_pair(const uint64_t *a, int la, const uint64_t *b, int lb, int s, int32_t *shared, int32_t *denom) {
    int i = 0, j = 0, sh = 0, dn = 0;
    while (dn < s && (i < la || j < lb)) {
        if (j >= lb) i++;
        else if (i >= la) j++;
        else {
            const uint64_t x = a[i], y = b[j];
            if (x < y) i++;
            else if (y < x) j++;
            else {
                sh++;
                i++;
                j++;
            }
        }
        dn++;
    }
    *shared = sh;
    *denom = dn;
}

// neighbour joining: the criterion, its order, the update and the guard
SP_LT_HD inline int64_t sp_lt_q(int n, int64_t d, int64_t ri, int64_t rj) { return (int64_t)(n - 2) * d - ri - rj; }
SP_LT_HD inline bool sp_lt_less(int64_t qa, int ia, int ja, int64_t qb, int ib, int jb) {
    return qa < qb || (qa == qb && (ia < ib || (ia == ib && ja < jb)));
}
SP_LT_HD inline int64_t sp_lt_floor_half(int64_t x) { return (x - (x & 1)) / 2; }
SP_LT_HD inline int64_t sp_lt_update(int64_t dik, int64_t djk, int64_t dij) { return sp_lt_floor_half(dik + djk - dij); }
SP_LT_HD inline bool sp_lt_guard(int64_t d, int64_t limit) { return d >= limit || d <= -limit; }

// ---- host drivers: the pieces above, looped in the stated orders
// codes: n bases, 0..3 or SP_LT_INVALID; sketch: s entries; returns len
static inline int32_t sp_lt_host_sketch(const uint8_t *codes, int64_t n, int k, int s, uint64_t *sketch) {
    int32_t len = 0;
    for (int t = 0; t < s; t++) sketch[t] = SP_LT_NONE;
    for (int64_t p = 0; p + k <= n; p++) {
        uint64_t w = 0;
        bool ok = true;
        for (int t = 0; t < k; t++) {
            if (codes[p + t] > 3) ok = false;
            w |= (uint64_t)(codes[p + t] & 3) << (2 * t);
        }
        if (!ok) continue;
        const uint64_t h = sp_lt_hash(w, k);
        // insert into the ascending list unless present or beyond its end
        int at = 0;
        while (at < len && sketch[at] < h) at++;
        if (at < len && sketch[at] == h) continue;
        if (at >= s) continue;
        const int last = len < s ? len : s - 1;      // index the tail moves up to
        for (int t = last; t > at; t--) sketch[t] = sketch[t - 1];
        sketch[at] = h;
        if (len < s) len++;
    }
    return len;
}
// sketch: n x s, len: n; shared, denom: n x n
static inline void sp_lt_host_pairs(const uint64_t *sketch, const int32_t *len, int n, int s, int32_t *shared, int32_t *denom) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++)
            sp_lt_pair(sketch + (int64_t)i * s, len[i], sketch + (int64_t)j * s, len[j], s, shared + (int64_t)i * n + j,
                       denom + (int64_t)i * n + j);
}
// D: N x N, rewritten; live: N bytes and R: N words of scratch; merges: (N - 1) x 5; limit: the guard (SP_LT_DMAX); returns
// the status
static inline int sp_lt_host_nj(int64_t *D, int N, uint8_t *live, int64_t *R, int64_t *merges, int64_t limit) {
    for (int i = 0; i < N; i++) {
        live[i] = 1;
        R[i] = 0;
        for (int k = 0; k < N; k++) R[i] += D[(int64_t)i * N + k];
    }
    int done = 0;
    for (int n = N; n > 2; n--) {
        int64_t bq = 0;
        int bi = -1, bj = -1;
        for (int i = 0; i < N; i++) {
            if (!live[i]) continue;
            for (int j = i + 1; j < N; j++) {
                if (!live[j]) continue;
                const int64_t q = sp_lt_q(n, D[(int64_t)i * N + j], R[i], R[j]);
                if (bi < 0 || sp_lt_less(q, i, j, bq, bi, bj)) {
                    bq = q;
                    bi = i;
                    bj = j;
                }
            }
        }
        const int64_t dij = D[(int64_t)bi * N + bj];
        int64_t *m = merges + 5 * (int64_t)done++;
        m[0] = bi;
        m[1] = bj;
        m[2] = dij;
        m[3] = R[bi];
        m[4] = R[bj];
        live[bj] = 0;
        int64_t ri = 0;
        for (int k = 0; k < N; k++) {
            if (!live[k] || k == bi) continue;
            const int64_t a = D[(int64_t)bi * N + k], b = D[(int64_t)bj * N + k], v = sp_lt_update(a, b, dij);
            if (sp_lt_guard(v, limit)) return SP_LT_GUARD;
            D[(int64_t)bi * N + k] = v;
            D[(int64_t)k * N + bi] = v;
            R[k] += v - a - b;
            ri += v;
        }
        R[bi] = ri;
    }
    int a = -1, b = -1;
    for (int i = 0; i < N; i++)
        if (live[i]) {
            if (a < 0) a = i;
            else b = i;
        }
    int64_t *m = merges + 5 * (int64_t)done;
    m[0] = a;
    m[1] = b;
    m[2] = D[(int64_t)a * N + b];
    m[3] = 0;
    m[4] = 0;
    return SP_LT_OK;
}
