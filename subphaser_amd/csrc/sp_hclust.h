// sp_hclust.h -- the arithmetic of the heatmap's dendrograms (Cluster.heatmap, the reference's Jellyfish.py:524-609, where
// R's heatmap.2 clusters the sampled k-mers and the chromosomes): Euclidean distances and complete-linkage clustering by
// the nearest-neighbour chain, with every order of operations and every tie rule stated, so that the result is
// bit-defined.  Sorting the merges by height and relabelling them to a linkage is host work (subphaser_amd/heatmap.py).
//
// __host__ __device__ and free of runtime calls, so that tests/test_hclust_host.py builds it with the host compiler and
// checks it against the numpy twin (tests/hclust_ref.py).  Build with -ffp-contract=off: the orders below are the
// definition, and a fused multiply-add changes the sums.  The square root is the correctly rounded one.
//
// Input: pts, P x D fp64 row-major, all finite; 2 <= P <= SP_HC_MAXP, D >= 1.
// Distance
//   d(i, j) = sqrt((p_i0 - p_j0)^2 + (p_i1 - p_j1)^2 + ...)   the sum strictly left to right from +0, every difference
//   and every square rounded before it is added.  (a - b)^2 == (b - a)^2 and a - a == +0 exactly, so the P x P matrix is
//   symmetric with a zero diagonal by construction; no entry is -0.
// Nearest-neighbour chain, complete linkage.  size[i] = 1 for all i; the chain starts empty.  For each of the P - 1 merges
//   - an empty chain starts at the lowest live index (live: size > 0);
//   - growing: x is the chain top, the candidate y the element below it with cur = D[x][y] (a chain of one: y none,
//     cur = +inf).  Among the live i != x with D[x][i] < cur, strictly, the smallest D[x][i] wins, the lowest i among
//     equals.  If nobody beats cur the element below stays the winner and the growing stops; otherwise the winner is
//     pushed and the step repeats;
//   - the two top elements are popped and ordered x < y; the record is (x, y, cur, size[x] + size[y]); then
//     size[y] = size[x] + size[y], size[x] = 0, and for every live i != y:  D[i][y] = D[y][i] = max(D[i][x], D[i][y]).
// Output: merges, (P - 1) x 4 doubles, the records in merge order with the raw slot ids, unsorted.
// "The smallest (value, index) pair, lowest index on ties, and then `value < cur`" picks the same winner as the sequential
// scan above and does not depend on the order of the comparisons: that is what lets a parallel reduction stand in for it.
// A scan either pushes or ends a merge, the chain is popped twice per merge, so at most 3 (P - 1) scans happen; a driver
// that counts more than 4 P, or meets a chain of one with no neighbour below +inf (a distance overflowed), stops.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_HC_HD __host__ __device__ __forceinline__
#else
#define SP_HC_HD static inline
#endif

#define SP_HC_MAXP 16384     // points: a 2 GiB fp64 matrix

// status of a chain run
#define SP_HC_OK 0
#define SP_HC_SCANS 1        // more than 4 P scans
#define SP_HC_NONE 2         // a chain of one found no neighbour

SP_HC_HD double sp_hc_term(double a, double b) {
    const double d = a - b;
    return d * d;
}
// one distance: the walk over the D coordinates of two points
SP_HC_HD double sp_hc_dist(const double *pi, const double *pj, int D) {
    double s = 0.0;
    for (int c = 0; c < D; c++) s += sp_hc_term(pi[c], pj[c]);
    return sqrt(s);
}
// is candidate (va, ia) a better neighbour than (vb, ib)?
SP_HC_HD bool sp_hc_less(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }
SP_HC_HD double sp_hc_max(double a, double b) { return a > b ? a : b; }
SP_HC_HD int64_t sp_hc_max_scans(int P) { return 4 * (int64_t)P; }

// ---- host drivers: the pieces above, looped in the stated orders
// dist: P x P
static inline void sp_hc_host_dist(const double *pts, int P, int D, double *dist) {
    for (int i = 0; i < P; i++)
        for (int j = 0; j < P; j++) dist[(int64_t)i * P + j] = sp_hc_dist(pts + (int64_t)i * D, pts + (int64_t)j * D, D);
}
// dist: P x P, rewritten as the clusters merge; size, chain: P ints of scratch; merges: (P - 1) x 4; returns the status
static inline int sp_hc_host_chain(double *dist, int P, int *size, int *chain, double *merges, int64_t *n_scans) {
    int len = 0;
    int64_t scans = 0;
    for (int i = 0; i < P; i++) size[i] = 1;
    for (int k = 0; k < P - 1; k++) {
        if (len == 0) {
            for (int i = 0; i < P; i++)
                if (size[i] > 0) {
                    chain[len++] = i;
                    break;
                }
        }
        int x, y;
        double cur;
        for (;;) {
            x = chain[len - 1];
            y = len > 1 ? chain[len - 2] : -1;
            cur = len > 1 ? dist[(int64_t)x * P + y] : INFINITY;
            if (++scans > sp_hc_max_scans(P)) {
                *n_scans = scans;
                return SP_HC_SCANS;
            }
            for (int i = 0; i < P; i++) {
                if (size[i] == 0 || i == x) continue;
                const double d = dist[(int64_t)x * P + i];
                if (d < cur) {
                    cur = d;
                    y = i;
                }
            }
            if (y < 0) {
                *n_scans = scans;
                return SP_HC_NONE;
            }
            if (len > 1 && y == chain[len - 2]) break;
            chain[len++] = y;
        }
        len -= 2;
        if (x > y) {
            const int t = x;
            x = y;
            y = t;
        }
        const int nx = size[x], ny = size[y];
        merges[4 * (int64_t)k] = (double)x;
        merges[4 * (int64_t)k + 1] = (double)y;
        merges[4 * (int64_t)k + 2] = cur;
        merges[4 * (int64_t)k + 3] = (double)(nx + ny);
        size[x] = 0;
        size[y] = nx + ny;
        for (int i = 0; i < P; i++) {
            if (size[i] == 0 || i == y) continue;
            const double v = sp_hc_max(dist[(int64_t)i * P + x], dist[(int64_t)i * P + y]);
            dist[(int64_t)i * P + y] = v;
            dist[(int64_t)y * P + i] = v;
        }
    }
    *n_scans = scans;
    return SP_HC_OK;
}
