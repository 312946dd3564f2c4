// sp_kboot.h -- one replicate of the k-means bootstrap (Cluster.bootstrap, the reference's Cluster.py:82-118) in Gram
// space: everything kb_bootstrap (sp_kboot.hip) computes after it has gathered its columns, as plain fp64 arithmetic.
//
// __host__ __device__ and free of runtime calls, so that tests/test_kboot_host.py builds it with the host compiler and
// checks it against the numpy twin (tests/kboot_ref.py).  Build with -ffp-contract=off: the orders below are the
// definition, and a fused multiply-add changes the sums.
//
// k-means on C points needs only G[a][b] = sum_t z[a][t] z[b][t] over the replicate's sampled columns:
//   |x_a - x_b|^2         = D2[a][b] = max(0, (G[a][a] + G[b][b]) - 2 G[a][b])
//   |x_a - mean(m)|^2     = (G[a][a] - 2 S[a] / |m|) + T / |m|^2,   S[a] = sum_{j in m} G[a][j],  T = sum_{a in m} S[a]
// (members in ascending index order, every sum started from its first term).
//
// RNG  u(seed, rep, i) = (mix(mix(seed ^ rep * 0xD6E8FEB86659FD93) + i) >> 11) * 2^-53, the counter hash of sp_synth.hip;
//      i counts the draws of the replicate: 0 the first centre, 1 + (c - 1) * trials + t trial t of centre c >= 1.
// Init greedy k-means++ (scikit-learn's _kmeans_plusplus): first centre min(floor(u C), C - 1); every further centre the
//      best of trials = 2 + floor(ln K) candidates, candidate = first index whose running sum of `closest` (index order)
//      exceeds r = u * pot, clipped to C - 1; the smallest new potential wins, the first trial on ties.
// Lloyd from the labels nearest to the centres; argmin with the lowest index on ties; an empty cluster is at +inf and
//      stays empty; stops when no label changes or after SP_KB_MAXIT iterations (the count includes the last one).
//
// The pieces are written per point / per cluster / per trial: the host driver below loops over them, the kernel gives
// one to each lane and puts a barrier where the driver starts a new loop.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define SP_KB_HD __host__ __device__ __forceinline__
#define SP_KB_HDM __host__ __device__ __forceinline__
#else
#define SP_KB_HD static inline
#define SP_KB_HDM inline
#endif

#define SP_KB_MAXC 128     // points (chromosomes): the symmetric half of G, 66 KB, beside the staging tile in LDS
#define SP_KB_MAXK 32      // clusters
#define SP_KB_MAXIT 300    // scikit-learn's max_iter
#define SP_KB_TILE 32      // columns staged per chunk of the Gram pass
#define SP_KB_MAXTRIALS 8  // 2 + floor(ln K) <= 5 for K <= 32

SP_KB_HD uint64_t sp_kb_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
SP_KB_HD double sp_kb_u(uint64_t seed, uint64_t rep, uint64_t i) {
    const uint64_t h = sp_kb_mix(sp_kb_mix(seed ^ (rep * 0xD6E8FEB86659FD93ULL)) + i);
    return (double)(h >> 11) * 1.1102230246251565e-16;   // 2^-53: exact
}
// 2 + floor(ln K) without a logarithm: floor(ln K) = number of powers e^j <= K, j >= 1 (K < 2981)
SP_KB_HD int sp_kb_trials(int K) {
    return 2 + (K >= 3) + (K >= 8) + (K >= 21) + (K >= 55) + (K >= 149) + (K >= 404) + (K >= 1097);
}
// the symmetric half, row a holding columns 0 .. a
SP_KB_HD int sp_kb_tri(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }
struct sp_kb_half {     // G stored as that half
    const double *g;
    SP_KB_HDM double operator()(int a, int b) const { return g[sp_kb_tri(a, b)]; }
};
struct sp_kb_full {     // G stored C x C
    const double *g;
    int C;
    SP_KB_HDM double operator()(int a, int b) const { return g[(int64_t)a * C + b]; }
};

template <typename GR>
SP_KB_HD double sp_kb_d2(const GR &G, int a, int b) {
    const double d = (G(a, a) + G(b, b)) - 2.0 * G(a, b);
    return d > 0.0 ? d : 0.0;
}
SP_KB_HD int sp_kb_first_centre(uint64_t seed, uint64_t rep, int C) {
    const int c = (int)(sp_kb_u(seed, rep, 0) * (double)C);
    return c < C - 1 ? c : C - 1;
}
// sum of closest[0 .. C) in index order
SP_KB_HD double sp_kb_potential(const double *closest, int C) {
    double s = closest[0];
    for (int a = 1; a < C; a++) s += closest[a];
    return s;
}
// one k-means++ trial: the candidate r = u * pot selects, and the potential with it as a centre
template <typename GR>
SP_KB_HD void sp_kb_trial(const GR &G, int C, const double *closest, double pot, double u, int *cand, double *newpot) {
    const double r = u * pot;
    int c = C - 1;
    double run = closest[0];
    for (int a = 0; a < C; a++) {
        if (a) run += closest[a];
        if (run > r) {
            c = a;
            break;
        }
    }
    double s = 0.0;
    for (int a = 0; a < C; a++) {
        const double d = sp_kb_d2(G, c, a), m = d < closest[a] ? d : closest[a];
        s = a ? s + m : m;
    }
    *cand = c;
    *newpot = s;
}
// the first trial with the smallest potential
SP_KB_HD int sp_kb_best_trial(const double *newpot, int trials) {
    int best = 0;
    for (int t = 1; t < trials; t++)
        if (newpot[t] < newpot[best]) best = t;
    return best;
}
template <typename GR>
SP_KB_HD double sp_kb_closer(const GR &G, int centre, int a, double closest_a) {
    const double d = sp_kb_d2(G, centre, a);
    return d < closest_a ? d : closest_a;
}
// label of point a at the start: the nearest centre, the lowest cluster on ties
template <typename GR>
SP_KB_HD int sp_kb_nearest_centre(const GR &G, int K, const int *centre, int a) {
    int best = 0;
    double bd = sp_kb_d2(G, a, centre[0]);
    for (int c = 1; c < K; c++) {
        const double d = sp_kb_d2(G, a, centre[c]);
        if (d < bd) {
            bd = d;
            best = c;
        }
    }
    return best;
}
// S[c * ld + a] = sum of G[a][j] over the members j of cluster c, ascending, for every c
template <typename GR>
SP_KB_HD void sp_kb_point_sums(const GR &G, int C, int K, const int *lab, int a, double *S, int ld) {
    uint32_t seen = 0;     // clusters with a member so far (K <= 32)
    for (int j = 0; j < C; j++) {
        const int c = lab[j];
        const double g = G(a, j);
        S[c * ld + a] = ((seen >> c) & 1u) ? S[c * ld + a] + g : g;
        seen |= 1u << c;
    }
    for (int c = 0; c < K; c++)
        if (!((seen >> c) & 1u)) S[c * ld + a] = 0.0;
}
// T = sum of S[c][a] over the members a of cluster c, ascending; returns the number of members
SP_KB_HD int sp_kb_cluster_total(int C, const int *lab, int c, const double *S, int ld, double *T) {
    int cnt = 0;
    double t = 0.0;
    for (int a = 0; a < C; a++)
        if (lab[a] == c) {
            t = cnt ? t + S[c * ld + a] : S[c * ld + a];
            cnt++;
        }
    *T = t;
    return cnt;
}
SP_KB_HD double sp_kb_dist(double gaa, double s, double t, int cnt) {
    if (cnt == 0) return INFINITY;
    const double m = (double)cnt;
    return (gaa - 2.0 * s / m) + t / (m * m);
}
template <typename GR>
SP_KB_HD int sp_kb_point_assign(const GR &G, int K, int a, const double *S, int ld, const double *T, const int *cnt) {
    const double gaa = G(a, a);
    int best = 0;
    double bd = sp_kb_dist(gaa, S[a], T[0], cnt[0]);
    for (int c = 1; c < K; c++) {
        const double d = sp_kb_dist(gaa, S[c * ld + a], T[c], cnt[c]);
        if (d < bd) {
            bd = d;
            best = c;
        }
    }
    return best;
}

// host driver: the pieces above, looped.  work: (SP_KB_MAXK + 1) * C doubles; returns the iteration count
template <typename GR>
static inline int sp_kb_solve(const GR &G, int C, int K, uint64_t seed, uint64_t rep, int32_t *labels, double *work) {
    double *closest = work, *S = work + C;
    double T[SP_KB_MAXK], newpot[SP_KB_MAXTRIALS];
    int centre[SP_KB_MAXK], cnt[SP_KB_MAXK], cand[SP_KB_MAXTRIALS], lab[SP_KB_MAXC], next[SP_KB_MAXC];
    const int trials = sp_kb_trials(K);
    centre[0] = sp_kb_first_centre(seed, rep, C);
    for (int a = 0; a < C; a++) closest[a] = sp_kb_d2(G, centre[0], a);
    double pot = sp_kb_potential(closest, C);
    for (int c = 1; c < K; c++) {
        for (int t = 0; t < trials; t++)
            sp_kb_trial(G, C, closest, pot, sp_kb_u(seed, rep, 1 + (uint64_t)(c - 1) * trials + t), &cand[t], &newpot[t]);
        const int b = sp_kb_best_trial(newpot, trials);
        centre[c] = cand[b];
        pot = newpot[b];
        for (int a = 0; a < C; a++) closest[a] = sp_kb_closer(G, centre[c], a, closest[a]);
    }
    for (int a = 0; a < C; a++) lab[a] = sp_kb_nearest_centre(G, K, centre, a);
    int it = 0;
    for (;;) {
        it++;
        for (int a = 0; a < C; a++) sp_kb_point_sums(G, C, K, lab, a, S, C);
        for (int c = 0; c < K; c++) cnt[c] = sp_kb_cluster_total(C, lab, c, S, C, &T[c]);
        int changed = 0;
        for (int a = 0; a < C; a++) {
            next[a] = sp_kb_point_assign(G, K, a, S, C, T, cnt);
            changed |= next[a] != lab[a];
        }
        for (int a = 0; a < C; a++) lab[a] = next[a];
        if (!changed || it >= SP_KB_MAXIT) break;
    }
    for (int a = 0; a < C; a++) labels[a] = lab[a];
    return it;
}
