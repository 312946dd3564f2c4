// sp_listplan.h -- host planning of the list filter's join (sp_listfilter.hip) as plain C++: no HIP types, so the host
// compiler alone builds it (tests/listplan_host_check.cpp).  What the kernels and the planner both need to know -- the
// round size, the descriptor bits, the list limits of the two join kernels -- is defined here.
#pragma once
#include <stdint.h>

#include <vector>

#define SPS_MAXC 64          // lists sps_join_blk takes (a lane of wave 0 per list); sps_join_wide above
#ifndef BJ_T
#define BJ_T 1024            // entries per round of sps_join_blk
#endif
#define BJ_FC 128            // row descriptors of the uniform walk held in LDS (more: generic decisions)
#define JOIN_CHUNK 256       // rows handed out per grab of the global row cursor
#define JD_CHROM_MASK 0xfffff
#define JD_UNIT_END (1 << 20)
#define JD_SET_END (1 << 21)
#define JD_BI1 (1 << 22)     // the set's baseline is the second largest frequency (else the smallest)

// key ranges: R = 2^rb of them, range of a key = key >> shift
struct sp_range_plan {
    bool wide;               // sps_join_wide (more than SPS_MAXC lists)
    int bits, rb, shift;
    long long R;
    int64_t per_range;       // entries a range is sized for
};

// nslots > 0: list mode (k <= 15, the keys are dense slots below nslots); else the keys are 2k-bit canonical k-mers
inline sp_range_plan sp_plan_ranges(int64_t total, int C, int k, int64_t nslots) {
    sp_range_plan P;
    P.wide = C > SPS_MAXC;
    P.bits = 2 * k;
    if (nslots > 0) {
        P.bits = 0;
        while ((1LL << P.bits) < nslots) P.bits++;
    }
    if (P.bits > 64) P.bits = 64;
    // one workgroup per range of ~2/3 of a round; sps_join_wide: 32 entries per list (the range-edge table is C x (R + 1)
    // words, an eighth of the lists' bytes), a range spans several rounds
    P.per_range = P.wide ? (int64_t)32 * C : (int64_t)BJ_T * 2 / 3;
    P.rb = 0;
    while (P.rb < P.bits && P.rb < 23 && ((int64_t)1 << P.rb) * P.per_range < total) P.rb++;
    if (P.bits - P.rb > 63) P.rb = P.bits - 63;      // k = 32 and a handful of k-mers: `key >> 64` is not a shift (fuzz case k32_join)
    P.R = 1LL << P.rb;
    P.shift = P.bits - P.rb;
    return P;
}

// differential rows are rare (a fraction of a percent of the union on the BASELINE genomes): the staging area holds
// total / 16 rows (at least 2^20); if a filter configuration keeps more, the pass is repeated with what it asked for
inline unsigned long long sp_plan_row_slack(int n_cu) {       // every resident workgroup may strand one chunk
    return (unsigned long long)n_cu * 16 * JOIN_CHUNK;
}
inline unsigned long long sp_plan_row_cap(int64_t total, int n_cu) {
    unsigned long long row_cap = (unsigned long long)(total / 16);
    if (row_cap < (1ULL << 20)) row_cap = (unsigned long long)(total < (1LL << 20) ? total : (1LL << 20));
    return row_cap + sp_plan_row_slack(n_cu);
}
inline unsigned long long sp_plan_row_retry(unsigned long long asked, int n_cu) { return asked + sp_plan_row_slack(n_cu); }

// the uniform fp32 walk of sps_join_blk (k3_eval's P.fast): every non-singleton set uses baseline 1 or -1 and has no
// empty unit.  rd: chromosome | JD_UNIT_END | JD_SET_END | JD_BI1, the non-singleton sets in config order; rinv:
// 1 / (unit length) at unit ends, fp32.  Both empty when fast = 0.
struct sp_walk_plan {
    int fast;
    std::vector<int32_t> rd;
    std::vector<float> rinv;
};

inline sp_walk_plan sp_plan_walk(int n_sets, const int32_t *set_off, const int32_t *unit_off, const int32_t *unit_chrom,
                                 const double *unit_inv, int baseline, bool generic /* SP_JOIN_GENERIC: cross-check switch */) {
    sp_walk_plan W;
    int n_multi = 0;
    for (int st = 0; st < n_sets; st++) n_multi += (set_off[st + 1] - set_off[st]) > 1;
    W.fast = n_multi > 0 ? 1 : 0;
    for (int st = 0; st < n_sets; st++) {
        const int nu = set_off[st + 1] - set_off[st];
        if (nu == 1) continue;
        const int bi = baseline < 0 ? nu + baseline : baseline;
        if (!(bi == 1 || bi == nu - 1)) W.fast = 0;
        for (int u = set_off[st]; u < set_off[st + 1]; u++)
            if (unit_off[u + 1] == unit_off[u]) W.fast = 0;
    }
    if (generic) W.fast = 0;
    if (!W.fast) return W;
    for (int st = 0; st < n_sets; st++) {
        const int nu = set_off[st + 1] - set_off[st];
        if (nu == 1) continue;
        const int bi = baseline < 0 ? nu + baseline : baseline;
        for (int u = set_off[st]; u < set_off[st + 1]; u++)
            for (int j = unit_off[u]; j < unit_off[u + 1]; j++) {
                int d = unit_chrom[j];
                if (j == unit_off[u + 1] - 1) {
                    d |= JD_UNIT_END;
                    if (u == set_off[st + 1] - 1) d |= JD_SET_END | (bi == 1 ? JD_BI1 : 0);
                }
                W.rd.push_back(d);
                W.rinv.push_back(j == unit_off[u + 1] - 1 ? (float)unit_inv[u] : 0.0f);
            }
    }
    if (W.rd.size() > BJ_FC) {
        W.fast = 0;
        W.rd.clear();
        W.rinv.clear();
    }
    return W;
}

// per chromosome: bit s set if it belongs to non-singleton set number s (screen of the join kernels)
struct sp_mask_plan {
    int screen;                              // the masks are usable
    std::vector<unsigned long long> cs;
};

inline sp_mask_plan sp_plan_masks(int C, int n_sets, const int32_t *set_off, const int32_t *unit_off,
                                  const int32_t *unit_chrom, bool phase_a, double min_fold) {
    sp_mask_plan M;
    M.cs.assign((size_t)C, 0ULL);
    int ms = 0;
    for (int st = 0; st < n_sets; st++) {
        if (set_off[st + 1] - set_off[st] <= 1) continue;
        if (ms < 32)
            for (int u = set_off[st]; u < set_off[st + 1]; u++)
                for (int j = unit_off[u]; j < unit_off[u + 1]; j++) M.cs[(size_t)unit_chrom[j]] |= 1ULL << ms;
        ms++;
    }
    M.screen = ms <= 32 ? 1 : 0;      // (sps_join_blk keeps 32-bit masks)
    // the screen takes a set the key does not touch for a failed fold test, which min_fold <= 0 breaks (an all-zero
    // set passes): phase A of sps_filter_passengers does without it then
    if (phase_a && !(min_fold > 0)) M.screen = 0;
    return M;
}

// sps_join_wide: per chromosome the non-singleton sets it belongs to (CSR: cso has C + 1 entries)
inline void sp_plan_wide_csr(int C, int n_sets, const int32_t *set_off, const int32_t *unit_off, const int32_t *unit_chrom,
                             std::vector<int32_t> &cso, std::vector<int32_t> &cs) {
    std::vector<std::vector<int32_t>> of((size_t)C);
    for (int st = 0; st < n_sets; st++) {
        if (set_off[st + 1] - set_off[st] <= 1) continue;
        for (int j = unit_off[set_off[st]]; j < unit_off[set_off[st + 1]]; j++) {
            std::vector<int32_t> &v = of[(size_t)unit_chrom[j]];
            if (v.empty() || v.back() != st) v.push_back(st);
        }
    }
    for (int c = 0; c < C; c++) {
        cso.push_back((int32_t)cs.size());
        cs.insert(cs.end(), of[(size_t)c].begin(), of[(size_t)c].end());
    }
    cso.push_back((int32_t)cs.size());
}

// phase A of sps_filter_passengers: the set chromosomes (named by a set of two or more units) renumbered in ascending
// order, the sets of one unit left out.  num[c]: the list number of chromosome c, -1 for a passenger.
struct sp_passenger_plan {
    std::vector<int> pick, num;
    std::vector<int32_t> a_so, a_uo, a_uc;
    std::vector<double> a_den;            // denominators, then their reciprocals
};

inline sp_passenger_plan sp_plan_passengers(int C, int n_sets, const int32_t *set_off, const int32_t *unit_off,
                                            const int32_t *unit_chrom, const double *den /* 2 x n_units */) {
    sp_passenger_plan P;
    const int n_units = set_off[n_sets];
    P.num.assign((size_t)C, -1);
    for (int st = 0; st < n_sets; st++)
        if (set_off[st + 1] - set_off[st] > 1)
            for (int j = unit_off[set_off[st]]; j < unit_off[set_off[st + 1]]; j++) P.num[(size_t)unit_chrom[j]] = 0;
    for (int c = 0; c < C; c++)
        if (P.num[(size_t)c] == 0) {
            P.num[(size_t)c] = (int)P.pick.size();
            P.pick.push_back(c);
        }
    P.a_so.assign(1, 0);
    P.a_uo.assign(1, 0);
    std::vector<double> a_inv;
    for (int st = 0; st < n_sets; st++) {
        if (set_off[st + 1] - set_off[st] <= 1) continue;
        for (int u = set_off[st]; u < set_off[st + 1]; u++) {
            for (int j = unit_off[u]; j < unit_off[u + 1]; j++) P.a_uc.push_back(P.num[(size_t)unit_chrom[j]]);
            P.a_uo.push_back((int32_t)P.a_uc.size());
            P.a_den.push_back(den[(size_t)u]);
            a_inv.push_back(den[(size_t)(n_units + u)]);
        }
        P.a_so.push_back((int32_t)P.a_den.size());
    }
    P.a_den.insert(P.a_den.end(), a_inv.begin(), a_inv.end());
    P.a_uc.push_back(0);      // (never read: keeps .data() valid when every unit is empty)
    return P;
}
