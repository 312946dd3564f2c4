// mapslots_host_check.cpp -- csrc/sp_mapslots.h on the CPU (tests/test_mapslots_host.py), exhaustive over small inputs.
//   bins      map_slot / map_slot_end / map_nslots_host / map_params_of and the one-slot shortcut of the bins accumulator
//   stack     map_chunk_of_slot inverts the chunk of map_slot
//   features  map_unit_fit and the cursor map_feat_locate against a naive search per start
//   planes    map_plane_mask and map_span against a decode per bit
// The references are loops over single starts and single bits: never the closed forms under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sp_mapslots.h"

static long long n_checks = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        n_checks++;                                     \
        if (!(c)) {                                     \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            exit(1);                                    \
        }                                               \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {      // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}

// the chunk of a start, as Seqs.chunk_chromfiles cuts: chunk j >= 1 begins k - 1 bases before j * W.  Asked for starts in
// increasing order, it walks the chunk boundaries.
struct ref_chunks {
    int64_t W;
    int k;
    int64_t j = 0;
    int64_t at(int64_t s) {
        if (W > 0)
            while ((j + 1) * W - (k - 1) <= s) j++;
        return j;
    }
};

struct geom {
    int k;
    int64_t bin, chunk;
};
// the geometries of the issue, and three bins of a whole range and more: only those make the one-slot shortcut true
static std::vector<geom> geoms() {
    const int64_t bins[] = {1, 2, 37, 64, 100, 163, 1000, 10000}, chunks[] = {0, 40, 1000, 5000};
    const int64_t wide[] = {MAP_RANGE, 40000, 100000}, wide_chunks[] = {0, 50000, 100000};
    std::vector<geom> g;
    for (int k : {15, 17}) {
        for (int64_t b : bins)
            for (int64_t c : chunks) g.push_back({k, b, c});
        for (int64_t b : wide)
            for (int64_t c : wide_chunks) g.push_back({k, b, c});
    }
    return g;
}
// a few thousand bases, at and one off a multiple of the bin, the chunk and the unit (a bin or chunk beyond that: itself)
static std::vector<int64_t> lengths(const geom &g) {
    std::vector<int64_t> L = {1, g.k - 1, g.k, 3001};
    for (int64_t m : {g.bin, g.chunk, (int64_t)SP_UNIT}) {
        if (m <= 0) continue;
        const int64_t at = m >= 3000 ? m : (3000 / m) * m;
        if (at > 100000) continue;
        for (int64_t d = -1; d <= 1; d++)
            if (at + d > 0) L.push_back(at + d);
    }
    return L;
}

static void check_bins() {
    for (const geom &g : geoms()) {
        const int k = g.k;
        for (int64_t len : lengths(g)) {
            const int64_t nslots = map_nslots_host(len, g.bin, g.chunk, k);
            const sp_map_params P = map_params_of(len, g.bin, g.chunk, nslots, 3);
            CHECK(P.n_units == (len + SP_UNIT - 1) / SP_UNIT, "n_units");
            // every valid start's slot is the bin of the start plus its chunk, and lies inside the table
            ref_chunks rc{g.chunk, k};
            for (int64_t s = 0; s + k <= len; s++) {
                const int64_t slot = map_slot(s, P, k);
                CHECK(slot == s / g.bin + rc.at(s), "slot of %lld: bin %lld chunk %lld k %d", (long long)s,
                      (long long)g.bin, (long long)g.chunk, k);
                CHECK(slot < nslots, "slot %lld of start %lld >= %lld slots (len %lld bin %lld chunk %lld k %d)", (long long)slot,
                      (long long)s, (long long)nslots, (long long)len, (long long)g.bin, (long long)g.chunk, k);
            }
            // the pieces of every unit: they tile it, and a piece is the starts of one slot
            for (int64_t u = 0; u < P.n_units; u++) {
                const int64_t s0 = u * SP_UNIT;
                unsigned long long covered = 0ULL;
                int64_t p = s0;
                while (p < s0 + SP_UNIT) {
                    const int64_t end = map_slot_end(p, P, k);
                    CHECK(end > p, "map_slot_end(%lld) = %lld", (long long)p, (long long)end);
                    CHECK(map_slot(end, P, k) != map_slot(p, P, k), "start %lld is in the slot that ends there", (long long)end);
                    const int64_t e = end > s0 + SP_UNIT ? s0 + SP_UNIT : end;
                    const unsigned long long within = map_span(p - s0, e - s0);
                    CHECK(within && !(covered & within), "pieces overlap at %lld", (long long)p);
                    covered |= within;
                    for (int64_t s = p; s < e; s++)
                        CHECK(map_slot(s, P, k) == map_slot(p, P, k), "start %lld is not in the slot of %lld", (long long)s, (long long)p);
                    p = e;
                }
                CHECK(covered == ~0ULL, "unit %lld is not tiled", (long long)u);
            }
        }
        // per range of MAP_RANGE starts (the rule does not depend on the length): the one-slot shortcut is the truth, and
        // where map_params_of chooses the LDS histogram, every slot of the range lies inside it
        const sp_map_params P0 = map_params_of(4 * (int64_t)MAP_RANGE, g.bin, g.chunk, 0, 1);
        for (int64_t r = 0; r < 4; r++) {
            const int64_t lo = r * MAP_RANGE, hi = (r + 1) * MAP_RANGE;
            const int64_t slot_lo = map_slot(lo, P0, k);
            const bool one_slot = map_slot_end(lo, P0, k) >= hi;
            int64_t slot_hi = slot_lo;
            for (int64_t s = lo; s < hi; s++) {
                const int64_t slot = map_slot(s, P0, k);
                CHECK(slot >= slot_hi, "slots decrease at %lld", (long long)s);
                slot_hi = slot;
            }
            CHECK(one_slot == (slot_hi == slot_lo), "one_slot %d, slots %lld .. %lld (range %lld bin %lld chunk %lld k %d)", (int)one_slot,
                  (long long)slot_lo, (long long)slot_hi, (long long)r, (long long)g.bin, (long long)g.chunk, k);
            for (int S = 1; S <= 7; S++) {
                const sp_map_params P = map_params_of(4 * (int64_t)MAP_RANGE, g.bin, g.chunk, 0, S);
                if (P.use_lds)
                    CHECK((slot_hi - slot_lo) * S + S <= MAP_LDS_ENTRIES, "LDS: slots %lld .. %lld x %d (range %lld bin %lld chunk %lld k %d)",
                          (long long)slot_lo, (long long)slot_hi, S, (long long)r, (long long)g.bin, (long long)g.chunk, k);
            }
        }
    }
}

// the LDS rule at its edge: for every S the smallest bin at which map_params_of chooses the histogram, and the next one, without
// chunks and with chunks of 5000 -- the geometries above all lie far from it
static void check_lds_edges() {
    for (int k : {15, 17})
        for (int S = 1; S <= 7; S++)
            for (int64_t chunk : {(int64_t)0, (int64_t)5000}) {
                int64_t edge = 1;
                while (!map_params_of(0, edge, chunk, 0, S).use_lds) edge++;
                CHECK(edge > 1 && edge < MAP_RANGE, "no edge for S = %d", S);
                for (int64_t bin = edge; bin <= edge + 1; bin++) {
                    const sp_map_params P = map_params_of(0, bin, chunk, 0, S);
                    for (int64_t r = 0; r < 8; r++) {
                        const int64_t slot_lo = map_slot(r * MAP_RANGE, P, k), slot_hi = map_slot((r + 1) * MAP_RANGE - 1, P, k);
                        CHECK((slot_hi - slot_lo) * S + S <= MAP_LDS_ENTRIES, "LDS edge: slots %lld .. %lld x %d (range %lld bin %lld chunk %lld k %d)",
                              (long long)slot_lo, (long long)slot_hi, S, (long long)r, (long long)bin, (long long)chunk, k);
                    }
                }
            }
}

static void check_stack() {
    for (const geom &g : geoms()) {
        if (g.chunk <= 0) continue;
        const sp_map_params P = map_params_of(0, g.bin, g.chunk, 0, 1);
        const int64_t top = g.bin >= MAP_RANGE ? 4 * (int64_t)MAP_RANGE : 12000;
        ref_chunks rc{g.chunk, g.k};
        for (int64_t s = 0; s < top; s++) {
            const int64_t slot = map_slot(s, P, g.k), chunk = rc.at(s);
            CHECK(map_chunk_of_slot(slot, g.bin, g.chunk, g.k) == chunk, "chunk of slot %lld (start %lld): %lld, not %lld (bin %lld chunk %lld k %d)",
                  (long long)slot, (long long)s, (long long)map_chunk_of_slot(slot, g.bin, g.chunk, g.k), (long long)chunk,
                  (long long)g.bin, (long long)g.chunk, g.k);
        }
    }
}

// the feature whose bases hold start s (never an empty one), by a scan from the front
static int64_t ref_feature(const std::vector<int64_t> &foff, int64_t s) {
    for (size_t f = 0; f + 1 < foff.size(); f++)
        if (foff[f] <= s && s < foff[f + 1]) return (int64_t)f;
    return -1;
}

static void check_features() {
    for (int k : {15, 17}) {
        for (int rep = 0; rep < 60; rep++) {
            // empty features, features shorter than k, ordinary ones, and ones that span several units
            std::vector<int64_t> foff = {0};
            const int n_feat = 1 + (int)(rnd() % 40);
            for (int f = 0; f < n_feat; f++) {
                const uint64_t kind = rnd() % 8;
                const int64_t len = kind == 0 ? 0 : kind <= 2 ? 1 + (int64_t)(rnd() % (uint64_t)(k - 1)) : kind <= 5 ? k + (int64_t)(rnd() % 70)
                                                                                                            : 130 + (int64_t)(rnd() % 300);
                foff.push_back(foff.back() + len);
            }
            const int64_t total = foff.back(), n_units = (total + SP_UNIT - 1) / SP_UNIT;
            for (int64_t u = 0; u < n_units; u++) {
                const int64_t s0 = u * SP_UNIT;
                int64_t first = -1;
                const unsigned long long fit = map_unit_fit(foff.data(), n_feat, s0, k, first);
                CHECK(first >= 0 && first < n_feat && foff[(size_t)first] <= s0 && (first + 1 == n_feat || foff[(size_t)first + 1] > s0),
                      "unit %lld starts in feature %lld", (long long)u, (long long)first);
                for (int pass = 0; pass < 2; pass++) {      // every start in order, then a random subset in order (what a filter lets through)
                    map_feat_cursor cur;
                    cur.f = -1;
                    cur.next = 0;
                    for (int64_t s = s0; s < s0 + SP_UNIT && s < total; s++) {
                        const int64_t f = ref_feature(foff, s);
                        const bool inside = f >= 0 && s + k <= foff[(size_t)f + 1];
                        if (pass == 0)
                            CHECK((bool)((fit >> (s - s0)) & 1ULL) == inside, "fit of start %lld: %d, k %d, feature %lld", (long long)s, (int)!inside, k,
                                  (long long)f);
                        else if (rnd() & 1)
                            continue;
                        const bool got = map_feat_locate(cur, s, k, foff.data(), n_feat);
                        CHECK(got == inside, "cursor at start %lld: %d, k %d, feature %lld", (long long)s, (int)got, k, (long long)f);
                        if (inside) CHECK(cur.f == f, "cursor at start %lld names feature %lld, not %lld", (long long)s, (long long)cur.f, (long long)f);
                    }
                }
            }
        }
    }
}

static void check_planes() {
    for (int a = 0; a <= 64; a++)
        for (int b = 0; b <= 64; b++) {
            unsigned long long m = 0ULL;
            for (int j = a; j < b; j++) m |= 1ULL << j;
            CHECK(map_span(a, b) == m, "map_span(%d, %d)", a, b);
        }
    for (int rep = 0; rep < 2000; rep++) {
        unsigned long long lab[3] = {rnd(), rnd(), rnd()};
        if (rep % 3 == 0) lab[2] = 0ULL;      // (two planes: the compact tables, labels 1 .. 3)
        for (int sg = 0; sg < 7; sg++) {
            unsigned long long m = 0ULL;
            for (int j = 0; j < 64; j++) {
                const int l = (int)((lab[0] >> j) & 1ULL) | (int)(((lab[1] >> j) & 1ULL) << 1) | (int)(((lab[2] >> j) & 1ULL) << 2);
                if (l == sg + 1) m |= 1ULL << j;
            }
            CHECK(map_plane_mask(lab, sg) == m, "map_plane_mask, label %d", sg + 1);
        }
    }
}

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "bins")) check_bins(), check_lds_edges();
    else if (!strcmp(what, "stack")) check_stack();
    else if (!strcmp(what, "features")) check_features();
    else if (!strcmp(what, "planes")) check_planes();
    else {
        printf("usage: %s bins | stack | features | planes\n", argv[0]);
        return 2;
    }
    printf("OK %lld\n", n_checks);
    return 0;
}
