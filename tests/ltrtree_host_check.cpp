// Host check of subphaser_amd/csrc/sp_ltrtree.h (tests/test_ltrtree_host.py builds and runs it).
// Input file: records, each led by an int64 tag, until tag 0:
//   1  sketch: int64 k, s, n, then n base codes (bytes: 0..3, anything else invalid)   -> s uint64, int64 len
//   2  pair:   int64 s, la, lb, then la + lb uint64                                    -> int64 shared, denom
//   3  nj:     int64 N, limit (the guard), then the N x N int64 matrix                                   -> int64 status, (N - 1) x 5 int64
//   4  pairs:  int64 s, n, then n x s uint64 and n int32                               -> n x n int32 shared, n x n int32 denom
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sp_ltrtree.h"

template <typename T>
static bool get(FILE *f, T *out, size_t n = 1) { return n == 0 || fread(out, sizeof(T), n, f) == n; }
template <typename T>
static bool put(FILE *f, const T *in, size_t n = 1) { return n == 0 || fwrite(in, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    for (;;) {
        int64_t tag = 0;
        if (!get(f, &tag)) return 3;
        if (tag == 0) break;
        if (tag == 1) {
            int64_t k, s, n;
            if (!get(f, &k) || !get(f, &s) || !get(f, &n)) return 3;
            if (sp_lt_check((int)k, (int)s) || n < 0 || n > SP_LT_MAXLEN) return 4;
            std::vector<uint8_t> codes((size_t)n);
            std::vector<uint64_t> sk((size_t)s);
            if (!get(f, codes.data(), codes.size())) return 3;
            const int64_t len = sp_lt_host_sketch(codes.data(), n, (int)k, (int)s, sk.data());
            if (!put(o, sk.data(), sk.size()) || !put(o, &len)) return 5;
        } else if (tag == 2) {
            int64_t s, la, lb;
            if (!get(f, &s) || !get(f, &la) || !get(f, &lb)) return 3;
            if (la < 0 || lb < 0 || la > s || lb > s) return 4;
            std::vector<uint64_t> a((size_t)la), b((size_t)lb);
            if (!get(f, a.data(), a.size()) || !get(f, b.data(), b.size())) return 3;
            int32_t sh, dn;
            sp_lt_pair(a.data(), (int)la, b.data(), (int)lb, (int)s, &sh, &dn);
            const int64_t out[2] = {sh, dn};
            if (!put(o, out, 2)) return 5;
        } else if (tag == 3) {
            int64_t N, limit;
            if (!get(f, &N) || !get(f, &limit)) return 3;
            if (N < 2 || N > SP_LT_MAXN || limit < 1 || limit > SP_LT_DMAX) return 4;
            std::vector<int64_t> D((size_t)(N * N)), R((size_t)N), merges((size_t)((N - 1) * 5), -1);
            std::vector<uint8_t> live((size_t)N);
            if (!get(f, D.data(), D.size())) return 3;
            const int64_t status = sp_lt_host_nj(D.data(), (int)N, live.data(), R.data(), merges.data(), limit);
            if (!put(o, &status) || !put(o, merges.data(), merges.size())) return 5;
        } else if (tag == 4) {
            int64_t s, n;
            if (!get(f, &s) || !get(f, &n)) return 3;
            std::vector<uint64_t> sk((size_t)(n * s));
            std::vector<int32_t> len((size_t)n), sh((size_t)(n * n)), dn((size_t)(n * n));
            if (!get(f, sk.data(), sk.size()) || !get(f, len.data(), len.size())) return 3;
            sp_lt_host_pairs(sk.data(), len.data(), (int)n, (int)s, sh.data(), dn.data());
            if (!put(o, sh.data(), sh.size()) || !put(o, dn.data(), dn.size())) return 5;
        } else
            return 4;
    }
    fclose(f);
    return fclose(o) ? 5 : 0;
}
