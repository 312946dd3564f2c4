"""Hand-made chromosomes for the k = 16..32 count chain (subphaser_amd/csrc/sp_sparse2.hip) with declared bucket occupancy, and
a small model of the rules by which that chain picks a code path bucket by bucket.  No GPU import: tests/test_s3cases_host.py
checks every construction against the oracle on the CPU, tests/test_gpu_sparse_paths.py runs them on the device.

A chromosome is a shuffled pile of blocks `k bases + N`: every block holds exactly one valid k-mer, so a chromosome is a
multiset of keys chosen by hand.  A key is (fine bucket << R2) | residual; its first base is A and its last base is not T
(or, for k <= 17 in bucket 0, the nine leading A's outnumber the rest), so the forward strand is the canonical one and the
oracle must report exactly the designed keys with the designed counts.  The design of a chromosome is a dict
{fine bucket: (residuals ascending, copies)}; what a case declares -- n and the distinct count of each designed bucket, per
piece where s3_final splits it, the first finish kernel, whether the bucket is handed to s3_final, the branch there, the number
of give-up buckets and whether the library sort runs -- is route_bucket() applied to that design with the literals below
(tests/test_s3plan_host.py holds them equal to sp_s3plan.h).

The routes are chosen so that they do not depend on the device's hash functions: `lower` 1 where the two-stage hashed path is
meant (every key survives stage 1), buckets above 2048 keys otherwise (no stage 1), all keys of a piece under one piece prefix
where a piece's content matters.  Where a route does depend on them the model says so (`handed` None, branch
"piece_hash_or_sort"); both outcomes end in the same kernels and neither is used as evidence."""
import functools

import numpy as np

# ---------------------------------------------------------------- the literals of sp_s3plan.h
LIT = dict(S3_P1_UNIT=32, S3_P1T32=512, S3_P1T64=256, S3_P2_THREADS=512, S3_P2_PER=16, S3_P2_KEYS=8192,
           S3_SORT_THREADS=256, S3_SORT_PER=8, S3_SORT_CAP=2048, S3_SMALL_PER=8, S3_SMALL_CAP=2048,
           S3_SPLIT_BITS=8, S3_DIRECT_BITS=12, S3_HASH_SLOTS=2048, S3_HASH_MAX=1536,
           S3H_COUNTERS=4096, S3H_SLOTS=2048, S3H_CAP=1536, S3H_PER=8,
           S3_BM_MAXBITS=16, S3_BM_CAP=4096, S3_BM_NMAX=1 << 22, S3_BM_PER=8,
           S3B_SPREAD=32, S3B_KCAP=4096, S3B_MAXBIG=1024, S3_SAMPLE_MIN_LEN=1 << 24)
globals().update(LIT)

ACGT = np.frombuffer(b"ACGT", np.uint8)
NN = ord("N")
SMALL_BASES = 1_000_000          # cases below this many bases also run with exact sizing and side by side on lanes


class Plan:
    """s3_make_plan"""

    def __init__(self, k):
        self.B1 = 10
        self.B2 = 8 if k <= 17 else 9
        self.R1 = 2 * k - self.B1
        self.R2 = self.R1 - self.B2
        self.F1, self.F2 = 1 << self.B1, 1 << self.B2
        self.wide1, self.wide2 = self.R1 > 32, self.R2 > 32
        self.tile1 = (S3_P1T64 if self.wide1 else S3_P1T32) * S3_P1_UNIT       # starts per s3_part1 tile


def split_bits(n, R2):
    """s3_split_bits"""
    sb = 1
    while sb < S3_SPLIT_BITS and (n >> sb) > S3_SORT_CAP // 2:
        sb += 1
    return min(sb, R2)


# ---------------------------------------------------------------- the routing model
def _sort_per(n):
    """size class of a sort inside s3_final (keys per thread)"""
    return 2 if n <= 2 * S3_SORT_THREADS else 4 if n <= 4 * S3_SORT_THREADS else S3_SORT_PER


def _final_route(k, lower, res, cnt, hash_pieces, r):
    """s3_final on one bucket it was handed; fills r["branch"], r["pieces"], r["give_up"], r["tags"]"""
    R2 = Plan(k).R2
    n, tags = r["n"], r["tags"]
    if n <= S3_SORT_CAP:
        r["branch"] = "sort_per_%d" % _sort_per(n)
        tags.add("final:whole_sort")
        return
    sb = split_bits(n, R2)
    rem = R2 - sb
    piece = (res >> np.uint64(rem)).astype(np.int64)
    r["branch"], r["sb"], r["rem"], r["pieces"] = "split", sb, rem, []
    tags.add("final:split")
    for d in np.unique(piece):
        sel = piece == d
        m, dd = int(cnt[sel].sum()), int(sel.sum())
        if hash_pieces and m <= S3_SORT_THREADS * S3H_PER and (dd <= S3H_CAP):
            br = "piece_hash"
        elif hash_pieces and m <= S3_SORT_THREADS * S3H_PER and lower > 1:
            br = "piece_hash_or_sort"            # which singletons survive stage 1 decides whether the table closes
        elif m <= S3_SORT_CAP:
            br = "piece_sort_per_%d" % _sort_per(m)
        elif rem <= S3_DIRECT_BITS:
            br = "direct"
        elif dd > S3_HASH_MAX:
            br = "give_up"
        else:
            br = "hotkey_one" if dd == 1 else "hotkey_multi"
        r["pieces"].append((int(d), m, dd, br))
        tags.add("final:" + ("piece_sort" if br.startswith("piece_sort") else br))
        if br == "give_up":
            r["give_up"] = True
            break                                # the pieces behind it are not looked at
    if r["give_up"]:
        r["kept"] = int((cnt >= lower).sum())
        tags.add("big:kcap_fallback" if r["kept"] > S3B_KCAP else "big:class")


def route_bucket(k, lower, res, cnt, sort_mode=False):
    """The path of one fine bucket holding residual res[i] cnt[i] times (res ascending and distinct): a dict with n,
    distinct, first (the finish kernel that meets the bucket first), handed (to s3_final: True / False / None = decided by
    stage-1 collisions), branch, sb, rem, pieces [(piece, keys, distinct, branch)], give_up, kept and tags."""
    res, cnt = np.asarray(res, np.uint64), np.asarray(cnt, np.int64)
    R2 = Plan(k).R2
    n, d = int(cnt.sum()), int(len(res))
    tags = set()
    r = dict(n=n, distinct=d, handed=False, branch=None, sb=None, rem=None, pieces=None, give_up=False, kept=None, tags=tags)
    two_stage_max = S3_SORT_THREADS * S3H_PER
    if R2 <= S3_BM_MAXBITS:
        r["first"] = "s3_final_bitmap"
        if n > S3_BM_NMAX:
            r["handed"] = True
            tags.add("bitmap:punt_nmax")
        else:
            prefetch = S3_BM_PER * S3_SORT_THREADS
            tags.add("bitmap:prefetch_only" if n <= prefetch else "bitmap:streamed_tail")
            if abs(n - prefetch) <= 1:
                tags.add("bitmap:n=prefetch%+d" % (n - prefetch))
            if n == S3_BM_NMAX:
                tags.add("bitmap:n=nmax")
            if d == 1 << S3_BM_MAXBITS:
                tags.add("bitmap:all_bits")
            if d > S3_BM_CAP:
                r["handed"] = True
                tags.add("bitmap:punt_cap")
            else:
                tags.add("bitmap:stay")
            if abs(d - S3_BM_CAP) <= 1:
                tags.add("bitmap:distinct=cap%+d" % (d - S3_BM_CAP))
    elif not sort_mode:
        r["first"] = "s3_final_hash"
        if n > S3_BM_NMAX:
            r["handed"] = True
            tags.add("hash:punt_nmax")
        elif n <= two_stage_max:
            if d <= S3H_CAP:
                tags.add("hash:two_stage_stay")
            elif lower == 1:
                r["handed"] = True
                tags.add("hash:two_stage_punt")
            else:
                r["handed"] = None
                tags.add("hash:two_stage_collisions")
            if lower == 1 and abs(d - S3H_CAP) <= 1:
                tags.add("hash:two_stage_distinct=cap%+d" % (d - S3H_CAP))
        else:
            if d > S3H_CAP:
                r["handed"] = True
                tags.add("hash:stream_punt")
            else:
                tags.add("hash:stream_stay")
            if abs(d - S3H_CAP) <= 1:
                tags.add("hash:stream_distinct=cap%+d" % (d - S3H_CAP))
            if n == S3_BM_NMAX:
                tags.add("hash:n=nmax")
        if abs(n - two_stage_max) <= 1:
            tags.add("hash:n=two_stage%+d" % (n - two_stage_max))
    else:
        r["first"] = "s3_final_small"
        if n <= S3_SMALL_CAP:
            per = 1 if n <= S3_SORT_THREADS else 2 if n <= 2 * S3_SORT_THREADS else 4 if n <= 4 * S3_SORT_THREADS else S3_SMALL_PER
            r["branch"] = "small_per_%d" % per
            tags.add("small:per_%d" % per)
            for edge in (S3_SORT_THREADS, 2 * S3_SORT_THREADS, 4 * S3_SORT_THREADS, S3_SMALL_CAP):
                if abs(n - edge) <= 1:
                    tags.add("small:n=%d%+d" % (edge, n - edge))
        else:
            r["handed"] = True
    if r["handed"] is not False:
        fr = r if r["handed"] else dict(r, tags=set())        # (a bucket that may or may not be handed over: no tags from it)
        _final_route(k, lower, res, cnt, hash_pieces=not sort_mode and R2 > S3_BM_MAXBITS, r=fr)
        if not r["handed"]:
            assert fr["branch"].startswith("sort_per")         # n <= 2048: one sort, whatever stage 1 decides
    return r


# ---------------------------------------------------------------- keys <-> sequence
def revcomp(keys, k):
    x = ~np.asarray(keys, np.uint64)
    m2, m4 = np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
    x = ((x >> np.uint64(2)) & m2) | ((x & m2) << np.uint64(2))
    x = ((x >> np.uint64(4)) & m4) | ((x & m4) << np.uint64(4))
    return x.byteswap() >> np.uint64(64 - 2 * k)


def valid_res(k, i):
    """the i-th residual (ascending) a block chromosome may use in any bucket: for k >= 18 the last base is not T; always
    below 2^(R2 - 1) for the i used here, so the residual's top bit is 0 as behind the ten-A prefix"""
    i = np.asarray(i, np.uint64)
    return i if k <= 17 else (i // np.uint64(3)) * np.uint64(4) + i % np.uint64(3)


def under(k, top, top_bits, low):
    """residual with `top` in the `top_bits` bits that s3_final's split looks at first (for k >= 18 below the bit the tenth A
    holds at 0) and `low` in the low bits"""
    R2 = Plan(k).R2
    free = R2 if k <= 17 else R2 - 1
    return (np.asarray(top, np.uint64) << np.uint64(free - top_bits)) | np.asarray(low, np.uint64)


def seq_of_keys(k, keys, copies, seed):
    keys = np.asarray(keys, np.uint64)
    idx = np.repeat(np.arange(len(keys)), np.broadcast_to(np.asarray(copies, np.int64), keys.shape))
    np.random.RandomState(seed).shuffle(idx)
    kk = keys[idx]
    shifts = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    blocks = np.empty((len(kk), k + 1), np.uint8)
    blocks[:, :k] = ACGT[((kk[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.intp)]
    blocks[:, k] = NN
    return blocks.reshape(-1)


class Chrom:
    """one chromosome: `design` {bucket: (residuals, copies)} (None: plain sequence, nothing declared) and its bases"""

    def __init__(self, k, design=None, seq=None, seed=0, note=""):
        self.k, self.note, self._seq, self.seed = k, note, seq, seed
        self.design = None
        if design is not None:
            self.design = {}
            for b, (res, cp) in design.items():
                res = np.asarray(res, np.uint64)
                cp = np.broadcast_to(np.asarray(cp, np.int64), res.shape).copy()
                o = np.argsort(res, kind="stable")
                assert (res[o][1:] > res[o][:-1]).all(), "residuals must be distinct"
                self.design[int(b)] = (res[o], cp[o])

    def keys(self):
        """(keys ascending, copies) of the design"""
        R2 = np.uint64(Plan(self.k).R2)
        ks = np.concatenate([(np.uint64(b) << R2) | res for b, (res, _) in sorted(self.design.items())])
        cs = np.concatenate([cp for _, (_, cp) in sorted(self.design.items())])
        return ks, cs

    def seq(self):
        if self._seq is not None:
            return self._seq() if callable(self._seq) else self._seq
        ks, cs = self.keys()
        assert (ks < revcomp(ks, self.k)).all(), "a designed key is not its own canonical form"
        return seq_of_keys(self.k, ks, cs, self.seed)


class Case:
    def __init__(self, name, k, lowers, chroms, sort_mode=False, bases=None):
        self.name, self.k, self.lowers, self.chroms, self.sort_mode = name, k, tuple(lowers), chroms, sort_mode
        self._bases = bases

    @functools.lru_cache(maxsize=None)
    def seqs(self):
        return [c.seq() for c in self.chroms]

    def n_bases(self):
        if self._bases is not None:
            return self._bases
        n = 0
        for c in self.chroms:
            n += sum(int(cp.sum()) * (self.k + 1) for _, cp in c.design.values()) if c.design is not None else len(c.seq())
        return n

    @property
    def small(self):
        return self.n_bases() < SMALL_BASES

    def env(self):
        return {"SP_S3_FINAL": "sort"} if self.sort_mode else {}

    def declared(self, lower, designs=None):
        """The declaration at one `lower`: per chromosome {bucket: route}, and for the case the first finish kernel, the
        largest number of give-up buckets of a chromosome and whether the library sort + s3_big_rle runs.  `designs`:
        the per-chromosome designs to route instead of the hand-made ones (what the oracle found)."""
        P = Plan(self.k)
        first = "s3_final_bitmap" if P.R2 <= S3_BM_MAXBITS else "s3_final_small" if self.sort_mode else "s3_final_hash"
        out = dict(first=first, chroms=[], n_big=0, rle=False, tags=set())
        for ci, c in enumerate(self.chroms):
            design = c.design if designs is None else designs[ci]
            routes = {}
            if design is not None:
                for b, (res, cp) in design.items():
                    routes[b] = route_bucket(self.k, lower, res, cp, self.sort_mode)
                    assert routes[b]["first"] == first
                    out["tags"] |= routes[b]["tags"]
                out["tags"] |= _chrom_tags(self.k, design, c.note)
            big = [r for r in routes.values() if r["give_up"]]
            out["n_big"] = max(out["n_big"], len(big))
            out["rle"] |= any(r["kept"] > S3B_KCAP for r in big) or len(big) > S3B_MAXBIG
            out["chroms"].append(routes)
        return out


def _chrom_tags(k, design, note):
    """what a chromosome's design means for the two partition kernels"""
    P = Plan(k)
    tags = set()
    per_l1 = {}
    for b, (_, cp) in design.items():
        per_l1[b >> P.B2] = per_l1.get(b >> P.B2, 0) + int(cp.sum())
    for n in per_l1.values():                     # a level-1 bucket of n keys is cut into part2 tiles of S3_P2_KEYS
        for t in (1, 2):
            if abs(n - t * S3_P2_KEYS) <= 1:
                tags.add("part2:n=%dx%d%+d" % (t, S3_P2_KEYS, n - t * S3_P2_KEYS))
    if note.startswith("every_start:"):           # poly-A: every start is valid and has the same key
        n = int(note.split(":")[1])
        if len(per_l1) == 1 and sum(per_l1.values()) == n and n >= P.tile1:
            tags.add("part1:tile_one_bucket_rank_%d" % (P.tile1 - 1))
    return tags


# ---------------------------------------------------------------- the cases
def _seed(*a):
    """a shuffle seed of its own for every chromosome"""
    return sum((i + 1) * 7919 * int(x) for i, x in enumerate(a)) & 0x7FFFFFFF


def _singles(k, d, stride=1):
    return valid_res(k, np.arange(d, dtype=np.uint64) * np.uint64(stride))


def _polyA(k, copies):
    n = copies + k - 1
    return Chrom(k, {0: ([0], [copies])}, seq=lambda: np.full(n, ord("A"), np.uint8), note="every_start:%d" % copies)


def _acgt(rng, n):
    return ACGT[rng.randint(0, 4, size=n)].copy()


def _with_n(seq, *pos):
    s = seq.copy()
    for p in pos:
        s[p] = NN
    return s


def _build():
    cases = []

    def add(name, k, lowers, chroms, **kw):
        cases.append(Case(name, k, lowers, chroms if isinstance(chroms, list) else [chroms], **kw))

    # ---- bitmap finish (k = 16, 17)
    for k in (16, 17):
        R2 = Plan(k).R2
        stride = (1 << R2) // (S3_BM_CAP + 1) - (1 << R2) // (S3_BM_CAP + 1) % 2 + 1       # odd: 3 at k = 16, 15 at k = 17
        for d in (S3_BM_CAP, S3_BM_CAP + 1):
            # residuals spread over the whole range: a punted bucket splits into pieces of about 1024 keys that are sorted
            add("bitmap_%d_distinct_x1_k%d" % (d, k), k, (1,), Chrom(k, {0: (_singles(k, d, stride), 1)}, seed=_seed(k, d, 1)))
            add("bitmap_%d_distinct_x2_k%d" % (d, k), k, (2, 3), Chrom(k, {0: (_singles(k, d, stride), 2)}, seed=_seed(k, d, 2)))
        for n in (2047, 2048, 2049):
            add("bitmap_%d_keys_k%d" % (n, k), k, (1,), Chrom(k, {0: (_singles(k, n, 7), 1)}, seed=_seed(k, n)))
        # copies 1..4 cycling over 600 residuals: counts of lower - 1, lower and lower + 1 side by side for lower = 2 and 3
        add("bitmap_lower_edges_k%d" % k, k, (2, 3),
            Chrom(k, {0: (_singles(k, 600, 13), 1 + np.arange(600) % 4)}, seed=_seed(k, 600)))
    add("bitmap_all_65536_k17", 17, (1,), Chrom(17, {0: (np.arange(65536, dtype=np.uint64), 1)}, seed=17))

    # ---- more than 2^22 keys in one bucket; every part1 tile in one level-1 bucket
    for k in (17, 18, 21, 26):
        add("polyA_nmax_k%d" % k, k, (1,), _polyA(k, S3_BM_NMAX), bases=S3_BM_NMAX + k - 1)
        add("polyA_nmax_plus_1_k%d" % k, k, (1,), _polyA(k, S3_BM_NMAX + 1), bases=S3_BM_NMAX + k)

    def poly_c(k):
        s = np.full(3 * Plan(k).tile1 + 77, ord("A"), np.uint8)
        s[Plan(k).tile1 + Plan(k).tile1 // 2 + 5] = ord("C")
        return s
    for k in (21, 22):
        add("polyA_one_C_k%d" % k, k, (1, 2), Chrom(k, seq=functools.partial(poly_c, k)), bases=3 * Plan(k).tile1 + 77)

    # ---- s3_final's direct count with many distinct residuals: k = 17, 2^19 keys, sb = 8, 8 bits left; the 256 pieces hold
    # 31, 32 or 33 distinct residuals x 64 copies = 1984, 2048 (sorted) or 2112 keys (counted directly)
    top = np.repeat(np.arange(256), 31 + np.arange(256) % 3)
    low = np.concatenate([np.arange(31 + j % 3) * 7 % 256 for j in range(256)])
    add("direct_many_distinct_k17", 17, (1, 64, 65), Chrom(17, {0: (under(17, top, 8, low), 64)}, seed=1764))

    # ---- hashed finish (k >= 18): u32 / u32, u64 / u32 and u64 / u64 records
    for k in (18, 21, 25, 32):
        two = S3_SORT_THREADS * S3H_PER
        add("hash_%d_keys_k%d" % (two, k), k, (1, 2), Chrom(k, {0: (_singles(k, two // 2, 5), 2)}, seed=_seed(k, two)))
        add("hash_%d_keys_k%d" % (two + 1, k), k, (1, 2),
            Chrom(k, {0: (_singles(k, two // 2 + 1, 5), [2] * (two // 2) + [1])}, seed=_seed(k, two + 1)))
        for d in (S3H_CAP, S3H_CAP + 1):
            # streaming (3072 / 3074 keys): the table closes at the 1537th distinct residual; the punted bucket splits in
            # two (sb = 2, the residuals alternate between the pieces), each piece is counted by the hashed path
            r = under(k, np.arange(d) % 2, 1, valid_res(k, np.arange(d) // 2 * 3))
            add("hash_stream_%d_distinct_x2_k%d" % (d, k), k, (2,), Chrom(k, {0: (r, 2)}, seed=_seed(k, d, 2)))
            # two stages at lower 1 (every key survives stage 1): stays / punt and one sort of <= 2048 keys
            add("hash_two_stage_%d_distinct_k%d" % (d, k), k, (1,), Chrom(k, {0: (r, 1)}, seed=_seed(k, d, 1)))
        # stage-1 collisions must not leak singletons: 2000 singletons + 20 doubles at lower 2
        add("hash_singletons_beside_doubles_k%d" % k, k, (2,),
            Chrom(k, {0: (_singles(k, 2020, 11), [1] * 2000 + [2] * 20)}, seed=_seed(k, 2020)))

    # ---- s3_final's hot-key hash with several distinct residuals
    for k in (21, 26):
        # the smallest: 1600 singletons under piece 0 (punt: > 1536 distinct; the piece: hashed count, sorted when its
        # table closes) and 3 residuals x 800 copies under piece 1 (2400 keys: past one sort, more than 12 bits left)
        crowd = under(k, 0, 1, valid_res(k, np.arange(1600) * 3))
        hot = under(k, 1, 1, valid_res(k, np.array([5, 77, 4000])))
        add("hotkey_3_distinct_k%d" % k, k, (1, 2, 800, 801),
            Chrom(k, {0: (np.concatenate([crowd, hot]), [1] * 1600 + [800] * 3)}, seed=_seed(k, 1603)))
    # 2048 distinct x 160 copies: sb = 8, rem = 15, 128 pieces of 16 distinct residuals and 2560 keys
    add("hotkey_2048_distinct_x160_k21", 21, (2,),
        Chrom(21, {0: (under(21, np.arange(2048) // 16, 7, valid_res(21, np.arange(2048) % 16 * 5)), 160)}, seed=2148))

    # ---- give-up: one piece of more than 2048 keys, more than 12 bits left, more than S3_HASH_MAX distinct
    for k in (21, 32):
        add("give_up_1600_distinct_x2_k%d" % k, k, (1, 2, 3), Chrom(k, {0: (_singles(k, 1600, 3), 2)}, seed=_seed(k, 1600)))
        add("give_up_4200_distinct_x2_k%d" % k, k, (2, 3), Chrom(k, {0: (_singles(k, 4200, 3), 2)}, seed=_seed(k, 4200)))

    # ---- sort size classes (SP_S3_FINAL=sort): eleven fine buckets, copies 1..3 mixed
    for k in (21, 26):
        design = {}
        for j, n in enumerate((1, 255, 256, 257, 512, 513, 1024, 1025, 2047, 2048, 2049)):
            cp = 1 + (np.arange(n) + j) % 3          # then trimmed so that the bucket holds exactly n keys
            d = int(np.searchsorted(np.cumsum(cp), n)) + 1
            cp = cp[:d].copy()
            cp[-1] -= int(cp.sum()) - n
            design[3 * j + 1] = (_singles(k, d, 9), cp)
        add("sort_size_classes_k%d" % k, k, (1, 2, 3), Chrom(k, design, seed=_seed(k, 11)), sort_mode=True)

    # ---- part1 seams per record width: all-ACGT chromosomes of 3 tiles + {0, 1, 31, 32, 33}, one N each, tiny ones
    for k in (17, 21, 25, 32):
        tile = Plan(k).tile1

        def seams(k=k, tile=tile):
            rng = np.random.RandomState(5000 + k)
            seqs = [_acgt(rng, 3 * tile + extra) for extra in (0, 1, 31, 32, 33)]
            base = _acgt(rng, 3 * tile + 33)
            wave = tile + 2 * 2048                        # a wave of the second tile (64 units of 32 starts)
            seqs += [_with_n(base, wave + 0 * 32 + 31),   # first lane of a wave (starts p - k + 1 .. p lie in one unit)
                     _with_n(base, wave + 63 * 32 + 31),  # last lane of a wave
                     _with_n(base, 3 * tile + 31),        # the last unit
                     _with_n(base, 0), _with_n(base, len(base) - 1),
                     _with_n(base, wave + 7 * 32 + 32 - (k - 1)),      # k - 1 bases before a unit boundary
                     _with_n(base, 2 * tile + 3),         # the spoiled starts straddle two units and a tile boundary
                     _acgt(rng, k - 1), _acgt(rng, k), _acgt(rng, k + 1), np.empty(0, np.uint8)]
            return seqs
        n_chrom = 16
        chroms = [Chrom(k, seq=(lambda i=i, f=functools.lru_cache(maxsize=None)(seams): f()[i])) for i in range(n_chrom)]
        add("part1_seams_k%d" % k, k, (1,), chroms, bases=12 * 3 * tile + (1 + 31 + 32 + 33) + 7 * 33 + 3 * k)

    # ---- part2 seams: every key in level-1 bucket 0; tiles of 8191, 8192, 8193 keys, two tiles + 511 / 513
    for k in (17, 21, 25, 26):
        F2 = Plan(k).F2
        chroms = []
        for n in (S3_P2_KEYS - 1, S3_P2_KEYS, S3_P2_KEYS + 1, 2 * S3_P2_KEYS + 511, 2 * S3_P2_KEYS + 513):
            per = np.bincount(np.arange(n) % F2, minlength=F2)
            chroms.append(Chrom(k, {0: (_singles(k, n, 3), 1)}, seed=_seed(k, n, 0)))
            chroms.append(Chrom(k, {b: (_singles(k, int(per[b]), 3), 1) for b in range(F2)}, seed=_seed(k, n, 1)))
        add("part2_seams_k%d" % k, k, (1,), chroms)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every path the suite did not reach before must be the declared route of at least one case (tests/test_s3cases_host.py)
REQUIRED_TAGS = {
    "bitmap:stay", "bitmap:punt_cap", "bitmap:punt_nmax", "bitmap:all_bits", "bitmap:n=nmax",
    "bitmap:distinct=cap+0", "bitmap:distinct=cap+1",
    "bitmap:prefetch_only", "bitmap:streamed_tail", "bitmap:n=prefetch-1", "bitmap:n=prefetch+0", "bitmap:n=prefetch+1",
    "hash:two_stage_stay", "hash:two_stage_punt", "hash:two_stage_collisions", "hash:stream_stay", "hash:stream_punt",
    "hash:punt_nmax", "hash:n=nmax",
    "hash:two_stage_distinct=cap+0", "hash:two_stage_distinct=cap+1", "hash:stream_distinct=cap+0", "hash:stream_distinct=cap+1",
    "hash:n=two_stage+0", "hash:n=two_stage+1",
    "final:whole_sort", "final:split", "final:piece_hash", "final:piece_sort", "final:direct",
    "final:hotkey_one", "final:hotkey_multi", "final:give_up", "big:class", "big:kcap_fallback",
    "small:per_1", "small:per_2", "small:per_4", "small:per_8",
    "part1:tile_one_bucket_rank_16383", "part1:tile_one_bucket_rank_8191",
    "part2:n=1x8192-1", "part2:n=1x8192+0", "part2:n=1x8192+1",
}


@functools.lru_cache(maxsize=None)
def oracle_counts(name):
    """the oracle's (keys ascending, counts) at lower 1 of every chromosome of a case, computed once per session"""
    import pyoracle as po
    case = BY_NAME[name]
    return [po.count(s, case.k, 1, nthreads=4) for s in case.seqs()]


def oracle_at(name, lower):
    return [(k[c >= lower], c[c >= lower]) for k, c in oracle_counts(name)]
