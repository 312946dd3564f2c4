"""Inputs shared by test_ltrtree_host.py and test_gpu_ltrtree.py, with the twin's answers computed once and never changed."""
import random

import numpy as np

import ltrtree_ref as lt

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- sketches: (name, string, k, s)
def sketch_cases():
    def make():
        rng = random.Random(5)
        base = lt.rand_seq(rng, 700)
        out = [("n-runs", base[:200] + "N" * 7 + base[200:230] + "NN" + base[230:400] + "N" * 40 + base[400:], 13, 64),
               ("all-n", "N" * 300, 13, 16),
               ("short", base[:12], 13, 16),
               ("one-kmer", base[:13], 13, 16),
               ("fewer", base[:40], 13, 64),
               ("more", base, 13, 64),
               ("k9", base, 9, 16),
               ("k31", base, 31, 1024),
               ("tandem", base[:37] * 12, 13, 64)]
        L = 13
        while len(lt.hashes(base[:L], 13)) < 64:
            L += 1
        out.append(("exactly", base[:L], 13, 64))
        out += [("forward", base[50:450], 13, 64), ("revcomp", lt.revcomp(base[50:450]), 13, 64)]
        return [(n, s, k, sz, lt.sketch(s, k, sz)) for n, s, k, sz in out]
    return _once("sketch", make)


# ---- pairs: (name, a, b, s) with a, b ascending lists of distinct hashes
def pair_cases():
    def make():
        rng = random.Random(6)
        pool = sorted(rng.sample(range(1, 1 << 63), 200))
        out = [("identical", pool[:64], pool[:64], 64),
               ("disjoint", pool[0:128:2], pool[1:128:2], 64),
               ("one-empty", pool[:30], [], 64),
               ("other-empty", [], pool[:64], 64),
               ("both-empty", [], [], 64),
               ("unequal", pool[:64], pool[10:25], 64),
               ("short-union", pool[:10], pool[5:20], 64),
               ("cut-at-s", pool[0:128:2], sorted(pool[1:100:2] + pool[0:28:2]), 64),
               ("top-values", pool[:5] + [lt.NONE - 1], pool[3:9] + [lt.NONE - 1], 16)]
        return [(n, a, b, s, lt.pair(a, b, s)) for n, a, b, s in out]
    return _once("pair", make)


def hand_sketches(n, s, seed):
    """n hand-made sketches of s entries that overlap in many ways: (sketch uint64 [n, s], len int32 [n])"""
    rng = random.Random(seed)
    pool = sorted(rng.sample(range(1, 1 << 63), 3 * s))
    sk, ln = np.full((n, s), lt.NONE, np.uint64), np.zeros(n, np.int32)
    for i in range(n):
        kind = i % 5
        m = [s, 0, rng.randrange(1, s), s, rng.randrange(1, s)][kind]
        lo = [0, 0, rng.randrange(0, s), s // 2, 0][kind]
        row = sorted(rng.sample(pool[lo:lo + 2 * s], m))
        sk[i, :m], ln[i] = np.array(row, np.uint64), m
    return sk, ln


# ---- neighbour joining: (name, matrix)
NJ_SIZES = (2, 3, 4, 5, 33, 64, 65)


def nj_matrices(sizes=NJ_SIZES):
    out = []
    for N in sizes:
        out += [("random-%d" % N, lt.random_matrix(N, N)), ("tied-%d" % N, lt.tied_matrix(N)), ("zero-%d" % N, np.zeros((N, N), np.int64)),
                ("negative-%d" % N, lt.negative_matrix(N, N))]
    return out


def nj_expected(name, D):
    """the twin's records, computed once per name"""
    def make():
        r = lt.nj_numpy(D)
        r.setflags(write=False)
        return r
    return _once(("nj", name), make)


def tree_cases(sizes=(4, 5, 9, 33)):
    return [("tree-%d" % N,) + lt.random_tree(N, N) for N in sizes]


def tree_splits(edges, N):
    from subphaser_amd import ltrtree
    return ltrtree.splits(edges, N)


# ---- the planted end-to-end case
def planted(seed):
    """4 families of 8 members of 2000 bases: every member is its family's random ancestor with 5 % substitutions, half of
    them reverse-complemented; one chromosome, the members 100 random bases apart"""
    rng = random.Random(seed)
    members = []
    for fam in range(4):
        anc = lt.rand_seq(rng, 2000)
        for m in range(8):
            x = lt.mutate(rng, anc, 0.05)
            members.append((fam, lt.revcomp(x) if m % 2 else x))
    rng.shuffle(members)
    chrom, el = "", []
    for fam, x in members:
        chrom += lt.rand_seq(rng, 100)
        el.append((len(chrom), len(chrom) + len(x)))
        chrom += x
    return chrom + lt.rand_seq(rng, 100), el, [fam for fam, _ in members]


def families_are_clades(records, fams):
    from subphaser_amd import ltrtree
    N = len(fams)
    sp = ltrtree.splits(ltrtree.unrooted_edges(records), N)
    everyone = set(range(N))
    for f in set(fams):
        side = frozenset(i for i in range(N) if fams[i] == f)
        if side not in sp and frozenset(everyone - side) not in sp:
            return False
    return True


PLANTED_SEEDS = (0, 1)


def planted_twin(seed, k=13, s=256):
    """the planted case through the twin alone, computed once: (chrom, elements, families, sketch, len, shared, denom, D, records)"""
    def make():
        from subphaser_amd import ltrtree
        chrom, el, fams = planted(seed)
        sk, ln = lt.sketches([chrom[a:b] for a, b in el], k, s)
        shared, denom = lt.pairs(sk, ln, s)
        D = ltrtree.distance_matrix(shared, denom, k, s)
        return chrom, el, fams, sk, ln, shared, denom, D, lt.nj_numpy(D)
    return _once(("planted", seed, k, s), make)
