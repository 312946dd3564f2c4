"""Cases of the domain search (sp_domains.h), shared by the host check and the GPU tests: the smallest at which the
search can still go wrong.  A case is (name, inner sequence, profile names); genome() lays the sequences out on
chromosomes for the device."""
import random

import domains_ref as dr

_cache = {}


def profiles():
    """name -> profile"""
    if "profiles" in _cache:
        return _cache["profiles"]
    rng = random.Random(20261)
    P = {}
    for M in (1, 2, 5, 63, 64, 65, 129):
        P["m%d" % M] = dr.random_profile(rng, M, name="m%d" % M)
    P["star65"] = dr.random_profile(rng, 65, star=0.25, name="star65")
    P["star200"] = dr.random_profile(rng, 200, star=0.1, name="star200")
    P["m600"] = dr.random_profile(rng, 600, name="m600")              # tables from global memory
    P["m2048"] = dr.random_profile(rng, 2048, name="m2048")
    for name, M in (("c60", 60), ("c200", 200), ("c700", 700)):
        P[name] = dr.consensus_profile(rng, dr.rand_protein(rng, M), name=name)
        P[name]["consensus"] = "".join(max(pe, key=pe.get) for pe, _ in P[name]["probs"])
    _cache["profiles"] = P
    return P


def cases():
    if "cases" in _cache:
        return _cache["cases"]
    rng = random.Random(77)
    P = profiles()
    small = ["m1", "m2", "m5"]
    out = []
    for n in (0, 1, 2, 3, 4, 5, 30, 31, 32):
        out.append(("len%d" % n, dr.rand_dna(rng, n), small + ["m65"]))
    out.append(("sizes", dr.rand_dna(rng, 300), ["m1", "m2", "m63", "m64", "m65", "m129", "star65", "star200"]))
    out.append(("m2048", dr.rand_dna(rng, 120), ["m2048"]))
    out.append(("m600", dr.rand_dna(rng, 240), ["m600", "m64"]))
    c60, c200 = P["c60"]["consensus"], P["c200"]["consensus"]
    dom = dr.back_translate(rng, c60)
    flank = lambda n: dr.rand_dna(rng, n)
    out.append(("planted", flank(50) + dom + flank(40), ["c60", "m64"]))
    out.append(("planted_rc", flank(31) + dr.revcomp(dom) + flank(17), ["c60"]))
    out.append(("n_run", flank(20) + dom[:60] + "N" * 7 + dom[67:] + flank(20), ["c60"]))
    out.append(("stop", flank(21) + dom[:90] + "TAA" + dom[93:120] + "TGA" + dom[123:] + flank(9), ["c60"]))
    out.append(("iupac_lower", flank(12) + dom[:30].lower() + "RYK" + dom[33:] + flank(5), ["c60"]))
    out.append(("delete70", flank(30) + dr.back_translate(rng, c200[:60] + c200[130:]) + flank(30), ["c200"]))
    out.append(("insert70", flank(30) + dr.back_translate(rng, c200[:100] + dr.rand_protein(rng, 70) + c200[100:]) + flank(30), ["c200"]))
    out.append(("start_tie", flank(30) + dom + "ACGTAC" + dom + flank(30), ["c60"]))
    half = flank(30) + dom + flank(12)
    out.append(("frame_tie", half + dr.revcomp(half), ["c60", "m5"]))
    c700 = dr.back_translate(rng, P["c700"]["consensus"])
    out.append(("res700", flank(10) + c700 + flank(11), ["m65", "m129", "c700", "c60"]))
    _cache["cases"] = out
    return out


def many(n=2000):
    """(inner sequences, profile names): n elements drawn from a pool of 40 sequences of 0..90 bases, against 8 profiles
    of mixed sizes -- the twin computes each (sequence, profile) once"""
    rng = random.Random(5)
    pool = [dr.rand_dna(rng, rng.randint(0, 90)) for _ in range(40)]
    return [pool[rng.randrange(40)] for _ in range(n)], ["m1", "m2", "m5", "m63", "m64", "m65", "m129", "m600"]


def genome(seqs, n_chrom=2, seed=9):
    """lay the sequences out on n_chrom chromosomes with random spacers of 0..40 bases; the first starts at base 0 of
    its chromosome and the last ends on the last base of its one.  Returns (chromosomes, chrom, start, end)."""
    rng = random.Random(seed)
    parts, chrom, start, end = [[] for _ in range(n_chrom)], [], [], []
    length = [0] * n_chrom
    per = (len(seqs) + n_chrom - 1) // n_chrom
    for q, s in enumerate(seqs):
        c = q // per
        if length[c]:
            sp = dr.rand_dna(rng, rng.randint(0, 40))
            parts[c].append(sp)
            length[c] += len(sp)
        chrom.append(c)
        start.append(length[c])
        parts[c].append(s)
        length[c] += len(s)
        end.append(length[c])
    return ["".join(p) or "ACGT" for p in parts], chrom, start, end
