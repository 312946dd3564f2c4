"""Cases of the ungapped prefilter (sp_domains.hip: dm_ssv), shared by the GPU test and the CPU check of their names: the
smallest at which the kernel's tiles of 128 nodes, its lanes per diagonal and its workgroups of 1024 diagonals can go wrong."""
import random

import numpy as np

import domains_cases as dc
import domains_ref as dr
import domssv_ref as sr

TILE = 128      # SP_DM_STILE in sp_domains.hip
_cache = {}


def spike(M, k, name):
    """node k emits W at +3000, every other emission is -1000 (X 0, stop -8 bits as read_hmm makes them); m->m costs 300"""
    emis = np.full((M, 22), -1000, np.int64)
    emis[k - 1, dr.AA.index("W")] = 3000
    emis[:, dr.X], emis[:, dr.STOP] = 0, -dr.STOPCOST
    return dr.make_profile(M, emis, np.full((M, 7), -300, np.int64), name=name)


def dull(rng, n):
    """n codons that are neither W nor a stop"""
    pool = [c for c, r in dr.CODON.items() if r not in ("W", "*")]
    return "".join(rng.choice(pool) for _ in range(n))


def world():
    """(names, sequences, profiles by name, profile names)"""
    if "world" in _cache:
        return _cache["world"]
    rng = random.Random(4242)
    P = {"m%d" % M: dr.random_profile(rng, M, star=0.05, name="m%d" % M) for M in (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE)}
    P["m2048"] = dc.profiles()["m2048"]
    P["c200"] = dc.profiles()["c200"]
    P["w_first"], P["w_last"], P["w_mid"] = spike(70, 1, "w_first"), spike(70, 70, "w_last"), spike(TILE + 40, TILE, "w_mid")
    seqs = [("len%d" % n, dr.rand_dna(rng, n)) for n in (0, 1, 2, 3, 5, 191, 192, 193, 196, 400)]
    seqs += [("all_invalid", "N" * 61), ("one_in_three", "ACN" * 21), ("stops", dr.rand_dna(rng, 30) + "TAATGATAG" * 9 + dr.rand_dna(rng, 31))]
    seqs += [("w_at_first", "TGG" + dull(rng, 40)), ("w_at_last", dull(rng, 40) + "TGG"), ("w_inside", dull(rng, 17) + "TGG" + dull(rng, 23))]
    seqs += [("c200", dr.rand_dna(rng, 31) + dr.back_translate(rng, P["c200"]["consensus"]) + dr.rand_dna(rng, 20)),
             ("c200_rc", dr.revcomp(dr.rand_dna(rng, 10) + dr.back_translate(rng, P["c200"]["consensus"]) + dr.rand_dna(rng, 5)))]
    _cache["world"] = ([s[0] for s in seqs], [s[1] for s in seqs], P, list(P))
    return _cache["world"]


def expected():
    """the twin's int32 [n, P, 6] of the world"""
    if "expected" not in _cache:
        names, seqs, P, pn = world()
        _cache["expected"] = sr.ssv(seqs, [P[p] for p in pn])
    return _cache["expected"]


def check_names():
    """the cases do what their names say (by the twin)"""
    names, seqs, P, pn = world()
    exp = expected()
    res = {n: {p: exp[i, j].tolist() for j, p in enumerate(pn)} for i, n in enumerate(names)}
    assert res["len0"]["m1"] == [dr.INT32_MIN] * 6 and res["len2"]["m64"] == [dr.INT32_MIN] * 6
    assert [s > dr.INT32_MIN for s in res["len3"]["m1"]] == [True, False, False, True, False, False]
    assert [s > dr.INT32_MIN for s in res["len5"]["m65"]] == [True] * 6
    lens = sorted({len(dr.translate(s, f)) for n, s in zip(names, seqs) if n.startswith("len") for f in range(6)})
    assert lens == [0, 1, 63, 64, 65, 132, 133]
    e70, emid = dr.entry_score(70), dr.entry_score(TILE + 40)
    assert res["all_invalid"]["w_first"] == [e70] * 6 and res["all_invalid"]["m2048"][0] == P["m2048"]["entry"]      # X scores 0: the best cell is one cell
    assert dr.translate(seqs[names.index("stops")], 0).count(dr.STOP) == 27
    assert res["w_at_first"]["w_first"][0] == e70 + 3000 == res["w_at_first"]["w_last"][0]      # cell (0, 1) and cell (0, M)
    assert res["w_at_last"]["w_first"][0] == e70 + 3000 == res["w_at_last"]["w_last"][0]        # cell (n - 1, 1) and cell (n - 1, M)
    assert res["w_inside"]["w_mid"][0] == emid + 3000                                           # cell (17, 128): the last node of the first tile
    hit = dr.frame_hit(dr.translate(seqs[names.index("c200")], 1), P["c200"])
    assert (hit[1] % 2048, hit[3]) == (0, 200) and res["c200"]["c200"][1] == hit[0] > 200 * 2 * 256      # nodes 1..200 without a gap: across node 128
    assert res["c200_rc"]["c200"][3 + 10 % 3] > 200 * 2 * 256      # the reverse strand read from its first base has 10 bases in front of the domain
