"""Cases of the profile alignment (sp_domalign.h), shared by the host check and the GPU tests: the smallest at which the
fill or the trace can still go wrong.  cases() returns (sequences, profiles, items, names): an item is (sequence index,
frame, i0, i1, profile index); domains_cases.genome() lays the sequences out on chromosomes for the device."""
import random

import numpy as np

import domains_ref as dr

_cache = {}
SIZES = (1, 2, 63, 64, 65, 128, 129, 512, 513, 2048)      # lane blocks of 1, 2, 3 nodes; the LDS / global table seam; the largest state


def flat_profile(M, emis=0, trans=-256):
    """all emissions and all transitions equal: every maximum over predecessors is a tie"""
    e = np.full((M, 22), emis, np.int64)
    return dr.make_profile(M, e, np.full((M, 7), trans, np.int64), name="flat%d" % M)


def hand_profile(residues, **trans):
    """node k emits residues[k - 1] at +1000 and everything else at -1000; transitions -2000 but the named ones
    (name_k = value, k the 1-based node)"""
    M = len(residues)
    emis = np.full((M, 22), -1000, np.int64)
    for k, a in enumerate(residues):
        emis[k, dr.AA.index(a)] = 1000
    emis[:, dr.X], emis[:, dr.STOP] = 0, -dr.STOPCOST
    t = np.full((M, 7), -2000, np.int64)
    for name, v in trans.items():
        kind, k = name.split("_")
        t[int(k) - 1, getattr(dr, kind)] = v
    return dr.make_profile(M, emis, t)


def cases():
    if "cases" in _cache:
        return _cache["cases"]
    rng = random.Random(4711)
    seqs, profs, items, names = [], [], [], []

    def seq(s):
        seqs.append(s)
        return len(seqs) - 1

    def prof(p):
        profs.append(p)
        return len(profs) - 1

    def item(name, s, f, i0, i1, p):
        assert 0 <= i0 <= i1 < len(dr.translate(seqs[s], f)), name
        items.append((s, f, i0, i1, p))
        names.append(name)
    # every size, a window of 40 residues inside a frame of 60 (M = 2048: the largest state) and one of 130 (three stages)
    s180, s480 = seq(dr.rand_dna(rng, 181)), seq(dr.rand_dna(rng, 480))
    by_size = {}
    for M in SIZES:
        by_size[M] = prof(dr.random_profile(rng, M, name="m%d" % M))
        item("m%d" % M, s180, M % 6, 5, 44, by_size[M])
        if M <= 513:
            item("m%d_130" % M, s480, (M + 1) % 6, 12, 141, by_size[M])
    # the residue stage: windows of 1, 2, 64, 65, 129 residues; both ends of the frame; all six frames
    p65, p5 = by_size[65], prof(dr.random_profile(rng, 5, star=0.2, name="m5"))
    for f in range(6):
        nres = len(dr.translate(seqs[s480], f))
        for n in (1, 2, 64, 65, 129):
            item("head%d_f%d" % (n, f), s480, f, 0, n - 1, (p65, p5)[n % 2])
            item("tail%d_f%d" % (n, f), s480, f, nres - n, nres - 1, (p5, p65)[n % 2])
        item("whole_f%d" % f, s480, f, 0, nres - 1, p65)
    # one window of 8192 residues at M = 65
    s_long = seq(dr.rand_dna(rng, 3 * 8200 + 2))
    item("win8192", s_long, 1, 3, 8194, p65)
    # a planted domain with N runs and stop codons; one insertion; one deletion
    c60 = dr.consensus_profile(rng, dr.rand_protein(rng, 60), name="c60")
    cons = "".join(max(pe, key=pe.get) for pe, _ in c60["probs"])
    pc60 = prof(c60)
    dom = dr.back_translate(rng, cons)
    flank = lambda n: dr.rand_dna(rng, n)
    s_n = seq(flank(21) + dom[:60] + "N" * 7 + dom[67:90] + "TAA" + dom[93:] + flank(30))
    item("n_run_stop", s_n, 0, 0, len(dr.translate(seqs[s_n], 0)) - 1, pc60)
    s_rc = seq(dr.revcomp(seqs[s_n]))
    item("n_run_stop_rc", s_rc, 3 + 0, 2, len(dr.translate(seqs[s_rc], 3)) - 3, pc60)
    s_ins = seq(flank(30) + dr.back_translate(rng, cons[:25] + "W" + cons[25:]) + flank(30))
    item("insert1", s_ins, 0, 0, len(dr.translate(seqs[s_ins], 0)) - 1, pc60)
    s_del = seq(flank(30) + dr.back_translate(rng, cons[:40] + cons[41:]) + flank(30))
    item("delete1", s_del, 0, 0, len(dr.translate(seqs[s_del], 0)) - 1, pc60)
    # ties: the flat profiles, on random residues
    for M in (3, 7, 70):
        pf = prof(flat_profile(M))
        item("flat%d" % M, s180, 2, 0, 30, pf)
    pz = prof(flat_profile(6, emis=0, trans=0))
    item("flat_zero", s180, 4, 3, 20, pz)
    _cache["cases"] = (seqs, profs, items, names)
    return _cache["cases"]


def mixed(n=200):
    """n items over a pool of short sequences and the profiles of 1..130 nodes: (sequences, profiles, items)"""
    rng = random.Random(99)
    seqs = [dr.rand_dna(rng, rng.randint(30, 400)) for _ in range(12)]
    profs = [dr.random_profile(rng, M, star=0.1 if M % 2 else 0.0, name="x%d" % M) for M in (1, 2, 9, 63, 64, 65, 130, 600)]
    items = []
    while len(items) < n:
        s, f = rng.randrange(len(seqs)), rng.randrange(6)
        nres = len(dr.translate(seqs[s], f))
        i0 = rng.randrange(nres)
        i1 = min(nres - 1, i0 + rng.randrange(0, 90))
        p = rng.randrange(len(profs))
        if profs[p]["M"] == 600 and rng.random() < 0.8:
            continue
        items.append((s, f, i0, i1, p))
    return seqs, profs, items
