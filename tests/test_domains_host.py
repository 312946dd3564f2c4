"""CPU: the arithmetic of the domain search (subphaser_amd/csrc/sp_domains.h) and its twin (tests/domains_ref.py).

tests/domains_host_check.cpp is compiled against the header with the host C++ compiler and its driver -- rows in sequence,
nodes in sequence -- is compared with the twin with `==` on all six outputs over tests/domains_cases.py.  The twin's
row-at-a-time search is compared with a plain triple loop over tuples on tiny cases and with hand-computed cases, and it is
checked against planted truth."""
import random
import struct

import numpy as np
import pytest

import domains_cases as dc
import domains_ref as dr
import host_check

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _record(seq, prof):
    codes = bytes(CODE.get(c, 4) for c in seq.upper())
    return (struct.pack("<qqq", 1, len(seq), prof["M"]) + codes + prof["emis"].astype("<i4").tobytes() + prof["trans"].astype("<i4").tobytes()
            + struct.pack("<i", prof["entry"]))


def _header(tmp, pairs):
    data, res = tmp / "in.bin", tmp / "out.bin"
    data.write_bytes(b"".join(_record(s, p) for s, p in pairs) + struct.pack("<q", 0))
    r = host_check.run(tmp, "domains_host_check", [data, res])
    assert host_check.ok_count(r) == len(pairs)
    return np.frombuffer(res.read_bytes(), "<i4").reshape(len(pairs), 7)


def test_header_is_the_twin(tmp_path):
    P = dc.profiles()
    names, pairs = [], []
    for name, seq, profs in dc.cases():
        for p in profs:
            names.append((name, p))
            pairs.append((seq, P[p]))
    seqs, profs = dc.many(60)
    for q, s in enumerate(seqs):
        for p in profs[:6]:
            names.append(("many%d" % q, p))
            pairs.append((s, P[p]))
    got = _header(tmp_path, pairs)
    memo = {}
    want = np.array([dr.element(s, p, memo=memo) for s, p in pairs], np.int32)
    bad = np.flatnonzero((got[:, :6] != want).any(axis=1))
    assert bad.size == 0, [(names[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    assert (got[:, 6] == 1).all()
    res = {n: r for n, r in zip(names, want.tolist())}
    # the cases do what their names say
    for n in (0, 1, 2):
        assert res[("len%d" % n, "m1")] == [dr.INT32_MIN, 0, 0, 0, 0, 0]
    assert res[("len3", "m1")][0] > dr.INT32_MIN and res[("len3", "m1")][2:] == [0, 0, 1, 1]
    assert res[("planted", "c60")][1:] == [2, 16, 75, 1, 60]                                     # 50 bases in front: frame 2, residue 16
    assert res[("planted_rc", "c60")][1] == 3 + 17 % 3 and res[("planted_rc", "c60")][4:] == [1, 60]
    for n in ("n_run", "stop", "iupac_lower"):
        assert res[(n, "c60")][4:] == [1, 60] and res[(n, "c60")][0] < res[("planted", "c60")][0]
    d = res[("delete70", "c200")]
    assert d[4:] == [1, 200] and d[3] - d[2] + 1 == 130
    ins = res[("insert70", "c200")]
    assert ins[4:] == [1, 200] and ins[3] - ins[2] + 1 == 270
    assert res[("start_tie", "c60")][1:] == [0, 10, 69, 1, 60]                                    # the first of two equal copies
    assert res[("frame_tie", "c60")][1] == 0 and res[("frame_tie", "c60")][2:] == [10, 69, 1, 60]  # frames 0 and 3 read the same residues
    assert res[("res700", "c700")][2:] == [3, 702, 1, 700]


def test_tables_out_of_range_are_seen(tmp_path):
    rng = random.Random(3)
    pairs = []
    for col, val in ((("emis", 0, 3), (1 << 15) + 1), (("emis", 2, 21), dr.NEG - 1), (("trans", 1, 6), 1), (("trans", 0, 0), dr.NEG - 1), (("entry",), 1),
                     (("emis", 0, 3), 1 << 15), (("trans", 1, 6), dr.NEG)):
        p = dr.random_profile(rng, 3)
        if col[0] == "entry":
            p["entry"] = val
        else:
            p[col[0]][col[1], col[2]] = val
        pairs.append(("", p))
    assert _header(tmp_path, pairs)[:, 6].tolist() == [0, 0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("seed", range(6))
def test_row_search_is_the_triple_loop(seed):
    rng = random.Random(seed)
    for _ in range(12):
        M = rng.choice([1, 2, 3, 4, 7, 12])
        prof = dr.random_profile(rng, M, star=rng.choice([0.0, 0.3]))
        if rng.random() < 0.4:      # few distinct scores: ties everywhere
            prof["emis"][:, :20] = np.array([[rng.choice([-256, 0, 256]) for _ in range(20)] for _ in range(M)])
            prof["trans"][:] = np.array([[rng.choice([-512, -256, 0]) for _ in range(7)] for _ in range(M)])
        seq = dr.rand_dna(rng, rng.randint(0, 40))
        if rng.random() < 0.3 and len(seq) > 6:
            seq = seq[:3] + "N" + seq[4:]
        assert dr.element(seq, prof) == dr.element(seq, prof, engine=dr.frame_hit_plain), (M, seq)


def test_jobs_side_by_side_are_jobs_alone():
    rng = random.Random(12)
    jobs = []
    for M in (1, 2, 3, 9, 30, 5, 1, 17):
        prof = dr.random_profile(rng, M, star=0.2)
        for n in (0, 1, 7, 40, 3):
            jobs.append(([rng.randrange(22) for _ in range(n)], prof))
    rng.shuffle(jobs)
    got = dr.frames_hits(jobs)
    assert got == [dr.frames_hits([j])[0] for j in jobs] and sum(g is None for g in got) == 8
    assert got == [dr.frame_hit_plain(r, p) for r, p in jobs]
    seqs = [dr.rand_dna(rng, n) for n in (0, 2, 50, 33, 90)]
    profs = [p for _, p in jobs[:5]]
    assert dr.search(seqs, profs, batch=7).tolist() == [[dr.element(s, p) for p in profs] for s in seqs]


def _hand_profile(residues, **trans):
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


def test_hand_computed_cases():
    assert [dr.entry_score(M) for M in (1, 2, 3)] == [0, -406, -662]
    # M = 1: A A; the first of the two equal cells
    assert dr.element("GCTGCT", _hand_profile("A")) == [1000, 0, 0, 0, 1, 1]
    # one insert: A W C against the nodes A C -- M1 -> I1 -> M2
    assert dr.element("GCTTGGTGT", _hand_profile("AC", MI_1=-100, IM_1=-50)) == [2000 - 406 - 150, 0, 0, 2, 1, 2]
    # one delete: A D against the nodes A C D -- M1 -> D2 -> M3
    assert dr.element("GCTGAT", _hand_profile("ACD", MD_1=-120, DM_2=-30)) == [2000 - 662 - 150, 0, 0, 1, 1, 3]
    # a `*` on the way into the insert: a finite, very expensive step -- the two single cells tie and the first wins
    assert dr.element("GCTTGGTGT", _hand_profile("AC", MI_1=dr.NEG, IM_1=-50)) == [1000 - 406, 0, 0, 0, 1, 1]
    # ... and when every other way is worse still, the path goes through it
    p = _hand_profile("AC", MI_1=dr.NEG, IM_1=-50)
    p["emis"][:, :20] -= 3 << 20
    p["emis"][0, dr.AA.index("A")] = p["emis"][1, dr.AA.index("C")] = 1000
    assert dr.element("GCTTGGTGT", p, engine=dr.frame_hit_plain)[0] == 1000 - 406
    # two equal copies: A C W A C against the nodes A C -- the smaller start wins
    assert dr.element("GCTTGTTGGGCTTGT", _hand_profile("AC", MM_1=-10)) == [2000 - 406 - 10, 0, 0, 1, 1, 2]
    # the same on the other strand: frame 3 reads the reverse complement from its first base
    assert dr.element(dr.revcomp("GCTTGTTGGGCTTGT"), _hand_profile("AC", MM_1=-10)) == [2000 - 406 - 10, 3, 0, 1, 1, 2]


def _mutated(rng, protein, sub, indel):
    out = [rng.choice(dr.AA) if rng.random() < sub else a for a in protein]
    at = rng.randrange(10, len(out) - 10)
    if indel == "ins":
        out.insert(at, rng.choice(dr.AA))
    elif indel == "del":
        del out[at]
    return "".join(out)


def test_planted_domains_are_found():
    """Rates: 10 % of the residues substituted and one residue inserted or deleted; the consensus residue has 0.8 in its
    node.  A node on its consensus scores log2(0.8 / q) >= 2.3 bits and a substituted one about -2.5 bits at the worst
    background, so 90 matches of 100 leave some 180 bits against an indel of about 7 + 1.3: nothing else comes near."""
    rng = random.Random(11)
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, M), name="d%d" % M) for M in (80, 110, 150)]
    cons = ["".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs]
    n = found = 0
    for q, (prof, c) in enumerate(zip(profs, cons)):
        for f in range(6):
            dna = dr.back_translate(rng, _mutated(rng, c, 0.10, ("ins", "del")[(q + f) % 2]))
            lead = 30 + f % 3
            fwd = dr.rand_dna(rng, lead) + dna + dr.rand_dna(rng, 45)
            seq = fwd if f < 3 else dr.revcomp(fwd)
            got = dr.search([seq], profs)[0]
            n += 1
            hit = got[q]
            assert hit[1] == f and hit[5] - hit[4] + 1 >= 0.9 * prof["M"], (q, f, hit.tolist())
            assert abs(hit[2] - 10) <= 0.1 * prof["M"]
            # the other profiles find nothing of the kind
            assert all(got[o][0] < hit[0] // 4 for o in range(3) if o != q)
            found += 1
    assert n == found == 18
