"""CPU: the ungapped prefilter of the domain search (subphaser_amd/csrc/sp_domains.h: sp_dm_ssv_cell, sp_dm_host_ssv_frame)
and its twins (tests/domssv_ref.py).

tests/domssv_host_check.cpp is compiled against the header with the host C++ compiler; its driver is compared with the
twin with `==`: M in 1, 2, 3, 64, 65 x frames of 0, 1, 2, 5, 70 residues over tables that take the whole legal range
(`*` transitions, emissions at -2^20 and 2^15, entry at 0 and at -2^20, stop and X columns), the frame of 21845 residues
against 2048 nodes at 2^15 an emission, and the six frames of every case of tests/domains_cases.py.  The twin is compared
with the maximum over all ungapped segments summed directly, the bound ssv <= the hit's score is checked on every (case,
profile, frame), with equality where no gap can pay, and the filtered twin is checked at its seams."""
import random
import struct

import numpy as np
import pytest

import domains_cases as dc
import domains_ref as dr
import domssv_ref as sr
import host_check

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _tables(prof):
    return prof["emis"].astype("<i4").tobytes() + prof["trans"].astype("<i4").tobytes() + struct.pack("<i", prof["entry"])


def _run(tmp, records, width):
    data, res = tmp / "in.bin", tmp / "out.bin"
    data.write_bytes(b"".join(records) + struct.pack("<q", 0))
    r = host_check.run(tmp, "domssv_host_check", [data, res])
    assert host_check.ok_count(r) == len(records)
    return np.frombuffer(res.read_bytes(), "<i4").reshape(len(records), width)


def _frame_record(res, prof):
    return struct.pack("<qqq", 1, len(res), prof["M"]) + bytes(res) + _tables(prof)


def _wild_profile(rng, M, entry):
    """tables over the whole legal range: a quarter of the transitions `*`, emissions at both ends of theirs"""
    emis = np.array([[rng.choice([dr.NEG, 1 << 15, rng.randint(-3000, 3000), rng.randint(dr.NEG, 1 << 15)]) for _ in range(22)] for _ in range(M)], np.int64)
    trans = np.array([[dr.NEG if rng.random() < 0.25 else -rng.randint(0, 4000) for _ in range(7)] for _ in range(M)], np.int64)
    return dr.make_profile(M, emis, trans, entry=entry)


def test_header_is_the_twin_on_frames(tmp_path):
    rng = random.Random(31)
    jobs = []
    for M in (1, 2, 3, 64, 65):
        for n in (0, 1, 2, 5, 70):
            for entry in (0, dr.NEG, dr.entry_score(M)):
                jobs.append(([rng.randrange(22) for _ in range(n)], _wild_profile(rng, M, entry)))
            jobs.append(([rng.choice([dr.X, dr.STOP, 3]) for _ in range(n)], dr.random_profile(rng, M)))      # stop and X columns of read_hmm's kind
    # the top of the range proof: every residue the best one, 2^15 an emission
    top = dr.make_profile(2048, np.full((2048, 22), 1 << 15), np.zeros((2048, 7)), entry=0)
    jobs.append(([7] * 21845, top))
    # ... and its bottom: one cell, entry and emission at -2^20
    jobs.append(([4], dr.make_profile(1, np.full((1, 22), dr.NEG), np.full((1, 7), dr.NEG), entry=dr.NEG)))
    got = _run(tmp_path, [_frame_record(r, p) for r, p in jobs], 1)[:, 0]
    want = [sr.ssv_frame(r, p) for r, p in jobs]
    assert got.tolist() == want
    assert want[-2] == 2048 << 15 and want[-1] == 2 * dr.NEG      # the longest diagonal has 2048 cells
    assert sum(w == dr.INT32_MIN for w in want) == 5 * 4 and max(want[:-2]) >= 1 << 15


def test_header_is_the_twin_on_the_cases(tmp_path):
    P = dc.profiles()
    pairs = [(seq, P[p]) for _, seq, profs in dc.cases() for p in profs]
    recs = [struct.pack("<qqq", 2, len(s), p["M"]) + bytes(CODE.get(c, 4) for c in s.upper()) + _tables(p) for s, p in pairs]
    got = _run(tmp_path, recs, 6)
    want = np.array([[sr.ssv_frame(dr.translate(s, f), p) for f in range(6)] for s, p in pairs], np.int64)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert (want == dr.INT32_MIN).any() and (want > 0).any()


@pytest.mark.parametrize("seed", range(4))
def test_twins_are_the_best_ungapped_segment(seed):
    rng = random.Random(100 + seed)
    for _ in range(40):
        M, n = rng.randint(1, 6), rng.randint(0, 6)
        prof = dr.random_profile(rng, M, star=rng.choice([0.0, 0.3])) if rng.random() < 0.6 else _wild_profile(rng, M, rng.choice([0, dr.NEG, -700]))
        res = [rng.randrange(22) for _ in range(n)]
        want = sr.ssv_brute(res, prof)
        assert sr.ssv_frame_plain(res, prof) == want and sr.ssv_frame(res, prof) == want, (M, res)
    # larger, the two twins against each other
    for M, n in ((64, 70), (65, 5), (130, 131)):
        prof = dr.random_profile(rng, M, star=0.1)
        res = [rng.randrange(22) for _ in range(n)]
        assert sr.ssv_frame_plain(res, prof) == sr.ssv_frame(res, prof)
    # the frames side by side, a node at a time
    prof = dr.random_profile(rng, 9, star=0.2)
    frames = [[rng.randrange(22) for _ in range(n)] for n in (0, 1, 40, 7, 0, 9, 10, 3)]
    for cells in (1 << 22, 50, 1):
        assert sr.ssv_frames(frames, prof, cells) == [sr.ssv_frame_plain(f, prof) for f in frames]


@pytest.fixture(scope="module")
def case_hits():
    """[(case, profile name, hits of the six frames, ssv of the six frames)] over domains_cases"""
    P = dc.profiles()
    out = []
    for name, seq, profs in dc.cases():
        frames = [dr.translate(seq, f) for f in range(6)]
        for p in profs:
            hits = dr.frames_hits([(fr, P[p]) for fr in frames])
            out.append((name, p, hits, [sr.ssv_frame(fr, P[p]) for fr in frames]))
    return out


def test_ssv_never_exceeds_the_hit(case_hits):
    n = below = 0
    for name, p, hits, scores in case_hits:
        for h, s in zip(hits, scores):
            assert (h is None) == (s == dr.INT32_MIN), (name, p)
            if h is not None:
                assert s <= h[0], (name, p, s, h)
                n += 1
                below += s < h[0]
    assert n > 100 and below > 10 and below < n      # gaps pay in some frames (delete70, insert70, ...) and not in others


def test_ssv_is_the_hit_where_no_gap_can_pay():
    """all gap transitions at `*` (-2^20) and emissions within +-2^10: a path with a gap loses 2^20 and can gain at most
    2^10 a residue over fewer than 2^10 residues, so the Viterbi path is ungapped and its score IS the ssv"""
    rng = random.Random(9)
    for M in (1, 2, 7, 40, 65):
        emis = np.array([[rng.randint(-1024, 1024) for _ in range(22)] for _ in range(M)], np.int64)
        trans = np.full((M, 7), dr.NEG, np.int64)
        trans[:, dr.MM] = [-rng.randint(0, 600) for _ in range(M)]
        prof = dr.make_profile(M, emis, trans)
        for n in (0, 3, 17, 90, 200):
            seq = dr.rand_dna(rng, n)
            for f in range(6):
                res = dr.translate(seq, f)
                h = dr.frame_hit(res, prof)
                assert sr.ssv_frame(res, prof) == (dr.INT32_MIN if h is None else h[0]), (M, n, f)


def test_the_device_cases_do_what_their_names_say():
    import domssv_cases as sc
    sc.check_names()


def test_filtered_twin_at_its_seams(case_hits):
    P = dc.profiles()
    cases = [c for c in dc.cases() if c[0] in ("len2", "len5", "len32", "sizes", "planted", "planted_rc", "frame_tie", "stop")]
    seqs, plist = [c[1] for c in cases], [P["c60"], P["m5"], P["m65"], P["m64"], P["star65"]]
    memo, smemo = {}, {}
    plain = dr.search(seqs, plist)
    scores = sr.ssv(seqs, plist, smemo)
    with_res = int((scores != dr.INT32_MIN).sum())
    got, items, passed = sr.search(seqs, plist, dr.INT32_MIN, memo, smemo)
    assert (got == plain).all() and items == passed == with_res and 0 < with_res < scores.size
    got, items, passed = sr.search(seqs, plist, int(scores.max()) + 1, memo, smemo)
    assert (got[:, :, 0] == dr.INT32_MIN).all() and not got[:, :, 1:].any() and (items, passed) == (with_res, 0)
    # one item: the winning frame of an (element, profile) where another frame has the higher ssv.  At its own score it
    # stays; one above it goes, and the element's best frame moves to another
    a, b, f = pick_item(plain, scores)
    T = int(scores[a, b, f])
    keep, _, n_keep = sr.search(seqs, plist, T, memo, smemo)
    drop, _, n_drop = sr.search(seqs, plist, T + 1, memo, smemo)
    assert (keep[a, b] == plain[a, b]).all() and n_keep == int((scores >= T).sum()) > 0
    assert drop[a, b, 1] != f and drop[a, b, 0] <= plain[a, b, 0] and n_drop == int((scores >= T + 1).sum()) < n_keep
    assert drop[a, b, 0] > dr.INT32_MIN
    # the planted domain: above its ssv nothing of the element is left for the profile
    a = [c[0] for c in cases].index("planted")
    T = int(scores[a, 0, plain[a, 0, 1]])
    assert T == scores[a, 0].max() and sr.search(seqs, plist, T + 1, memo, smemo)[0][a, 0].tolist() == [dr.INT32_MIN, 0, 0, 0, 0, 0]


def pick_item(plain, scores):
    """(element, profile, frame): the frame of the search's hit, where another frame of the pair has a higher ssv"""
    for a in range(plain.shape[0]):
        for b in range(plain.shape[1]):
            f = int(plain[a, b, 1])
            if plain[a, b, 0] != dr.INT32_MIN and scores[a, b, f] < scores[a, b].max():
                return a, b, f
    raise AssertionError("no (element, profile) whose winning frame has not the highest ssv")
