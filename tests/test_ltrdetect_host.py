"""The arithmetic of the LTR detection on the host: subphaser_amd/csrc/sp_ltrdetect.h against its twin
(tests/ltrdetect_ref.py), the twin against an O(n^2) restatement of the definitions, and the host side of the detector
(ltr.chain_hsps, candidates, similarity, write_scn) on hand-made lists and on the planted genome.

tests/ltrdetect_host_check.cpp is compiled against the header with the host C++ compiler (once more with
-fsanitize=address,undefined) and strings the header's functions together as the device does; everything is `==`."""
import io
import os
import random
import re

import numpy as np
import pytest

import host_check
import ltrdetect_cases as lc
import ltrdetect_ref as ld
from subphaser_amd import ltr


def _by_name():
    return {name: (seqs, par) for name, seqs, par in lc.hand_cases()}


# ------------------------------------------------------------------------------------------------ the twin itself
def _restated(seq, L, X, dmin, dmax, maxlen):
    """the definitions once more, as directly as they read: every pair of starts compared, strings not codes"""
    s = seq.upper()
    ok = lambda c: c in "ACGT"
    valid = [p for p in range(len(s) - L + 1) if all(ok(c) for c in s[p:p + L])]
    seeds = []
    for p in valid:
        later = [q for q in valid if q > p and s[q:q + L] == s[p:p + L]]
        kept = []
        for q in later[:ld.SCAN]:
            if q - p > dmax:
                break
            if q - p >= dmin:
                kept.append(q)
        for q in kept[:ld.FANOUT]:
            if p == 0 or not ok(s[p - 1]) or not ok(s[q - 1]) or s[p - 1] != s[q - 1]:
                seeds.append((p, q))
    out = set()
    for p, q in seeds:
        d = q - p
        cap = min(d, maxlen)
        e, sc, best, r = L, 0, 0, L
        while e < cap and q + e < len(s) and ok(s[p + e]) and ok(s[q + e]):
            sc += 2 if s[p + e] == s[q + e] else -2
            e += 1
            if sc > best:
                best, r = sc, e
            elif sc < best - X:
                break
        e, sc, best, l = 0, 0, 0, 0
        while p - e - 1 >= 0 and r + e < cap and ok(s[p - e - 1]) and ok(s[q - e - 1]):
            sc += 2 if s[p - e - 1] == s[q - e - 1] else -2
            e += 1
            if sc > best:
                best, l = sc, e
            elif sc < best - X:
                break
        out.add((p - l, r + l, d))
    return len(seeds), sorted(out)


def test_twin_is_the_definition():
    n = 0
    for name, seqs, par in lc.hand_cases():
        for s, got in zip(seqs, lc.twin(seqs, par)):
            if len(s) <= 1000:
                assert got == _restated(s, **par), name
                n += 1
    assert n >= 25
    rng = random.Random(5)
    for trial in range(12):      # two-letter strings: many words repeat, every cap is reached
        s = "".join(rng.choice("AC" if trial % 2 else "ACGTN") for _ in range(300))
        par = dict(L=12, X=rng.choice((0, 4, 20)), dmin=rng.choice((1, 13, 50)), dmax=rng.choice((60, 250)), maxlen=rng.choice((30, 100)))
        assert ld.hsps(s, **par) == _restated(s, **par), (trial, par)


def test_hand_cases_mean_what_they_say():
    c = _by_name()
    seeds = lambda name: [n for n, _ in lc.twin(*c[name])]
    hsps = lambda name: lc.twin(*c[name])[0][1]
    assert seeds("run_L") == [1] and hsps("run_L") == [(100, 12, 200)] and seeds("run_L-1") == [0]
    assert [seeds("d=%d" % d) for d in (49, 50, 300, 301)] == [[0], [1], [1], [0]]
    assert hsps("ends") == [(0, 40, 200)] and hsps("ends_inside") == [(1, 40, 200)]
    assert hsps("n_inside") == [(100, 40, 250), (141, 39, 250)]            # a seed on either side of the N
    assert hsps("n_at_p-1") == [(100, 30, 250)] and hsps("n_at_q-1") == [(100, 30, 250)]
    assert hsps("iupac") == [(100, 20, 250), (121, 29, 250), (151, 29, 250)]
    assert hsps("lower_case") == hsps("mixed_case") == [(100, 80, 250)]
    assert seeds("short_and_all_n") == [0, 0, 0, 1, 0]
    # the first of ten occurrences has nine partners and keeps eight; every occurrence is left-maximal
    assert seeds("fanout_9") == [sum(min(8, 9 - i) for i in range(10))] and seeds("fanout_8") == [sum(range(9))]
    assert seeds("tandem_unseen") == [0] and seeds("tandem_seen")[0] >= 1
    assert seeds("homopolymer") == [0] and seeds("homopolymer_near")[0] >= 1      # low complexity loses its seeds by the scan cap
    # ten mismatches cost exactly X: both extensions cross them; eleven cost X + 2: both stop
    assert hsps("xdrop_10") == [(100, 200, 400)]
    assert hsps("xdrop_11") == [(100, 100, 400), (211, 89, 400)]
    assert hsps("xdrop_10_x0") == [(100, 100, 400), (210, 90, 400)] and hsps("xdrop_11_x0") == [(100, 100, 400), (211, 89, 400)]
    assert (30, 150, 150) in hsps("cap_d") and max(n for _, n, _ in hsps("cap_d")) == 150
    assert hsps("cap_maxlen") == [(50, 100, 400)] and hsps("cap_maxlen_left") == [(50, 37, 400)]
    assert seeds("mod32") [0] >= 32 and seeds("chunk_edges") == [5] and seeds("chunk_edges_small")[0] >= 5


# ------------------------------------------------------------------------------------------------ the header
@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_header_is_the_twin(tmp_path, flags):
    cases = [(s, par) for _, seqs, par in lc.hand_cases() for s in seqs if len(s) <= 2000]
    flank = lc.flank_case()[0]
    cases += [(flank[:9000], lc.DEFAULT), (lc.planted()[0][0][:30000], lc.DEFAULT)]
    rng = random.Random(6)
    cases += [("".join(rng.choice("ACN" if t % 3 == 0 else "AC") for _ in range(400)), dict(L=12 + t, X=2 * t, dmin=1 + 7 * t, dmax=90 + 20 * t, maxlen=20 + 15 * t))
              for t in range(9)]
    digits = lambda s: "".join(map(str, ld.encode(s).tolist()))
    data, res = tmp_path / "cases.txt", tmp_path / "answers.txt"
    data.write_text("".join("%d %d %d %d %d %d\n%s\n" % (p["L"], p["X"], p["dmin"], p["dmax"], p["maxlen"], len(s), digits(s)) for s, p in cases))
    r = host_check.run(tmp_path, "ltrdetect_host_check", [data, res], flags=list(flags))
    assert host_check.ok_count(r) == len(cases)
    lines = res.read_text().split("\n")[:-1]
    at = n_seeds = 0
    for s, p in cases:
        n_valid, wsum, n_pairs, rows = ld.trace(s, **p)
        assert lines[at] == "C %d %d %d %d" % (n_valid, wsum, n_pairs, len(rows)), (s[:30], p)
        assert [tuple(map(int, x.split())) for x in lines[at + 1:at + 1 + len(rows)]] == rows, (s[:30], p)
        at += 1 + len(rows)
        n_seeds += len(rows)
    assert at == len(lines) and n_seeds > 100


def test_limits_are_the_headers():
    text = open(os.path.join(host_check.ROOT, "subphaser_amd", "csrc", "sp_ltrdetect.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (SP_LD_[A-Z_]+) \(?(-?\d+)\)?\s", text)}
    assert (const["SP_LD_LMIN"], const["SP_LD_LMAX"], const["SP_LD_SCAN"], const["SP_LD_FANOUT"]) == (ld.LMIN, ld.LMAX, ld.SCAN, ld.FANOUT) == (12, 20, 32, 8)
    assert (const["SP_LD_MAXDIST"], const["SP_LD_MAXLEN"], const["SP_LD_INVALID"]) == (ld.MAXDIST, ld.MAXLEN, ld.INVALID)
    assert (const["SP_LD_MATCH"], const["SP_LD_MISMATCH"], const["SP_LD_POS_BITS"]) == (ld.MATCH, ld.MISMATCH, 24)
    import ltralign_ref as lr
    assert ld.MAXLEN == lr.MAXLEN                                   # every candidate can be aligned
    assert ld.BODY + ld.MAXDIST + ld.LMAX <= 1 << 24
    d = ld.DEFAULTS
    assert (d["L"], d["X"], d["dmin"], d["dmax"], d["maxlen"]) == (ltr.LTR_SEED, ltr.LTR_XDROP, ltr.LTR_MINDIST, ltr.LTR_MAXDIST, ltr.LTR_MAXLEN)


def test_entries_are_declared_and_bound():
    from subphaser_amd import _native
    text = open(os.path.join(host_check.ROOT, "include", "subphaser_hip.h")).read()
    for name in ("sp_ltr_seeds", "sp_ltr_hsps", "sp_ltr_detect_set_chunk", "sp_ltr_detect_set_capacity"):
        assert re.search(r"\bint %s\(sp_ctx \*ctx" % name, text) and name in _native.SYMBOLS
    for name in ("ltr_seeds", "ltr_hsps", "ltr_detect_set_chunk", "ltr_detect_set_capacity"):
        assert callable(getattr(_native.Context, name))


# ------------------------------------------------------------------------------------------------ chaining
def test_chaining_on_hand_made_lists():
    ch = lambda hsps, **kw: ltr.chain_hsps(hsps, **kw)
    # one HSP, one chain: the hulls of its two copies
    assert ch([(100, 50, 2000)]) == [(100, 150, 2100, 2150)]
    # a second HSP behind the first on a diagonal 32 away joins, 33 away does not
    assert ch([(100, 50, 2000), (160, 40, 2032)]) == [(100, 200, 2100, 2232)]
    assert ch([(100, 50, 2000), (160, 40, 1968)]) == [(100, 200, 2100, 2168)]
    assert ch([(100, 50, 2000), (160, 40, 2033)]) == [(100, 150, 2100, 2150), (160, 200, 2193, 2233)]
    assert ch([(100, 50, 2000), (160, 40, 1967)]) == [(100, 150, 2100, 2150), (160, 200, 2127, 2167)]
    # the distance from the chain's end: 200 joins, 201 closes the chain
    assert ch([(100, 50, 2000), (350, 40, 2000)]) == [(100, 390, 2100, 2390)]
    assert ch([(100, 50, 2000), (351, 40, 2000)]) == [(100, 150, 2100, 2150), (351, 391, 2351, 2391)]
    # a closed chain stays closed: the third HSP is within reach of the first chain's diagonal but that chain is gone
    assert ch([(100, 50, 2000), (351, 10, 2500), (352, 40, 2000)], join=200) == [(100, 150, 2100, 2150), (351, 361, 2851, 2861), (352, 392, 2352, 2392)]
    # an HSP must end behind the chain's end, begin at or behind its last HSP on the left and on the right
    assert ch([(100, 50, 2000), (110, 40, 2000)]) == [(100, 150, 2100, 2150), (110, 150, 2110, 2150)]       # ends at the end
    assert ch([(100, 50, 2000), (100, 60, 1990)]) == [(100, 150, 2100, 2150), (100, 160, 2090, 2150)]       # its right copy begins before
    assert ch([(100, 50, 2000), (100, 60, 2000)]) == [(100, 160, 2100, 2160)]
    # two open chains qualify: the one with the larger end takes it; on equal ends the one opened first
    two = [(100, 50, 2000), (120, 40, 2100)]                                   # ends 150 and 160, diagonals 100 apart
    assert ch(two + [(170, 30, 2050)], indel=50) == [(100, 150, 2100, 2150), (120, 200, 2220, 2260)]
    tie = [(100, 60, 2000), (120, 40, 2100)]                                   # both end at 160
    assert ch(tie + [(170, 30, 2050)], indel=50) == [(100, 200, 2100, 2250), (120, 160, 2220, 2260)]
    # joining replaces the last diagonal: a drift of 30 a step is followed
    drift = [(100 + 60 * i, 50, 2000 + 30 * i) for i in range(5)]
    assert ch(drift) == [(100, 390, 2100, 2510)]
    assert ch([]) == []


def test_candidates_on_hand_made_chains():
    c = ltr.candidates
    ok = (1000, 1100, 2000, 2100)
    assert c([ok]) == [ok]
    assert c([(1000, 1099, 2000, 2100)]) == [] and c([(1000, 1100, 2000, 2099)]) == []            # an LTR below minlen
    assert c([(1000, 8000, 9000, 16000)]) == [(1000, 8000, 9000, 16000)] and c([(1000, 8001, 9000, 16000)]) == []
    assert c([(1000, 1100, 1999, 2100)]) == [] and c([(1000, 1100, 16000, 16100)]) == [(1000, 1100, 16000, 16100)]
    assert c([(1000, 1100, 16001, 16101)]) == []
    assert c([(0, 1200, 1100, 2300)]) == [] and c([(0, 1100, 1100, 2200)]) == [(0, 1100, 1100, 2200)]   # the copies may touch
    assert c([ok], minlen=101) == [] and c([ok], maxlen=99) == [] and c([ok], dmin=1001) == [] and c([ok], dmax=999) == []


def test_similarity_filter():
    counts = np.array([[0, 85, 10, 5, 3, 0], [0, 849, 100, 51, 0, 1], [0, 0, 0, 0, 9, 0], [0, 0, 0, 0, 0, ltr.FLAG_BAND],
                       [0, 0, 0, 0, 0, ltr.FLAG_LEN], [0, 100, 0, 0, 0, ltr.FLAG_EDGE]], np.int32)
    sims, keep, dropped = ltr.similarity(counts, 85)
    assert sims == [85.0, 84.9, None, None, None, 100.0] and keep == [0, 5] and dropped == 3


def test_flank_controlled_pairs_come_back_exactly():
    s, want = lc.flank_case()
    n_seeds, hsps = ld.hsps(s, **lc.DEFAULT)
    assert hsps == [(a0, a1 - a0, b0 - a0) for a0, a1, b0, b1 in want] and n_seeds == len(want)
    assert ltr.candidates(ltr.chain_hsps(hsps)) == want


def test_recall_on_the_planted_genome():
    """every planted element has a candidate that covers at least half of each of its LTRs (the prototype's worst case
    was 68 %).  The boundary errors are printed, not asserted: profiles/ltrdetect_notes.md records them."""
    seqs, truth = lc.planted()
    worst, errs, missed = 100.0, [], []
    for ci, (s, els) in enumerate(zip(seqs, truth)):
        n_seeds, hsps = lc.twin([s], lc.DEFAULT)[0]
        cands = ltr.candidates(ltr.chain_hsps(hsps))
        print("chromosome %d: %d seeds, %d HSPs, %d candidates" % (ci, n_seeds, len(hsps), len(cands)))
        for a0, a1, b0, b1 in els:
            cov = 0.0
            for c0, c1, d0, d1 in cands:
                left = max(0, min(a1, c1) - max(a0, c0)) / (a1 - a0)
                right = max(0, min(b1, d1) - max(b0, d0)) / (b1 - b0)
                if min(left, right) > cov:
                    cov, err = min(left, right), (c0 - a0, c1 - a1, d0 - b0, d1 - b1)
            if cov < 0.5:
                missed.append((ci, a0, a1, b0, b1, round(100 * cov, 1)))
            else:
                errs.append(max(map(abs, err)))
            worst = min(worst, 100 * cov)
    errs.sort()
    print("planted right LTRs drawn again for want of a shared word: %d" % lc.PLANTED_REDRAWN[0])
    print("worst coverage %.1f %%; boundary error: median %d, 90 %% %d, max %d" % (worst, errs[len(errs) // 2], errs[len(errs) * 9 // 10], errs[-1]))
    assert not missed, missed


# ------------------------------------------------------------------------------------------------ the .scn
def test_scn_round_trip(tmp_path):
    recs = [ltr.Record.from_coords("A1", 0, 99, 300, 1899, 2100, 95.5), ltr.Record.from_coords("A1", 0, 5000, 5120, 9000, 9131, 100 * 849 / 1000),
            ltr.Record.from_coords("chr|B", 3, 0, 100, 1000, 1100, 100.0)]
    assert recs[0].columns() == [100, 2100, 2001, 100, 300, 201, 1900, 2100, 201, "95.50", 0, "A1"]
    assert (recs[0].id, recs[1].similarity) == ("A1:100-2100:300-1900", 84.9)
    buf = io.StringIO()
    ltr.write_scn(buf, recs)
    path = tmp_path / "x.scn"
    path.write_text(buf.getvalue())
    lines = buf.getvalue().splitlines()
    assert lines[0].startswith("#") and "# s(ret) e(ret) l(ret) s(lLTR) e(lLTR) l(lLTR) s(rLTR) e(rLTR) l(rLTR) sim(LTRs) seq-nr chr" in lines
    assert lines[-1] == "1 1100 1100 1 100 100 1001 1100 100 100.00 3 chr|B #device"
    back = ltr.read_scn(str(path))
    assert [r.columns() for r in back] == [r.columns() for r in recs]
    assert [(r.start, r.end, r.element_len, r.lltr, r.rltr, r.similarity, r.seq_nr, r.seq_id) for r in back] == \
           [(r.start, r.end, r.element_len, r.lltr, r.rltr, r.similarity, r.seq_nr, r.seq_id) for r in recs]
    again = io.StringIO()
    ltr.write_scn(again, back)
    assert again.getvalue() == buf.getvalue()
