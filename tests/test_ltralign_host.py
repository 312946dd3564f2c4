"""The arithmetic of subphaser_amd/csrc/sp_ltralign.h on the host, and its twin against a full-matrix alignment.

tests/ltralign_host_check.cpp is compiled against the header with the host C++ compiler (once more with
-fsanitize=address,undefined) and compared with the twin (tests/ltralign_ref.py, written from the definition) with `==`
on all six outputs: hand cases, random pairs with substitutions, indels and invalid bases under bands from 0 to wider than
the sequences, and the limits.  The twin is held against the textbook full-matrix loop whenever the band covers the matrix."""
import random

import pytest

import host_check
import ltralign_ref as lr

X = "ACGGTCATGCAATCG"          # no period: one best alignment
# (a, b, w) -> (score, match, mismatch, gap, skip, flags)
HAND = [
    (("ACGTACGT", "ACGTACGT", 2), (16, 8, 0, 0, 0, 0)),                # identical
    (("ACGTACGT", "ACGTACGT", 0), (16, 8, 0, 0, 0, 0)),
    (("ACGTACGT", "ACGAACGT", 2), (12, 7, 1, 0, 0, 0)),                # one substitution
    (("ACGTACGT", "ACGTTACGT", 1), (13, 8, 0, 1, 0, 0)),               # one base more on the right
    (("ACGTTACGT", "ACGTACGT", 1), (13, 8, 0, 1, 0, 0)),               # ... on the left
    (("ACGNACGT", "ACGTACGT", 2), (14, 7, 0, 0, 1, 0)),                # an invalid base
    (("ACGTACGT", "ACGRACGT", 2), (14, 7, 0, 0, 1, 0)),
    (("acgtACGT", "ACGTacgt", 2), (16, 8, 0, 0, 0, 0)),                # lower case is valid
    (("A", "A", 0), (2, 1, 0, 0, 0, 0)),                               # length 1
    (("A", "C", 0), (-2, 0, 1, 0, 0, 0)),
    (("A", "C", 3), (-2, 0, 1, 0, 0, 0)),
    (("N", "N", 1), (0, 0, 0, 0, 1, 0)),
    (("ACGT", "ACGTA", 0), (5, 4, 0, 1, 0, 0)),                        # w = 0, la != lb: no edge without a margin
    (("ACGTA", "ACGT", 0), (5, 4, 0, 1, 0, 0)),
    (("T" + X, X + "T", 1), (24, 15, 0, 2, 0, lr.F_EDGE)),             # the best path runs along the lowest diagonal
    ((X + "T", "T" + X, 1), (24, 15, 0, 2, 0, lr.F_EDGE)),             # ... the highest
    (("T" + X, X + "T", 2), (24, 15, 0, 2, 0, 0)),                     # a wider band: the same path, not on its edge
    (("A", "A" * 1024, 0), (2 - 3 * 1023, 1, 0, 1023, 0, 0)),          # band of exactly MAXBAND diagonals
    (("A", "A" * 1025, 0), (0, 0, 0, 0, 0, lr.F_BAND)),                # one more
    (("A" * 1025, "A", 0), (0, 0, 0, 0, 0, lr.F_BAND)),
    (("ACGT", "ACGT", 512), (0, 0, 0, 0, 0, lr.F_BAND)),               # 2 w + 1 = 1025
    (("ACGT", "ACGA", 511), (4, 3, 1, 0, 0, 0)),
    (("A" * (lr.MAXLEN + 1), "A" * 10, 0), (0, 0, 0, 0, 0, lr.F_LEN)),  # over MAXLEN (and over MAXBAND: the length goes first)
    (("A" * 10, "A" * (lr.MAXLEN + 1), 64), (0, 0, 0, 0, 0, lr.F_LEN)),
]


def mutate(rng, seq, subs, indels, n_run=0):
    s = list(seq)
    for _ in range(subs):
        p = rng.randrange(len(s))
        s[p] = rng.choice("ACGT")
    for _ in range(indels):
        p = rng.randrange(len(s))
        if rng.random() < 0.5 and len(s) > 4:
            del s[p:p + rng.randrange(1, 4)]
        else:
            s[p:p] = [rng.choice("ACGT") for _ in range(rng.randrange(1, 4))]
    if n_run:
        p = rng.randrange(len(s))
        s[p:p + n_run] = "N" * len(s[p:p + n_run])
    return "".join(s) or "A"


def random_pairs(seed=11):
    rng = random.Random(seed)
    pairs = []
    for n in (1, 2, 3, 7, 31, 64, 65, 130):
        for w in (0, 1, 2, 5, 200):
            a = "".join(rng.choice("ACGT") for _ in range(n))
            pairs.append((a, mutate(rng, a, n // 8, rng.randrange(3), rng.randrange(3)), w))
            pairs.append((mutate(rng, a, n // 5, 2, 1), a, w))
            pairs.append((a, "".join(rng.choice("ACGTN") for _ in range(rng.randrange(1, n + 9))), w))      # unrelated
    for alphabet in ("A", "AC"):      # many equal scores: the tie order decides the counts
        for w in (0, 1, 3, 40):
            pairs.append(("".join(rng.choice(alphabet) for _ in range(23)), "".join(rng.choice(alphabet) for _ in range(29)), w))
    return pairs


def test_hand_cases():
    for (a, b, w), want in HAND:
        assert lr.align(lr.encode(a), lr.encode(b), w) == want, (a[:20], b[:20], w)
        if len(a) * len(b) < 5000:
            assert lr.align_rows(lr.encode(a), lr.encode(b), w) == want, (a[:20], b[:20], w)


def test_both_walks_of_the_twin_agree():
    for a, b, w in random_pairs(seed=13):
        assert lr.align(lr.encode(a), lr.encode(b), w) == lr.align_rows(lr.encode(a), lr.encode(b), w), (a, b, w)


def test_twin_is_the_full_matrix_when_the_band_covers_it():
    n = 0
    for a, b, w in random_pairs():
        if w < max(len(a), len(b)):
            continue
        ca, cb = lr.encode(a), lr.encode(b)
        got = lr.align(ca, cb, w)
        assert got[:5] == lr.full_dp(ca, cb), (a, b, w)
        assert got[5] in (0, lr.F_EDGE)
        n += 1
    assert n >= 20


def test_band_only_costs_score():
    """a narrower band searches fewer paths: the score never rises; every path spends the bases of both sequences"""
    for a, b, w in random_pairs(seed=12):
        ca, cb = lr.encode(a), lr.encode(b)
        got, full = lr.align(ca, cb, w), lr.full_dp(ca, cb)
        assert got[0] <= full[0]
        assert got[0] == lr.MATCH * got[1] + lr.MISMATCH * got[2] + lr.GAP * got[3]
        assert 2 * (got[1] + got[2] + got[4]) + got[3] == len(a) + len(b)
        if w == 0:
            assert got[5] == 0 and got[3] >= abs(len(a) - len(b)) and (got[3] - abs(len(a) - len(b))) % 2 == 0


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_header_is_the_twin(tmp_path, flags):
    rng = random.Random(3)
    long_a = "".join(rng.choice("ACGT") for _ in range(700))
    pairs = [p for p, _ in HAND] + random_pairs() + random_pairs(seed=12) + [(long_a, mutate(rng, long_a, 60, 6, 9), 64),
                                                                              (long_a, mutate(rng, long_a, 20, 30, 0), 8)]
    want = [lr.align(lr.encode(a), lr.encode(b), w) for a, b, w in pairs]
    for (_, exp), got in zip(HAND, want):
        assert got == exp
    digits = lambda s: "".join(map(str, lr.encode(s).tolist()))
    data, res = tmp_path / "pairs.txt", tmp_path / "answers.txt"
    data.write_text("".join("%d %d %d %s %s\n" % (w, len(a), len(b), digits(a), digits(b)) for a, b, w in pairs))
    r = host_check.run(tmp_path, "ltralign_host_check", [data, res], flags=list(flags))
    assert host_check.ok_count(r) == len(pairs)
    got = [tuple(map(int, line.split())) for line in res.read_text().split("\n")[:-1]]
    assert got == want
    assert any(g[5] & lr.F_EDGE for g in got) and any(g[3] for g in got) and any(g[4] for g in got)


def test_limits_are_the_headers():
    import os
    import re
    text = open(os.path.join(host_check.ROOT, "subphaser_amd", "csrc", "sp_ltralign.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (SP_LA_[A-Z_]+) \(?(-?\d+)\)?\s", text)}
    assert (const["SP_LA_MAXLEN"], const["SP_LA_MAXBAND"], const["SP_LA_INVALID"]) == (lr.MAXLEN, lr.MAXBAND, lr.INVALID)
    assert (const["SP_LA_MATCH"], const["SP_LA_MISMATCH"], const["SP_LA_GAP"]) == (lr.MATCH, lr.MISMATCH, lr.GAP)
    assert (const["SP_LA_F_EDGE"], const["SP_LA_F_BAND"], const["SP_LA_F_LEN"]) == (lr.F_EDGE, lr.F_BAND, lr.F_LEN)
    from subphaser_amd import _native
    assert (_native.LTR_ALIGN_MAXLEN, _native.LTR_ALIGN_MAXBAND) == (lr.MAXLEN, lr.MAXBAND)
    assert (_native.LTR_ALIGN_EDGE, _native.LTR_ALIGN_BAND, _native.LTR_ALIGN_LEN) == (lr.F_EDGE, lr.F_BAND, lr.F_LEN)
