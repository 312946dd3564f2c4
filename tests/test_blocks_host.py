"""The arithmetic of subphaser_amd/csrc/sp_blocks.h on the host, the twin against brute force, and the block walk.

tests/blocks_host_check.cpp is compiled against the header with the host C++ compiler and compared with the twin
(tests/blocks_ref.py, written from the definition) with `==`: the splitmix64 finaliser on fixed and random keys (0 and
2^62 - 1 among them), the sampling decision for every s, the parameter check, the window count, and the vote's tie rules
on hand-made cell lists.  The same program is built and run once more with -fsanitize=address,undefined.

The twin is held against brute force on sequences of a few hundred bases: anchors from Python string slicing and str
reverse complement, independent of the 2-bit key code.  The block walk of subphaser_amd/blocks.py is compared with the
twin's loop on hand-made vote arrays and on random ones."""
import os
import random

import numpy as np
import pytest

import blocks_cases as bc
import blocks_ref as br
import host_check
from subphaser_amd import blocks as bl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYS = [0, 1, 2, (1 << 62) - 1, (1 << 62) - 2, (1 << 34) - 1, 0x123456789abcdef, 0xbf58476d1ce4e5b9 & ((1 << 62) - 1)]
# hand-made windows: {(wb, opp): count} -> the call
VOTES = [
    ({}, (-1, 0, 0, 0)),                                              # an empty window
    ({(7, 0): 1}, (7, 0, 1, 1)),                                      # a single anchor
    ({(7, 1): 1}, (7, 1, 1, 1)),
    ({(5, 1): 4, (9, 0): 4}, (9, 0, 4, 8)),                           # equal counts across opp: opp = 0 first
    ({(5, 1): 4, (5, 0): 4}, (5, 0, 4, 8)),
    ({(9, 0): 4, (5, 0): 4, (7, 0): 4}, (5, 0, 4, 12)),               # equal counts across wb: the smaller wb
    ({(9, 1): 4, (5, 1): 4}, (5, 1, 4, 8)),
    ({(3, 1): 4, (9, 0): 4, (8, 0): 4, (2, 1): 4}, (8, 0, 4, 16)),    # both rules
    ({(3, 1): 5, (9, 0): 4, (8, 0): 4}, (3, 1, 5, 13)),               # the count goes first
    ({(0, 0): 1, (0, 1): 2}, (0, 1, 2, 3)),
    ({(2147483646, 1): 3, (2147483646, 0): 3, (0, 1): 2}, (2147483646, 0, 3, 8)),      # the largest window number
    ({(1, 0): 2147483647}, (1, 0, 2147483647, 2147483647)),
]


def _commands():
    rng = random.Random(5)
    keys = KEYS + [rng.getrandbits(62) for _ in range(500)]
    cmds, want = [], []
    for k in keys:
        cmds.append("M %d" % k)
        want.append(str(br.mix(k)))
    for k in keys[:60]:
        for s in range(0, 17):
            cmds.append("S %d %d" % (k, s))
            want.append(str(int(br.sampled(k, s))))
    for kb in range(14, 35):
        for s in (-1, 0, 4, 16, 17):
            for b in (0, 1, 10000):
                cmds.append("C %d %d %d" % (kb, s, b))
                try:
                    br.check_params(kb, s, b)
                    want.append("0")
                except ValueError as e:
                    want.append(str(["kb", "s", "bin"].index(str(e)) + 1))
    for n, b in ((0, 1), (1, 1), (999, 1000), (1000, 1000), (1001, 1000), (2 ** 31 - 17, 1), (2 ** 31 - 17, 7)):
        cmds.append("W %d %d" % (n, b))
        want.append(str(-(-n // b)))
    for k in keys[:100]:
        for cap in (64, 65, 1000003, 2 ** 32 - 1):
            cmds.append("H %d %d" % (br.mix(k), cap))
            want.append(str(((br.mix(k) >> 32) * cap) >> 32))
    for cells, call in VOTES:
        assert br.vote_cells(cells) == call
    random_cells = []
    for _ in range(300):
        d = {(rng.randrange(6), rng.randrange(2)): rng.randrange(1, 4) for _ in range(rng.randrange(0, 8))}
        random_cells.append(d)
    for d in [c for c, _ in VOTES] + random_cells:
        items = list(d.items())
        rng.shuffle(items)
        cmds.append("V %d %s" % (len(items), " ".join("%d %d %d" % (wb, o, n) for (wb, o), n in items)))
        want.append("%d %d %d %d" % br.vote_cells(d))
    return cmds, want


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_header_is_the_twin(tmp_path, flags):
    cmds, want = _commands()
    data, res = tmp_path / "commands.txt", tmp_path / "answers.txt"
    data.write_text("\n".join(cmds) + "\n")
    r = host_check.run(tmp_path, "blocks_host_check", [data, res], flags=list(flags))
    assert host_check.ok_count(r) == len(cmds)
    got = res.read_text().split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(c, g, w) for c, g, w in zip(cmds, got, want) if g != w]
    assert not bad, bad[:5]


def test_mix_known_values():
    # the finaliser of splitmix64 is a bijection with mix(0) = 0; one value worked by hand from the three steps
    assert br.mix(0) == 0
    z = 1
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 % 2 ** 64
    z ^= z >> 27
    z = z * 0x94d049bb133111eb % 2 ** 64
    z ^= z >> 31
    assert br.mix(1) == z
    assert len({br.mix(k) for k in range(10000)}) == 10000
    assert all(br.sampled(k, 0) for k in KEYS)
    n = sum(br.sampled(k, 4) for k in range(1 << 16))
    assert 3600 < n < 4600          # 4096 expected, sd 62


# ---------------------------------------------------------------------------------------------- twin against brute force
def _small_inputs():
    rng = np.random.RandomState(3)
    base = bc.rand_seq(rng, 420)
    out = {}
    # lower case, IUPAC and N runs
    a = base[:100].lower() + base[100:200] + "NNNNNNN" + base[207:300] + "R" + base[301:]
    b = bc.mutate(rng, base, 0.02)
    b = b[:50] + "nnn" + b[53:240] + "Y" + b[241:]
    out["case-and-N"] = (a, b)
    # a k-mer present twice in A: forward and as its reverse complement
    w = base[40:80]
    out["twice-in-A-fw-rc"] = (base[:200] + bc.revcomp(w) + base[200:], base)
    # once in A, twice in B
    out["once-A-twice-B"] = (base, base[:300] + w + base[300:])
    out["rc-whole"] = (base, bc.revcomp(base))
    out["shorter-than-kb"] = (base[:16], base)
    out["both-short"] = ("ACGT", "ACG")
    out["empty"] = ("", base)
    return out


@pytest.mark.parametrize("name", sorted(_small_inputs()))
@pytest.mark.parametrize("kb", [17, 31])
@pytest.mark.parametrize("s", [0, 2])
def test_twin_against_brute_force(name, kb, s):
    a, b = _small_inputs()[name]
    for x, y in ((a, b), (b, a)):
        ia, ta = br.index(x, kb, s)
        ib, _ = br.index(y, kb, s)
        got = br.anchors(ia, ib)
        assert got == br.brute_anchors(x, y, kb, s)
        assert ta[1] == len(ia) and ta[0] >= ta[1]
        assert [p for p, _, _ in got] == sorted({p for p, _, _ in got})       # ascending and unique posA
    if name == "twice-in-A-fw-rc" and s == 0:
        # the k-mers of the repeated word are in neither index; the k-mers around it still anchor
        ia, _ = br.index(a, kb, 0)
        pos = {p for p, _ in ia.values()}
        assert not any(40 <= p <= 80 - kb for p in pos) and not any(200 <= p <= 240 - kb for p in pos)
        assert len(br.anchors(ia, br.index(b, kb, 0)[0])) > 100
    if name == "once-A-twice-B" and s == 0:
        anch = br.anchors(br.index(a, kb, 0)[0], br.index(b, kb, 0)[0])
        assert not any(40 <= pa <= 80 - kb for pa, _, _ in anch) and len(anch) > 100
    if name == "rc-whole" and s == 0:
        anch = br.anchors(br.index(a, kb, 0)[0], br.index(b, kb, 0)[0])
        assert len(anch) == len(a) - kb + 1 and all(o == 1 and pa + pb == len(a) - kb for pa, pb, o in anch)
    if name in ("shorter-than-kb", "both-short", "empty"):
        assert br.pair(a, b, kb, s, 10)[0] == []


def test_vote_arrays_of_the_twin():
    a, b = bc.edges()
    anch, win_b, opp, votes, total = br.pair(a, b, 21, 0, 64)
    assert len(win_b) == -(-len(a) // 64) and total.sum() == len(anch)
    assert ((win_b == -1) == (total == 0)).all() and (votes <= total).all() and (votes[total > 0] > 0).all()
    # windows 31 and 32 (bases 1984..2111) hold the N run 2040..2055: no start within 20 bases before it is valid
    assert total[31] <= 2040 - 20 - 1984 and total[32] <= 2112 - 2056


# ---------------------------------------------------------------------------------------------- the walk
def _walk_both(win_b, opp, votes, len_a, len_b, bin_size, min_votes, max_gap, min_block):
    got = bl.walk(np.array(win_b, np.int32), np.array(opp, np.uint8), np.array(votes, np.int32), len_a, len_b, bin_size,
                  min_votes, max_gap, min_block)
    assert got == br.blocks(win_b, opp, votes, len_a, len_b, bin_size, min_votes, max_gap, min_block)
    return got


def _arrays(n, calls):
    """calls: {wa: (wb, opp, votes)}"""
    win_b, opp, votes = [-1] * n, [0] * n, [0] * n
    for wa, (wb, o, v) in calls.items():
        win_b[wa], opp[wa], votes[wa] = wb, o, v
    return win_b, opp, votes


def test_walk_gap_of_max_gap_and_one_more():
    # max_gap = 2: windows 0, 1 and 4 chain (two windows skipped), 0, 1 and 5 do not
    arr = _arrays(10, {0: (0, 0, 5), 1: (1, 0, 5), 4: (4, 0, 5)})
    assert _walk_both(*arr, 1000, 1000, 100, 3, 2, 0) == [(0, 500, 0, 500, "+", 3, 15)]
    arr = _arrays(10, {0: (0, 0, 5), 1: (1, 0, 5), 5: (5, 0, 5)})
    assert _walk_both(*arr, 1000, 1000, 100, 3, 2, 0) == [(0, 200, 0, 200, "+", 2, 10), (500, 600, 500, 600, "+", 1, 5)]


def test_walk_diagonal_drift_on_both_sides_of_the_bound():
    # dA = 1; dB = 3 (|dB - dA| = 2 = max_gap) joins, dB = 4 does not; dB = -1 (|..| = 2) joins, dB = -2 does not
    for wb, joined in ((13, True), (14, False), (9, True), (8, False)):
        arr = _arrays(4, {0: (10, 0, 3), 1: (wb, 0, 3)})
        assert (len(_walk_both(*arr, 400, 4000, 100, 3, 2, 0)) == 1) == joined, wb


def test_walk_strand_change_and_votes_threshold():
    arr = _arrays(6, {0: (0, 0, 3), 1: (1, 0, 3), 2: (2, 1, 3), 3: (1, 1, 3), 4: (4, 0, 2), 5: (5, 0, 3)})
    assert _walk_both(*arr, 600, 600, 100, 3, 5, 0) == [(0, 200, 0, 200, "+", 2, 6), (200, 400, 100, 300, "-", 2, 6),
                                                         (500, 600, 500, 600, "+", 1, 3)]


def test_walk_min_block_exactly_and_one_window_less():
    arr = _arrays(8, {i: (i, 0, 4) for i in range(5)})
    assert _walk_both(*arr, 800, 800, 100, 3, 5, 500) == [(0, 500, 0, 500, "+", 5, 20)]
    arr = _arrays(8, {i: (i, 0, 4) for i in range(4)})
    assert _walk_both(*arr, 800, 800, 100, 3, 5, 500) == []


def test_walk_last_window_clipped_to_the_length():
    arr = _arrays(5, {3: (7, 0, 4), 4: (8, 0, 4)})
    assert _walk_both(*arr, 437, 871, 100, 3, 5, 0) == [(300, 437, 700, 871, "+", 2, 8)]
    assert _walk_both(*arr, 437, 871, 100, 3, 5, 137) == [(300, 437, 700, 871, "+", 2, 8)]
    assert _walk_both(*arr, 437, 871, 100, 3, 5, 138) == []


def test_walk_opposite_strand_descends():
    arr = _arrays(6, {1: (9, 1, 3), 2: (8, 1, 3), 3: (7, 1, 3), 5: (5, 1, 3)})
    assert _walk_both(*arr, 600, 1000, 100, 3, 5, 0) == [(100, 600, 500, 1000, "-", 4, 12)]
    # ascending wb on the opposite strand is a drift of 2 per window: |(-1) - 1| = 2
    arr = _arrays(6, {1: (7, 1, 3), 2: (8, 1, 3)})
    assert len(_walk_both(*arr, 600, 1000, 100, 3, 1, 0)) == 2 and len(_walk_both(*arr, 600, 1000, 100, 3, 2, 0)) == 1


def test_walk_random_arrays():
    rng = np.random.RandomState(12)
    for _ in range(200):
        n = int(rng.randint(0, 60))
        win_b = rng.randint(-1, 12, n)
        votes = np.where(win_b < 0, 0, rng.randint(1, 6, n))
        opp = np.where(win_b < 0, 0, rng.randint(0, 2, n))
        _walk_both(win_b.tolist(), opp.tolist(), votes.tolist(), n * 50 - int(rng.randint(0, 50)) if n else 0, 600, 50,
                   int(rng.randint(1, 5)), int(rng.randint(0, 4)), int(rng.randint(0, 300)))
    assert bl.walk([], [], [], 0, 0, 10) == []


def test_planted_case_meets_its_claims_on_the_twin():
    """the seed of the GPU test's planted case is chosen so that the twin alone shows the structure"""
    a, b = bc.planted()
    _, win_b, opp, votes, _ = br.pair(a, b, 21, 2, 1000)
    bc.check_planted(br.blocks(win_b, opp, votes, len(a), len(b), 1000, 3, 2, 3000), 1000)


def test_library_exports_the_entries():
    from subphaser_amd import _native
    lib = _native.load()
    for name in ("sp_blocks_index", "sp_blocks_pair", "sp_blocks_anchors", "sp_blocks_release", "sp_blocks_set_cells"):
        assert hasattr(lib, name) and name in _native.SYMBOLS
    header = open(os.path.join(ROOT, "subphaser_amd", "csrc", "sp_blocks.h")).read()
    assert "#define SP_BK_KMIN 17" in header and "#define SP_BK_KMAX 31" in header and "#define SP_BK_SMAX 16" in header
    assert _native.BLOCKS_K_RANGE == (17, 31) and _native.BLOCKS_MAX_SAMPLE == 16
    assert (bl.BLOCK_K, bl.BLOCK_SAMPLE, bl.BLOCK_BIN, bl.BLOCK_VOTES, bl.BLOCK_GAP, bl.MIN_BLOCK) == (21, 4, 50000, 5, 5, 100000)
