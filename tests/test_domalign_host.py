"""CPU: the arithmetic of the profile alignment (subphaser_amd/csrc/sp_domalign.h) and its twin (tests/domalign_ref.py).

tests/domalign_host_check.cpp is compiled against the header with the host C++ compiler; its driver -- a full plane, filled
row by row, node by node, then traced -- is compared with the twin with `==` on hit, col and the residues over
tests/domalign_cases.py and random items, and the eight-bytes-a-step pair comparison (sp_swar.h) with numpy.  The twin
itself is checked against independent facts: its path starts and ends where the hit says, the path's entry, emissions and
transitions re-added from the tables give the score, tiny cases equal the maximum over ALL enumerated local paths, a
whole-frame window gives domains_ref's hit, a flat profile takes the first argument of every tie, and hand cases with one
planted insertion and one planted deletion have the columns worked out by hand."""
import random
import struct

import numpy as np
import pytest

import domalign_cases as dac
import domalign_ref as da
import domains_ref as dr
import host_check

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _item_record(seq, f, i0, i1, prof):
    codes = bytes(CODE.get(c, 4) for c in seq.upper())
    return (struct.pack("<qqqqqq", 1, len(seq), f, i0, i1, prof["M"]) + codes + prof["emis"].astype("<i4").tobytes()
            + prof["trans"].astype("<i4").tobytes() + struct.pack("<i", prof["entry"]))


def _header_items(tmp, seqs, profs, items):
    data, res = tmp / "in.bin", tmp / "out.bin"
    data.write_bytes(b"".join(_item_record(seqs[s], f, i0, i1, profs[p]) for s, f, i0, i1, p in items) + struct.pack("<q", 0))
    r = host_check.run(tmp, "domalign_host_check", [data, res])
    assert host_check.ok_count(r) == len(items)
    raw, out, at = res.read_bytes(), [], 0
    for s, f, i0, i1, p in items:
        M, n = profs[p]["M"], i1 - i0 + 1
        hit = np.frombuffer(raw, "<i4", 5, at).tolist()
        col = np.frombuffer(raw, "<i4", M, at + 20).tolist()
        pep = list(raw[at + 20 + 4 * M:at + 20 + 4 * M + n])
        out.append((hit, col, pep))
        at += 20 + 4 * M + n
    assert at == len(raw)
    return out


@pytest.fixture(scope="module")
def twin_of_cases():
    seqs, profs, items, names = dac.cases()
    return [da.align(da.window_residues(seqs[s], f, i0, i1), i0, profs[p]) for s, f, i0, i1, p in items]


def test_header_is_the_twin(tmp_path, twin_of_cases):
    seqs, profs, items, names = dac.cases()
    got = _header_items(tmp_path, seqs, profs, items)
    for name, (s, f, i0, i1, p), (hit, col, pep), (whit, wcol, _) in zip(names, items, got, twin_of_cases):
        assert pep == da.window_residues(seqs[s], f, i0, i1), name
        assert hit == whit and col == wcol, (name, hit, whit)


def test_header_is_the_twin_on_mixed_items(tmp_path):
    seqs, profs, items = dac.mixed(120)
    got = _header_items(tmp_path, seqs, profs, items)
    for it, (hit, col, pep) in zip(items, got):
        s, f, i0, i1, p = it
        whit, wcol, _ = da.align(da.window_residues(seqs[s], f, i0, i1), i0, profs[p])
        assert hit == whit and col == wcol, it


def test_paths_start_and_end_at_the_hit_and_add_up(twin_of_cases):
    seqs, profs, items, names = dac.cases()
    n_ins = n_del = 0
    for name, (s, f, i0, i1, p), (hit, col, path) in zip(names, items, twin_of_cases):
        res = da.window_residues(seqs[s], f, i0, i1)
        score, i_s, i_e, k_s, k_e = hit
        assert path[0] == ("M", i_s, k_s) and path[-1] == ("M", i_e, k_e), name
        assert da.path_score(path, res, i0, profs[p]) == score, name
        assert i0 <= i_s <= i_e <= i1 and 1 <= k_s <= k_e <= profs[p]["M"]
        # col is the path's match states, and nothing else
        want = [-1] * profs[p]["M"]
        for state, i, k in path:
            if state == "M":
                want[k - 1] = i
        assert col == want, name
        placed = [c for c in col if c >= 0]
        assert placed == sorted(set(placed)) and all(c == -1 for c in col[:k_s - 1] + col[k_e:])
        n_ins += sum(st == "I" for st, _, _ in path)
        n_del += sum(st == "D" for st, _, _ in path)
    assert n_ins and n_del


def _all_local_paths(n, M):
    """every local path over rows 0 .. n - 1 and nodes 1 .. M: starts in an M cell, ends in an M cell"""
    out = []

    def grow(path):
        state, i, k = path[-1]
        if state == "M":
            out.append(list(path))
        nxt = []
        if state in "MI" and i + 1 < n and k <= M - 1:      # an insert after node k (I_M does not exist)
            nxt.append(("I", i + 1, k))
        if state in "MD" and k + 1 <= M:                    # a delete of node k + 1 (D_1 does not exist: k + 1 >= 2)
            nxt.append(("D", i, k + 1))
        if i + 1 < n and k + 1 <= M:
            nxt.append(("M", i + 1, k + 1))
        for c in nxt:
            grow(path + [c])
    for i in range(n):
        for k in range(1, M + 1):
            grow([("M", i, k)])
    return out


@pytest.mark.parametrize("seed", range(4))
def test_tiny_items_equal_the_maximum_over_all_paths(seed):
    rng = random.Random(seed)
    for _ in range(25):
        M, n = rng.randint(1, 3), rng.randint(1, 4)
        prof = dr.random_profile(rng, M, star=rng.choice([0.0, 0.3]))
        if rng.random() < 0.5:
            prof["emis"][:, :20] = np.array([[rng.choice([-256, 0, 256]) for _ in range(20)] for _ in range(M)])
            prof["trans"][:] = np.array([[rng.choice([-512, -256, 0]) for _ in range(7)] for _ in range(M)])
        res = [rng.randrange(22) for _ in range(n)]
        i0 = rng.randrange(5)
        shifted = [[(st, i + i0, k) for st, i, k in p] for p in _all_local_paths(n, M)]
        top = max(da.path_score(p, res, i0, prof) for p in shifted)
        for engine in (da.align, da.align_plain):
            hit, col, path = engine(res, i0, prof)
            assert hit[0] == top and da.path_score(path, res, i0, prof) == top


@pytest.mark.parametrize("seed", range(4))
def test_row_version_is_the_triple_loop(seed):
    rng = random.Random(100 + seed)
    for _ in range(15):
        M = rng.choice([1, 2, 3, 4, 7, 12, 20])
        prof = dr.random_profile(rng, M, star=rng.choice([0.0, 0.3]))
        if rng.random() < 0.5:      # few distinct scores: ties everywhere
            prof["emis"][:, :20] = np.array([[rng.choice([-256, 0, 256]) for _ in range(20)] for _ in range(M)])
            prof["trans"][:] = np.array([[rng.choice([-512, -256, 0]) for _ in range(7)] for _ in range(M)])
        res = [rng.randrange(22) for _ in range(rng.randint(1, 25))]
        i0 = rng.randrange(40)
        assert da.align(res, i0, prof) == da.align_plain(res, i0, prof), (M, res)


def test_whole_frame_window_is_the_search_hit():
    seqs, profs, items, names = dac.cases()
    n = 0
    for name, (s, f, i0, i1, p) in zip(names, items):
        res = dr.translate(seqs[s], f)
        if i0 != 0 or i1 != len(res) - 1:
            continue
        score, start, i, k = dr.frame_hit(res, profs[p])
        assert da.align(res, 0, profs[p])[0] == [score, start >> 11, i, (start & 2047) + 1, k], name
        n += 1
    assert n >= 9


def _codes(engine, res, i0, prof):
    """the back-pointers an engine hands to the trace: (state, i, k) -> predecessor state or None"""
    keep = {}
    orig = da.trace

    def spy(codes, *a):
        keep["codes"] = codes
        return orig(codes, *a)
    da.trace = spy
    try:
        engine(res, i0, prof)
    finally:
        da.trace = orig
    return keep["codes"]


def test_flat_profile_hits_and_paths():
    """all emissions equal, all transitions equal: the order of the pairs and of the hit decides everything"""
    res = [0, 1, 2, 3, 4]
    # emissions 0, transitions 0: every cell scores the entry; the best word has the smallest start, the first cell with it wins
    prof = dac.flat_profile(4, emis=0, trans=0)
    for engine in (da.align, da.align_plain):
        assert engine(res, 10, prof) == ([prof["entry"], 10, 10, 1, 1], [10, -1, -1, -1], [("M", 10, 1)])
    # every match adds a bit: the longest diagonal from the smallest start
    prof3 = dac.flat_profile(3, emis=256, trans=0)
    for engine in (da.align, da.align_plain):
        assert engine(res, 0, prof3) == ([prof3["entry"] + 3 * 256, 0, 2, 1, 3], [0, 1, 2], [("M", 0, 1), ("M", 1, 2), ("M", 2, 3)])
    # two rows, three nodes: M(0,1) -> M(1,2) and M(0,1) -> D(0,2) -> M(1,3) are equal words in different cells of one row:
    # the hit takes the smaller k
    for engine in (da.align, da.align_plain):
        hit, col, path = engine(res[:2], 0, prof3)
        assert hit == [prof3["entry"] + 512, 0, 1, 1, 2] and col == [0, 1, -1] and path == [("M", 0, 1), ("M", 1, 2)]
    # two nodes, four rows: the direct path M(0,1) -> M(1,2) ends on the earliest row
    prof2 = dac.flat_profile(2, emis=256, trans=0)
    for engine in (da.align, da.align_plain):
        assert engine(res[:4], 0, prof2)[0] == [prof2["entry"] + 512, 0, 1, 1, 2]


def test_tie_order_of_each_cell():
    """Emissions 0 and transitions 0 on three nodes and four rows: every existing word scores the entry, so a maximum is
    decided by the start alone (the smaller start wins) and arguments with EQUAL starts tie -- there the first argument, in
    the order of the definition, is the code.  The starts, worked out by hand:
      row 0: M(0,k) start (0,k); D(0,2) <- M(0,1): (0,1); D(0,3): M(0,2) has (0,2), D(0,2) has (0,1) -> D
      row 1: M(1,2): entry (1,2), M(0,1) (0,1) -> M;  M(1,3): M(0,2) (0,2), D(0,2) (0,1) -> D
             I(1,1) <- M(0,1) (0,1);  I(1,2) <- M(0,2) (0,2);  D(1,3): M(1,2) (0,1), D(1,2) <- M(1,1) (1,1) -> M
      row 2: I(2,1): M(1,1) (1,1), I(1,1) (0,1) -> I;  I(2,2): M(1,2) (0,1), I(1,2) (0,2) -> M
             M(2,2): M(1,1) (1,1), I(1,1) (0,1) -> I;  M(2,3): M(1,2) (0,1), I(1,2) (0,2), D(1,2) (1,1) -> M
             D(2,3): M(2,2) (0,1), D(2,2) <- M(2,1) (2,1) -> M
      row 3: I(3,2): M(2,2) (0,1) and I(2,2) (0,1): EQUAL words -> the first, M"""
    prof = dac.flat_profile(3, emis=0, trans=0)
    res = [0, 1, 2, 3]
    assert da.align(res, 0, prof) == da.align_plain(res, 0, prof)
    c = _codes(da.align_plain, res, 0, prof)
    assert c[("M", 1, 2)] == "M" and c[("D", 0, 2)] == "M" and c[("D", 0, 3)] == "D" and c[("M", 1, 3)] == "D"
    assert c[("I", 1, 1)] == "M" and c[("I", 2, 1)] == "I" and c[("I", 2, 2)] == "M" and c[("D", 1, 3)] == "M"
    assert c[("M", 2, 2)] == "I" and c[("M", 2, 3)] == "M" and c[("D", 2, 3)] == "M"
    assert c[("I", 3, 2)] == "M"
    assert c[("M", 0, 1)] is None and c[("M", 3, 1)] is None      # node 1 has no predecessor: the entry
    # the row engine keeps the same codes, cell by cell (a cell without a predecessor has the first name in both)
    row = _codes(da.align, res, 0, prof)
    assert all(row[key] == want for key, want in c.items()) and len(c) == 12 + 8 + 8


def test_a_deletion_is_the_only_two_match_path():
    """nodes A, any, C with free gaps; node 2 emits everything at 0"""
    prof = dac.hand_profile("ADC", MM_1=0, MM_2=0, MD_1=0, DM_2=0, MI_1=0, IM_1=0, II_1=0, DD_2=0, MI_2=0, IM_2=0)
    prof["emis"][1, :] = 0
    a, w, c_ = dr.AA.index("A"), dr.AA.index("W"), dr.AA.index("C")
    for engine in (da.align, da.align_plain):
        hit, col, path = engine([a, w, c_], 0, prof)
        assert hit == [2000 + prof["entry"], 0, 2, 1, 3] and col == [0, 1, 2]
        hit, col, path = engine([a, c_], 0, prof)
        assert hit == [2000 + prof["entry"], 0, 1, 1, 3] and col == [0, -1, 1] and path == [("M", 0, 1), ("D", 0, 2), ("M", 1, 3)]


def test_planted_insertion_and_deletion():
    # one insert: A W C against the nodes A C -- M1 -> I1 -> M2: W is in no column
    p = dac.hand_profile("AC", MI_1=-100, IM_1=-50)
    res = [dr.AA.index(a) for a in "AWC"]
    for engine in (da.align, da.align_plain):
        hit, col, path = engine(res, 7, p)
        assert hit == [2000 - 406 - 150, 7, 9, 1, 2] and col == [7, 9]
        assert path == [("M", 7, 1), ("I", 8, 1), ("M", 9, 2)] and 8 not in col
    # one delete: A D against the nodes A C D -- M1 -> D2 -> M3
    p = dac.hand_profile("ACD", MD_1=-120, DM_2=-30)
    res = [dr.AA.index(a) for a in "AD"]
    for engine in (da.align, da.align_plain):
        hit, col, path = engine(res, 0, p)
        assert hit == [2000 - 662 - 150, 0, 1, 1, 3] and col == [0, -1, 1]
    # the planted cases of the shared list: one residue more than nodes placed / one node without a residue
    seqs, profs, items, names = dac.cases()
    for name, want_gap in (("insert1", 0), ("delete1", 1)):
        s, f, i0, i1, pi = items[names.index(name)]
        hit, col, path = da.align(da.window_residues(seqs[s], f, i0, i1), i0, profs[pi])
        assert hit[3:] == [1, 60] and col.count(-1) == want_gap, (name, hit, col)
        assert hit[2] - hit[1] + 1 == (61 if name == "insert1" else 59)
        assert sum(st == "I" for st, _, _ in path) == (1 if name == "insert1" else 0)


def test_a_window_sees_nothing_outside_it():
    """rows before i0 do not exist: the window's result is that of the residues alone, shifted"""
    rng = random.Random(5)
    prof = dr.random_profile(rng, 9)
    res = [rng.randrange(20) for _ in range(30)]
    hit, col, path = da.align(res[8:20], 8, prof)
    hit0, col0, _ = da.align(res[8:20], 0, prof)
    assert hit == [hit0[0], hit0[1] + 8, hit0[2] + 8, hit0[3], hit0[4]] and col == [c + 8 if c >= 0 else -1 for c in col0]


def test_pair_comparison_eight_bytes_a_step(tmp_path):
    rng = np.random.default_rng(3)
    blocks, want = [], []
    for N, C in ((2, 1), (3, 7), (4, 8), (5, 9), (6, 33), (3, 64)):
        rows = rng.integers(0, 24, (N, C)).astype(np.uint8)
        rows[rng.random((N, C)) < 0.2] = 255
        rows[0, :] = rng.choice(np.array([19, 20, 21, 127, 128, 147, 148, 255], np.uint8), C)      # around every bit the flags lean on
        blocks.append(struct.pack("<qqq", 2, N, C) + rows.tobytes())
        want.append(da.aln_pairs(rows))
    data, res = tmp_path / "in.bin", tmp_path / "out.bin"
    data.write_bytes(b"".join(blocks) + struct.pack("<q", 0))
    assert host_check.ok_count(host_check.run(tmp_path, "domalign_host_check", [data, res])) == len(blocks)
    raw, at = np.frombuffer(res.read_bytes(), "<i4"), 0
    for same, both in want:
        nn = same.size
        assert (raw[at:at + nn] == same.ravel()).all() and (raw[at + nn:at + 2 * nn] == both.ravel()).all()
        at += 2 * nn
    assert at == raw.size


def test_pair_comparison_on_every_byte_pair(tmp_path):
    """all 65536 pairs of bytes, eight row pairs of 8192 columns through the header's eight-bytes-a-step arithmetic"""
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    a, b = a.ravel(), b.ravel()
    same, both = da.aln_pairs(np.stack([a, b]))
    assert both[0, 1] == 400 and same[0, 1] == 20 and same[0, 0] == both[0, 0] == 20 * 256
    data, res = tmp_path / "in.bin", tmp_path / "out.bin"
    data.write_bytes(b"".join(struct.pack("<qqq", 2, 2, 8192) + a[q:q + 8192].tobytes() + b[q:q + 8192].tobytes() for q in range(0, 65536, 8192))
                     + struct.pack("<q", 0))
    assert host_check.ok_count(host_check.run(tmp_path, "domalign_host_check", [data, res])) == 8
    raw = np.frombuffer(res.read_bytes(), "<i4").reshape(8, 2, 2, 2)
    for q in range(8):
        wsame, wboth = da.aln_pairs(np.stack([a[8192 * q:8192 * q + 8192], b[8192 * q:8192 * q + 8192]]))
        assert (raw[q, 0] == wsame).all() and (raw[q, 1] == wboth).all(), q
    assert raw[:, 1, 0, 1].sum() == 400 and raw[:, 0, 0, 1].sum() == 20
