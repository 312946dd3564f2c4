"""GPU: the profile alignment (sp_domalign.hip: da_residues, da_fill, da_trace; Context.dom_align, dom_peptide) against the
Python twin (tests/domalign_ref.py) and the pair comparison (da_pairs; Context.aln_pairs) against numpy, all with `==`.

Cases (tests/domalign_cases.py): M = 1, 2, 63, 64, 65, 128, 129, 512 (tables in LDS), 513 and 2048 (tables from global
memory, the largest state); windows of 1, 2, 64, 65 and 129 residues (the 64-row residue stage) at both ends of all six
frames, whole frames, one window of 8192 residues at M = 65; N runs and stop codons; flat profiles (ties in every cell);
one planted insertion and one planted deletion; 200 mixed items under batches of any size, 1 and 3 items; whole-frame
windows against dom_search; n = 0; every SP_EINVAL and SP_EUNSUP, none of which launches a kernel -- SP_ENOMEM is NOT
reached: it needs a workspace the device cannot hold.  aln_pairs: N around the tile of 32 rows, C around the word of 8 and
the chunk of 1024 columns, rows of gaps only, equal rows, X and stop as no residue."""
import ctypes as C

import numpy as np
import pytest

import domains_cases as dc
import domalign_cases as dac
import domalign_ref as da
import domains_ref as dr
from subphaser_amd import _native

pytestmark = pytest.mark.gpu
TILE, CHUNK = 32, 1024      # SP_DA_TILE, SP_DA_CHUNK in sp_domalign.hip


def _load(ctx, chroms):
    ctx.genome_reset(len(chroms))
    for i, s in enumerate(chroms):
        ctx.genome_add(i, s)


def _args(items, chrom, start, end):
    s, f, i0, i1, p = (np.array(c) for c in zip(*items))
    return [np.array(chrom)[s], np.array(start)[s], np.array(end)[s], f, i0, i1], p


@pytest.fixture(scope="module")
def laid_out():
    seqs, profs, items, names = dac.cases()
    chroms, chrom, start, end = dc.genome(seqs)
    want = da.align_items(seqs, items, profs)
    return seqs, profs, items, names, chroms, chrom, start, end, want


def test_kernels_are_the_twin(gpu_ctx, laid_out):
    seqs, profs, items, names, chroms, chrom, start, end, (whit, wcol, wcoff) = laid_out
    _load(gpu_ctx, chroms)
    where, p = _args(items, chrom, start, end)
    hit, col, coff = gpu_ctx.dom_align(*where, p, *dr.tables(profs))
    assert hit.dtype == np.int32 and col.dtype == np.int32 and (coff == wcoff).all()
    bad = [names[q] for q in range(len(items)) if (hit[q] != whit[q]).any() or (col[coff[q]:coff[q + 1]] != wcol[coff[q]:coff[q + 1]]).any()]
    assert not bad, (bad[:8], hit[names.index(bad[0])].tolist(), whit[names.index(bad[0])].tolist())
    # the cases do what their names say
    by = {n: q for q, n in enumerate(names)}
    assert whit[by["win8192"]][2] - whit[by["win8192"]][1] >= 0 and items[by["win8192"]][3] - items[by["win8192"]][2] + 1 == 8192
    ins, dele = by["insert1"], by["delete1"]
    assert (wcol[wcoff[ins]:wcoff[ins + 1]] == -1).sum() == 0 and whit[ins][2] - whit[ins][1] + 1 == 61
    assert (wcol[wcoff[dele]:wcoff[dele + 1]] == -1).sum() == 1 and whit[dele][2] - whit[dele][1] + 1 == 59


def test_peptides_are_the_twin(gpu_ctx, laid_out):
    seqs, profs, items, names, chroms, chrom, start, end, _ = laid_out
    _load(gpu_ctx, chroms)
    where, _p = _args(items, chrom, start, end)
    pep, poff = gpu_ctx.dom_peptide(*where)
    assert pep.dtype == np.uint8 and poff[-1] == pep.size
    for q, (s, f, i0, i1, _) in enumerate(items):
        assert pep[poff[q]:poff[q + 1]].tolist() == da.window_residues(seqs[s], f, i0, i1), names[q]
    assert {20, 21} <= set(pep.tolist())      # an invalid codon and a stop are among them
    z = np.zeros(0, np.int64)
    pep, poff = gpu_ctx.dom_peptide(z, z, z, z, z, z)
    assert pep.size == 0 and poff.tolist() == [0]


def test_batches_of_any_size_give_the_same_bytes(gpu_ctx):
    seqs, profs, items = dac.mixed(200)
    chroms, chrom, start, end = dc.genome(seqs, n_chrom=3)
    _load(gpu_ctx, chroms)
    where, p = _args(items, chrom, start, end)
    want = da.align_items(seqs, items, profs)
    got = {}
    try:
        for batch in (0, 1, 3):
            gpu_ctx.dom_align_set_batch(batch)
            got[batch] = gpu_ctx.dom_align(*where, p, *dr.tables(profs))
    finally:
        gpu_ctx.dom_align_set_batch(0)
    for batch in (0, 1, 3):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[batch], got[0])), batch
    assert (got[0][0] == want[0]).all() and (got[0][1] == want[1]).all() and (got[0][2] == want[2]).all()
    with pytest.raises(ValueError, match="below 0"):
        gpu_ctx.dom_align_set_batch(-1)


def test_whole_frame_windows_give_the_search_hit(gpu_ctx):
    import random
    rng = random.Random(31)
    seqs = [dr.rand_dna(rng, n) for n in (90, 200, 333, 64, 12)]
    profs = [dr.random_profile(rng, M) for M in (5, 64, 130)]
    chroms, chrom, start, end = dc.genome(seqs)
    _load(gpu_ctx, chroms)
    tab = dr.tables(profs)
    found = gpu_ctx.dom_search(chrom, start, end, *tab)
    items = [(s, int(found[s, p, 1]), 0, len(dr.translate(seqs[s], int(found[s, p, 1]))) - 1, p) for s in range(len(seqs)) for p in range(len(profs))]
    where, p = _args(items, chrom, start, end)
    hit, col, coff = gpu_ctx.dom_align(*where, p, *tab)
    for q, (s, f, _, _, pi) in enumerate(items):
        assert hit[q].tolist() == found[s, pi, [0, 2, 3, 4, 5]].tolist(), (s, pi)


def test_empty_call_and_errors(gpu_ctx, laid_out):
    seqs, profs, items, names, chroms, chrom, start, end, (whit, wcol, wcoff) = laid_out
    _load(gpu_ctx, chroms)
    plist = [profs[0], profs[4]]
    tab = dr.tables(plist)
    moff, emis, trans, entry = tab
    s0 = items[0][0]
    base = ([chrom[s0]], [start[s0]], [end[s0]], [1], [2], [20])
    want = da.align_items(seqs, [(s0, 1, 2, 20, 1)], plist)

    def good():
        got = gpu_ctx.dom_align(*base, [1], *tab)
        assert all((a == b).all() for a, b in zip(got, want))
    z = np.zeros(0, np.int64)
    hit, col, coff = gpu_ctx.dom_align(z, z, z, z, z, z, z, *tab)
    assert hit.shape == (0, 5) and col.size == 0 and coff.tolist() == [0]
    good()
    n0, nres = len(chroms[chrom[s0]]), len(dr.translate(seqs[s0], 1))

    def with_(idx, val):
        a = [list(x) for x in base]
        a[idx] = [val]
        return a

    def changed(arr, idx, val):
        a = arr.copy()
        a[idx] = val
        return a
    big = dr.tables([dr.make_profile(2049, np.zeros((2049, 22)), np.zeros((2049, 7)))])
    many = dr.tables([plist[0]] * 4097)
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        for args, msg in [((with_(0, 7), [1]) + tab, "chromosome 7 out of range"),
                          ((with_(1, -1), [1]) + tab, "outside chromosome"),
                          ((with_(2, n0 + 1), [1]) + tab, "outside chromosome"),
                          ((with_(3, 6), [1]) + tab, "frame 6 is outside 0..5"),
                          ((with_(3, -1), [1]) + tab, "frame -1 is outside 0..5"),
                          ((with_(4, 21), [1]) + tab, "is empty or starts below 0"),
                          ((with_(4, -1), [1]) + tab, "is empty or starts below 0"),
                          ((with_(5, nres), [1]) + tab, "ends beyond the %d residues" % nres),
                          ((base, [2]) + tab, "profile 2 is outside 0..1"),
                          ((base, [-1]) + tab, "profile -1 is outside 0..1"),
                          ((base, [0], np.zeros(1, np.int32), emis[:0], trans[:0], entry[:0]), "0 profiles"),
                          ((base, [1], changed(moff, 1, 0), emis, trans, entry), "has 0 nodes"),
                          ((base, [1], changed(moff, 0, 1), emis, trans, entry), "start at 1"),
                          ((base, [1], moff, changed(emis, (0, 0), (1 << 15) + 1), trans, entry), "outside its range"),
                          ((base, [1], moff, emis, changed(trans, (0, 2), 1), entry), "outside its range"),
                          ((base, [1], moff, emis, trans, changed(entry, 1, 5)), "outside its range"),
                          ((base, [0]) + big, "2049 nodes"),
                          ((base, [1]) + many, "4097 profiles")]:
            with pytest.raises(ValueError, match=msg):
                gpu_ctx.dom_align(*args[0], *args[1:])
        for idx, val, msg in [(0, 7, "chromosome 7 out of range"), (3, 6, "frame 6"), (4, 21, "is empty"), (5, nres, "ends beyond")]:
            with pytest.raises(ValueError, match=msg):
                gpu_ctx.dom_peptide(*with_(idx, val))
        # bad offsets and NULL pointers, through the C entries themselves (Context never passes either)
        arrs = [np.array(a, t) for a, t in zip(base, (np.int32, np.int64, np.int64, np.int32, np.int32, np.int32))]
        pr, hit, col = np.ones(1, np.int32), np.zeros((1, 5), np.int32), np.zeros(64, np.int32)
        M1 = int(moff[2] - moff[1])
        full = arrs + [pr, moff, emis, trans, entry, hit, np.array([0, M1], np.int64), col]

        def call(ptrs):
            return gpu_ctx.L.sp_dom_align(gpu_ctx.h, 1, *ptrs[:7], 2, *ptrs[7:])
        for coff_bad, msg in (([0, M1 - 1], b"the offsets leave"), ([1, M1 + 1], b"start at 1")):
            ptrs = [a.ctypes.data_as(C.c_void_p) for a in full]
            bad = np.array(coff_bad, np.int64)
            ptrs[12] = bad.ctypes.data_as(C.c_void_p)
            assert call(ptrs) == _native.SP_EINVAL and msg in gpu_ctx.L.sp_last_error(gpu_ctx.h)
        for q in range(len(full)):
            ptrs = [None if j == q else a.ctypes.data_as(C.c_void_p) for j, a in enumerate(full)]
            assert call(ptrs) == _native.SP_EINVAL and b"bad arguments" in gpu_ctx.L.sp_last_error(gpu_ctx.h), q
        assert gpu_ctx.L.sp_dom_align(None, 0, *([None] * 7), 2, *([None] * 7)) == _native.SP_EINVAL
        pep, poff = np.zeros(64, np.uint8), np.array([0, 19], np.int64)
        pfull = arrs + [poff, pep]
        for q in range(len(pfull)):
            ptrs = [None if j == q else a.ctypes.data_as(C.c_void_p) for j, a in enumerate(pfull)]
            assert gpu_ctx.L.sp_dom_peptide(gpu_ctx.h, 1, *ptrs) == _native.SP_EINVAL, q
        poff[1] = 18
        assert gpu_ctx.L.sp_dom_peptide(gpu_ctx.h, 1, *[a.ctypes.data_as(C.c_void_p) for a in pfull]) == _native.SP_EINVAL
        assert b"the offsets leave 18 bytes" in gpu_ctx.L.sp_last_error(gpu_ctx.h)
        # the limits: a window of 8193 residues, an interval above 65536 bases
        long = dr.rand_dna(__import__("random").Random(1), 65540)
        _load(gpu_ctx, [long])
        with pytest.raises(ValueError, match="window of 8193 residues"):
            gpu_ctx.dom_align([0], [0], [65536], [0], [5], [8197], [1], *tab)
        with pytest.raises(ValueError, match="window of 8193 residues"):
            gpu_ctx.dom_peptide([0], [0], [65536], [0], [5], [8197])
        with pytest.raises(ValueError, match="65537 bases"):
            gpu_ctx.dom_align([0], [1], [65538], [0], [5], [9], [1], *tab)
        gpu_ctx.genome_reset(0)
        with pytest.raises(ValueError, match="no genome loaded"):
            gpu_ctx.dom_align(*base, [1], *tab)
        launched = gpu_ctx.prof_report()
    finally:
        gpu_ctx.prof_enable(False)
    assert not [k for k in launched if k.startswith("da_")], launched      # every refusal came before a launch
    _load(gpu_ctx, chroms)
    good()


# ---------------------------------------------------------------------------------------------- aligned rows
def _rows(rng, N, Cn):
    rows = rng.integers(0, 20, (N, Cn)).astype(np.uint8)
    rows[rng.random((N, Cn)) < 0.25] = 255
    rows[rng.random((N, Cn)) < 0.05] = 20      # X
    rows[rng.random((N, Cn)) < 0.05] = 21      # stop
    return rows


@pytest.mark.parametrize("N", [2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_pairs_around_the_tile(gpu_ctx, N):
    rng = np.random.default_rng(N)
    for Cn in (1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1):
        rows = _rows(rng, N, Cn)
        rows[0] = 255                       # a row of gaps only
        rows[N - 1] = rows[N // 2]          # equal rows (N = 2: both are the gap row)
        same, both = gpu_ctx.aln_pairs(rows)
        wsame, wboth = da.aln_pairs(rows)
        assert same.dtype == np.int32 and (same == wsame).all() and (both == wboth).all(), (N, Cn)
        assert (same == same.T).all() and (both == both.T).all() and (both[0] == 0).all()
        own = (rows < 20).sum(axis=1)
        assert (np.diag(same) == own).all() and (np.diag(both) == own).all()
        assert same[N - 1, N // 2] == both[N - 1, N // 2] == own[N // 2]


def test_pairs_at_the_widest_row(gpu_ctx):
    rng = np.random.default_rng(8192)
    rows = _rows(rng, TILE + 2, 8192)
    rows[3, :] = np.arange(8192) % 22       # X and stop are no residue
    same, both = gpu_ctx.aln_pairs(rows)
    wsame, wboth = da.aln_pairs(rows)
    assert (same == wsame).all() and (both == wboth).all()
    assert both[3, 3] == (rows[3] < 20).sum() < 8192


def test_pairs_errors(gpu_ctx):
    rows = np.zeros((3, 5), np.uint8)
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        for bad, msg in ((np.zeros((1, 5), np.uint8), "1 rows of 5 columns"), (np.zeros((3, 0), np.uint8), "3 rows of 0 columns"),
                         (np.zeros((4097, 1), np.uint8), "4097 rows"), (np.zeros((2, 8193), np.uint8), "8193 columns")):
            with pytest.raises(ValueError, match=msg):
                gpu_ctx.aln_pairs(bad)
        out = np.zeros((3, 3), np.int32)
        full = [rows, out, out.copy()]
        for q in range(3):
            ptrs = [None if j == q else a.ctypes.data_as(C.c_void_p) for j, a in enumerate(full)]
            assert gpu_ctx.L.sp_aln_pairs(gpu_ctx.h, 3, 5, *ptrs) == _native.SP_EINVAL
        assert gpu_ctx.L.sp_aln_pairs(None, 3, 5, None, None, None) == _native.SP_EINVAL
        launched = gpu_ctx.prof_report()
    finally:
        gpu_ctx.prof_enable(False)
    assert "da_pairs" not in launched
    same, both = gpu_ctx.aln_pairs(rows)
    assert (same == 5).all() and (both == 5).all()
