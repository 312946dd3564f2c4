"""GPU: the ungapped prefilter of the domain search (sp_domains.hip: dm_ssv; Context.dom_ssv, Context.dom_search(prefilter=),
-ltr_dom_prefilter) against the Python twins (tests/domssv_ref.py) with `==`.

dm_ssv gives a lane diagonals, a workgroup `span` (1024) consecutive diagonals of one profile's line of all frames, and walks
the nodes in tiles of `tile` (128).  Cases: M = 1, 2, 63, 64, 65, 127, 128, 129 and 256 (one below, at, one above and twice
the tile) and 2048; inner sequences of 0, 1, 2, 3, 5, 191, 192, 193, 196 and 400 bases (frames of 0, 1, 63, 64, 65 and 133
residues at all six offsets; tests/domssv_cases.py, whose names tests/test_domssv_host.py checks); every codon invalid; a
run of stop codons; the best segment a single cell at the first or the last residue and at node 1 or node M; a whole consensus of 200 nodes (the segment crosses the tile boundary at node
128); all in ONE call, so that frames share workgroups and the 400-base frames against 256 and 2048 nodes (388 and 2180
diagonals) are cut over waves and workgroups.  A diagonal is never split: what a boundary between lanes, waves or
workgroups can cut is a frame, and the same call at (tile, span) = (1, 1), (7, 100), (128, 64) and the default gives the
same bytes.  2000 elements x 8 profiles in one call.  sp_dom_search_pre: INT32_MIN is sp_dom_search byte for byte on all of
tests/domains_cases.py; thresholds at an item's ssv and one above against the filtered twin; a threshold above every
score; the counts; the dm_search grid of sp_prof_report = the survivors.  The refusals of sp_dom_search with their codes,
through both new entries.  The command line against the filtered twin's files.
The kernel caps no grid and loops over no items (its grid is the spans of diagonals of the call), so there is no
SP_CU_LIMIT case; the span setter is what moves the cuts.  SP_ENOMEM and the refusal of more than 2^31 - 1 workgroups
are NOT reached: they need a workspace the device cannot hold, or 2^41 diagonals."""
import random

import numpy as np
import pytest

import domains_cases as dc
import domains_ref as dr
import domssv_cases as sc
import domssv_ref as sr
from subphaser_amd import _native

pytestmark = pytest.mark.gpu

TILE = sc.TILE


def _load(ctx, chroms):
    ctx.genome_reset(len(chroms))
    for i, s in enumerate(chroms):
        ctx.genome_add(i, s)


@pytest.fixture(scope="module")
def world():
    return sc.world()


@pytest.fixture(scope="module")
def expected():
    return sc.expected()


def _call(ctx, world, tile=0, span=0):
    names, seqs, P, pn = world
    chroms, chrom, start, end = dc.genome(seqs)
    _load(ctx, chroms)
    ctx.dom_ssv_set_tile(tile, span)
    try:
        return ctx.dom_ssv(chrom, start, end, *dr.tables([P[p] for p in pn]))
    finally:
        ctx.dom_ssv_set_tile(0, 0)


def test_kernel_is_the_twin(gpu_ctx, world, expected):
    names, seqs, P, pn = world
    got = _call(gpu_ctx, world)
    assert got.dtype == np.int32 and got.shape == (len(seqs), len(pn), 6)
    bad = np.argwhere(got != expected)
    assert bad.size == 0, [(names[i], pn[p], f, int(got[i, p, f]), int(expected[i, p, f])) for i, p, f in bad[:8]]


@pytest.mark.parametrize("tile,span", [(1, 1), (7, 100), (TILE, 64), (2 * TILE // 3, 1024)])
def test_no_result_depends_on_tile_or_span(gpu_ctx, world, expected, tile, span):
    assert (_call(gpu_ctx, world, tile, span) == expected).all()
    with pytest.raises(ValueError, match="a tile of %d nodes" % (TILE + 1)):
        gpu_ctx.dom_ssv_set_tile(TILE + 1, 0)
    with pytest.raises(ValueError, match="1025 diagonals a workgroup"):
        gpu_ctx.dom_ssv_set_tile(0, 1025)
    with pytest.raises(ValueError, match="a tile of -1 nodes"):
        gpu_ctx.dom_ssv_set_tile(-1, 0)


def test_two_thousand_elements_by_eight_profiles(gpu_ctx, monkeypatch):
    seqs, names = dc.many(2000)
    chroms, chrom, start, end = dc.genome(seqs, n_chrom=3)
    _load(gpu_ctx, chroms)
    plist = [dc.profiles()[p] for p in names]
    got = gpu_ctx.dom_ssv(chrom, start, end, *dr.tables(plist))
    want = sr.ssv(seqs, plist)
    bad = np.argwhere(got != want)
    assert got.shape == (2000, 8, 6) and bad.size == 0, [(seqs[i], names[p], f, int(got[i, p, f]), int(want[i, p, f])) for i, p, f in bad[:5]]
    assert (want == dr.INT32_MIN).any() and (want > 0).any()
    # the slices of Context.dom_ssv: 8 elements a call
    monkeypatch.setattr(_native, "DOMAINS_CALL_ENTRIES", 64)
    assert (gpu_ctx.dom_ssv(chrom[:300], start[:300], end[:300], *dr.tables(plist)) == want[:300]).all()


# ------------------------------------------------------------------------------------------ the search behind the filter
def test_pass_all_threshold_is_the_search(gpu_ctx):
    cases = dc.cases()
    chroms, chrom, start, end = dc.genome([c[1] for c in cases])
    _load(gpu_ctx, chroms)
    P = dc.profiles()
    for names in (["m1", "m2", "m63", "m64", "m65", "m129", "star65", "star200", "c60", "c200", "m600"], ["m2048", "c700", "m5"]):
        tab = dr.tables([P[p] for p in names])
        stats = {}
        plain = gpu_ctx.dom_search(chrom, start, end, *tab)
        got = gpu_ctx.dom_search(chrom, start, end, *tab, prefilter=dr.INT32_MIN, stats=stats)
        assert got.tobytes() == plain.tobytes()
        items = sum(len(dr.translate(c[1], f)) > 0 for c in cases for f in range(6)) * len(names)
        assert stats == {"items": items, "passed": items}


def _profiled(ctx, call):
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        out = call()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    return out, {k: int(v["grid"]) for k, v in rep.items()}


def test_thresholds_against_the_filtered_twin(gpu_ctx, monkeypatch):
    P = dc.profiles()
    cases = [c for c in dc.cases() if c[0] in ("len2", "len5", "len32", "sizes", "planted", "planted_rc", "frame_tie", "stop")]
    seqs, plist = [c[1] for c in cases], [P["c60"], P["m5"], P["m65"], P["m64"], P["star65"]]
    chroms, chrom, start, end = dc.genome(seqs)
    _load(gpu_ctx, chroms)
    tab = dr.tables(plist)
    hmemo, smemo = {}, {}
    scores = sr.ssv(seqs, plist, smemo)
    assert (gpu_ctx.dom_ssv(chrom, start, end, *tab) == scores).all()
    plain = dr.search(seqs, plist)
    from test_domssv_host import pick_item
    a, b, f = pick_item(plain, scores)
    T = int(scores[a, b, f])
    moved = None
    for thr in (T, T + 1, int(np.median(scores[scores != dr.INT32_MIN])), int(scores.max()), int(scores.max()) + 1):
        want, items, passed = sr.search(seqs, plist, thr, hmemo, smemo)
        stats = {}
        got, grid = _profiled(gpu_ctx, lambda: gpu_ctx.dom_search(chrom, start, end, *tab, prefilter=thr, stats=stats))
        assert (got == want).all(), (thr, np.argwhere((got != want).any(axis=2))[:5].tolist())
        assert stats == {"items": items, "passed": passed} and passed == int((scores >= thr).sum())
        # only the survivors ran: one workgroup of dm_search per item, every profile here has its tables in LDS
        assert grid.get("dm_search", 0) == passed and "dm_search_wide" not in grid and grid["dm_ssv"] >= 1
        if thr == T:
            assert (got[a, b] == plain[a, b]).all()
        if thr == T + 1:
            moved = got[a, b].tolist()
    assert moved[1] != f and moved[0] > dr.INT32_MIN
    assert passed == 0 and (got[:, :, 0] == dr.INT32_MIN).all() and not got[:, :, 1:].any()      # above every score: no hit anywhere
    # the counts add up over the slices of Context.dom_search
    monkeypatch.setattr(_native, "DOMAINS_CALL_ENTRIES", 10)
    stats = {}
    want, items, passed = sr.search(seqs, plist, T, hmemo, smemo)
    assert (gpu_ctx.dom_search(chrom, start, end, *tab, prefilter=T, stats=stats) == want).all() and stats == {"items": items, "passed": passed}


def test_empty_call_and_errors(gpu_ctx):
    import ctypes as C
    P = dc.profiles()
    seq = dc.cases()[12][1]
    chroms = [seq + "ACGT", "ACGTACGT"]
    _load(gpu_ctx, chroms)
    plist = [P["m5"], P["m64"]]
    tab = dr.tables(plist)
    want_s, want_h = sr.ssv([seq], plist), dr.search([seq], plist)

    def ssv(*a):
        return gpu_ctx.dom_ssv(*a)

    def pre(*a):
        return gpu_ctx.dom_search(*a, prefilter=dr.INT32_MIN, stats={})

    def good():
        assert (ssv([0], [0], [len(seq)], *tab) == want_s).all() and (pre([0], [0], [len(seq)], *tab) == want_h).all()
    z = np.zeros(0, np.int64)
    stats = {}
    assert ssv(z, z, z, *tab).shape == (0, 2, 6)
    assert gpu_ctx.dom_search(z, z, z, *tab, prefilter=5, stats=stats).shape == (0, 2, 6) and stats == {"items": 0, "passed": 0}
    good()
    n0 = len(chroms[0])
    moff, emis, trans, entry = tab

    def changed(arr, idx, val):
        a = arr.copy()
        a[idx] = val
        return a
    big = dr.tables([dr.make_profile(2049, np.zeros((2049, 22)), np.zeros((2049, 7)))])
    many = dr.tables([P["m1"]] * 4097)
    for args, msg in [(([2], [0], [5]) + tab, "chromosome 2 out of range"),
                      (([-1], [0], [5]) + tab, "chromosome -1 out of range"),
                      (([0], [-1], [5]) + tab, "outside chromosome"),
                      (([0], [0], [n0 + 1]) + tab, "outside chromosome"),
                      (([0], [6], [5]) + tab, "ends before it starts"),
                      (([0], [0], [5], np.zeros(1, np.int32), emis[:0], trans[:0], entry[:0]), "0 profiles"),
                      (([0], [0], [5], changed(moff, 1, 0), emis, trans, entry), "has 0 nodes"),
                      (([0], [0], [5], changed(moff, 0, 1), emis, trans, entry), "start at 1"),
                      (([0], [0], [5], moff, changed(emis, (0, 0), (1 << 15) + 1), trans, entry), "outside its range"),
                      (([0], [0], [5], moff, emis, changed(trans, (3, 2), 1), entry), "outside its range"),
                      (([0], [0], [5], moff, emis, trans, changed(entry, 1, 5)), "outside its range"),
                      (([0], [0], [5]) + big, "2049 nodes"),
                      (([0], [0], [5]) + many, "4097 profiles")]:
        for call, who in ((ssv, "sp_dom_ssv"), (pre, "sp_dom_search_pre")):
            with pytest.raises(ValueError, match=who + ".*" + msg):
                call(*args)
        good()
    # the codes, and NULL pointers, through the C entries themselves
    ch, st, en = np.zeros(1, np.int32), np.zeros(1, np.int64), np.full(1, 5, np.int64)
    out, cnt = np.zeros((1, 2, 6), np.int32), np.zeros(2, np.int64)
    L, h = gpu_ctx.L, gpu_ctx.h
    full = [ch, st, en, moff, emis, trans, entry, out, cnt]
    for q in range(len(full)):
        ptr = [None if j == q else a.ctypes.data_as(C.c_void_p) for j, a in enumerate(full)]
        if q < 8:
            assert L.sp_dom_ssv(h, 1, ptr[0], ptr[1], ptr[2], 2, ptr[3], ptr[4], ptr[5], ptr[6], ptr[7]) == _native.SP_EINVAL
            assert b"sp_dom_ssv: bad arguments" in L.sp_last_error(h), q
        assert L.sp_dom_search_pre(h, 1, ptr[0], ptr[1], ptr[2], 2, ptr[3], ptr[4], ptr[5], ptr[6], 0, ptr[7], ptr[8]) == _native.SP_EINVAL
        assert b"sp_dom_search_pre: bad arguments" in L.sp_last_error(h), q
        good()
    p = [a.ctypes.data_as(C.c_void_p) for a in full]
    bigp = [a.ctypes.data_as(C.c_void_p) for a in big]
    assert L.sp_dom_ssv(h, 1, p[0], p[1], p[2], 1, bigp[0], bigp[1], bigp[2], bigp[3], p[7]) == _native.SP_EUNSUP
    assert L.sp_dom_search_pre(h, 1, p[0], p[1], p[2], 1, bigp[0], bigp[1], bigp[2], bigp[3], 0, p[7], p[8]) == _native.SP_EUNSUP
    assert L.sp_dom_ssv(None, 0, None, None, None, 2, None, None, None, None, None) == _native.SP_EINVAL
    assert L.sp_dom_search_pre(None, 0, None, None, None, 2, None, None, None, None, 0, None, None) == _native.SP_EINVAL
    assert L.sp_dom_ssv(h, 0, None, None, None, 2, p[3], p[4], p[5], p[6], None) == _native.SP_OK      # n = 0
    assert L.sp_dom_search_pre(h, 0, None, None, None, 2, p[3], p[4], p[5], p[6], 0, None, p[8]) == _native.SP_OK
    good()
    long = dr.rand_dna(random.Random(1), 65540)
    _load(gpu_ctx, [long])
    for call in (ssv, pre):
        with pytest.raises(ValueError, match="65537 bases"):
            call([0], [1], [65538], *tab)
    assert ssv([0], [0], [0], *tab).ravel().tolist() == [dr.INT32_MIN] * 12
    gpu_ctx.genome_reset(0)
    for call in (ssv, pre):
        with pytest.raises(ValueError, match="no genome loaded"):
            call([0], [0], [5], *tab)
    _load(gpu_ctx, chroms)
    good()


def test_an_interval_at_the_length_limit(gpu_ctx):
    """65536 bases against 12 and 2048 nodes: 21845 residues in frame 0, lines of 65 000 and 13 million diagonals -- the
    twin a node at a time is cheap at 12 nodes; at 2048 the planted spike's cell is known"""
    rng = random.Random(8)
    prof = dr.consensus_profile(rng, dr.rand_protein(rng, 12), name="c12")
    no_w = [c for c, r in dr.CODON.items() if r not in ("W", "*")]
    seq = "".join(rng.choice(no_w) for _ in range(21844)) + "TGG" + "A"
    assert len(seq) == 65536
    spike = sc.spike(2048, 2048, "w2048")
    _load(gpu_ctx, [seq])
    got = gpu_ctx.dom_ssv([0], [0], [65536], *dr.tables([prof, spike]))
    assert (got[0, 0] == sr.ssv([seq], [prof])[0, 0]).all()
    assert got[0, 1, 0] == dr.entry_score(2048) + 3000      # cell (21844, 2048)


# ---------------------------------------------------------------------------------------------- the command line
def test_cli_with_the_prefilter(gpu_ctx, toy, tmp_path, caplog):
    """-ltr_denovo -ltr_hmm -ltr_dom_prefilter 30 on the toy genome of test_gpu_domains.py: `.ltr.dom.gff3` and
    `.ltr.cls.tsv` are the filtered twin's, byte for byte, and the log has the counts"""
    import io

    from subphaser_amd import domains, ltr
    from test_gpu_domains import planted_world
    from test_gpu_ltrdetect import _cli
    seqs, elements, kinds, profs, text = planted_world(toy)
    hmm = tmp_path / "toy.hmm"
    hmm.write_text(text)
    base, log = _cli(gpu_ctx, toy, seqs, tmp_path / "pre", caplog,
                     ["-ltr_denovo", "-ltr_maxdist", "2600", "-ltr_hmm", str(hmm), "-ltr_dom_prefilter", "30"])
    P = domains.read_hmm(str(hmm))
    twins = [dr.make_profile(M, P.emis[a:a + M], P.trans[a:a + M], entry=e, name=n) for M, a, e, n in zip(P.M, P.moff.tolist(), P.entry.tolist(), P.names)]
    recs = ltr.read_scn(base + ".ltr.scn")
    ival = [domains.inner_interval(r) for r in recs]
    hits, items, passed = sr.search([seqs[r.seq_id][a:b] for r, (a, b) in zip(recs, ival)], twins, 30 * 256)
    doms = domains.best_domains([r.id for r in recs], [b - a for a, b in ival], hits, P)
    gff, cls = io.StringIO(), io.StringIO()
    domains.write_gff(gff, doms)
    domains.write_cls(cls, domains.classify(doms))
    assert open(base + ".ltr.dom.gff3").read() == gff.getvalue() and open(base + ".ltr.cls.tsv").read() == cls.getvalue()
    assert len(doms) >= 8 and 0 < passed < items // 10      # (30 bits: a random frame of some 800 residues against 40 nodes reaches them about once in 2^30 / 32000)
    assert any(m.endswith("; ungapped prefilter at 30.0 bits: %d of %d (frame, profile) pairs (%.2f%%) searched" % (passed, items, 1e2 * passed / items))
               for m in log)
