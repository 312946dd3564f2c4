"""The four map modes of the device -- bins, windows, features, intervals -- against the positional reference
(tests/mappos_ref.py: plain numpy over the label of every start, chunks walked one by one), on the small genome and
the geometries of tests/mappos_cases.py.  Equal, never close.  tests/test_mappos_host.py shows on the CPU that the
reference and the oracle agree on the same cases.

Every test reads prof_report() and asserts that the kernels named for its (k, S) ran.  The last tests are the refusals
of the entries: each is followed by a good call that still gives the reference's numbers.  The stale-table refusals use
only mismatches that stay inside every table when the entry does not refuse (a smaller bin, chunks where none were
mapped, fewer slots, fewer subgenomes, fewer or shorter chromosomes): without the refusal they fail by assertion."""
import ctypes

import numpy as np
import pytest

import mappos_cases as mc
from test_gpu_cu_limit import FEATURE_KERNELS, MAP_KERNELS, profiled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the refusals depend on what the context has been asked before"""
    from subphaser_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


_LOADED = {}


def _load(ctx, k, seqs=None):
    """the genome of the cases (or `seqs`) resident, k fixed by a count"""
    if seqs is None and _LOADED.get(id(ctx)) == k:
        return
    _LOADED[id(ctx)] = k if seqs is None else None
    seqs = mc.genome(k)[0] if seqs is None else seqs
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)
    ctx.count(k, 1, 1)          # (fixes k; the label set is hand-made)


def _ran(grids, names):
    missing = [n for n in names if grids.get(n, 0) < 1]
    assert not missing, (missing, sorted(grids))


def _same(got, exp, where):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (where, got.shape, exp.shape)
    assert (got == exp).all(), (where, np.argwhere(got != exp)[:5])


# ----------------------------------------------------------------------------------------------------------- bins
@pytest.mark.parametrize("k,S", mc.BIN_KS)
def test_bins(ctx, k, S):
    """map_bins per chromosome and map_bins_all at every geometry: counts, shapes, n_mapped, labels_hit"""
    keys, lab = mc.labels(k, S)
    lens = mc.lengths(k)

    def stage(ctx):
        _load(ctx, k)
        ctx.labels_set(keys, lab, S)
        for bin_size, W in mc.bin_geoms(S):
            tabs, n_exp, _ = mc.bins_expected(k, S, bin_size, W)
            for i in range(len(lens)):
                assert ctx.map_nslots(i, bin_size, W) == tabs[i].shape[0], (bin_size, W, i)
                got, n = ctx.map_bins(i, bin_size, W)
                _same(got, tabs[i], ("map_bins", bin_size, W, i))
                assert n == n_exp[i], (bin_size, W, i)
        seen_each = ctx.labels_hit()
        ctx.labels_set(keys, lab, S)
        for bin_size, W in mc.bin_geoms(S):
            tabs, n_exp, _ = mc.bins_expected(k, S, bin_size, W)
            got, n = ctx.map_bins_all(bin_size, W)
            assert len(got) == len(tabs)
            for i in range(len(lens)):
                _same(got[i], tabs[i], ("map_bins_all", bin_size, W, i))
            assert n.tolist() == n_exp, (bin_size, W)
        return seen_each, ctx.labels_hit()

    (seen_each, seen_all), grids = profiled(ctx, stage)
    assert seen_each == seen_all == mc.labels_hit_all(k, S)
    _ran(grids, MAP_KERNELS[(k, S)])


# -------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("k,S", mc.WINDOW_KS)
def test_windows(ctx, k, S):
    """stack_windows at every window geometry; stack_enrich: the same table, and its four result arrays byte-equal to
    enrich() of the full table, empty rows included"""
    keys, lab = mc.labels(k, S)
    lens = mc.lengths(k)

    def stage(ctx):
        _load(ctx, k)
        ctx.labels_set(keys, lab, S)
        for bin_size, W, window in mc.WINDOW_GEOMS:
            exp, woff = mc.windows_expected(k, S, bin_size, window)
            ctx.map_bins_all(bin_size, W)
            win, goff = ctx.stack_windows(bin_size, W, window, lens)
            _same(goff, woff, ("win_off", bin_size, W, window))
            _same(win, exp, ("stack_windows", bin_size, W, window))
            res = [np.array(x) for x in ctx.stack_enrich(bin_size, W, window, lens, 0.05, 0.5)]
            _same(res[1], woff, ("win_off of stack_enrich", bin_size, W, window))
            _same(res[0], exp, ("stack_enrich", bin_size, W, window))
            assert (~exp.any(axis=1)).any()                                 # (there are empty rows)
            host = ctx.enrich(exp, 0.05, 0.5)
            for name, a, b in zip(("pvals", "argmin", "sig", "ratios"), res[2:], host):
                b = b.astype(np.uint8) if name == "sig" else b
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, bin_size, W, window)

    _, grids = profiled(ctx, stage)
    _ran(grids, [MAP_KERNELS[(k, S)][0], "k5_stack"])


@pytest.mark.parametrize("multiple", [True, False])
@pytest.mark.parametrize("k,S", mc.WINDOW_KS)
def test_windows_dev(ctx, k, S, multiple):
    """stack_windows_dev with a seg_start (a multiple of the bin / not one) into a table of the caller's, cleared by a
    host copy: one call gives the reference, a second one doubles it"""
    keys, lab = mc.labels(k, S)

    def stage(ctx):
        _load(ctx, k)
        ctx.labels_set(keys, lab, S)
        for bin_size, W, window in mc.WINDOW_GEOMS:
            seg = tuple(mc.seg_starts(bin_size, multiple))
            exp, woff = mc.windows_expected(k, S, bin_size, window, seg)
            ctx.map_bins_all(bin_size, W)
            d = ctx.dev_alloc(exp.nbytes)
            try:
                ctx.host_to_dev(d, np.zeros(exp.shape, np.int64))
                for rep in (1, 2):
                    ctx.stack_windows_dev(bin_size, W, window, woff[:-1], seg, d)
                    got = ctx.dev_to_host(d, exp.nbytes).view(np.int64).reshape(exp.shape)
                    _same(got, rep * exp, ("stack_windows_dev", bin_size, W, window, rep))
            finally:
                ctx.dev_free(d)

    _, grids = profiled(ctx, stage)
    _ran(grids, [MAP_KERNELS[(k, S)][0], "k5_stack"])


# ------------------------------------------------------------------------------------------ features / intervals
@pytest.mark.parametrize("k,S", mc.RANGE_KS)
def test_features_and_intervals(ctx, k, S):
    """the feature list as one buffer, as the same buffer at off[0] = 77 inside a longer one, and as intervals of the
    genome; the interval list, and its sub-sequences as features: the reference, and each other"""
    keys, lab = mc.labels(k, S)
    cat, off, cat77, off77 = mc.feature_buffers(k)
    f_chrom, f_st, f_en, _ = mc.features(k)
    i_chrom, i_st, i_en = mc.intervals(k)
    f_exp, _, f_seen = mc.features_expected(k, S)
    i_exp, i_seen = mc.ranges_expected(k, S, "intervals")
    i_off = np.concatenate(([0], np.cumsum(i_en - i_st))).astype(np.int64)
    i_cat = mc.cut(k, i_chrom, i_st, i_en)

    def stage(ctx):
        _load(ctx, k)
        out = {}
        for name, call in (("features", lambda: ctx.map_features_cat(cat, off)),
                           ("features at off[0] = 77", lambda: ctx.map_features_cat(cat77, off77)),
                           ("features as intervals", lambda: ctx.map_intervals(f_chrom, f_st, f_en)),
                           ("intervals", lambda: ctx.map_intervals(i_chrom, i_st, i_en)),
                           ("intervals as features", lambda: ctx.map_features_cat(i_cat, i_off))):
            ctx.labels_set(keys, lab, S)
            out[name] = (call(), ctx.labels_hit())
        return out

    out, grids = profiled(ctx, stage)
    for name in ("features", "features at off[0] = 77", "features as intervals"):
        _same(out[name][0], f_exp, name)
        assert out[name][1] == f_seen, name
    for name in ("intervals", "intervals as features"):
        _same(out[name][0], i_exp, name)
        assert out[name][1] == i_seen, name
    _ran(grids, (FEATURE_KERNELS.get((k, S)) or mc.RANGE_KERNELS_S5[(k, S)]) + ["kv_cover", "kv_count"])


# ------------------------------------------------------------------------------------------------------- refusals
K, S = 15, 3
GEOM = (100, 0, 250)        # bin, chunk, window (chunk 0: a stack call with a smaller bin stays inside the window table)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _slot_off(ctx, lens, bin_size, W):
    return np.concatenate(([0], np.cumsum([ctx.map_nslots(i, bin_size, W) for i in range(len(lens))]))).astype(np.int64)


def _raw_stack(ctx, entry, bin_size, W, window, off, woff, n_sg):
    """the C entries with slot and window offsets of the caller's own (the wrappers pass what map_bins_all left)"""
    rows = int(woff[-1])
    win = np.zeros((rows, n_sg), np.int64)
    if entry == "sp_stack_windows":
        ctx._ck(ctx.L.sp_stack_windows(ctx.h, bin_size, W, window, _p(off), _p(woff), _p(win)))
    elif entry == "sp_stack_enrich":
        pv, ra = np.empty((rows, n_sg)), np.empty((rows, n_sg))
        am, sig = np.empty(rows, np.int32), np.empty(rows, np.uint8)
        ctx._ck(ctx.L.sp_stack_enrich(ctx.h, bin_size, W, window, _p(off), _p(woff), 0.05, 0.5, _p(win), _p(pv), _p(am),
                                      _p(sig), _p(ra)))
    else:
        d = ctx.dev_alloc(win.nbytes)
        try:
            ctx.host_to_dev(d, win)
            ctx._ck(ctx.L.sp_stack_windows_dev(ctx.h, bin_size, W, window, _p(off), _p(woff), None, ctypes.c_void_p(d)))
            win = ctx.dev_to_host(d, win.nbytes).view(np.int64).reshape(win.shape)
        finally:
            ctx.dev_free(d)
    return win


ENTRIES = ("sp_stack_windows", "sp_stack_enrich", "sp_stack_windows_dev")


def _good(ctx):
    """labels, map_bins_all and the three stack entries at GEOM: the reference's numbers"""
    bin_size, W, window = GEOM
    exp, woff = mc.windows_expected(K, S, bin_size, window)
    ctx.labels_set(*mc.labels(K, S), S)
    got, n = ctx.map_bins_all(bin_size, W)
    tabs, n_exp, seen = mc.bins_expected(K, S, bin_size, W)
    for g, t in zip(got, tabs):
        _same(g, t, "map_bins_all after a refusal")
    assert n.tolist() == n_exp and ctx.labels_hit() == seen
    off = _slot_off(ctx, mc.lengths(K), bin_size, W)
    for entry in ENTRIES:
        _same(_raw_stack(ctx, entry, bin_size, W, window, off, woff, S), exp, entry + " after a refusal")
    return off, woff


def _refused(ctx, what, entry, bin_size, W, window, off, woff, n_sg):
    with pytest.raises(ValueError, match=what):
        _raw_stack(ctx, entry, bin_size, W, window, off, woff, n_sg)


@pytest.fixture(scope="module")
def fresh_ctx():
    """a context that has mapped nothing yet"""
    from subphaser_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def test_stack_needs_map_bins_all(fresh_ctx):
    """a stack entry before any map_bins_all, and after a later map_bins"""
    ctx = fresh_ctx
    bin_size, W, window = GEOM
    _load(ctx, K)
    ctx.labels_set(*mc.labels(K, S), S)
    off = _slot_off(ctx, mc.lengths(K), bin_size, W)
    woff = mc.window_offsets(K, window)
    for entry in ENTRIES:
        _refused(ctx, "call sp_map_bins_all first", entry, bin_size, W, window, off, woff, S)
    _good(ctx)
    ctx.map_bins(1, bin_size, W)
    for entry in ENTRIES:
        _refused(ctx, "call sp_map_bins_all first", entry, bin_size, W, window, off, woff, S)
    _good(ctx)


def test_short_tables_are_refused(ctx):
    """win_off one row short, slot_off one slot short, decreasing feature offsets"""
    bin_size, W, window = GEOM
    _load(ctx, K)
    off, woff = _good(ctx)
    short = woff.copy()
    short[-1] -= 1
    for entry in ("sp_stack_windows", "sp_stack_enrich"):
        _refused(ctx, "chromosome 4 needs %d windows" % (woff[5] - woff[4]), entry, bin_size, W, window, off, short, S)
    _good(ctx)
    short = off.copy()
    short[2:] -= 1            # chromosome 1 one slot short
    out = np.zeros((int(off[-1]), S), np.int32)
    nm = np.zeros(5, np.int64)
    with pytest.raises(ValueError, match="chromosome 1 needs %d slots" % (off[2] - off[1])):
        ctx._ck(ctx.L.sp_map_bins_all(ctx.h, bin_size, W, _p(short), _p(out), _p(nm)))
    exp, _ = mc.windows_expected(K, S, bin_size, window)
    for entry in ENTRIES:     # the call was refused for its arguments: the table of the last good one is still there
        _same(_raw_stack(ctx, entry, bin_size, W, window, off, woff, S), exp, entry + " after a refused map_bins_all")
    _good(ctx)
    cat, f_off, _, _ = mc.feature_buffers(K)
    bad = f_off.copy()
    bad[3], bad[4] = bad[4], bad[3]
    assert bad[4] < bad[3] and bad[-1] == f_off[-1]
    with pytest.raises(ValueError, match="offsets must be non-decreasing"):
        ctx.map_features_cat(cat, bad)
    ctx.labels_set(*mc.labels(K, S), S)
    _same(ctx.map_features_cat(cat, f_off), mc.features_expected(K, S)[0], "features after a refusal")
    _good(ctx)


def test_stale_tables_are_refused(ctx):
    """the stack entries take bin_size, chunk_size, slot_off, n_sg and the genome from the caller and the context: what
    differs from the table map_bins_all left is refused.  (Each mismatch stays inside the tables where it is not.)"""
    bin_size, W, window = GEOM
    lens = mc.lengths(K)
    seqs, _ = mc.genome(K)
    keys, lab = mc.labels(K, S)
    _load(ctx, K)
    # a smaller bin than the map call's
    off, woff = _good(ctx)
    for entry in ENTRIES:
        _refused(ctx, "bin_size 50", entry, 50, W, window, off, woff, S)
    # chunks where none were mapped (a slot's chunk is taken off its bin index: smaller windows, never larger)
    for entry in ENTRIES:
        _refused(ctx, "chunk_size 2000", entry, bin_size, 2000, window, off, woff, S)
    # slot offsets of another geometry (fewer slots a chromosome: inside the table)
    off, woff = _good(ctx)
    for entry in ENTRIES:
        _refused(ctx, "slot_off", entry, bin_size, W, window, _slot_off(ctx, lens, 200, W), woff, S)
    # a label set of fewer subgenomes
    off, woff = _good(ctx)
    ctx.labels_set(keys, np.minimum(lab, 1), 2)
    for entry in ENTRIES:
        _refused(ctx, "call sp_map_bins_all first", entry, bin_size, W, window, off, woff, 2)
    # the genome loaded again with shorter chromosomes, then with fewer
    off, woff = _good(ctx)
    _load(ctx, K, [s[:s.size // 2] for s in seqs])
    for entry in ENTRIES:
        _refused(ctx, "call sp_map_bins_all first", entry, bin_size, W, window, off, woff, S)
    _load(ctx, K)
    off, woff = _good(ctx)
    _load(ctx, K, seqs[:4])
    for entry in ENTRIES:
        _refused(ctx, "call sp_map_bins_all first", entry, bin_size, W, window, off[:5].copy(), woff[:5].copy(), S)
    # a count (it may change k)
    _load(ctx, K)
    off, woff = _good(ctx)
    ctx.count(K, 1, 1)
    for entry in ENTRIES:
        _refused(ctx, "call sp_map_bins_all first", entry, bin_size, W, window, off, woff, S)
    _good(ctx)
