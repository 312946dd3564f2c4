"""GPU: every grid-capped kernel at several passes per workgroup.

The capped launches size their grids from the context's compute-unit count and walk the work in a grid-stride loop.
On 256 compute units the second pass of k5_map or k0_pack begins at 134 Mb, far above what an oracle follows.  A
context created under SP_CU_LIMIT=n (sp_culimit.h) reckons with n compute units, so every capped kernel takes several
passes on the 1.5 / 3.3 Mb genomes of tests/cu_limit_cases.py.  No output depends on the count: every result here is
compared with `==` against the CPU oracle (or the Python twin), and against the unlimited session context on the same
input, which tells a defect of a later pass from a defect the input alone shows.

Limits: 1 (the most passes; `n_cu / 2` workgroups is none there, which c2_hist_sample's launch clamps) and 3 (odd: the
`/ 2` of the sample histogram and the `* per_cu / n` of the batched chain do not divide evenly).  The whole file takes
about 11 s on an MI355X.

Proof that the later passes ran: after each stage the limited context's prof_report() gives the largest grid per kernel
name.  For k0_pack, k5_map, kv_cover and kv_count the work is computed from the input and must be >= 2 * grid + 1 (some
workgroup takes three passes).  For every other capped kernel the grid must equal FACTOR x limit, the factor read off
its launch site, and be smaller than the grid the same call records on the unlimited context: the cap bound, and the
work exceeded it.

    kernel (launch site)                          factor x limit       work on the input (limit 1 / 3)      shown
    k0_pack (sp_ctx.hip genome_add_impl)          64                   130 / 386 tiles of 256 mask words    >= 3 passes
    k1_count_atomic (sp_count.hip:243 grid_for)   16                   41 / 101 blocks of 256 units         >= 2 passes
    k1_narrow (sp_count.hip:592)                  8                    1024 (k = 13) / 2048 buckets         >= 3 passes
    c2_hist_sample (sp_count2.hip:1548)           max(1, limit / 2)    3 / 7 sampled tiles                  >= 3 passes
    c2_hist_fine (sp_count2.hip:1548, exact)      2                    41 / 101 tiles                       >= 3 passes
    c2_part1 (sp_count2.hip:1544)                 8                    41 / 101 tiles of 16 384 starts      >= 3 passes
    c2_part2 (sp_count2.hip:1562)                 8                    2048 or more provisioned tiles       >= 3 passes
    c2_count16 (sp_count2.hip:1598)               2                    1024 / 16 384 buckets (k = 13 / 15)  >= 3 passes
    batched chain (sp_count2.hip:1713 cap_grid)   ceil(limit * per_cu / 3) x 3 chromosomes, per_cu = 2, 8, 8 for
      c2_hist_sample, c2_part1, c2_part2                               3 / 7, 41 / 101, 683 or more tiles   >= 2 passes
    s3_hist1 (sp_sparse2.hip:1742)                8                    81 / 201 blocks of 256 units         >= 3 passes
    s3_part1 (sp_sparse2.hip:1805)                8                    41 / 101 tiles (81 / 201 at k = 22)  >= 3 passes
    s3_hist2_sample (sp_sparse2.hip:1813)         8                    1104 / 1223 tiles at most            >= 2 passes
    s3_part2 (sp_sparse2.hip:1824)                16                   1104 / 1223 tiles at most            >= 2 passes
    s3_final_bitmap, s3_final_hash (:1842)        64                   262 144 / 524 288 buckets (k 17/22)  >= 3 passes
    s3_final (sp_sparse2.hip:1860)                8                    the same buckets                     >= 3 passes
    s3_gather (sp_sparse2.hip:1995)               32                   a block for every four buckets       >= 3 passes
    sps_keygen (sp_sparse.hip:872)                16                   41 / 101 blocks of 256 units         >= 2 passes
    sps_join (sp_listfilter.hip:1105)             16                   32 / 64 key ranges                   >= 2 passes
    sps_join_wide (sp_listfilter.hip:1105)        16                   64 / 256 key ranges of 130 lists     >= 3 passes
    sps_bounds (sp_listfilter.hip:1199)           16 x 130 lists       576 / 2071 blocks a list             >= 3 passes
    row plan (sp_listplan.h, :1230/1270)          the slack of 16 x limit chunks is no grid: the rows are compared
    k5_map (sp_map.h map_grid, :980)              16                   47 / 104 ranges of 32 768 starts     >= 3 passes
    k5_map_lab (map_grid, sp_map.hip:1004)        16                   21 / 51 ranges of chromosome 0       >= 2 passes
    k5_map_sparse(_lab) (sp_sparse.hip:992)       16                   21 / 51 ranges of chromosome 0       >= 2 passes
    k5_map_feat(_lab) (sp_map.hip:1016)           16                   35 / 71 ranges of features           >= 2 passes
    k5_map_feat_sparse(_lab) (sp_sparse.hip:1014) 16                   36 / 75 ranges of features           >= 2 passes
    k5_map_mask(_lab) (sp_map.hip:1039)           16                   21 / 51 ranges of chromosome 0       >= 2 passes
    k5_map_mask_sparse(_lab) (sp_sparse.hip:1075) 16                   21 / 51 ranges of chromosome 0       >= 2 passes
    kv_cover, kv_count (sp_map.hip:1452)          32                   200 / 400 blocks of 4 intervals      >= 3 passes
    k4_ctab_seen, k4_pair_seen (sp_map.hip:1064)  4                    7261 / 12 749 labels, 256 a block    >= 3 passes
    k4_count_seen (sp_map.hip:1073)               8                    the label table of 2^29 slots        >= 3 passes
    sq_seen, sps_pair_seen (sp_sparse.hip:1099)   4                    7154 / 12 255 labels, 256 a block    >= 3 passes
    sps_count_seen (sp_sparse.hip:1108)           4                    the hash table's entries             >= 3 passes
    sps_pair_init (sp_sparse.hip:972)             8                    the hash table's entries             >= 3 passes
    bk_count, bk_build, bk_anchors (:293 bk_grid) 8                    18 / 52 blocks of 256 units          >= 2 passes
    bk_singles (sp_blocks.hip:293 bk_grid)        8                    214 / 621 blocks of index entries    >= 3 passes
    bk_pair (sp_blocks.hip:441)                   16                   141 / 421 windows                    >= 3 passes
    synth_fill (sp_synth.hip:113)                 32                   259 / 777 blocks of 4096 bases       >= 3 passes

(The work of the kernels that are checked by grid alone is the grid the unlimited context records, its cap of 256 x
factor being far away.)

Not covered -- these never reach their cap here, or no stage of this file calls them:
    k3_slow (sp_filter.hip:878): the dense filter's slow queue stays empty on these genomes;
    kx_merge, kx_lengths (sp_count.hip:840/868): the multi-GPU table exchange (test_gpu_table_exchange.py);
    k4_label_max (sp_map.hip:1152): one workgroup below 65 536 labels;
    c2_count (sp_count2.hip:1565): runs only under SP_C2_COUNT16=0;
    c2_count_list (sp_count2.hip:1579/1733): at most 256 buckets a workgroup, which sets its grid above the cap;
    s3_hist1_sample, s3_hist2, s3_final_small (the sites of s3_hist1, s3_hist2_sample and s3_final_bitmap under other
    names): chromosomes long enough to sample, SP_S3_EXACT=1, SP_S3_FINAL=sort (s3_hist2 and s3_final_small run, below
    their caps, in test_gpu_sparse_paths.py: every small case under SP_S3_EXACT=1, the sort_size_classes cases)."""
import contextlib

import numpy as np
import pytest

import blocks_ref as br
import cu_limit_cases as cc
import test_gpu_blocks as tb

pytestmark = pytest.mark.gpu

LIMITS = cc.LIMITS


def _batch(per_cu):
    """cap_grid of the batched list count: ceil(limit * per_cu / n) workgroups for each of the genome's 3 chromosomes"""
    return lambda limit: -(-limit * per_cu // 3) * 3


# kernel name -> workgroups per compute unit at its capped launch site (a callable: the grid of `limit` units)
FACTOR = {
    "k0_pack": 64,
    "k1_count_atomic": 16, "k1_narrow": 8,
    "c2_hist_sample": lambda limit: max(1, limit // 2), "c2_hist_fine": 2, "c2_part1": 8, "c2_part2": 8, "c2_count16": 2,
    "s3_hist1": 8, "s3_part1": 8, "s3_hist2_sample": 8, "s3_part2": 16, "s3_final_bitmap": 64, "s3_final_hash": 64,
    "s3_final": 8, "s3_gather": 32, "sps_keygen": 16,
    "sps_join": 16, "sps_join_wide": 16, "sps_bounds": 16 * 130,      # (sps_bounds: x 130 lists in grid.y, test_filter_wide)
    "k5_map": 16, "k5_map_lab": 16, "k5_map_sparse": 16, "k5_map_sparse_lab": 16,
    "k5_map_feat": 16, "k5_map_feat_lab": 16, "k5_map_feat_sparse": 16, "k5_map_feat_sparse_lab": 16,
    "k5_map_mask": 16, "k5_map_mask_lab": 16, "k5_map_mask_sparse": 16, "k5_map_mask_sparse_lab": 16,
    "kv_cover": 32, "kv_count": 32,
    "k4_ctab_seen": 4, "k4_pair_seen": 4, "k4_count_seen": 8, "sq_seen": 4, "sps_pair_seen": 4, "sps_count_seen": 4,
    "sps_pair_init": 8,
    "bk_count": 8, "bk_build": 8, "bk_singles": 8, "bk_anchors": 8, "bk_pair": 16,
    "synth_fill": 32,
}
# the batched chain of count engine 3 launches under the names of the per-chromosome chain
FACTOR_BATCH = {"c2_hist_sample": _batch(2), "c2_part1": _batch(8), "c2_part2": _batch(8)}


@contextlib.contextmanager
def limited(monkeypatch, limit):
    """a context of its own that reckons with `limit` compute units (the switch is read at creation only)"""
    from subphaser_amd import _native
    monkeypatch.setenv("SP_CU_LIMIT", str(limit))
    ctx = _native.Context(0)
    monkeypatch.delenv("SP_CU_LIMIT")
    try:
        yield ctx
    finally:
        ctx.close()


def profiled(ctx, stage):
    """stage(ctx) and the largest grid per kernel name it launched"""
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        out = stage(ctx)
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    return out, {name: int(e["grid"]) for name, e in rep.items()}


def same(a, b, where=""):
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (where, a.shape, b.shape)
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), (where, np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).ravel())[:5])
        else:
            assert (a == b).all(), (where, np.flatnonzero((a != b).ravel())[:5])
    else:
        assert a == b, (where, a, b)


def both(gpu_ctx, lim_ctx, stage):
    """the stage on the limited context and on the session context: the limited results (equal to the unlimited ones)
    and the two grid tables"""
    got, g_lim = profiled(lim_ctx, stage)
    ref, g_full = profiled(gpu_ctx, stage)
    same(got, ref, "limited vs unlimited")
    return got, g_lim, g_full


def capped(limit, g_lim, g_full, names, factor=FACTOR, work=None):
    """every kernel of `names` ran at FACTOR x limit workgroups, fewer than on the unlimited context; `work`: kernel
    name -> work items, each >= 2 * grid + 1"""
    print("limit %d grids (limited / unlimited): %s" % (limit, {n: (g_lim.get(n), g_full.get(n)) for n in sorted(set(g_lim) | set(g_full))}))
    bad = []
    for name in names:
        f = factor[name]
        want = f(limit) if callable(f) else f * limit
        if g_lim.get(name) != want or not g_full.get(name, 0) > want:
            bad.append((name, "limited", g_lim.get(name), "want", want, "unlimited", g_full.get(name)))
    for name, items in (work or {}).items():
        if not items >= 2 * g_lim.get(name, 1 << 60) + 1:
            bad.append((name, "work", items, "grid", g_lim.get(name)))
    assert not bad, bad


def load(ctx, seqs):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)


def count_dump(ctx, seqs, k, engine):
    """as test_gpu_parity's _count_both, without its oracle run: the dumps and lengths()"""
    load(ctx, seqs)
    ctx.count(k, cc.LOWER, engine)
    return [tuple(np.array(x) for x in ctx.dump(i)) for i in range(len(seqs))], np.array(ctx.lengths())


def check_counts(got, limit, k):
    dumps, lens = got
    exp = cc.counts(limit, k)
    same(dumps, [tuple(e) for e in exp], "dump vs oracle")
    assert lens.tolist() == [int(c.astype(np.int64).sum()) for _, c in exp]


# ---------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("limit", LIMITS)
def test_pack(gpu_ctx, monkeypatch, limit):
    """genome_add, genome_add_device from a 16-byte aligned and from an odd address, genome_unpack: numpy's answer.
    k0_pack: mask words / 256 >= 2 * grid + 1."""
    s = cc.pack_seq(limit)
    exp = cc.unpacked(s)

    def stage(ctx):
        d = ctx.dev_alloc(s.size + 16)
        try:
            ctx.host_to_dev(d, s)
            ctx.genome_reset(3)
            ctx.genome_add(0, s[5:])
            ctx.genome_add_device(1, d, s.size)
            ctx.genome_add_device(2, d + 1, s.size - 1)
            return [np.array(ctx.genome_unpack(i)) for i in range(3)]
        finally:
            ctx.sync()
            ctx.dev_free(d)

    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    same(got, [exp[5:], exp, exp[1:]], "unpack vs numpy")
    tiles = ((s.size + 31) // 32 + 8 + 255) // 256
    capped(limit, g_lim, g_full, ["k0_pack"], work={"k0_pack": tiles})


# --------------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("k,engine,exact", [(13, 1, 0), (15, 1, 0), (13, 2, 0), (15, 2, 0), (15, 2, 1), (13, 3, 0), (15, 3, 0)])
def test_dense_count(gpu_ctx, monkeypatch, limit, k, engine, exact):
    """engines 1, 2, 3 at k = 13 and 15, engine 2 once from the exact histogram (SP_C2_EXACT=1): po.count, lengths()"""
    seqs = cc.genome(limit)
    if exact:
        monkeypatch.setenv("SP_C2_EXACT", "1")
    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, lambda ctx: count_dump(ctx, seqs, k, engine))
    check_counts(got, limit, k)
    if engine == 1:
        capped(limit, g_lim, g_full, ["k1_count_atomic", "k1_narrow"])
    elif engine == 2:
        capped(limit, g_lim, g_full, ["c2_hist_fine" if exact else "c2_hist_sample", "c2_part1", "c2_part2", "c2_count16"])
    else:
        capped(limit, g_lim, g_full, list(FACTOR_BATCH), factor=FACTOR_BATCH)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("k,engine", [(17, 0), (22, 0), (17, 1)])
def test_sparse_count(gpu_ctx, monkeypatch, limit, k, engine):
    """the partition engine at k = 17 and 22 (u32 / u64 residuals) and the sort engine at k = 17: po.count"""
    seqs = cc.genome(limit)
    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, lambda ctx: count_dump(ctx, seqs, k, engine))
    check_counts(got, limit, k)
    if engine == 1:
        capped(limit, g_lim, g_full, ["sps_keygen"])
    else:
        capped(limit, g_lim, g_full, ["s3_hist1", "s3_part1", "s3_hist2_sample", "s3_part2",
                                      "s3_final_bitmap" if k == 17 else "s3_final_hash", "s3_final", "s3_gather"])


# --------------------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("k,list_engine", [(15, "0"), (15, "1"), (17, "1")])
def test_filter(gpu_ctx, monkeypatch, limit, k, list_engine):
    """the dense filter (byte tables) and the list filter at k = 15, the list filter at k = 17: keys, counts, freqs,
    tot and the fold-passing histogram of OracleContext.filter"""
    seqs = cc.genome(limit)
    monkeypatch.setenv("SP_LIST_ENGINE", list_engine)

    def stage(ctx):
        load(ctx, seqs)
        ctx.count(k, cc.LOWER, 0)
        return cc.run_filter(ctx)

    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    exp = cc.filtered(limit, k)
    assert exp[0][1] > 3000
    same(got, exp, "filter vs oracle")
    capped(limit, g_lim, g_full, ["sps_join"] if list_engine == "1" else [])


@pytest.mark.parametrize("limit", LIMITS)
def test_filter_wide(gpu_ctx, oracle_ctx, monkeypatch, limit):
    """130 chromosomes at k = 17 (sps_join_wide, and the row plan with the slack of 16 x limit chunks)"""
    import test_gpu_wide_join as tw
    seqs = cc.wide_genome(limit)
    C = len(seqs)
    sgs, baseline = tw.layouts(C)["two_units_b1"]

    def stage(ctx):
        tw._load(ctx, seqs, 17)
        return tw._filter(ctx, sgs, C, baseline)

    exp = stage(oracle_ctx)
    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    assert exp[0][1] >= 100
    tw._same(got, exp)
    capped(limit, g_lim, g_full, ["sps_join_wide", "sps_bounds"])


# --------------------------------------------------------------------------------------------------- labels + map
def map_stage(seqs, limit, k, S, device_labels):
    keys, sg = cc.labels(limit, k, S)

    def stage(ctx):
        load(ctx, seqs)
        ctx.count(k, cc.LOWER, 0)
        if not device_labels:
            ctx.labels_set(keys, sg, S)
            return cc.run_map(ctx, len(seqs))
        d_keys, d_sg = ctx.dev_alloc(keys.size * 8), ctx.dev_alloc(sg.size)
        try:
            ctx.host_to_dev(d_keys, keys)
            ctx.host_to_dev(d_sg, sg)
            ctx.labels_set_device(d_keys, d_sg, keys.size, S)
            return cc.run_map(ctx, len(seqs))
        finally:
            ctx.sync()
            ctx.dev_free(d_keys)
            ctx.dev_free(d_sg)
    return stage


MAP_KERNELS = {   # (k, S) -> the capped kernels of map_bins / map_bins_all / labels_hit
    (15, 3): ["k5_map", "k4_ctab_seen"], (15, 5): ["k5_map", "k4_pair_seen"], (15, 9): ["k5_map_lab", "k4_count_seen"],
    (17, 3): ["k5_map_sparse", "sq_seen"], (17, 5): ["k5_map_sparse", "sps_pair_seen", "sps_pair_init"],
    (17, 9): ["k5_map_sparse_lab", "sps_count_seen"],
}


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("k,S,device_labels", [(15, 3, False), (15, 5, True), (15, 9, False), (17, 3, True), (17, 5, False), (17, 9, False)])
def test_labels_and_map(gpu_ctx, monkeypatch, limit, k, S, device_labels):
    """labels_set / labels_set_device, then map_bins of every chromosome and map_bins_all at (10000, 10 000 000),
    (333, 50 000) and (64, 0) with S = 3 (compact / quad-bucket table), 5 (direct / hash table) and 9 (label-table
    engine): the oracle's bins, n_mapped per chromosome, labels_hit().  k5_map: ranges >= 2 * grid + 1."""
    seqs = cc.genome(limit)
    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, map_stage(seqs, limit, k, S, device_labels))
    exp = cc.mapped(limit, k, S)
    assert 0 < exp[-1] < cc.labels(limit, k, S)[0].size and all(int(n) > 1000 for n in exp[3][1])
    same(got, exp, "map vs oracle")
    ranges = sum((-(-n // 64) + 511) // 512 for n in cc.LENGTHS[limit])
    capped(limit, g_lim, g_full, MAP_KERNELS[(k, S)], work={"k5_map": ranges} if "k5_map" in MAP_KERNELS[(k, S)] else None)


# ------------------------------------------------------------------------------------------ features / intervals
FEATURE_KERNELS = {
    (15, 3): ["k5_map_feat", "k5_map_mask"], (15, 9): ["k5_map_feat_lab", "k5_map_mask_lab"],
    (17, 3): ["k5_map_feat_sparse", "k5_map_mask_sparse"], (17, 9): ["k5_map_feat_sparse_lab", "k5_map_mask_sparse_lab"],
}


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("k,S", sorted(FEATURE_KERNELS))
def test_features_and_intervals(gpu_ctx, monkeypatch, limit, k, S):
    """800 / 1600 features cut from all three chromosomes (1 .. 10 000 bases, some below k, some overlapping) through
    map_features_cat, and as map_intervals with their real chromosome indices: the oracle's totals and labels_hit().
    kv_cover / kv_count: blocks of four intervals >= 2 * grid + 1."""
    seqs = cc.genome(limit)

    def stage(ctx):
        load(ctx, seqs)
        ctx.count(k, cc.LOWER, 0)
        return cc.run_features(ctx, limit, k, S)

    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    exp = cc.featured(limit, k, S)
    assert int(exp[0].sum()) > 10000 and len(set(cc.features(limit, k)[0].tolist())) == 3
    same(got, exp, "features vs oracle")
    blocks = (cc.features(limit, k)[0].size + 3) // 4
    capped(limit, g_lim, g_full, FEATURE_KERNELS[(k, S)] + ["kv_cover", "kv_count"], work={"kv_cover": blocks, "kv_count": blocks})


# -------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("k", [15, 17])
def test_windows(gpu_ctx, monkeypatch, limit, k):
    """stack_windows and stack_enrich behind a multi-pass map_bins_all: the oracle's window table and calls (p-values
    and ratios within the 1e-6 of the suite's enrichment tests against the oracle, `==` against the unlimited context)"""
    seqs = cc.genome(limit)

    def stage(ctx):
        load(ctx, seqs)
        ctx.count(k, cc.LOWER, 0)
        return cc.run_windows(ctx, limit, k, 3)

    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    win, woff, (e_win, e_woff, pvals, argmin, sig, ratios) = got
    o_win, o_woff, (_, _, o_p, o_arg, o_sig, o_ratios) = cc.windowed(limit, k, 3)
    same((win, woff, e_win, e_woff), (o_win, o_woff, o_win, o_woff), "windows vs oracle")
    assert int(o_sig.sum()) > 10
    nz = win.any(axis=1)
    assert np.abs(pvals[nz] - o_p[nz]).max() <= 1e-6
    assert (argmin[nz] == o_arg[nz]).all() and (sig.astype(bool)[nz] == o_sig[nz]).all()
    assert np.allclose(ratios[nz], o_ratios[nz], rtol=1e-9, atol=0, equal_nan=True)
    capped(limit, g_lim, g_full, ["k5_map" if k == 15 else "k5_map_sparse"])


# --------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("limit", LIMITS)
def test_blocks(gpu_ctx, monkeypatch, limit):
    """blocks_index and blocks_pair on a homoeologous pair of 140 003 x limit bases, bin = 1000 (141 / 421 windows for
    16 x limit workgroups): the index tallies, anchors and vote arrays of tests/blocks_ref.py"""
    a, b = cc.blocks_pair(limit)
    kb, s, bin_size = 21, 2, 1000
    ref = tb.twin("cu_limit_%d" % limit, a, b, kb, s, bin_size)
    idx = [br.index(seq, kb, s)[1] for seq in (a, b)]

    def stage(ctx):
        tb.load(ctx, [a, b])
        try:
            tallies = [ctx.blocks_index(i, kb, s) for i in range(2)]
            return tallies, [np.array(x) for x in tb.check_pair(ctx, 0, 1, ref, kb, s, bin_size)]
        finally:
            ctx.blocks_release()

    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    assert got[0] == idx
    assert len(ref[1]) >= 2 * 16 * limit + 1
    capped(limit, g_lim, g_full, ["bk_count", "bk_build", "bk_singles", "bk_anchors", "bk_pair"], work={"bk_pair": len(ref[1])})


# ---------------------------------------------------------------------------------------------------------- synth
@pytest.mark.parametrize("limit", LIMITS)
def test_synth(gpu_ctx, monkeypatch, limit):
    """synth_chrom of 1 060 003 x limit bases: the generator has no host twin, so the bytes of the unlimited context"""
    n = 1_060_003 * limit

    def stage(ctx):
        d = ctx.dev_alloc(n)
        try:
            ctx.synth_chrom(d, n, seed=11, set_id=1, sg_id=1, n_sg=3, chrom_id=2)
            return np.array(ctx.dev_to_host(d, n))
        finally:
            ctx.sync()
            ctx.dev_free(d)

    with limited(monkeypatch, limit) as lim:
        got, g_lim, g_full = both(gpu_ctx, lim, stage)
    assert got.size == n and len(np.unique(got)) >= 4
    capped(limit, g_lim, g_full, ["synth_fill"], work={"synth_fill": ((n + 15) // 16 + 255) // 256})
