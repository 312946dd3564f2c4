"""The list filter (csrc/sp_listfilter.hip: sps_join_blk, sps_join_wide, the sort cross-check, the row-staging retry
of sps_filter_join) on hand-made lists through sp_sparse_view, and k3_eval on the same rows through sp_filter_view:
fold decisions on, next to and far from the threshold in both length regimes, 32-bit count sums, tot and include /
n_multi on their bounds, keys on the range edges, ranges of hundreds of rounds, every entry a row, stranded chunks and
the second pass of the row staging.  Every output is compared with listfilter_ref.filter with `==`; what the inputs
cover is asserted in test_listfilter_ref.py."""
import contextlib
import functools

import numpy as np
import pytest

import listfilter_cases as lc
import listfilter_ref as lr

pytestmark = pytest.mark.gpu

N_MATRIX = 20000
N_WIDE = 6000        # rows of the matrix at C = 65 / 130 (the Python reference walks up to 50 sets per row)


# ------------------------------------------------------------------ plumbing
@contextlib.contextmanager
def sparse_view(ctx, lists, lengths, k):
    """the context counted at k over C one-line chromosomes, the lists uploaded and installed as the view"""
    C = len(lists)
    ctx.genome_reset(C)
    for c in range(C):
        ctx.genome_add(c, b"ACGTTGCATGCAACGGTCATGCATCGATACCGTAGGCT")
    ctx.count(k, 1, 0)
    bufs, pk, pc = [], [], []
    try:
        for keys, cnts in lists:
            dk, dc = ctx.dev_alloc(max(len(keys), 1) * 8), ctx.dev_alloc(max(len(keys), 1) * 4)
            bufs += [dk, dc]
            if len(keys):
                ctx.host_to_dev(dk, np.ascontiguousarray(keys, np.uint64))
                ctx.host_to_dev(dc, np.ascontiguousarray(cnts, np.uint32))
            pk.append(dk), pc.append(dc)
        ctx.sparse_view(pk, pc, [len(x) for x, _ in lists], lengths, k, 1)
        try:
            yield
        finally:
            ctx.sparse_view(None, None, None, None, 0, 0)
    finally:
        for d in bufs:
            ctx.dev_free(d)


def run_filter(ctx, sgs, C, kw):
    from subphaser_amd.config import sets_to_csr
    nu, nr, nh = ctx.filter(*sets_to_csr(sgs, list(range(C))), kw["min_fold"], kw["baseline"], kw["min_freq"],
                            kw["max_freq"], kw["ratio"])
    keys, counts, freqs, tot = ctx.filter_fetch(nr, sort=False)
    return nu, nr, nh, keys, counts, freqs, tot, np.sort(ctx.filter_hist(nh))


def same(got, ref, what=""):
    nu, nr, nh, keys, counts, freqs, tot, hist = got
    n_union, rkeys, rcounts, rtot, rhist, rfreqs = ref
    assert (nu, nr, nh) == (n_union, len(rkeys), len(rhist)), (what, nu, nr, nh, n_union, len(rkeys), len(rhist))
    assert (keys == rkeys).all(), what
    assert (tot == rtot).all(), what
    assert (hist == rhist).all(), what
    assert counts.shape == rcounts.shape and (counts == rcounts).all(), what
    assert freqs.shape == rfreqs.shape and (freqs == rfreqs).all(), what


PATHS = {"walk": {}, "generic": {"SP_JOIN_GENERIC": "1"}, "sort": {"SP_LIST_FILTER": "sort"}}


def set_path(monkeypatch, path):
    for name in ("SP_JOIN_GENERIC", "SP_LIST_FILTER"):
        monkeypatch.delenv(name, raising=False)
    for name, v in PATHS[path].items():
        monkeypatch.setenv(name, v)


def join_calls(ctx, fn):
    """fn() with the profiler on -> (its result, launches per kernel label)"""
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        out = fn()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    return out, {name: v["calls"] for name, v in rep.items()}


def device_cu_count():
    """multiProcessorCount of device 0, what sp_ctx_create sizes the row staging's slack with, asked of the HIP runtime
    the library is linked against (through the library's own handle: one runtime in the process)"""
    import ctypes
    from subphaser_amd import _native
    v = ctypes.c_int(0)
    rc = _native.load().hipDeviceGetAttribute(ctypes.byref(v), 63, 0)      # 63: hipDeviceAttributeMultiprocessorCount
    assert rc == 0 and 0 < v.value <= 4096, (rc, v.value)
    return v.value


# ------------------------------------------------------------------ a. the threshold matrix
@functools.lru_cache(maxsize=None)
def matrix(C, regime):
    if C == 12:
        return lc.threshold_matrix(12, regime, N_MATRIX, seed=1)
    return lc.threshold_matrix(C, regime, N_WIDE, seed=C, fill=0.05)


@functools.lru_cache(maxsize=None)
def matrix_lists(C, regime, k):
    mat, lengths = matrix(C, regime)
    return lc.lists_of(lc.random_keys(len(mat), k, seed=5 + k), mat)


_memo = {}


@functools.lru_cache(maxsize=None)
def matrix_ref(C, regime, k, argset):
    """-> sgs, kw, listfilter_ref.filter of the matrix (the fold decisions per distinct row are kept across k)"""
    mat, lengths = matrix(C, regime)
    lists = matrix_lists(C, regime, k)
    memos = _memo.setdefault((C, regime, argset), {})

    def filt(sgs, **kw):
        return lr.filter(lists, lengths, sgs, memo=memos.setdefault(kw["ratio"], {}), **kw)
    sgs, kw = lc.resolve_args(argset, C, filt)
    return sgs, kw, filt(sgs, **kw)


def _argset_id(a):
    return "%s-f%g-b%d-r%s_%s-%s" % (a[0], a[1], a[2], a[3][0], a[3][1], a[4])


@pytest.mark.parametrize("argset", lc.ARGSETS_12, ids=_argset_id)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("regime", ["long", "short"])
@pytest.mark.parametrize("k", [17, 32])
def test_threshold_matrix(gpu_ctx, monkeypatch, k, regime, path, argset):
    """C = 12 (sps_join_blk): the fast fp32 walk with its fp64 band, the generic decision for every k-mer, the sort
    cross-check; structure b2 (baseline 2) and `many` (132 walk descriptors) take generic decisions on their own.
    k = 17: 32-bit residuals, k = 32: 64-bit ones."""
    _, lengths = matrix(12, regime)
    lists = matrix_lists(12, regime, k)
    _, shift = lc.plan_ranges(sum(len(x) for x, _ in lists), 12, k)
    assert (shift <= 31) == (k == 17)
    sgs, kw, ref = matrix_ref(12, regime, k, argset)
    set_path(monkeypatch, path)
    with sparse_view(gpu_ctx, lists, lengths, k):
        same(run_filter(gpu_ctx, sgs, 12, kw), ref, (k, regime, path, argset))
    assert len(ref[1]) > 20


@pytest.mark.parametrize("argset", lc.ARGSETS_WIDE, ids=_argset_id)
@pytest.mark.parametrize("C,k,regime,path", [(65, 17, "long", "walk"), (130, 32, "short", "walk"),
                                             (65, 32, "short", "generic")])
def test_threshold_matrix_wide(gpu_ctx, monkeypatch, C, k, regime, path, argset):
    """the same rows block by block at C = 65 and C = 130 (sps_join_wide; at 130 structure s5 has 50 sets of two or
    more units: no set screen)"""
    _, lengths = matrix(C, regime)
    lists = matrix_lists(C, regime, k)
    sgs, kw, ref = matrix_ref(C, regime, k, argset)
    set_path(monkeypatch, path)
    with sparse_view(gpu_ctx, lists, lengths, k):
        got, calls = join_calls(gpu_ctx, lambda: run_filter(gpu_ctx, sgs, C, kw))
    assert calls.get("sps_join_wide") == 1 and "sps_join" not in calls, calls
    same(got, ref, (C, k, regime, path, argset))
    assert len(ref[1]) > 20


# ------------------------------------------------------------------ b. keys and ranges
@pytest.mark.parametrize("C,k", [(12, 17), (12, 32), (65, 21)])
def test_edge_keys(gpu_ctx, monkeypatch, C, k):
    """key 0, the largest legal key, neighbours across every possible range edge, empty lists, one list with every key"""
    lists, _ = lc.edge_keys(k, C, seed=k)
    lengths = lc.lengths_for(C, "short")
    sgs = lc.structures(C)["s5"]
    kw = dict(min_fold=2.0, baseline=1, min_freq=5.0, max_freq=1e9, ratio=0.4)
    ref = lr.filter(lists, lengths, sgs, **kw)
    with sparse_view(gpu_ctx, lists, lengths, k):
        for path in PATHS:
            if path == "sort" and C > 64:
                continue
            set_path(monkeypatch, path)
            same(run_filter(gpu_ctx, sgs, C, kw), ref, (C, k, path))
        # with the bounds open and ratio 0 every key is a row: 0 and the largest key come back in their places
        set_path(monkeypatch, "walk")
        allrows = run_filter(gpu_ctx, sgs, C, lc.ROWS_KW)
        same(allrows, lr.filter(lists, lengths, sgs, **lc.ROWS_KW), (C, k, "all rows"))
        assert allrows[3][0] == 0 and int(allrows[3][-1]) == lc.key_max(k)


@pytest.mark.parametrize("C,k,wide_bits", [(4, 21, False), (4, 32, True), (65, 32, True)])
def test_skew_one_range(gpu_ctx, monkeypatch, C, k, wide_bits):
    """200 000 keys that share their top 24 bits: one range worked off in hundreds of rounds, the others empty"""
    n = 200000
    keys = lc.skew_keys(n, k, seed=4)
    if C == 4:       # both pairs hold every key: 800 000 entries (k = 21: 2^11 ranges, 31-bit residuals)
        mat = np.hstack([lc.pair_matrix(n, 2, seed=4), lc.pair_matrix(n, 2, seed=5)])
    else:
        mat = lc.pair_matrix(n, C, seed=4)
    lists = lc.lists_of(keys, mat)
    rb, shift = lc.plan_ranges(int((mat > 0).sum()), C, k)
    assert (shift > 31) == wide_bits and len(set((keys >> np.uint64(shift)).tolist())) == 1 and rb >= 8
    lengths, sgs = lc.lengths_for(C, "long"), lc.pair_sets(C)
    kw = dict(lc.ROWS_KW, ratio=0.5 if C == 4 else 1 / len(sgs), min_freq=12.0 if C == 4 else 7.0)
    ref = lr.filter(lists, lengths, sgs, vec=True, **kw)
    assert n // 4 < len(ref[1]) < len(ref[4]) < n
    with sparse_view(gpu_ctx, lists, lengths, k):
        for path in ("walk", "generic"):
            set_path(monkeypatch, path)
            same(run_filter(gpu_ctx, sgs, C, kw), ref, (C, k, path))


# ------------------------------------------------------------------ c. every entry a row
@pytest.mark.parametrize("make", [lc.all_present_case, lc.disjoint_case, lc.fifth_case], ids=lambda f: f.__name__)
@pytest.mark.parametrize("C", [4, 65])
def test_every_entry_a_row(gpu_ctx, monkeypatch, make, C):
    """50 000 keys: in all C lists / in one list each (the row queue of a round and the chunk grabs at their largest),
    and one kept entry in five (half of every chunk of the row staging stranded)"""
    n = 50000
    lists, lengths, sgs, kw = make(n, C, 17, seed=2)
    ref = lr.filter(lists, lengths, sgs, vec=True, **kw)
    assert len(ref[1]) == (n // 5 if make is lc.fifth_case else n)
    set_path(monkeypatch, "walk")
    with sparse_view(gpu_ctx, lists, lengths, 17):
        same(run_filter(gpu_ctx, sgs, C, kw), ref, (make.__name__, C))


# ------------------------------------------------------------------ d. the second pass of the row staging
@pytest.mark.parametrize("variant", ["ratio0", "pairs"])
@pytest.mark.parametrize("C,kernel", [(4, "sps_join"), (65, "sps_join_wide")])
def test_row_staging_second_pass(gpu_ctx, monkeypatch, C, kernel, variant):
    """More kept rows than the staging area is planned for (2^20 + the slack of n_cu * 16 chunks): the join runs twice,
    the second time with the size the first asked for; the same lists with a max_freq that keeps 2^20 - 1000 rows run
    it once.  Compared in full (C = 65: 0.6 GB of counts)."""
    n_cu = device_cu_count()
    rows_kept, rows_control = (1 << 20) + n_cu * 4096 + 200000, (1 << 20) - 1000
    lists, lengths, sgs, kw, kwc = lc.second_pass_case(C, variant, rows_kept, rows_control, 17, seed=3)
    total = sum(len(x) for x, _ in lists)
    assert total < 16 << 20 and lc.row_cap(total, n_cu) == (1 << 20) + n_cu * 4096 < rows_kept
    joined = lr.union(lists)
    set_path(monkeypatch, "walk")
    with sparse_view(gpu_ctx, lists, lengths, 17):
        for args, n_rows, launches in ((kw, rows_kept, 2), (kwc, rows_control, 1)):
            ref = lr.filter(lists, lengths, sgs, vec=True, joined=joined, **args)
            assert len(ref[1]) == n_rows and len(ref[4]) == rows_kept
            got, calls = join_calls(gpu_ctx, lambda: run_filter(gpu_ctx, sgs, C, args))
            assert calls.get(kernel) == launches, calls
            same(got, ref, (C, variant, n_rows))
            del got, ref


# ------------------------------------------------------------------ e. the dense twin
@pytest.mark.parametrize("argset", lc.ARGSETS_12, ids=_argset_id)
def test_dense_twin_absorbed_regime(gpu_ctx, argset):
    """k3_eval (byte tables + overflow pairs through sp_filter_view, k = 9) on the rows of the short-length matrix: the
    regime in which the 1e-20 of the fold test is absorbed and a k-mer exactly on the threshold passes"""
    from subphaser_amd import kmer as km
    from subphaser_amd.config import sets_to_csr
    k, C = 9, 12
    n = km.dense_slots(k)
    assert n == 1 << 17
    mat, lengths = matrix(C, "short")
    slots = np.sort(np.random.RandomState(9).choice(n, len(mat), replace=False)).astype(np.uint64)
    ckeys = km.keys_of_slots(slots, k)
    order = np.argsort(ckeys, kind="stable")
    lists = lc.lists_of(ckeys[order], mat[order])
    memos = _memo.setdefault((C, "short", argset), {})

    def filt(sgs, **kw):
        return lr.filter(lists, lengths, sgs, memo=memos.setdefault(kw["ratio"], {}), **kw)
    sgs, kw = lc.resolve_args(argset, C, filt)
    ref = filt(sgs, **kw)
    gpu_ctx.genome_reset(C)
    for c in range(C):
        gpu_ctx.genome_add(c, b"ACGTACGTACGT")
    gpu_ctx.count(k, 1, 1)
    bufs, d_tabs, d_ovf, n_ovf = [], [], [], []
    try:
        for c in range(C):
            tab = np.zeros(n, np.uint32)
            tab[slots.astype(np.int64)] = mat[:, c]
            d_tabs.append(gpu_ctx.dev_alloc(n))
            bufs.append(d_tabs[-1])
            gpu_ctx.host_to_dev(d_tabs[-1], np.minimum(tab, 255).astype(np.uint8))
            big = np.flatnonzero(tab >= 255)
            d_ovf.append(gpu_ctx.dev_alloc(max(8 * len(big), 8)))
            bufs.append(d_ovf[-1])
            if len(big):
                gpu_ctx.host_to_dev(d_ovf[-1], np.ascontiguousarray(np.stack([big.astype(np.uint32), tab[big]], axis=1)))
            n_ovf.append(len(big))
        gpu_ctx.filter_view(d_tabs, 0, n, lengths, k, 1, d_ovf, n_ovf)
        try:
            nu, nr, nh = gpu_ctx.filter(*sets_to_csr(sgs, list(range(C))), kw["min_fold"], kw["baseline"],
                                        kw["min_freq"], kw["max_freq"], kw["ratio"])
            keys, counts, freqs, tot = gpu_ctx.filter_fetch(nr)       # (dense rows come in slot order: sorted by key)
            hist = np.sort(gpu_ctx.filter_hist(nh))
        finally:
            gpu_ctx.filter_view(None, 0, 0, None, 0, 0)
    finally:
        for d in bufs:
            gpu_ctx.dev_free(d)
    same((nu, nr, nh, keys, counts, freqs, tot, hist), ref, argset)
    assert len(ref[1]) > 20
