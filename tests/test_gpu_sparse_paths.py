"""Engine 0 at k = 16..32 (the MSD partition chain of sp_sparse2.hip) where its kernels change path: the hand-made chromosomes
of tests/s3_cases.py, whose fine buckets hold a declared number of keys and of distinct residuals exactly at the thresholds of
the bitmap finish, the hashed finish, s3_final's split / sort / direct count / hot-key hash / give-up and the oversized-bucket
paths, and whose lengths sit on the tile seams of s3_part1 and s3_part2.  The twin of test_gpu_count_paths.py.

Every comparison is bit-exact against the oracle: `dump(i, sort=False)` -- the list AS THE DEVICE EMITS IT, which the list
filter and the label look-ups binary-search and merge as it stands -- must equal the oracle's keys and counts, the keys must be
strictly ascending, and `dump_size` and `lengths()` must agree.

Evidence of the path: the count runs between prof_enable / prof_report.  Exactly the declared first finish kernel (s3_final_bitmap,
s3_final_hash or s3_final_small) appears; s3_big_sort's grid equals the declared number of give-up buckets and s3_big_class's
32 times that; s3_big_rle appears if and only if the library path is declared (a kept list beyond S3B_KCAP).  A punt inside
s3_final (whole sort, split, hashed piece, sorted piece, direct count, hot-key hash) has no kernel name of its own: there the
evidence is tests/test_s3cases_host.py, which holds the bucket's content, and with it the route the model derives, to what
the case declares."""
import numpy as np
import pytest

import s3_cases as sc

pytestmark = pytest.mark.gpu

FIRST = {"s3_final_bitmap", "s3_final_hash", "s3_final_small"}
NAMES = [c.name for c in sc.CASES]
GIVE_UP = [c.name for c in sc.CASES if any(c.declared(lo)["n_big"] for lo in c.lowers)]


def _load(ctx, seqs):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)


def _check(ctx, want, where):
    """the lists as emitted against the oracle's"""
    total = []
    for i, (ok, oc) in enumerate(want):
        gk, gc = ctx.dump(i, sort=False)
        assert ctx.dump_size(i) == len(ok), (where, i, ctx.dump_size(i), len(ok))
        assert gk.shape == ok.shape, (where, i, gk.shape, ok.shape)
        assert (gk[1:] > gk[:-1]).all(), (where, i, "the emitted keys do not ascend", np.flatnonzero(gk[1:] <= gk[:-1])[:5])
        assert (gk == ok).all() and (gc == oc).all(), (where, i, np.flatnonzero((gk != ok) | (gc != oc))[:5])
        total.append(int(oc.astype(np.int64).sum()))
    assert ctx.lengths().tolist() == total, where


def _profiled_count(ctx, k, lower, engine):
    """the count and the largest grid per kernel name it launched"""
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        ctx.count(k, lower, engine)
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    return {name: int(e["grid"]) for name, e in rep.items()}


def _evidence(grids, dec, where, library=False):
    assert FIRST & set(grids) == {dec["first"]}, (where, sorted(FIRST & set(grids)))
    if dec["n_big"] == 0:
        assert not {"s3_big_class", "s3_big_sort", "s3_big_rle"} & set(grids), (where, sorted(grids))
        return
    if library:          # SP_S3_BIG=sort: the library sort always
        assert "s3_big_class" not in grids and "s3_big_sort" not in grids and grids["s3_big_rle"] == dec["n_big"], (where, grids)
        return
    assert grids["s3_big_sort"] == dec["n_big"] and grids["s3_big_class"] == sc.S3B_SPREAD * dec["n_big"], (where, grids)
    assert ("s3_big_rle" in grids) == dec["rle"], (where, dec["rle"], sorted(grids))
    if dec["rle"]:
        assert grids["s3_big_rle"] == dec["n_big"], (where, grids)


@pytest.mark.parametrize("name", NAMES)
def test_case_on_the_partition_engine(gpu_ctx, monkeypatch, name):
    """every case at each of its `lower` values, with the sampled sizing and (cases below 1 Mb) with SP_S3_EXACT=1"""
    case = sc.BY_NAME[name]
    for var, val in case.env().items():
        monkeypatch.setenv(var, val)
    _load(gpu_ctx, case.seqs())
    for exact in ((None, "1") if case.small else (None,)):
        if exact:
            monkeypatch.setenv("SP_S3_EXACT", exact)
        for lower in case.lowers:
            where = (name, lower, exact)
            grids = _profiled_count(gpu_ctx, case.k, lower, 0)
            _check(gpu_ctx, sc.oracle_at(name, lower), where)
            _evidence(grids, case.declared(lower), where)
            assert ("s3_hist2" in grids) == bool(exact) and ("s3_hist2_sample" in grids) == (not exact), (where, sorted(grids))


@pytest.mark.parametrize("name", GIVE_UP)
def test_give_up_cases_through_the_library_sort(gpu_ctx, monkeypatch, name):
    """the give-up buckets once more under SP_S3_BIG=sort: the segmented library sort and s3_big_rle instead of the hash classes"""
    case = sc.BY_NAME[name]
    monkeypatch.setenv("SP_S3_BIG", "sort")
    _load(gpu_ctx, case.seqs())
    for lower in case.lowers:
        dec = case.declared(lower)
        grids = _profiled_count(gpu_ctx, case.k, lower, 0)
        _check(gpu_ctx, sc.oracle_at(name, lower), (name, lower, "library"))
        _evidence(grids, dec, (name, lower, "library"), library=True)


@pytest.mark.parametrize("k", sorted({c.k for c in sc.CASES if c.small and not c.sort_mode}))
def test_small_cases_side_by_side_on_three_lanes(gpu_ctx, monkeypatch, k):
    """all small cases of one k as the chromosomes of one genome, three chains in flight (SP_LANES_SPARSE=3), lower 2"""
    monkeypatch.setenv("SP_LANES_SPARSE", "3")
    cases = [c for c in sc.CASES if c.k == k and c.small and not c.sort_mode]
    _load(gpu_ctx, [s for c in cases for s in c.seqs()])
    gpu_ctx.count(k, 2, 0)
    _check(gpu_ctx, [w for c in cases for w in sc.oracle_at(c.name, 2)], (k, "lanes"))


@pytest.mark.parametrize("name", NAMES)
def test_case_on_the_sort_engine(gpu_ctx, name):
    """every case once through engine 1 (sp_sparse.hip, the device-wide sort): the same oracle applies"""
    case = sc.BY_NAME[name]
    _load(gpu_ctx, case.seqs())
    lower = case.lowers[-1]
    gpu_ctx.count(case.k, lower, 1)
    _check(gpu_ctx, sc.oracle_at(name, lower), (name, lower, "engine 1"))
