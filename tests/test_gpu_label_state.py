"""GPU: when a label set is usable, and that the table switches are read on every sp_labels_set call.

The label tables belong to the k they were built at.  sp_count with another k -- k > 15 to k > 15, k > 15 to k <= 15 and
back, k <= 15 to k <= 15 -- ends the set: map_bins, map_bins_all, map_features, map_intervals and labels_hit refuse
("call sp_labels_set first", before any launch) until labels are set again, and then the bins equal the oracle's.  A
recount at the same k keeps the set.  SP_CTAB flipped between two sp_labels_set calls on one context changes the table
(read off the *_seen kernel that labels_hit launches), and the bins equal the oracle's under each.

Two chromosomes of 40 kb with planted repeats and a few thousand labels, as in test_filter_and_map_sparse_engine; the
oracle's bins are computed once per k and shared."""
import numpy as np
import pytest

import pyoracle as po
from test_gpu_parity import _rand_seq

pytestmark = pytest.mark.gpu

S = 3
SHAPE = (1000, 10000)       # bin_size, chunk_size
_cache = {}


def genome():
    if "genome" not in _cache:
        rng = np.random.RandomState(1700)
        reps = [_rand_seq(rng, 350, 0, 0) for _ in range(4)]
        seqs = []
        for c in range(2):
            s = _rand_seq(rng, 40000 + 501 * c)
            for _ in range(50):
                r = reps[rng.randint(0, 2 + 2 * c)]      # chromosome 1 holds the families of chromosome 0 too
                p = rng.randint(0, s.size - 400)
                s[p:p + r.size] = r
            s.setflags(write=False)
            seqs.append(s)
        _cache["genome"] = seqs
    return _cache["genome"]


def case(k):
    """(keys, labels, [(bins, n_mapped) of every chromosome by the oracle]) at k: the repeated k-mers of chromosome 0
    and a tenth of the others, labelled round robin"""
    if k not in _cache:
        seqs = genome()
        rng = np.random.RandomState(k)
        keys, cnts = po.count(seqs[0], k, 1)
        sel = keys[(cnts >= 2) | (rng.rand(keys.size) < 0.1)]
        assert 2000 < sel.size < 20000
        sg = (np.arange(sel.size) % S).astype(np.uint8)
        exp = []
        for s in seqs:
            b, _, n = po.map_bins(s, k, sel, sg, S, *SHAPE, nthreads=2)
            b.setflags(write=False)
            exp.append((b, int(n)))
        assert sum(n for _, n in exp) > sel.size
        sel.setflags(write=False)
        sg.setflags(write=False)
        _cache[k] = (sel, sg, exp)
    return _cache[k]


def load(ctx):
    seqs = genome()
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)


def assert_bins(ctx, k, where=""):
    for i, (b, n) in enumerate(case(k)[2]):
        got, gn = ctx.map_bins(i, *SHAPE)
        assert (got == b).all() and gn == n, (k, i, where)


def no_switches(monkeypatch):
    for name in ("SP_MAP_ENGINE", "SP_CTAB", "SP_CTAB_FACTOR"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("ks", [(17, 21), (17, 15, 17), (15, 13)], ids=lambda ks: "-".join(map(str, ks)))
def test_stale_labels_are_refused(gpu_ctx, monkeypatch, ks):
    no_switches(monkeypatch)
    load(gpu_ctx)
    for k in ks[:-1]:
        gpu_ctx.count(k, 1)
        gpu_ctx.labels_set(*case(k)[:2], S)
    assert_bins(gpu_ctx, ks[-2], "before the recount")
    k = ks[-1]
    gpu_ctx.count(k, 1)
    entries = {
        "sp_map_bins": lambda: gpu_ctx.map_bins(0, *SHAPE),
        "sp_map_bins_all": lambda: gpu_ctx.map_bins_all(*SHAPE),
        "sp_map_features": lambda: gpu_ctx.map_features([bytes(genome()[0][100:900])]),
        "sp_map_intervals": lambda: gpu_ctx.map_intervals([0, 1], [0, 50], [5000, 900]),
        "sp_labels_hit": gpu_ctx.labels_hit,
    }
    for name, call in entries.items():
        with pytest.raises(ValueError, match=name + ": call sp_labels_set first"):
            call()
    gpu_ctx.labels_set(*case(k)[:2], S)
    assert_bins(gpu_ctx, k, "after labels_set at the new k")
    allb, nm = gpu_ctx.map_bins_all(*SHAPE)
    for got, gn, (b, n) in zip(allb, nm, case(k)[2]):
        assert (got == b).all() and int(gn) == n
    assert gpu_ctx.labels_hit() > 0


@pytest.mark.parametrize("k", [15, 17])
def test_same_k_recount_keeps_the_set(gpu_ctx, monkeypatch, k):
    no_switches(monkeypatch)
    load(gpu_ctx)
    gpu_ctx.count(k, 1)
    gpu_ctx.labels_set(*case(k)[:2], S)
    gpu_ctx.count(k, 1)
    assert_bins(gpu_ctx, k, "after the recount")


@pytest.mark.parametrize("k,ctab,seen", [(17, (None, "0", None), ("sq_seen", "sps_pair_seen", "sq_seen")),
                                         (15, ("1", "0", "1"), ("k4_ctab_seen", "k4_pair_seen", "k4_ctab_seen"))])
def test_switch_flipped_between_two_labels_set_calls(gpu_ctx, monkeypatch, k, ctab, seen):
    no_switches(monkeypatch)
    load(gpu_ctx)
    gpu_ctx.count(k, 1)
    all_seen = {"sq_seen", "sps_pair_seen", "sps_count_seen", "k4_ctab_seen", "k4_pair_seen", "k4_count_seen"}
    hits = []
    for value, kernel in zip(ctab, seen):
        if value is None:
            monkeypatch.delenv("SP_CTAB", raising=False)
        else:
            monkeypatch.setenv("SP_CTAB", value)
        gpu_ctx.labels_set(*case(k)[:2], S)
        assert_bins(gpu_ctx, k, "SP_CTAB=%s" % value)
        gpu_ctx.prof_reset()
        gpu_ctx.prof_enable(True)
        try:
            hits.append(gpu_ctx.labels_hit())
            rep = gpu_ctx.prof_report()
        finally:
            gpu_ctx.prof_enable(False)
            gpu_ctx.prof_reset()
        assert all_seen & set(rep) == {kernel}, (k, value, sorted(rep))
    assert hits[0] > 0 and hits == [hits[0]] * len(hits)
