"""GPU: complete-linkage clustering on the device (sp_hclust.hip: hc_dist, hc_chain; Context.hclust_complete) against the
numpy twin (tests/hclust_ref.py) with `==` on the merges and on the distance matrix; the error codes through the raw
entry; repeated calls; Cluster.heatmap through the real context; the CLI on the toy genome.

Shapes: P = 2, 3 and 65 (across a wave), 1025 and 2049 points in 21 dimensions (across the workgroup's stride of 1024
columns and across 32 x 32 tiles), 21 points in 2049 dimensions (the chromosome shape: 65 staging steps of 32
coordinates, the last of one), 300 points with small-integer coordinates and duplicates (ties, zero heights) and 70 equal
points.  Nothing here needs the 10 000-point workload.

Not bit for bit: the CLI's heatmap against scipy on the written `.kmer.mat`.  The orders are compared with `==` -- the toy
matrix holds duplicated k-mer rows (zero heights), but no tie that rounding could separate: on it the twin's linkages
equal scipy's bit for bit (checked with the CPU oracle context).  The written Z-scores are compared with `==` too."""
import ctypes
import logging

import numpy as np
import pytest

import hclust_ref as hc
from subphaser_amd import _native, cluster, heatmap as hm

pytestmark = pytest.mark.gpu

# name -> (P, D, kind)
SHAPES = {"2x1": (2, 1, "random"), "3x5": (3, 5, "random"), "65x21": (65, 21, "random"), "1025x21": (1025, 21, "random"),
          "2049x21": (2049, 21, "random"), "21x2049": (21, 2049, "random"), "tied-300x4": (300, 4, "tied"),
          "tied-65x1": (65, 1, "tied"), "equal-70x3": (70, 3, "equal")}
_twin = {}


def _case(name):
    """points and the twin's answers, computed once per shape and left unchanged"""
    if name not in _twin:
        P, D, kind = SHAPES[name]
        if kind == "random":
            pts = hc.random_points(7 * P + D, P, D)
        elif kind == "tied":
            pts = hc.tied_points(7 * P + D, P, D)
        else:
            pts = np.full((P, D), -2.5)
        m, d = hc.hclust(pts)
        for a in (pts, m, d):
            a.setflags(write=False)
        _twin[name] = (pts, m, d)
    return _twin[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_merges_and_distances_are_the_twin(gpu_ctx, name):
    pts, m, d = _case(name)
    merges, dist = gpu_ctx.hclust_complete(pts, want_dist=True)
    assert (dist == d).all(), np.argwhere(dist != d)[:5]
    assert (merges == m).all(), np.argwhere(merges != m)[:5]
    only = gpu_ctx.hclust_complete(pts)
    assert only.tobytes() == merges.tobytes()


def test_tied_case_holds_ties():
    _, m, d = _case("tied-300x4")
    off = d[np.triu_indices(300, 1)]
    assert (off == 0).any() and len(np.unique(off)) < 40 and (m[:, 2] == 0).any()


def test_calls_leave_no_state(gpu_ctx):
    """a large call, a small one and the large one again on one context: the buffers are reused, the answers are not"""
    big, small = _case("1025x21"), _case("tied-65x1")
    a = gpu_ctx.hclust_complete(big[0], want_dist=True)
    b = gpu_ctx.hclust_complete(small[0], want_dist=True)
    c = gpu_ctx.hclust_complete(big[0], want_dist=True)
    e = gpu_ctx.hclust_complete(big[0], want_dist=True)
    assert (b[0] == small[1]).all() and (b[1] == small[2]).all()
    for got in (a, c, e):
        assert (got[0] == big[1]).all() and (got[1] == big[2]).all()


def _raw(ctx, P, D, poison=None):
    pts = np.ones((max(P, 1), max(D, 1)))
    if poison is not None:
        pts[-1, -1] = poison
    merges = np.full((max(P - 1, 1), 4), -7.0)
    vp = ctypes.c_void_p
    rc = ctx.L.sp_hclust_complete(ctx.h, vp(pts.ctypes.data), P, D, vp(merges.ctypes.data), None)
    return rc, (merges == -7).all()


@pytest.mark.parametrize("P,D,poison,code", [
    (1, 3, None, _native.SP_EINVAL), (5, 0, None, _native.SP_EINVAL), (5, 3, np.nan, _native.SP_EINVAL),
    (5, 3, np.inf, _native.SP_EINVAL), (16385, 1, None, _native.SP_EUNSUP)])
def test_error_codes(gpu_ctx, P, D, poison, code):
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        rc, untouched = _raw(gpu_ctx, P, D, poison)
        launched = gpu_ctx.prof_report()
    finally:
        gpu_ctx.prof_enable(False)
    assert rc == code, gpu_ctx.L.sp_last_error(gpu_ctx.h)
    assert untouched and not any(k.startswith("hc_") for k in launched)      # nothing launched, nothing written
    assert b"sp_hclust_complete" in gpu_ctx.L.sp_last_error(gpu_ctx.h)


def test_null_pointers_are_invalid(gpu_ctx):
    pts, merges = np.ones((4, 2)), np.ones((3, 4))
    vp = ctypes.c_void_p
    assert gpu_ctx.L.sp_hclust_complete(gpu_ctx.h, None, 4, 2, vp(merges.ctypes.data), None) == _native.SP_EINVAL
    assert gpu_ctx.L.sp_hclust_complete(gpu_ctx.h, vp(pts.ctypes.data), 4, 2, None, None) == _native.SP_EINVAL
    assert b"sp_hclust_complete" in gpu_ctx.L.sp_last_error(gpu_ctx.h)


def test_binding_raises_value_error(gpu_ctx):
    with pytest.raises(ValueError, match="sp_hclust_complete"):
        gpu_ctx.hclust_complete(np.ones((1, 3)))
    with pytest.raises(ValueError, match="sp_hclust_complete"):
        gpu_ctx.hclust_complete(np.array([[0.0, 1.0], [np.nan, 2.0]]))
    with pytest.raises(ValueError, match="P x D"):
        gpu_ctx.hclust_complete(np.ones(5))


def _toy_matrix(ctx, toy):
    import parity_cases as pc
    from subphaser_amd import jellyfish
    _, dumps = pc.count_toy(ctx, toy)
    jd = jellyfish.JellyfishDumps(dumps, toy["labels"])
    return jd.filter(jd.to_matrix(), jd.lengths, toy["sgs"], min_freq=30, min_fold=2)


def test_cluster_heatmap_on_the_device(gpu_ctx, toy, caplog):
    """the k-mer order is the linkage's own (scipy's leaves_list); the chromosome order is that linkage reordered by the
    mean Z, as heatmap.2 reorders it, so it is held against reorder() and shown to be a permutation of the leaves"""
    from scipy.cluster.hierarchy import leaves_list
    d2 = _toy_matrix(gpu_ctx, toy)
    assert d2.ctx is gpu_ctx
    cl = cluster.Cluster(d2, n_clusters=2, sg_assigned=dict(toy["sg_assigned"]), seed=1)
    labels = cl.output_kmers(open("/dev/null", "w"))
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        cl.heatmap(labels, size=10000)
    assert cl.heatmap_engine == "device"
    assert any("on the device" in r.getMessage() for r in caplog.records)
    z = cl.heatmap_z
    C, N = z.shape
    assert C == len(toy["labels"]) and N >= 50
    col = hm.to_linkage(hc.hclust(z.T)[0], N)
    row = hm.to_linkage(hc.hclust(z)[0], C)
    assert (cl.heatmap_col_linkage == col).all() and (cl.heatmap_row_linkage == row).all()
    assert (cl.heatmap_kmer_order == leaves_list(col)).all()
    assert (cl.heatmap_chrom_order == hm.reorder(row, z.mean(axis=1))).all()
    assert sorted(cl.heatmap_chrom_order.tolist()) == sorted(leaves_list(row).tolist()) == list(range(C))
    assert set(cl.heatmap_kmer_sg) <= set(labels.sg_names) | {"NA"} and set(cl.heatmap_kmer_sg) & set(labels.sg_names)


def test_cli_writes_the_heatmap(gpu_ctx, toy, tmp_path, caplog):
    from subphaser_amd import pipeline, runtime
    fa = tmp_path / "toy.fa"
    with open(fa, "w") as f:
        for lab in toy["labels"]:
            f.write(">%s\n%s\n" % (lab, toy["seqs"][lab]))
    cfg = tmp_path / "sg.config"
    cfg.write_text("\n".join("\t".join(",".join(u) for u in sg) for sg in toy["sgs"]) + "\n")
    asg = tmp_path / "assigned.tsv"
    asg.write_text("".join("%s\t%s\n" % kv for kv in toy["sg_assigned"].items()))
    out, tmpd = tmp_path / "out", tmp_path / "tmp"
    old = runtime._ctx
    runtime.set_context(gpu_ctx)
    try:
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-sg_assigned", str(asg), "-q", "30", "-k", "15", "-o", str(out),
                           "-tmpdir", str(tmpd), "-window_size", "2500", "-disable_ltr", "-disable_circos", "-figfmt", "png",
                           "-replicates", "20", "-bootstrap_seed", "1"])
    finally:
        runtime._ctx = old
    log = [r.getMessage() for r in caplog.records if r.getMessage().startswith("heatmap")]
    assert any("on the device" in m for m in log) and not any("using scipy" in m for m in log)
    base = str(out / "k15_q30_f2")
    ckp = str(tmpd / "k15_q30_f2")
    import os
    assert os.path.exists(ckp + ".kmer.mat.heatmap.tsv.ok")
    lines = open(base + ".kmer.mat.heatmap.tsv").read().rstrip("\n").split("\n")
    head = lines[0].split("\t")
    assert head[:2] == ["#kmer", "subgenome"] and sorted(head[2:]) == sorted(toy["labels"])
    kmers = [l.split("\t")[0] for l in lines[1:]]
    K = len(set(toy["sg_assigned"].values()))
    ref = cluster.Cluster(base + ".kmer.mat", n_clusters=K, sg_assigned=dict(toy["sg_assigned"]), seed=1)
    from subphaser_amd import kmer as kmerlib
    all_kmers = kmerlib.decode_many(ref.keys, ref.k)
    assert len(set(kmers)) == len(kmers) and set(kmers) <= set(all_kmers)
    ref.heatmap(None, size=10000)
    assert ref.heatmap_engine == "scipy"
    assert head[2:] == [ref.chrs[i] for i in ref.heatmap_chrom_order]
    assert kmers == [all_kmers[ref.heatmap_rows[j]] for j in ref.heatmap_kmer_order]
    # and the written Z-scores are the scipy run's, to the bit: the matrix text is an exact round trip
    z = np.array([[float(v) for v in l.split("\t")[2:]] for l in lines[1:]])
    assert (z == ref.heatmap_z[np.ix_(ref.heatmap_chrom_order, ref.heatmap_kmer_order)].T).all()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    with open(base + ".kmer.mat.png", "rb") as f:
        assert f.read(4) == b"\x89PNG"
    assert os.path.exists(ckp + ".kmer.mat.png.ok")
