"""GPU: homoeologous blocks from shared single-copy k-mers (sp_blocks.hip: bk_count, bk_build, bk_pair, bk_anchors;
Context.blocks_index / blocks_pair / blocks_anchors / blocks_release) against the plain Python twin (tests/blocks_ref.py)
with `==`: the index tallies, the anchors, the four vote arrays.

Inputs (tests/blocks_cases.py) are the smallest at which the kernels can still go wrong: lengths that are no multiple
of 16 or 32, a valid k-mer at the very last start, N runs across a 32-start unit boundary and across window boundaries,
bin = 64 (windows of two units) and bin = 1000 (windows that start inside a unit), kb = 17, 21, 31; planted structure of
40 kb; a window of `bin` anchors in one cell, and windows with many cells -- with the default 4096-cell table and with
a table of 4 cells, which sends every window through the band passes; empty results; index reuse over three chromosomes;
every SP_EINVAL, each followed by a good call; the CLI on the toy genome."""
import logging
import os

import numpy as np
import pytest

import blocks_cases as bc
import blocks_ref as br
from subphaser_amd import blocks as bl

pytestmark = pytest.mark.gpu

_twin = {}


def twin(name, a, b, kb, s, bin_size):
    key = (name, kb, s, bin_size)
    if key not in _twin:
        _twin[key] = br.pair(a, b, kb, s, bin_size)
    return _twin[key]


def load(ctx, seqs):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)


def check_pair(ctx, a, b, ref, kb, s, bin_size):
    """blocks_pair(a, b) and its anchors against the twin's (anchors, win_b, opp, votes, total)"""
    anch, win_b, opp, votes, total = ref
    g_wb, g_opp, g_votes, g_total, n = ctx.blocks_pair(a, b, kb, s, bin_size)
    assert n == len(anch)
    assert g_wb.dtype == np.int32 and g_opp.dtype == np.uint8 and g_votes.dtype == np.int32 and g_total.dtype == np.int32
    assert (g_total == total).all(), np.flatnonzero(g_total != total)[:5]
    assert (g_votes == votes).all(), np.flatnonzero(g_votes != votes)[:5]
    assert (g_wb == win_b).all(), np.flatnonzero(g_wb != win_b)[:5]
    assert (g_opp == opp).all(), np.flatnonzero(g_opp != opp)[:5]
    pa, pb, po = ctx.blocks_anchors(n)
    assert list(zip(pa.tolist(), pb.tolist(), po.tolist())) == anch
    return g_wb, g_opp, g_votes, g_total


@pytest.mark.parametrize("kb", [17, 21, 31])
@pytest.mark.parametrize("bin_size", [64, 1000])
def test_edges_and_breaks(gpu_ctx, kb, bin_size):
    a, b = bc.edges()
    load(gpu_ctx, [a, b])
    try:
        for i, seq in enumerate((a, b)):
            assert gpu_ctx.blocks_index(i, kb, 0) == br.index(seq, kb, 0)[1]
        ref = twin("edges", a, b, kb, 0, bin_size)
        assert ref[0][-1][0] == len(a) - kb and ref[0][-1][1] == len(b) - kb      # the very last start of both is an anchor
        check_pair(gpu_ctx, 0, 1, ref, kb, 0, bin_size)
    finally:
        gpu_ctx.blocks_release()


def test_planted_structure(gpu_ctx):
    a, b = bc.planted()
    kb, s, bin_size = 21, 2, 1000
    load(gpu_ctx, [a, b])
    try:
        for i, seq in enumerate((a, b)):
            assert gpu_ctx.blocks_index(i, kb, s) == br.index(seq, kb, s)[1]
        ref = twin("planted", a, b, kb, s, bin_size)
        win_b, opp, votes, _ = check_pair(gpu_ctx, 0, 1, ref, kb, s, bin_size)
    finally:
        gpu_ctx.blocks_release()
    blocks = bl.walk(win_b, opp, votes, len(a), len(b), bin_size, min_votes=3, max_gap=2, min_block=3000)
    assert blocks == br.blocks(ref[1], ref[2], ref[3], len(a), len(b), bin_size, 3, 2, 3000)
    bc.check_planted(blocks, bin_size)


@pytest.mark.parametrize("cells", [4096, 4])
@pytest.mark.parametrize("which", ["same", "shuffled"])
def test_worst_case_window(gpu_ctx, which, cells):
    a, same, shuffled = bc.worst()
    b = same if which == "same" else shuffled
    kb, bin_size = 21, (8192 if which == "same" else 1024)
    load(gpu_ctx, [a, b])
    try:
        gpu_ctx.blocks_set_cells(cells)
        gpu_ctx.blocks_index(0, kb, 0)
        gpu_ctx.blocks_index(1, kb, 0)
        ref = twin("worst-" + which, a, b, kb, 0, bin_size)
        if which == "same":
            assert ref[3][0] == ref[4][0] >= bin_size - 8      # one cell holds (nearly) `bin` anchors
        else:
            cells_of_window = {}
            for pa, pb, o in ref[0]:
                cells_of_window.setdefault(pa // bin_size, set()).add((pb // bin_size, o))
            assert max(map(len, cells_of_window.values())) > 4      # more cells than the small table: band passes
        check_pair(gpu_ctx, 0, 1, ref, kb, 0, bin_size)
        spilled = gpu_ctx.blocks_pair(0, 1, kb, 0, bin_size, want_spilled=True)[-1]
        assert (spilled > 0) == (cells == 4 and which == "shuffled")
    finally:
        gpu_ctx.blocks_set_cells(4096)
        gpu_ctx.blocks_release()


def test_worst_case_bin_8192_shuffled(gpu_ctx):
    """bin = 8192 over the shuffled copy: the 128 pieces of a window are spread over all three B-windows"""
    a, _, b = bc.worst()
    load(gpu_ctx, [a, b])
    try:
        gpu_ctx.blocks_index(0, 21, 0)
        gpu_ctx.blocks_index(1, 21, 0)
        check_pair(gpu_ctx, 0, 1, twin("worst-shuffled", a, b, 21, 0, 8192), 21, 0, 8192)
    finally:
        gpu_ctx.blocks_release()


def test_empty_results(gpu_ctx):
    u, v = bc.unrelated()
    seqs = [u, v, "N" * 1500, "ACGTACGTAC"]
    load(gpu_ctx, seqs)
    try:
        for i, seq in enumerate(seqs):
            assert gpu_ctx.blocks_index(i, 21, 0) == br.index(seq, 21, 0)[1]
        assert gpu_ctx.blocks_index(2, 21, 0) == (0, 0) and gpu_ctx.blocks_index(3, 21, 0) == (0, 0)
        for a, b in ((0, 1), (0, 2), (2, 0), (3, 0), (0, 3), (2, 3)):
            ref = twin("empty-%d-%d" % (a, b), seqs[a], seqs[b], 21, 0, 500)
            assert ref[0] == []
            win_b, opp, votes, total = check_pair(gpu_ctx, a, b, ref, 21, 0, 500)
            assert len(win_b) == -(-len(seqs[a]) // 500) and (win_b == -1).all() and not votes.any() and not total.any()
    finally:
        gpu_ctx.blocks_release()


def test_index_reuse(gpu_ctx):
    seqs = bc.trio()
    kb, s, bin_size = 21, 1, 500
    load(gpu_ctx, seqs)
    try:
        tallies = [gpu_ctx.blocks_index(i, kb, s) for i in range(3)]
        assert tallies == [br.index(seq, kb, s)[1] for seq in seqs]
        got = {}
        for a, b in ((0, 1), (0, 2), (1, 2), (1, 0)):
            ref = twin("trio-%d-%d" % (a, b), seqs[a], seqs[b], kb, s, bin_size)
            assert len(ref[0]) > 100
            check_pair(gpu_ctx, a, b, ref, kb, s, bin_size)
            got[(a, b)] = ref[0]
            assert [gpu_ctx.blocks_index(i, kb, s) for i in range(3)] == tallies      # stored, not rebuilt
        assert sorted((pb, pa, o) for pa, pb, o in got[(1, 0)]) == got[(0, 1)]
        assert any(o for _, _, o in got[(0, 2)])       # the inverted middle of the third chromosome
        # one index released: its pairs are refused, the others still answer
        gpu_ctx.blocks_release(2)
        with pytest.raises(ValueError, match="no index"):
            gpu_ctx.blocks_pair(0, 2, kb, s, bin_size)
        check_pair(gpu_ctx, 0, 1, twin("trio-0-1", seqs[0], seqs[1], kb, s, bin_size), kb, s, bin_size)
    finally:
        gpu_ctx.blocks_release()


def test_error_codes(gpu_ctx):
    seqs = bc.trio()
    kb, s, bin_size = 21, 1, 500
    gpu_ctx.genome_reset(4)          # chromosome 3 never gets a sequence
    for i, seq in enumerate(seqs):
        gpu_ctx.genome_add(i, seq)
    ref = twin("trio-0-1", seqs[0], seqs[1], kb, s, bin_size)

    def good():
        check_pair(gpu_ctx, 0, 1, ref, kb, s, bin_size)
    try:
        gpu_ctx.blocks_index(0, kb, s)
        with pytest.raises(ValueError, match="no index"):       # a pair call before both indexes exist
            gpu_ctx.blocks_pair(0, 1, kb, s, bin_size)
        gpu_ctx.blocks_index(1, kb, s)
        good()
        for bad_k in (16, 20, 15, 33):
            with pytest.raises(ValueError, match="block_k"):
                gpu_ctx.blocks_index(0, bad_k, s)
            with pytest.raises(ValueError, match="block_k"):
                gpu_ctx.blocks_pair(0, 1, bad_k, s, bin_size)
            good()
        for bad_s in (-1, 17):
            with pytest.raises(ValueError, match="block_sample"):
                gpu_ctx.blocks_index(0, kb, bad_s)
            with pytest.raises(ValueError, match="block_sample"):
                gpu_ctx.blocks_pair(0, 1, kb, bad_s, bin_size)
            good()
        for bad_bin in (0, -5):
            with pytest.raises(ValueError, match="block_bin"):
                gpu_ctx.blocks_pair(0, 1, kb, s, bad_bin)
            good()
        with pytest.raises(ValueError, match="not paired with itself"):
            gpu_ctx.blocks_pair(1, 1, kb, s, bin_size)
        good()
        for bad in (-1, 4, 99):
            with pytest.raises(ValueError, match="outside the genome"):
                gpu_ctx.blocks_index(bad, kb, s)
            with pytest.raises(ValueError, match="outside the genome"):
                gpu_ctx.blocks_pair(0, bad, kb, s, bin_size)
            good()
        with pytest.raises(ValueError, match="no packed sequence"):
            gpu_ctx.blocks_index(3, kb, s)
        good()
        with pytest.raises(ValueError, match="was built with"):      # an index built with another kb / s
            gpu_ctx.blocks_pair(0, 1, 23, s, bin_size)
        with pytest.raises(ValueError, match="was built with"):
            gpu_ctx.blocks_pair(0, 1, kb, s + 1, bin_size)
        good()
        n = len(ref[0])
        with pytest.raises(ValueError, match="anchors, not"):
            gpu_ctx.blocks_anchors(n + 1)
        good()
        gpu_ctx.blocks_release()
        with pytest.raises(ValueError, match="no pair"):
            gpu_ctx.blocks_anchors(n)
        with pytest.raises(ValueError, match="no index"):
            gpu_ctx.blocks_pair(0, 1, kb, s, bin_size)
        gpu_ctx.blocks_index(0, kb, s)
        gpu_ctx.blocks_index(1, kb, s)
        good()
    finally:
        gpu_ctx.blocks_release()


# the toy chromosomes are 80 % repeat copies over a backbone with 8 % substitutions: short k-mers, every one of them, few votes
CLI_BLOCKS = ["-block_k", "17", "-block_sample", "0", "-block_bin", "2000", "-block_votes", "2", "-min_block", "4000"]


def _cli(gpu_ctx, toy, tmp, caplog, extra):
    from subphaser_amd import pipeline, runtime
    tmp.mkdir()
    fa = tmp / "toy.fa"
    with open(fa, "w") as f:
        for lab in toy["labels"]:
            f.write(">%s\n%s\n" % (lab, toy["seqs"][lab]))
    cfg = tmp / "sg.config"
    cfg.write_text("\n".join("\t".join(",".join(u) for u in sg) for sg in toy["sgs"]) + "\n")
    asg = tmp / "assigned.tsv"
    asg.write_text("".join("%s\t%s\n" % kv for kv in toy["sg_assigned"].items()))
    out, tmpd = tmp / "out", tmp / "tmp"
    old = runtime._ctx
    runtime.set_context(gpu_ctx)
    try:
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-sg_assigned", str(asg), "-q", "30", "-k", "15", "-o", str(out),
                           "-tmpdir", str(tmpd), "-window_size", "2500", "-disable_ltr", "-figfmt", "png",
                           "-replicates", "20", "-bootstrap_seed", "1", "-heatmap_size", "0"] + CLI_BLOCKS + extra)
    finally:
        runtime._ctx = old
    return out, tmpd


def test_cli_writes_the_blocks(gpu_ctx, toy, tmp_path, caplog):
    out, tmpd = _cli(gpu_ctx, toy, tmp_path / "with", caplog, [])
    log = [r.getMessage() for r in caplog.records]
    assert sum(m.startswith("blocks ") and " anchors, " in m for m in log) == len(toy["sgs"]) and any(m.startswith("blocks: 3 pairs") for m in log)
    assert any(m.startswith("Modules 3-4") for m in log)
    out0, _ = _cli(gpu_ctx, toy, tmp_path / "without", caplog, ["-disable_blocks"])
    base = str(out / "k15_q30_f2")
    names = sorted(os.listdir(out))
    mine = ["k15_q30_f2.block_link.txt", "k15_q30_f2.blocks.png", "k15_q30_f2.blocks.tsv"]
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        mine.remove("k15_q30_f2.blocks.png")
    assert [n for n in names if "block" in n] == mine
    assert sorted(os.listdir(out0)) == [n for n in names if n not in mine]
    for n in sorted(os.listdir(out0)):
        assert open(out / n, "rb").read() == open(out0 / n, "rb").read(), n
    for n in mine:
        assert os.path.exists(str(tmpd / n) + ".ok")
    # blocks.tsv is what blocks.py makes from the twin's votes
    rows = []
    for line in toy["sgs"]:
        (c1,), (c2,) = line
        a, b = toy["seqs"][c1], toy["seqs"][c2]
        _, win_b, opp, votes, _ = br.pair(a, b, 17, 0, 2000)
        rows.append((c1, c2, bl.walk(win_b, opp, votes, len(a), len(b), 2000, 2, bl.BLOCK_GAP, 4000)))
    assert [len(r[2]) for r in rows] == [4, 3, 5]
    import io
    want = io.StringIO()
    bl.write_tsv(want, rows)
    assert open(base + ".blocks.tsv").read() == want.getvalue()
    want = io.StringIO()
    bl.write_links(want, [[r] for r in rows])
    assert open(base + ".block_link.txt").read() == want.getvalue()
    if "k15_q30_f2.blocks.png" in mine:
        with open(base + ".blocks.png", "rb") as f:
            assert f.read(4) == b"\x89PNG"
