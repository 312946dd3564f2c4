"""GPU: the LTR detection (sp_ltrdetect.hip: ld_words, the sort, ld_seeds, ld_extend, the HSP sort; Context.ltr_seeds /
ltr_hsps) against the Python twin (tests/ltrdetect_ref.py) with `==` on the number of seeds and on every HSP, and the
command line under -ltr_denovo.

Inputs are those of tests/ltrdetect_cases.py: the hand cases, the flank-controlled pairs, the planted genome (3 x 200 kb)
and the dense two-letter chromosome.  Every case runs at chunk bodies of 4096 and 5000 starts and at the default, and once
more in a context created under SP_CU_LIMIT=1, where ld_words, ld_seeds and ld_extend take several passes."""
import logging
import os

import numpy as np
import pytest

import ltrdetect_cases as lc
import ltrdetect_ref as ld
from subphaser_amd import ltr
from test_gpu_cu_limit import limited, profiled
from test_pipeline_ltrdetect import expected_scn

pytestmark = pytest.mark.gpu


def all_cases():
    flank, planted, dense = lc.flank_case(), lc.planted(), lc.dense_case()
    return lc.hand_cases() + [("flank", [flank[0]], lc.DEFAULT), ("planted", planted[0], lc.DEFAULT), ("dense", [dense[0]], dense[1])]


def load(ctx, seqs):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)


def detect(ctx, i, par):
    n_seeds, n_hsps = ctx.ltr_seeds(i, par["L"], par["X"], par["dmin"], par["dmax"], par["maxlen"])
    p0, n, d = ctx.ltr_hsps(n_hsps)
    assert p0.dtype == n.dtype == d.dtype == np.int32 and len(p0) == len(n) == len(d) == n_hsps
    return n_seeds, list(zip(p0.tolist(), n.tolist(), d.tolist()))


def check_all(ctx, cases):
    total = 0
    for name, seqs, par in cases:
        load(ctx, seqs)
        want = lc.twin(seqs, par)
        for i in range(len(seqs)):
            got = detect(ctx, i, par)
            assert got[0] == want[i][0], (name, i, "seeds", got[0], want[i][0])
            assert got[1] == want[i][1], (name, i, [x for x in got[1] if x not in want[i][1]][:5], [x for x in want[i][1] if x not in got[1]][:5])
            total += got[0]
    return total


@pytest.mark.parametrize("chunk", lc.CHUNKS)
def test_kernels_are_the_twin(gpu_ctx, chunk):
    gpu_ctx.ltr_detect_set_chunk(chunk)
    try:
        assert check_all(gpu_ctx, all_cases()) > 5000
    finally:
        gpu_ctx.ltr_detect_set_chunk(0)


@pytest.mark.parametrize("chunk", [4096, 0])
def test_under_a_cu_limit(monkeypatch, chunk):
    """a context that reckons with one compute unit caps the three kernels at 8 workgroups of 256 lanes: the planted
    chromosomes have 6250 units of 32 starts (ld_words: four passes at the default chunk) and 199 981 sorted elements
    (ld_seeds), the dense chromosome more than 4096 seeds (ld_extend)"""
    cases = all_cases()
    with limited(monkeypatch, 1) as lim:
        lim.ltr_detect_set_chunk(chunk)
        total, grids = profiled(lim, lambda ctx: check_all(ctx, cases))
    print("grids under SP_CU_LIMIT=1:", {k: v for k, v in grids.items() if k.startswith("ld_")})
    assert grids["ld_seeds"] == 8 and grids["ld_extend"] == 8 and (grids["ld_words"] == 8 or chunk)       # (a chunk of 4096 has 600 units)
    dense, par = lc.dense_case()
    assert lc.twin([dense], par)[0][0] > 2 * 8 * 256                        # seeds of one ld_extend launch
    assert lc.PLANTED_LEN - 19 > 2 * 8 * 256 and lc.PLANTED_LEN // 32 > 2 * 8 * 256      # elements of ld_seeds, units of ld_words


@pytest.mark.parametrize("chunk", [4096, 0])
def test_seed_list_overflows_and_is_sized_from_the_count(gpu_ctx, chunk):
    """16 seeds of capacity: the dense chromosome has thousands (its first chunk alone overflows; with chunks of 4096 starts
    the seeds of the chunks before are moved over every time the list grows), the planted ones about 130"""
    dense, par = lc.dense_case()
    planted = lc.planted()[0]
    gpu_ctx.ltr_detect_set_capacity(16)
    gpu_ctx.ltr_detect_set_chunk(chunk)
    try:
        assert check_all(gpu_ctx, [("dense", [dense], par), ("planted", planted, lc.DEFAULT)]) > 16 * 100
        gpu_ctx.ltr_detect_set_capacity(lc.twin([dense], par)[0][0])       # exactly enough: no second run, nothing lost
        check_all(gpu_ctx, [("dense", [dense], par)])
    finally:
        gpu_ctx.ltr_detect_set_capacity(0)
        gpu_ctx.ltr_detect_set_chunk(0)


def test_errors_each_followed_by_a_good_call(gpu_ctx):
    name, seqs, par = [c for c in lc.hand_cases() if c[0] == "xdrop_11"][0]
    want = lc.twin(seqs, par)[0]
    load(gpu_ctx, seqs)

    def good():
        assert detect(gpu_ctx, 0, par) == want
    good()
    d = dict(par)
    for over, msg in [(dict(L=11), "seed length 11 is outside 12..20"), (dict(L=21), "seed length 21 is outside 12..20"),
                      (dict(dmax=32768), "maximum distance 32768 is above 32767"), (dict(maxlen=8193), "maximum LTR length 8193 is above 8192"),
                      (dict(dmin=601), "the minimum is below 1 or above the maximum"), (dict(dmin=0), "the minimum is below 1"),
                      (dict(X=-1), "X-drop -1 is below 0"), (dict(maxlen=0), "maximum LTR length 0 is below 1")]:
        q = dict(d, **over)
        with pytest.raises(ValueError, match=msg):
            gpu_ctx.ltr_seeds(0, q["L"], q["X"], q["dmin"], q["dmax"], q["maxlen"])
        with pytest.raises(ValueError, match="no list to answer for"):        # a failed call leaves no list behind
            gpu_ctx.ltr_hsps(0)
        good()
    for chrom in (-1, 1, 7):
        with pytest.raises(ValueError, match="chromosome %d is outside the genome" % chrom):
            gpu_ctx.ltr_seeds(chrom, 12, 20, 50, 300, 100)
        good()
    with pytest.raises(ValueError, match="the last call found %d HSPs, not %d" % (len(want[1]), len(want[1]) + 1)):
        gpu_ctx.ltr_hsps(len(want[1]) + 1)
    good()
    for bad in (-1, ld.BODY + 1):
        with pytest.raises(ValueError, match="sp_ltr_detect_set_chunk"):
            gpu_ctx.ltr_detect_set_chunk(bad)
        good()
    with pytest.raises(ValueError, match="sp_ltr_detect_set_capacity"):
        gpu_ctx.ltr_detect_set_capacity(-1)
    good()
    gpu_ctx.genome_reset(2)
    gpu_ctx.genome_add(0, seqs[0])
    with pytest.raises(ValueError, match="chromosome 1 has no packed sequence"):
        gpu_ctx.ltr_seeds(1, 12, 20, 50, 300, 100)
    good()
    # a chromosome shorter than the seed has no seed, and an empty list to fetch
    gpu_ctx.genome_add(1, "ACGTACGTACG")
    assert detect(gpu_ctx, 1, par) == (0, [])
    good()


# ---------------------------------------------------------------------------------------------- the command line
def _cli(gpu_ctx, toy, seqs, tmp, caplog, extra):
    from subphaser_amd import pipeline, runtime
    tmp.mkdir()
    fa = tmp / "toy.fa"
    with open(fa, "w") as f:
        for lab in toy["labels"]:
            f.write(">%s\n%s\n" % (lab, seqs[lab]))
    cfg = tmp / "sg.config"
    cfg.write_text("\n".join("\t".join(",".join(u) for u in sg) for sg in toy["sgs"]) + "\n")
    asg = tmp / "assigned.tsv"
    asg.write_text("".join("%s\t%s\n" % kv for kv in toy["sg_assigned"].items()))
    out, tmpd = tmp / "out", tmp / "tmp"
    old = runtime._ctx
    runtime.set_context(gpu_ctx)
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-sg_assigned", str(asg), "-q", "30", "-k", "15", "-o", str(out),
                           "-tmpdir", str(tmpd), "-window_size", "2500", "-disable_circos", "-figfmt", "png", "-replicates", "20",
                           "-bootstrap_seed", "1", "-heatmap_size", "0"] + extra)
    finally:
        runtime._ctx = old
    return str(out / "k15_q30_f2"), [r.getMessage() for r in caplog.records]


def test_cli_denovo(gpu_ctx, toy, tmp_path, caplog):
    """-ltr_denovo on the toy genome with planted elements: the `.ltr.scn` is what the twin-driven detection writes (the
    candidates aligned by Context.ltr_align, which tests/test_gpu_ltralign.py pins to its own twin), the downstream files
    exist, and a second run that reads the `.scn` through -ltr_scn writes them again byte for byte"""
    import ltr_cases
    labels = toy["labels"]
    seqs, _, elements = ltr_cases.plant_elements({lab: str(toy["seqs"][lab]) for lab in labels}, labels)
    base, log = _cli(gpu_ctx, toy, seqs, tmp_path / "denovo", caplog, ["-ltr_denovo"])
    chroms = [seqs[lab] for lab in labels]
    load(gpu_ctx, chroms)
    align = lambda _, ci, a0, la, b0, lb, band: gpu_ctx.ltr_align(ci, a0, la, b0, lb, band)
    text, n_seeds, n_hsps, n_chains, n_cand, n_kept = expected_scn(chroms, labels=labels, align=align)
    assert open(base + ".ltr.scn").read() == text
    assert any(m.startswith("%d seeds, %d extended seeds (HSPs), %d chains, %d candidates on %d chromosomes" % (n_seeds, n_hsps, n_chains, n_cand, len(labels)))
               for m in log)
    # most planted elements with LTRs of 120 bases or more are among the records, their ends within 20 bases
    recs = ltr.read_scn(base + ".ltr.scn")
    found = 0
    for lab, start, end, lltr, rltr in elements:
        if min(lltr, rltr) >= 120:
            found += any(r.seq_id == lab and abs(r.start - start) <= 20 and abs(r.end - end) <= 20 for r in recs)
    print("planted elements found within 20 bases: %d of %d" % (found, sum(min(e[3], e[4]) >= 120 for e in elements)))
    assert 2 * found >= sum(min(e[3], e[4]) >= 120 for e in elements) and n_kept == len(recs) > 0        # (a file of something else fails here)
    for ext in (".ltr.enrich", ".ltr.insert.data", ".ltr.bin.count", ".ltr.identity.tsv"):
        assert os.path.exists(base + ext), ext
    assert any(m.startswith("Of modules 3-4, TEsorter classification") for m in log)
    base2, log2 = _cli(gpu_ctx, toy, seqs, tmp_path / "fromfile", caplog, ["-ltr_scn", base + ".ltr.scn"])
    for ext in (".ltr.bin.count", ".ltr.enrich", ".ltr.identity.tsv", ".ltr.insert.data", ".ltr.insert.summary"):
        assert open(base2 + ext).read() == open(base + ext).read(), ext
    assert not os.path.exists(base2 + ".ltr.scn") and any(m.startswith("Of modules 3-4, LTR detection") for m in log2)
