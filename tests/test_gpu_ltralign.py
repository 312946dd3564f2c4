"""GPU: the LTR-pair alignment (sp_ltralign.hip: la_align; Context.ltr_align) against the numpy twin (tests/ltralign_ref.py)
with `==` on all six outputs, and the LTR stage of the command line.

Pairs (tests/ltr_cases.py) are the smallest at which the kernel can still go wrong: LTR lengths 1, 2, 63, 64, 65, 100, 1000
and one pair at SP_LA_MAXLEN; lb - la of 0, +-1, +-70 (a band wider than a wave) and just inside / outside SP_LA_MAXBAND;
band 0, 1 and 64; a_start at every residue modulo 32; a pair at offset 0 that ends on the last base of its chromosome;
runs of N, IUPAC codes, lower case; 2500 short pairs in one call; n = 0; every error, each followed by a good call."""
import io
import logging
import os

import numpy as np
import pytest

import ltr_cases as lc
import ltralign_ref as lr
from subphaser_amd import ltr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return lc.kernel_cases()


@pytest.fixture
def loaded(gpu_ctx, cases):
    seqs, lay = cases
    gpu_ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        gpu_ctx.genome_add(i, s)
    return gpu_ctx


def _check(ctx, cases, band, keep):
    seqs, lay = cases
    names, cols, want = lc.twin(seqs, lay, band, keep)
    got = ctx.ltr_align(*cols, band)
    assert got.dtype == np.int32 and got.shape == (len(names), 6)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(names[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    return names, got


@pytest.mark.parametrize("band", [0, 1, 64])
def test_kernel_is_the_twin(loaded, cases, band):
    names, got = _check(loaded, cases, band, lambda n: not n.startswith(("short", "maxlen")))
    res = dict(zip(names, got.tolist()))
    # the limits fall where the header puts them
    inside = {0: ("delta+1023", "delta-1023"), 1: ("delta+896",), 64: ("delta+895", "delta-895")}[band]
    outside = {0: ("delta+1024", "delta-1024"), 1: ("delta+1023",), 64: ("delta+896", "delta-896")}[band]
    for n in inside:
        assert not res[n][5] & lr.F_BAND and res[n][1] > 0
    for n in outside:
        assert res[n] == [0, 0, 0, 0, 0, lr.F_BAND]
    assert res["over_maxlen"] == [0, 0, 0, 0, 0, lr.F_LEN]
    assert res["all_n"][1] == res["all_n"][2] == 0 and res["all_n"][4] > 0
    assert res["n_run"][4] >= 40 and res["iupac"][4] == 4 and res["lower_case"][1] > 150
    assert res["len1"][:5] == [2, 1, 0, 0, 0]
    if band == 1:
        assert any(r[5] & lr.F_EDGE for r in res.values()) and any(r[5] == 0 for r in res.values())
    elif band == 0:
        assert not any(r[5] & lr.F_EDGE for r in res.values())


def test_a_pair_at_the_length_limit(loaded, cases):
    names, got = _check(loaded, cases, 64, lambda n: n == "maxlen")
    assert got[0][5] == 0 and got[0][1] > 7000 and got[0][2] > 100 and got[0][3] > 0


@pytest.mark.parametrize("band", [1, 64])
def test_more_pairs_than_waves_in_flight(loaded, cases, band):
    names, got = _check(loaded, cases, band, lambda n: n.startswith(("short", "len", "ends")))
    assert len(names) > 2500


def test_empty_call_and_errors(loaded, cases):
    seqs, lay = cases
    names, cols, want = lc.twin(seqs, lay, 1, lambda n: n.startswith("mod32"))

    def good():
        assert (loaded.ltr_align(*cols, 1) == want).all()
    z = np.zeros(0, np.int64)
    assert loaded.ltr_align(z, z, z, z, z, 64).shape == (0, 6)
    good()
    n0 = len(seqs[0])
    for args, msg in [(([3], [0], [5], [10], [5], 1), "chromosome 3 out of range"),
                      (([-1], [0], [5], [10], [5], 1), "chromosome -1 out of range"),
                      (([0], [-1], [5], [10], [5], 1), "left LTR"),
                      (([0], [0], [5], [n0 - 4], [5], 1), "right LTR"),
                      (([2], [0], [78], [10], [5], 1), "left LTR"),
                      (([0], [0], [0], [10], [5], 1), "left LTR"),
                      (([0], [0], [5], [10], [-2], 1), "right LTR"),
                      (([0], [0], [5], [10], [5], -1), "band = -1 is below 0")]:
        with pytest.raises(ValueError, match=msg):
            loaded.ltr_align(*args)
        good()
    # the last base of a chromosome is inside
    assert loaded.ltr_align([0], [0], [5], [n0 - 5], [5], 1).shape == (1, 6)
    loaded.genome_reset(0)
    with pytest.raises(ValueError, match="no genome loaded"):
        loaded.ltr_align([0], [0], [5], [10], [5], 1)
    loaded.genome_reset(len(seqs))
    with pytest.raises(ValueError, match="no packed sequence|outside chromosome"):
        loaded.ltr_align([0], [0], [5], [10], [5], 1)


# ---------------------------------------------------------------------------------------------- the command line
def _cli(gpu_ctx, toy, seqs, scn_text, tmp, caplog, extra):
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
    scn = tmp / "LTR.scn"
    scn.write_text(scn_text)
    out, tmpd = tmp / "out", tmp / "tmp"
    old = runtime._ctx
    runtime.set_context(gpu_ctx)
    caplog.clear()
    try:
        with caplog.at_level(logging.INFO, logger="subphaser_amd"):
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-sg_assigned", str(asg), "-q", "30", "-k", "15", "-o", str(out),
                           "-tmpdir", str(tmpd), "-window_size", "2500", "-disable_circos", "-figfmt", "png", "-replicates", "20",
                           "-bootstrap_seed", "1", "-heatmap_size", "0", "-ltr_scn", str(scn)] + extra)
    finally:
        runtime._ctx = old
    return out, [r.getMessage() for r in caplog.records]


@pytest.fixture(scope="module")
def planted(toy):
    seqs, scn_text, elements = lc.plant_elements({lab: str(toy["seqs"][lab]) for lab in toy["labels"]}, toy["labels"])
    band = ltr.LTR_BAND
    idx = [toy["labels"].index(e[0]) for e in elements]
    a0 = [e[1] - 1 for e in elements]
    b0 = [e[2] - e[4] for e in elements]
    counts = lr.align_intervals([seqs[lab] for lab in toy["labels"]], idx, a0, [e[3] for e in elements], b0, [e[4] for e in elements], band)
    return seqs, scn_text, elements, counts


@pytest.mark.parametrize("mode", ["align", "scn"])
def test_cli_ltr_stage(gpu_ctx, toy, planted, tmp_path, caplog, mode):
    seqs, scn_text, elements, counts = planted
    # the planted indels stay inside the band: no pair is band-limited, none falls back -- a kernel that flags everything fails here
    assert not counts[:, 5].any() and (counts[:, 1] + counts[:, 2] > 0).all() and counts[:, 3].max() <= 12 < ltr.LTR_BAND
    assert counts[:, 2].any() and counts[:, 3].any()
    out, log = _cli(gpu_ctx, toy, seqs, scn_text, tmp_path / mode, caplog, ["-ltr_identity", mode])
    base = str(out / "k15_q30_f2")
    scn = tmp_path / mode / "LTR.scn"
    ltrs = ltr.group_resolve_overlaps(ltr.read_scn(str(scn)))
    assert [(r.seq_id, r.start, r.end, r.lltr, r.rltr) for r in ltrs] == elements          # nothing overlaps, file order is start order
    divs, fell = ltr.divergences(ltrs, counts, mode)
    assert fell == 0
    ages = [ltr.estimate_age(d, 13e-9) for d in divs]
    want = io.StringIO()
    ltr.write_identity(want, ltrs, counts, divs, ages)
    assert open(base + ".ltr.identity.tsv").read() == want.getvalue()
    assert not any("take the similarity of the file" in m for m in log)
    assert any(m.startswith("%d LTR pairs aligned (band 64)" % len(ltrs)) and m.endswith("; 0 touched the edge of their band") for m in log)
    # the enrichment is the stage's own (device map and Fisher tests, pinned elsewhere); the age files follow from it
    rows = [line.split("\t") for line in open(base + ".ltr.enrich").read().splitlines()[1:]]
    d_enriched = {r[0]: r[1] for r in rows if r[1] != "None"}
    d_exchange = {r[0]: r[4] for r in rows}
    assert len(d_enriched) >= len(ltrs) // 2
    mapped = [line.split("\t")[0] for line in open(base + ".ltr.bin.count").read().splitlines()[1:]]
    assert mapped == [r[0] for r in rows] and set(mapped) <= {r.id for r in ltrs}
    data, summary = io.StringIO(), io.StringIO()
    d_data, _, _ = ltr.write_insert_data(data, ltrs, ages, d_enriched, d_exchange)
    ltr.summary_ltr_time(d_data, summary)
    assert open(base + ".ltr.insert.data").read() == data.getvalue()
    assert open(base + ".ltr.insert.summary").read() == summary.getvalue()
    assert "{} significant subgenome-specific LTR-RTs".format(len(d_enriched)) in log
    assert any(m.startswith("Of modules 3-4, ") for m in log)
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    for kind in ("density", "histo"):
        with open(base + ".ltr.insert.%s.png" % kind, "rb") as f:
            assert f.read(4) == b"\x89PNG"
