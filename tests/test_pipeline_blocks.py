"""The host side of the block stage without a GPU: the pair list, the two text formats, and Pipeline.stage_blocks over a
stub context whose votes come from the twin (tests/blocks_ref.py)."""
import io
import itertools
import logging
import os

import pytest

import blocks_cases as bc
import blocks_ref as br
from subphaser_amd import blocks as bl
from subphaser_amd import pipeline, runtime


# ---------------------------------------------------------------------------------------------- the pair list
def _pairs_by_the_rule(sgs):
    """per config line combinations(units, 2), then product of their chromosomes; first occurrence wins"""
    seen, groups = [], []
    for line in sgs:
        group = []
        for i in range(len(line)):
            for j in range(i + 1, len(line)):
                for c1 in line[i]:
                    for c2 in line[j]:
                        if (c1, c2) not in seen:
                            seen.append((c1, c2))
                            group.append((c1, c2))
        groups.append(group)
    return groups


def test_pair_list_on_the_example_configs(golden):
    cfgs = golden["G8_sgconfig"]
    assert len(cfgs) >= 5
    n = 0
    for name, ent in sorted(cfgs.items()):
        for parse in ent["parses"]:
            sgs = parse["sgs"]
            got = bl.pair_list(sgs)
            assert got == _pairs_by_the_rule(sgs), name
            assert len(got) == len(sgs)
            n += sum(map(len, got))
    assert n > 50


def test_pair_list_on_comma_joined_units_and_repeats():
    sgs = [[["a1", "a2"], ["b1"], ["c1", "c2"]], [["solo"]], [["a1"], ["b1"]], [["b1"], ["a1"]]]
    assert bl.pair_list(sgs) == [
        [("a1", "b1"), ("a2", "b1"), ("a1", "c1"), ("a1", "c2"), ("a2", "c1"), ("a2", "c2"), ("b1", "c1"), ("b1", "c2")],
        [],
        [],                      # (a1, b1) was on the first line
        [("b1", "a1")],          # the ordered pair is new
    ]
    assert bl.pair_list([]) == [] and bl.pair_list([[]]) == [[]]
    assert bl.pair_list([[["x"], ["y"]]]) == [list(itertools.product(["x"], ["y"]))]


# ---------------------------------------------------------------------------------------------- the two text formats
BLOCKS = [[("A1", "B1", [(0, 30000, 10000, 40000, "+", 3, 41), (50000, 120000, 60000, 130000, "-", 7, 90)]),
           ("A1", "C1", [])],
          [],
          [("A2", "B2", [(10000, 20000, 0, 10000, "+", 1, 5)]), ("A2", "C2", [(0, 30000, 0, 30000, "-", 3, 9)])]]


def test_blocks_tsv_byte_for_byte():
    out = io.StringIO()
    bl.write_tsv(out, [p for g in BLOCKS for p in g])
    assert out.getvalue() == ("#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tstrand\twindows\tanchors\n"
                              "A1\t0\t30000\tB1\t10000\t40000\t+\t3\t41\n"
                              "A1\t50000\t120000\tB1\t60000\t130000\t-\t7\t90\n"
                              "A2\t10000\t20000\tB2\t0\t10000\t+\t1\t5\n"
                              "A2\t0\t30000\tC2\t0\t30000\t-\t3\t9\n")


def test_block_link_byte_for_byte():
    out = io.StringIO()
    bl.write_links(out, BLOCKS)
    # one colour per config line (the empty line keeps its colour), a line's blocks by size ascending
    assert out.getvalue() == ("A1 0 30000 B1 10000 40000 color=chr1\n"
                              "A1 50000 120000 B1 60000 130000 color=chr1\n"
                              "A2 10000 20000 B2 0 10000 color=chr3\n"
                              "A2 0 30000 C2 0 30000 color=chr3\n")
    out = io.StringIO()
    bl.write_links(out, [[("x", "y", [(0, 300, 0, 300, "+", 3, 9), (500, 600, 500, 600, "-", 1, 3), (700, 1000, 700, 1000, "+", 3, 9)])]] * 3,
                   colors=["red", "blue"])
    lines = out.getvalue().split("\n")[:-1]
    assert lines[0] == "x 500 600 y 500 600 color=red" and lines[1] == "x 0 300 y 0 300 color=red"      # ties keep their order
    assert [l.rsplit("=", 1)[1] for l in lines] == ["red"] * 3 + ["blue"] * 3 + ["red"] * 3
    assert len(bl.LINK_COLORS) == 24 and bl.LINK_COLORS[0] == "chr1" and bl.LINK_COLORS[-1] == "chrY"


# ---------------------------------------------------------------------------------------------- the stage
class _Stub:
    """block entries answered by the twin; records the calls"""
    h = 1      # runtime.get_context takes a context with a handle for a live one

    def __init__(self, seqs):
        self.seqs, self.calls, self.indexed = seqs, [], set()

    def blocks_index(self, chrom, kb, s):
        self.calls.append(("index", chrom, kb, s))
        self.indexed.add(chrom)
        return br.index(self.seqs[chrom], kb, s)[1]

    def blocks_pair(self, a, b, kb, s, bin_size):
        assert a in self.indexed and b in self.indexed
        self.calls.append(("pair", a, b, kb, s, bin_size))
        anch, win_b, opp, votes, total = br.pair(self.seqs[a], self.seqs[b], kb, s, bin_size)
        return win_b, opp, votes, total, len(anch)

    def blocks_release(self, chrom=-1):
        self.calls.append(("release", chrom))
        self.indexed -= {chrom} if chrom >= 0 else set(self.indexed)


class _Lay:
    def __init__(self, root):
        self.root = str(root)

    def out(self, ext):
        return os.path.join(self.root, "run." + ext)

    def ckp(self, name):
        return os.path.join(self.root, os.path.basename(name) + ".ok")


LABELS = ["c0", "c1", "c2", "lone"]


def _pipe(tmp_path, sgs, **over):
    opts = dict(sgs=sgs, block_k=21, block_sample=1, block_bin=500, block_votes=3, block_gap=5, min_block=1500, figfmt="png")
    opts.update(over)
    p = pipeline.Pipeline.bare(**opts)
    seqs = list(bc.trio()) + ["ACGT" * 50]
    stub = _Stub(seqs)
    return p, stub, _Lay(tmp_path), {lab: len(s) for lab, s in zip(LABELS, seqs)}


@pytest.fixture
def with_ctx():
    old = runtime._ctx
    yield runtime.set_context
    runtime._ctx = old


def _expected(stub, pairs, p):
    rows = []
    for c1, c2 in pairs:
        a, b = LABELS.index(c1), LABELS.index(c2)
        _, win_b, opp, votes, _ = br.pair(stub.seqs[a], stub.seqs[b], p.block_k, p.block_sample, p.block_bin)
        rows.append((c1, c2, br.blocks(win_b, opp, votes, len(stub.seqs[a]), len(stub.seqs[b]), p.block_bin, p.block_votes,
                                       p.block_gap, p.min_block)))
    return rows


def test_stage_writes_the_files(tmp_path, with_ctx, caplog):
    p, stub, lay, d_size = _pipe(tmp_path, [[["c0"], ["c1"], ["c2"]], [["lone"]]])
    with_ctx(stub)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_blocks(lay, LABELS, d_size)
    rows = _expected(stub, [("c0", "c1"), ("c0", "c2"), ("c1", "c2")], p)
    assert sum(len(r[2]) for r in rows) >= 3 and any(b[4] == "-" for r in rows for b in r[2])
    want = io.StringIO()
    bl.write_tsv(want, rows)
    assert open(lay.out("blocks.tsv")).read() == want.getvalue()
    want = io.StringIO()
    bl.write_links(want, [rows, []])
    assert open(lay.out("block_link.txt")).read() == want.getvalue()
    assert os.path.exists(lay.ckp(lay.out("blocks.tsv"))) and os.path.exists(lay.ckp(lay.out("block_link.txt")))
    # every index built once, pairs in list order, everything released at the end
    assert [c for c in stub.calls if c[0] == "index"] == [("index", i, 21, 1) for i in range(3)]
    assert [c[1:3] for c in stub.calls if c[0] == "pair"] == [(0, 1), (0, 2), (1, 2)]
    assert not stub.indexed
    log = [r.getMessage() for r in caplog.records]
    assert sum(" anchors, " in m and m.startswith("blocks c") for m in log) == 3
    assert sum(m.startswith("blocks: 3 pairs, ") for m in log) == 1
    assert sum("has a single unit" in m for m in log) == 1
    # the figure is queued for the main thread, drawn there, and optional
    (name, wait, done), = p._background
    assert name == lay.out("blocks.png")
    wait()
    done()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert not os.path.exists(name)
        return
    with open(name, "rb") as f:
        assert f.read(4) == b"\x89PNG"
    assert os.path.exists(lay.ckp(name))


def test_alt_cfgs_replace_the_lines_for_this_stage(tmp_path, with_ctx):
    alt = tmp_path / "alt.config"
    alt.write_text("# another grouping\nold2,c1\tc0\n")
    p, stub, lay, d_size = _pipe(tmp_path, [[["c0"], ["c1"]]], alt_cfgs=[str(alt)], d_targets={"old2": "c2"})
    with_ctx(stub)
    p.stage_blocks(lay, LABELS, d_size)
    assert [c[1:3] for c in stub.calls if c[0] == "pair"] == [(2, 0), (1, 0)]
    assert p.sgs == [[["c0"], ["c1"]]]
    assert open(lay.out("blocks.tsv")).read().startswith(bl.HEADER)


def test_switches_that_skip_the_stage(monkeypatch):
    """-just_core, -disable_circos and -disable_blocks: the reference's conditions; the stage follows the feature stage"""
    def run(**flags):
        opts = dict(outdir="o", tmpdir="t", disable_ltr=True, custom_features=["f.bed"])
        opts.update(flags)
        p = pipeline.Pipeline.bare(**opts)
        order = []

        class _Cl:
            d_sg, sg_names = {}, []
        monkeypatch.setattr(pipeline, "Layout", lambda *a: "lay")
        monkeypatch.setattr(p, "stage_ingest", lambda lay: (order.append("ingest"), (["f"], ["c"], {"c": 1}, {}))[1], raising=False)
        monkeypatch.setattr(p, "stage_count_filter", lambda *a: order.append("count"), raising=False)
        monkeypatch.setattr(p, "stage_cluster", lambda *a: (order.append("cluster"), (_Cl(), None))[1], raising=False)
        monkeypatch.setattr(p, "stage_windows", lambda *a: order.append("windows"), raising=False)
        monkeypatch.setattr(p, "stage_features", lambda *a: order.append("features"), raising=False)
        monkeypatch.setattr(p, "stage_blocks", lambda *a: order.append("blocks"), raising=False)
        p._run()
        return order
    assert run() == ["ingest", "count", "cluster", "windows", "features", "blocks"]
    assert run(custom_features=None) == ["ingest", "count", "cluster", "windows", "blocks"]
    assert run(disable_blocks=True) == ["ingest", "count", "cluster", "windows", "features"]
    assert run(disable_circos=True) == ["ingest", "count", "cluster", "windows", "features"]
    assert run(just_core=True) == ["ingest", "count", "cluster"]


def test_one_line_fallbacks(tmp_path, with_ctx, caplog, monkeypatch):
    # a context without the entries
    p, stub, lay, d_size = _pipe(tmp_path, [[["c0"], ["c1"]]])
    class _Bare:
        h = 1
    with_ctx(_Bare())
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_blocks(lay, LABELS, d_size)
    assert [r.getMessage() for r in caplog.records] == ["blocks skipped: this context has no block entries"]
    assert not os.path.exists(lay.out("blocks.tsv")) and not p._background
    # a multi-rank run
    caplog.clear()
    with_ctx(stub)
    monkeypatch.setenv("WORLD_SIZE", "4")
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_blocks(lay, LABELS, d_size)
    assert [r.getMessage() for r in caplog.records] == ["blocks skipped: the stage runs on one GPU, this is a run of 4 ranks"]
    assert not stub.calls and not os.path.exists(lay.out("blocks.tsv"))
    monkeypatch.delenv("WORLD_SIZE")
    # -aligner / -aligner_options: one warning each, and the stage runs
    caplog.clear()
    p.aligner, p.aligner_options = "minimap2", "-x asm5"
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_blocks(lay, LABELS, d_size)
    warn = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warn) == 2 and all("no aligner is run" in m for m in warn)
    assert os.path.exists(lay.out("blocks.tsv"))


def test_a_failure_costs_the_files_and_nothing_else(tmp_path, with_ctx, caplog):
    p, stub, lay, d_size = _pipe(tmp_path, [[["c0"], ["c1"]]])

    def boom(*a):
        raise MemoryError("sp_blocks_index: an index of 1 bytes does not fit on the device")
    stub.blocks_index = boom
    earlier = tmp_path / "run.bin.enrich"
    earlier.write_text("kept\n")
    with_ctx(stub)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_blocks(lay, LABELS, d_size)          # does not raise
    warn = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert warn == ["blocks not written: sp_blocks_index: an index of 1 bytes does not fit on the device"]
    assert sorted(os.listdir(tmp_path)) == ["run.bin.enrich"] and earlier.read_text() == "kept\n"
    assert stub.calls[-1] == ("release", -1) and not p._background


def test_a_figure_that_fails_is_a_warning(tmp_path, with_ctx, caplog, monkeypatch):
    p, stub, lay, d_size = _pipe(tmp_path, [[["c0"], ["c1"]]])

    def boom(*a):
        raise OSError("no room for the figure")
    monkeypatch.setattr(bl, "plot", boom)
    with_ctx(stub)
    with caplog.at_level(logging.INFO, logger="subphaser_amd"):
        p.stage_blocks(lay, LABELS, d_size)
        p._finish_background()                       # does not raise: the run goes on
    warn = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warn) == 1 and warn[0].startswith("blocks not plotted: ") and not p._background
    try:
        import matplotlib  # noqa: F401
        assert warn == ["blocks not plotted: no room for the figure"]
    except ImportError:
        pass
    assert os.path.exists(lay.ckp(lay.out("blocks.tsv"))) and not os.path.exists(lay.ckp(lay.out("blocks.png")))


def test_cli_options():
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config"])
    assert (args.block_k, args.block_sample, args.block_bin, args.block_votes, args.block_gap, args.min_block) == (21, 4, 50000, 5, 5, 100000)
    assert args.alt_cfgs is None and not args.disable_blocks and args.aligner is None
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-block_k", "25", "-block_sample", "0", "-block_bin", "500",
                                  "-block_votes", "1", "-block_gap", "0", "-min_block", "7", "-alt_cfgs", "a", "b", "-disable_blocks"])
    assert (args.block_k, args.block_sample, args.block_bin, args.block_votes, args.block_gap, args.min_block) == (25, 0, 500, 1, 0, 7)
    assert args.alt_cfgs == ["a", "b"] and args.disable_blocks
