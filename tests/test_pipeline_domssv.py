"""Pipeline.stage_ltr under -ltr_dom_prefilter without a GPU: the world and the oracle context of
test_pipeline_domains.py, with the twins (tests/domains_ref.py, tests/domssv_ref.py) behind dom_search.  Without the flag
dom_search is called as before and the two files are byte for byte test_pipeline_domains.py's; with it they are the
filtered twin's; the bare flag takes domains.PREFILTER_BITS; the flag without -ltr_hmm is an error at both places; the
log line has the counts."""
import io
import math

import numpy as np
import pytest

import domains_ref as dr
import domssv_ref as sr
from test_pipeline_ltrdetect import with_ctx  # noqa: F401  (fixture)
from test_pipeline_domains import _DomCtx, _dom_run, world  # noqa: F401  (fixture)
from subphaser_amd import domains, ltr, pipeline


class _PreCtx(_DomCtx):
    def dom_search(self, chrom, start, end, moff, emis, trans, entry, **kw):
        if not kw:
            self.calls.append(("plain",))
            return _DomCtx.dom_search(self, chrom, start, end, moff, emis, trans, entry)
        assert set(kw) == {"prefilter", "stats"} and isinstance(kw["prefilter"], int)
        plain = _DomCtx.dom_search(self, chrom, start, end, moff, emis, trans, entry)      # (brings self.profs to the reader's integers)
        self.calls.append(("pre", kw["prefilter"]))
        seqs = [self._seq(c)[a:b] for c, a, b in zip(map(int, chrom), map(int, start), map(int, end))]
        out, items, passed = sr.search(seqs, self.profs, kw["prefilter"])
        kw["stats"]["items"] = kw["stats"].get("items", 0) + items
        kw["stats"]["passed"] = kw["stats"].get("passed", 0) + passed
        self.last = (out, items, passed, plain)
        return out


def _run(tmp, world, caplog, with_ctx, **over):
    world[2](_DomCtx)      # (the world hands its profiles to _DomCtx alone: _PreCtx inherits them)
    return _dom_run(tmp, world, caplog, with_ctx, cls=_PreCtx, **over)


_memo = {}


def _files(lay):
    return {ext: open(lay.out(ext)).read() for ext in ("ltr.dom.gff3", "ltr.cls.tsv")}


def _expected(world, T):
    """the two files by the filtered twin at threshold T (1/256 bit), straight from the `.scn` and the `.hmm`"""
    if T in _memo:
        return _memo[T]
    chroms, _, _, hmm, scn, _ = world
    labels = _labels()
    P = domains.read_hmm(hmm)
    twins = [dr.make_profile(M, P.emis[a:a + M], P.trans[a:a + M], entry=e, name=n) for M, a, e, n in zip(P.M, P.moff.tolist(), P.entry.tolist(), P.names)]
    recs = ltr.read_scn(scn)
    ival = [domains.inner_interval(r) for r in recs]
    seqs = [chroms[labels.index(r.seq_id)][a:b] for r, (a, b) in zip(recs, ival)]
    hits, items, passed = sr.search(seqs, twins, T)
    doms = domains.best_domains([r.id for r in recs], [b - a for a, b in ival], hits, P)
    gff, cls = io.StringIO(), io.StringIO()
    domains.write_gff(gff, doms)
    domains.write_cls(cls, domains.classify(doms))
    _memo[T] = ({"ltr.dom.gff3": gff.getvalue(), "ltr.cls.tsv": cls.getvalue()}, items, passed)
    return _memo[T]


def _labels():
    from test_pipeline_ltrdetect import LABELS
    return list(LABELS)


def test_flag_off_is_the_search_of_before(tmp_path, world, caplog, with_ctx):
    p0, lay0, ctx0, log0 = _dom_run(tmp_path / "before", world, caplog, with_ctx)                 # test_pipeline_domains.py's context
    p, lay, ctx, log = _run(tmp_path / "off", world, caplog, with_ctx)
    assert [c for c in ctx.calls if c[0] in ("plain", "pre")] == [("plain",)]
    assert _files(lay) == _files(lay0) and len(_files(lay)["ltr.dom.gff3"].splitlines()) == 40
    assert not any("prefilter" in m for m in log)
    assert pipeline.option_defaults()["ltr_dom_prefilter"] is None


def test_flag_on_is_the_filtered_twin(tmp_path, world, caplog, with_ctx):
    plain = _files(_run(tmp_path / "plain", world, caplog, with_ctx)[1])
    # 40 bits: every planted domain (40 nodes on their consensus, some 90 bits ungapped) passes and random frames do not
    p, lay, ctx, log = _run(tmp_path / "t40", world, caplog, with_ctx, ltr_dom_prefilter=40.0)
    assert ("pre", 40 * 256) in ctx.calls and ("plain",) not in ctx.calls
    want, items, passed = _expected(world, 40 * 256)
    assert _files(lay) == want == plain and (items, passed) == (12 * 6 * 10, 40)      # the 8 x 5 planted domains, each in its frame
    line = [m for m in log if "inner sequences x 10 profiles searched" in m]
    assert len(line) == 1 and line[0].endswith("; ungapped prefilter at 40.0 bits: %d of %d (frame, profile) pairs (%.2f%%) searched"
                                               % (passed, items, 1e2 * passed / items))
    # a threshold no segment reaches: no domain, no LTR
    p2, lay2, ctx2, log2 = _run(tmp_path / "t500", world, caplog, with_ctx, ltr_dom_prefilter=500.0)
    want2, items2, passed2 = _expected(world, 500 * 256)
    assert _files(lay2) == want2 and want2["ltr.dom.gff3"] == "" and (items2, passed2) == (items, 0)
    assert any(m.endswith("prefilter at 500.0 bits: 0 of %d (frame, profile) pairs (0.00%%) searched" % items) for m in log2)
    # a fractional threshold goes up to the next 1/256 bit, and one between the domains' scores loses some of them
    scores = np.sort(ctx.last[0][:, :, 0][ctx.last[0][:, :, 0] > 0])
    mid = float(scores[len(scores) // 2]) / 256 + 0.001      # (the hits' scores bound their ssv from above)
    p3, lay3, ctx3, log3 = _run(tmp_path / "mid", world, caplog, with_ctx, ltr_dom_prefilter=mid)
    assert ("pre", int(math.ceil(mid * 256))) in ctx3.calls
    want3, _, passed3 = _expected(world, int(math.ceil(mid * 256)))
    assert _files(lay3) == want3 and 0 < len(want3["ltr.dom.gff3"].splitlines()) < 40 and 0 < passed3 < passed


def test_bare_flag_takes_the_default(tmp_path, world, caplog, with_ctx):
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_hmm", "x.hmm", "-ltr_dom_prefilter"])
    assert args.ltr_dom_prefilter == domains.PREFILTER_BITS and float(domains.PREFILTER_BITS) == int(domains.PREFILTER_BITS)
    args = pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_hmm", "x.hmm", "-ltr_dom_prefilter", "21.5", "-ltr_dom_cov", "30"])
    assert (args.ltr_dom_prefilter, args.ltr_dom_cov) == (21.5, 30.0)
    assert pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_hmm", "x.hmm"]).ltr_dom_prefilter is None
    p, lay, ctx, log = _run(tmp_path / "bare", world, caplog, with_ctx, ltr_dom_prefilter=args_default())
    assert ("pre", int(math.ceil(domains.PREFILTER_BITS * 256))) in ctx.calls
    assert _files(lay) == _expected(world, int(math.ceil(domains.PREFILTER_BITS * 256)))[0]


def args_default():
    return pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_hmm", "x.hmm", "-ltr_dom_prefilter"]).ltr_dom_prefilter


def test_flag_without_ltr_hmm_is_an_error(tmp_path, world, caplog, with_ctx, capsys):
    with pytest.raises(SystemExit):
        pipeline.makeArgparse(["-i", "g.fa", "-c", "sg.config", "-ltr_dom_prefilter", "20"])
    assert "-ltr_dom_prefilter filters the domain search of the classification: give -ltr_hmm FILE as well" in capsys.readouterr().err
    with pytest.raises(ValueError, match="-ltr_dom_prefilter filters the domain search of the classification: give -ltr_hmm FILE"):
        _run(tmp_path / "nohmm", world, caplog, with_ctx, ltr_hmm=None, ltr_dom_prefilter=20.0)
