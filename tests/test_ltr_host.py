"""subphaser_amd/ltr.py against what the reference's LTR module made of the same `.scn` (tests/golden/golden_ltr.json.gz,
recorded by tests/golden/gen_golden_ltr.py): the reader and the derived coordinates, overlap resolution, ages, and the
`.ltr.insert.data` / `.ltr.insert.summary` writers under the four combinations of -exclude_exchanges and -non_specific."""
import gzip
import io
import json
import logging
import math
import os

import pytest

from subphaser_amd import ltr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    with gzip.open(os.path.join(HERE, "golden", "golden_ltr.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture
def records(gold, tmp_path):
    path = tmp_path / "LTR.scn"
    path.write_text(gold["scn"])
    return ltr.read_scn(str(path))


def test_reader_and_derived_coordinates(gold, records):
    got = [[r.id, r.start, r.end, r.element_len, r.lltr, r.rltr, r.lltr_e, r.rltr_s, r.similarity, r.seq_nr, r.seq_id] for r in records]
    assert got == gold["records"]
    assert any("#" in line and not line.startswith("#") for line in gold["scn"].splitlines())      # a trailing #source column
    assert any(r.element_len != r.end - r.start + 1 for r in records)
    for r in records:
        assert r.id == "%s:%d-%d:%d-%d" % (r.seq_id, r.start, r.end, r.start + r.lltr - 1, r.end - r.rltr + 1)


def test_raw_ltrharvest_format_names_the_missing_column(tmp_path):
    path = tmp_path / "raw.scn"
    path.write_text("# ltrharvest\n100 2100 2001 100 300 201 1900 2100 201 95.5 0\n")
    with pytest.raises(ValueError, match=r"raw\.scn:2: 11 columns.*column 12, the sequence id, is missing"):
        ltr.read_scn(str(path))
    path.write_text("100 2100 2001 100 300\n")
    with pytest.raises(ValueError, match="unrecognized LTRHarvest format"):
        ltr.read_scn(str(path))
    path.write_text("#only comments\n\n")
    assert ltr.read_scn(str(path)) == []


def _known(gold, records):
    return [r for r in records if r.seq_id in gold["d_sg"]]


def test_overlap_resolution(gold, records):
    known = _known(gold, records)
    assert len(known) == len(records) - 1
    got = ltr.group_resolve_overlaps(known)
    assert [r.id for r in got] == gold["resolved"]
    assert len(got) < len(known)
    # the cases the fixture was built around
    ids = set(gold["resolved"])
    assert "A1:1000-2999:1199-2800" not in ids            # listed twice: an equal record takes its key with it
    assert "B1:20000-21999:20199-21800" in ids and "B1:20150-21949:20349-21750" not in ids      # 90 %: the shorter goes
    # 21900-22899 overlaps the first by 9.9 % of its 1000 bases, which is not above max_ovl: it stays and is what the next is
    # compared with -- 10.9 %, and the next is longer
    assert "B1:21900-22899:22019-22780" not in ids and "B1:22790-23889:22909-23770" in ids
    runs = [r.seq_id for i, r in enumerate(got) if i == 0 or got[i - 1].seq_id != r.seq_id]
    assert runs.count("B1") == 2                          # a sequence that comes back is a run of its own


def test_overlap_rules_by_hand():
    def rec(start, end, length=None, lltr=100, rltr=100, chrom="c"):
        return ltr.Record([start, end, length or end - start + 1, start, start + lltr - 1, lltr, end - rltr + 1, end, rltr, 90.0, 0, chrom])
    a, b = rec(1, 1000), rec(950, 2500)                   # 50 / 1000 = 5 %
    assert ltr.resolve_overlaps([b, a]) == [a, b]
    a, b = rec(1, 1000), rec(800, 2500)                   # 20 %: the longer stays
    assert ltr.resolve_overlaps([a, b]) == [b]
    a, b, c = rec(1, 3000), rec(800, 2500), rec(2950, 4000)       # b goes, c is compared with a: 50 / 1051 below 10 %
    assert ltr.resolve_overlaps([a, b, c]) == [a, c]
    a, b = rec(1, 1000), rec(500, 1499)                   # equal lengths: the earlier stays
    assert ltr.resolve_overlaps([a, b]) == [a]
    a, b = rec(1, 1000), rec(1, 1000, lltr=120)           # equal start and end, another lltr_e: not equal, full overlap
    assert ltr.resolve_overlaps([a, b]) == [a]
    a, b, c = rec(1, 1000), rec(5000, 6000), rec(1, 1000)         # equal records: both go (set difference by key)
    assert ltr.resolve_overlaps([a, b, c]) == [b]
    a, b = rec(7, 900), rec(7, 100, length=5000)          # 93 / 894 = 10.4 %; lengths are the file's third column: b stays
    assert ltr.resolve_overlaps([a, b]) == [b]
    a, b = rec(7, 900), rec(7, 60)                        # 53 / 54: above -- a is longer
    assert ltr.resolve_overlaps([b, a]) == [a]
    a, b = rec(7, 900), rec(7, 2000)                      # equal starts, no winner by order: the output is sorted by end
    assert ltr.resolve_overlaps([b, a]) == [b]
    assert ltr.group_resolve_overlaps([]) == []
    x, y = rec(1, 1000, chrom="x"), rec(1, 1000, chrom="y")
    assert ltr.group_resolve_overlaps([x, y]) == [x, y]


def test_ages(gold, records):
    got = ltr.group_resolve_overlaps(_known(gold, records))
    divs, fell = ltr.divergences(got, None, "scn")
    assert fell == 0
    ages = [ltr.estimate_age(d, gold["mu"]) for d in divs]
    assert ages == gold["ages"]                           # the same float operations in the same order
    sims = {r.similarity for r in got}
    assert 100.0 in sims and 20.0 in sims and 25.0 in sims and 25.1 in sims
    assert ltr.estimate_age(0.0, 13e-9) == 0.0
    assert ltr.estimate_age(0.75, 13e-9) == 0.75 / (13e-9 * 2)
    assert ltr.estimate_age(0.8, 7e-9) == 0.8 / (7e-9 * 2)
    assert ltr.estimate_age(0.1, 7e-9) == -3 / 4 * math.log(1 - 4 * 0.1 / 3) / (7e-9 * 2)


def test_divergence_from_alignment_counts():
    class R:
        similarity = 90.0
    rows = [[10, 95, 5, 2, 1, 0], [10, 95, 5, 2, 1, ltr.FLAG_EDGE], [0, 0, 0, 3, 4, 0], [0, 0, 0, 0, 0, ltr.FLAG_BAND],
            [0, 0, 0, 0, 0, ltr.FLAG_LEN], [4, 2, 0, 0, 0, 0]]
    divs, fell = ltr.divergences([R()] * 6, rows, "align")
    assert divs == [0.05, 0.05, 1 - 90.0 / 100, 1 - 90.0 / 100, 1 - 90.0 / 100, 0.0] and fell == 3
    divs, fell = ltr.divergences([R()] * 6, rows, "scn")
    assert divs == [1 - 90.0 / 100] * 6 and fell == 0


@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("nonspec", [False, True])
def test_insert_data_and_summary(gold, records, caplog, excl, nonspec):
    got = ltr.group_resolve_overlaps(_known(gold, records))
    ages = [ltr.estimate_age(d, gold["mu"]) for d in ltr.divergences(got, None, "scn")[0]]
    want = gold["insert"]["%d%d" % (excl, nonspec)]
    data, summary = io.StringIO(), io.StringIO()
    d_data, enriched, excluded = ltr.write_insert_data(data, got, ages, gold["d_enriched"], gold["d_exchange"],
                                                       exclude_exchanges=excl, non_specific=nonspec)
    assert data.getvalue() == want["data"]
    assert len(enriched) == len(gold["d_enriched"])
    n_yes = sum(gold["d_exchange"][i] == "yes" for i in gold["d_enriched"])
    assert n_yes > 0 and excluded == (n_yes if excl else 0)
    assert ("non-specific" in d_data) == nonspec
    with caplog.at_level(logging.INFO):
        ltr.summary_ltr_time(d_data, summary)
    assert summary.getvalue() == want["summary"]
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("\tmedian: ") for m in msgs)
    assert any(m.startswith("A rough estimation of the divergence–hybridization period: ") for m in msgs)


def test_summary_by_hand(gold):
    hand = gold["summary_hand"]
    out = io.StringIO()
    assert ltr.summary_ltr_time(hand["d_data"], out) == hand["d_info"]
    assert out.getvalue() == hand["text"]
