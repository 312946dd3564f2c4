"""CPU: the host arithmetic of the domain trees (subphaser_amd/domtree.py): the common profile and its ties, the window
and its clipping at both ends of a frame, the row strings, trimming exactly on the threshold, `unique`, the distance units
and their cap, the three file formats, and catAln / format_id_for_iqtree of the reference as recorded in
tests/golden/golden_domtree.json.gz (tests/golden/gen_golden_domtree.py)."""
import gzip
import io
import json
import math
import os

import numpy as np
import pytest

import domalign_ref as da
from subphaser_amd import domains, domtree, ltrtree

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden_domtree():
    with gzip.open(os.path.join(HERE, "golden", "golden_domtree.json.gz"), "rt") as f:
        return json.load(f)


def test_common_profile_and_its_ties():
    assert domtree.common_profile([5]) == 5
    assert domtree.common_profile([7, 2, 7, 2, 7]) == 7
    assert domtree.common_profile([7, 2, 7, 2]) == 2            # a tie: the lowest index
    assert domtree.common_profile([9, 3, 4]) == 3
    assert domtree.common_profile(np.array([4, 4, 1, 1, 0], np.int32)) == 1


def test_window_is_clipped_at_both_ends_of_a_frame():
    assert domtree.PAD == 32
    assert domtree.window(100, 180, 400) == (68, 212)
    assert domtree.window(32, 180, 213) == (0, 212)             # exactly on both ends
    assert domtree.window(31, 180, 212) == (0, 211)             # clipped at both
    assert domtree.window(0, 0, 1) == (0, 0)
    assert domtree.window(5, 9, 100, pad=0) == (5, 9)
    # sp_dm_nres
    assert [domtree.n_residues(n, f) for n, f in ((0, 0), (1, 2), (2, 2), (3, 0), (10, 1), (10, 5), (11, 5))] == [0, 0, 0, 1, 3, 2, 3]


def test_row_strings():
    codes = [0, 19, 20, 21, 4]                                  # A Y X * F at frame indices 10 .. 14
    assert domtree.row_string([10, -1, 11, 12, 13, -1, 14], 10, codes) == "A-YX*-F"
    assert domtree.row_string([-1, -1], 3, []) == "--"
    assert domtree.peptide(codes) == "AYX*F" and domtree.LETTERS == da.LETTERS
    enc = domtree.encode(["A-YX*", "CCCCC"])
    assert enc.dtype == np.uint8 and enc.tolist() == [[0, 255, 19, 20, 21], [1, 1, 1, 1, 1]]


def test_trimming_exactly_on_the_threshold():
    rows = ["AA-A", "A--X", "A-A*", "A---"]                      # residues per column: 4, 1, 1, 1 (X and stop are none)
    assert domtree.trim_columns(rows, 50) == [0]
    assert domtree.trim_columns(rows, 25) == [0, 1, 2, 3]        # 100 * 1 >= 25 * 4: exactly on it
    assert domtree.trim_columns(rows, 26) == [0]
    assert domtree.trim_columns(rows, 0) == [0, 1, 2, 3] and domtree.trim_columns(rows, 100) == [0]
    assert domtree.trim(rows, 25) == rows and domtree.trim(rows, 50) == ["A", "A", "A", "A"]
    rows3 = ["A-", "AC", "-C"]                                   # 2 of 3 = 66.67 %
    assert domtree.trim_columns(rows3, 66) == [0, 1] and domtree.trim_columns(rows3, 67) == []
    assert domtree.trim(rows3, 67) == ["", "", ""]


def test_unique_drops_later_equal_rows():
    desc, kept, dropped = domtree.cat_rows(["a", "b", "c", "d"], [["AC", "AC", "A-", "AC"], ["K", "K", "K", "R"]], unique=True)
    assert desc == "genes:2 sites:3 blocks:[2, 1]" and kept == [("a", "ACK"), ("c", "A-K"), ("d", "ACR")] and dropped == 1
    desc, kept, dropped = domtree.cat_rows(["a", "b"], [["AC", "AC"]], unique=False)
    assert kept == [("a", "AC"), ("b", "AC")] and dropped == 0
    assert domtree.cat_rows([], [[], []]) == ("genes:2 sites:0 blocks:[0, 0]", [], 0)


def test_golden_rows_of_catAln(golden_domtree):
    for name, case in golden_domtree["cases"].items():
        for unique in (False, True):
            desc, kept, dropped = domtree.cat_rows(case["ids"], case["blocks"], unique=unique)
            out = io.StringIO()
            domtree.write_aln(out, kept, desc)
            assert out.getvalue() == case["text"][str(unique)], (name, unique)
            assert len(kept) + dropped == len(case["ids"])
    assert golden_domtree["cases"]["all_equal"]["text"]["True"].count(">") == 1
    for raw, want in golden_domtree["ids"].items():
        assert domtree.format_id_for_iqtree(raw) == want, raw


def test_distance_units_and_the_cap():
    U = ltrtree.UNIT
    assert domtree.D_CAP == 2130444828 == int(math.floor(-math.log(1 - 0.75 - 0.75 ** 2 / 5) * U + 0.5)) < 1 << 31
    assert domtree.kimura_units([40], [40]).tolist() == [0]                      # same == both
    assert domtree.kimura_units([30], [40]).tolist() == [int(math.floor(-math.log(1 - 0.25 - 0.0125) * U + 0.5))]
    # both sides of p = 0.75: 25 of 100, 24 of 100 (beyond: capped), 26 of 100 (below)
    assert domtree.kimura_units([25, 24, 0], [100, 100, 100]).tolist() == [domtree.D_CAP] * 3
    d26 = int(domtree.kimura_units([26], [100])[0])
    assert d26 == int(math.floor(-math.log(1 - 0.74 - 0.74 ** 2 / 5) * U + 0.5)) < domtree.D_CAP
    # both sides of the overlap: 19 shared columns are too few, 20 are enough
    assert domtree.OVERLAP == 20
    assert domtree.kimura_units([19, 20], [19, 20]).tolist() == [domtree.D_CAP, 0]
    assert domtree.kimura_units([4, 5], [4, 5], overlap=5).tolist() == [domtree.D_CAP, 0]
    assert domtree.kimura_units([0], [0], overlap=0).tolist() == [domtree.D_CAP]
    with pytest.raises(ValueError):
        domtree.kimura_units([5], [4])
    rows = domtree.encode(["ACDEFGHIKLMNPQRSTVWYAC", "ACDEFGHIKLMNPQRSTVWYAA", "----------------------", "ACDEFGHIKL------------"])
    same, both = da.aln_pairs(rows)
    D = domtree.distance_matrix(same, both)
    assert D.dtype == np.int64 and (D == D.T).all() and (np.diag(D) == 0).all() and D.max() <= domtree.D_CAP
    assert D[0, 1] == int(domtree.kimura_units([21], [22])[0]) and D[0, 2] == D[2, 3] == domtree.D_CAP
    assert D[0, 3] == domtree.D_CAP                              # 10 shared columns: below the overlap
    assert (D == domtree.kimura_units(same, both) * (1 - np.eye(4, dtype=np.int64))).all()


def test_the_three_file_formats():
    d = domains.Domain()
    d.element, d.profile, d.gene, d.clade, d.coverage, d.score = "chrA:10-2009:10-209", "Class_I/LTR/Ty1_copia/Ale:Ty1-RT", "RT", "Ale", 97.5, 1.25
    rows = [["chrA:10-2009:10-209", "LTR", "Copia", "Ale", "yes", "+", "RT|Ale"]]
    out = io.StringIO()
    domtree.write_pep(out, [d], rows, ["MKVL*X"])
    assert out.getvalue() == (">chrA:10-2009:10-209#LTR/Copia/Ale#RT|Ale ID=chrA:10-2009:10-209|Class_I/LTR/Ty1_copia/Ale:Ty1-RT;"
                              "Name=Ale-RT;gene=RT;clade=Ale;coverage=97.5;score=1.25\nMKVL*X\n")
    # what concat_domains reads back from such a record (its three regular expressions)
    import re
    head = out.getvalue().splitlines()[0][1:]
    rid, cid, did = re.compile(r"^(\S+)#(\S+)#(\S+)$").match(head.split()[0]).groups()
    assert (rid, cid, did) == ("chrA:10-2009:10-209", "LTR/Copia/Ale", "RT|Ale")
    assert re.compile(r"gene=([^;\s]+)").search(head).group(1) == "RT" and re.compile(r"clade=([^;\s]+)").search(head).group(1) == "Ale"
    assert domtree.fmt_cls("LTR", "Copia", "unknown") == "LTR/Copia" and domtree.fmt_cls("mixture", "mixture", "mixture") == "mixture"
    out = io.StringIO()
    domtree.write_aln(out, [("chrA_10_2009_10_209", "MK-V"), ("b", "MKAV")], "genes:1 sites:4 blocks:[4]")
    assert out.getvalue() == ">chrA_10_2009_10_209 genes:1 sites:4 blocks:[4]\nMK-V\n>b genes:1 sites:4 blocks:[4]\nMKAV\n"
    out = io.StringIO()
    ltrtree.write_map(out, ["chrA_10_2009_10_209", "b"], ["SG1", "SG2"], ["Ale", "Tekay"])
    assert out.getvalue() == "label\tClade\tSubgenome\nchrA_10_2009_10_209\tAle\tSG1\nb\tTekay\tSG2\n"


def test_select_keeps_the_elements_with_every_domain():
    doms = {"a": {"RT": 1, "INT": 1, "RH": 1}, "b": {"RT": 1, "INT": 1}, "c": {"RT": 1, "INT": 1, "RH": 1, "GAG": 1}, "d": {"RT": 1, "INT": 1, "RH": 1}}
    classes = {"a": ("LTR", "Copia"), "b": ("LTR", "Copia"), "c": ("LTR", "Copia"), "d": ("LTR", "Gypsy")}
    sel, counts = domtree.select(["a", "b", "c", "d", "e"], doms, classes, "LTR", "Copia", ["INT", "RT", "RH"])
    assert sel == ["a", "c"] and counts == {"INT": 3, "RT": 3, "RH": 2}
    sel, counts = domtree.select(["a", "b", "c", "d"], doms, classes, "LTR", "Copia", ["RT"])
    assert sel == ["a", "b", "c"] and counts == {"RT": 3}
    assert domtree.select(["a"], doms, classes, "LTR", "Gypsy", ["RT"]) == ([], {"RT": 0})
