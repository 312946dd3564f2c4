#!/usr/bin/env python3
"""Generate tests/golden/golden_domtree.json.gz by IMPORTING the reference's copy of TEsorter's concatenate_domains here.

Run where the reference checkout that gen_golden.py points at exists:

    python tests/golden/gen_golden_domtree.py

The reference is imported unmodified, with the stand-ins of gen_golden.py for the third-party packages this image lacks (its
FASTA reader stands in for Bio.SeqIO.parse: the id is the first word of the header, the sequence the joined lines).  What
runs is catAln on a few hand alignments, with and without `unique`, and format_id_for_iqtree on a few ids.  The fixture
holds inputs (the aligned rows per domain, the ids) and recorded results (the text catAln prints, the formatted ids) only."""
import gzip
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts oracle/, tests/ and the repository on sys.path)

# name -> (ids, blocks: per domain the rows of the ids, in order)
CASES = {
    "three_domains": (["chrA_10_2009_10_209", "chrA_3000_5000_3000_3100", "chrB_1_900_1_120"],
                      [["MKV-L", "MKVAL", "-KVAL"], ["QQ", "Q-", "QQ"], ["WYW--F", "WYWAAF", "WYW--F"]]),
    "duplicates": (["e1", "e2", "e3", "e4", "e5"], [["AC-", "AC-", "ACD", "AC-", "ACD"], ["GG", "GG", "GG", "GA", "GG"]]),
    "one_domain": (["x", "y"], [["ACDEFGHIKLMNPQRSTVWY", "ACDEFGHIKLMNPQRSTVW-"]]),
    "all_equal": (["p", "q", "r"], [["AAA", "AAA", "AAA"]]),
    "stop_and_x": (["s1", "s2"], [["A*X-", "AXX*"], ["-", "K"]]),
}
IDS = ["chrA:10-2009:10-209", "Chr01:1..5#LTR/Copia", "a|b;c=d", "plain_id", "x  y\tz", "a.b-c:d", "__a__", "é:1"]


def main():
    tmp = tempfile.mkdtemp(prefix="sp_golden_domtree_")
    gg.install_standins(tmp)
    import logging
    logging.disable(logging.CRITICAL)
    from subphaser.api.TEsorter.modules import concatenate_domains as cd  # noqa

    cases = {}
    for name, (ids, blocks) in CASES.items():
        files = []
        for d, rows in enumerate(blocks):
            path = os.path.join(tmp, "%s.%d.fa.alignment" % (name, d))
            with open(path, "w") as f:
                for i, row in zip(ids, rows):
                    f.write(">%s\n%s\n" % (i, row))
            files.append(path)
        text = {}
        for unique in (False, True):
            out = io.StringIO()
            handles = [open(path) for path in files]      # (the stand-in reader takes a handle where Bio.SeqIO.parse also takes a path)
            cd.catAln(handles, out, unique=unique)
            for h in handles:
                h.close()
            text[str(unique)] = out.getvalue()
        cases[name] = {"ids": ids, "blocks": blocks, "text": text}
    fixture = {"cases": cases, "ids": {i: cd.format_id_for_iqtree(i) for i in IDS}}
    path = os.path.join(HERE, "golden_domtree.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(fixture, sort_keys=True).encode())
    print("wrote %s (%d bytes): %d alignments, %d ids" % (path, os.path.getsize(path), len(cases), len(IDS)))


if __name__ == "__main__":
    main()
