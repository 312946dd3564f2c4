"""The hand-made chromosomes of tests/s3_cases.py against the oracle, on the CPU: the cap that keeps a device test from hiding
behind a wrong construction.

For every case the oracle counts every chromosome at lower 1 and its keys are grouped by fine bucket (key >> R2).  The designed
buckets must hold exactly the designed residuals with the designed copies -- so n and the distinct count of every bucket, and
of every piece s3_final cuts it into, are the declared ones -- no key may lie outside them, and every key must be its own
canonical form.  The routing model applied to what the oracle found must give the declaration the case was built with, at
every `lower` the case runs.  Finally every path that the suite did not reach before (s3_cases.REQUIRED_TAGS) must be the
declared route of at least one case: a set comparison."""
import numpy as np
import pytest

import s3_cases as sc


def _found(case):
    """per chromosome: the oracle's keys as a design {bucket: (residuals, counts)}"""
    R2 = np.uint64(sc.Plan(case.k).R2)
    out = []
    for keys, cnts in sc.oracle_counts(case.name):
        assert (keys <= sc.revcomp(keys, case.k)).all()
        assert (keys[1:] > keys[:-1]).all()
        b = (keys >> R2).astype(np.int64)
        res = keys & ((np.uint64(1) << R2) - np.uint64(1))
        ub, at = np.unique(b, return_index=True)              # (keys ascend, so a bucket is one stretch)
        end = np.append(at[1:], len(b))
        out.append({int(x): (res[i:j], cnts[i:j].astype(np.int64)) for x, i, j in zip(ub, at, end)})
    return out


def _plain(d):
    return {k: (sorted(v) if isinstance(v, set) else v) for k, v in d.items()}


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_case_holds_what_it_declares(name):
    case = sc.BY_NAME[name]
    found = _found(case)
    assert len(found) == len(case.chroms)
    for ci, c in enumerate(case.chroms):
        if c.design is None:
            continue
        assert sorted(found[ci]) == sorted(c.design), (name, ci, "keys outside the designed buckets")
        for b, (res, cp) in c.design.items():
            fres, fcnt = found[ci][b]
            assert len(fres) == len(res) and int(fcnt.sum()) == int(cp.sum()), (name, ci, b, len(fres), len(res), int(fcnt.sum()), int(cp.sum()))
            assert (fres == res).all() and (fcnt == cp).all(), (name, ci, b)
    designs = [found[ci] if c.design is not None else None for ci, c in enumerate(case.chroms)]
    for lower in case.lowers:
        want, got = case.declared(lower), case.declared(lower, designs)
        assert want["first"] == got["first"] and want["n_big"] == got["n_big"] and want["rle"] == got["rle"]
        assert want["tags"] == got["tags"]
        for rw, rg in zip(want["chroms"], got["chroms"]):
            assert sorted(rw) == sorted(rg)
            for b in rw:
                assert _plain(rw[b]) == _plain(rg[b]), (name, lower, b)
    assert sum(len(s) for s in case.seqs()) == case.n_bases()      # (what decides whether the case counts as small)


def test_every_new_path_is_some_cases_declared_route():
    covered = set()
    for case in sc.CASES:
        for lower in case.lowers:
            covered |= case.declared(lower)["tags"]
    assert sc.REQUIRED_TAGS - covered == set()
    # the named routes, by the case that was built for them
    def route(name, lower, chrom=0, bucket=0):
        return sc.BY_NAME[name].declared(lower)["chroms"][chrom][bucket]
    r = route("bitmap_4097_distinct_x1_k17", 1)
    assert r["handed"] and r["sb"] == 2 and all(p[3].startswith("piece_sort") for p in r["pieces"])
    r = route("bitmap_all_65536_k17", 1)
    assert r["handed"] and r["sb"] == 6 and len(r["pieces"]) == 64
    for k, rem, br in ((17, 8, "direct"), (18, 9, "direct"), (21, 15, "hotkey_one"), (26, 25, "hotkey_one")):
        assert not route("polyA_nmax_k%d" % k, 1)["handed"]
        r = route("polyA_nmax_plus_1_k%d" % k, 1)
        assert r["handed"] and r["sb"] == 8 and r["rem"] == rem and [p[3] for p in r["pieces"]] == [br]
    r = route("direct_many_distinct_k17", 1)
    assert r["sb"] == 8 and r["rem"] == 8 and {p[3] for p in r["pieces"]} == {"piece_sort_per_8", "direct"}
    assert {p[1] for p in r["pieces"]} == {1984, 2048, 2112}
    r = route("hotkey_2048_distinct_x160_k21", 2)
    assert r["sb"] == 8 and r["rem"] == 15 and len(r["pieces"]) == 128 and {p[1:] for p in r["pieces"]} == {(2560, 16, "hotkey_multi")}
    for k in (21, 26):
        r = route("hotkey_3_distinct_k%d" % k, 1)
        assert [p[1:] for p in r["pieces"]] == [(1600, 1600, "piece_sort_per_8"), (2400, 3, "hotkey_multi")]
    for k in (21, 32):
        d = sc.BY_NAME["give_up_1600_distinct_x2_k%d" % k].declared(2)
        assert d["n_big"] == 1 and not d["rle"] and d["chroms"][0][0]["pieces"] == [(0, 3200, 1600, "give_up")]
        d = sc.BY_NAME["give_up_4200_distinct_x2_k%d" % k].declared(2)
        assert d["n_big"] == 1 and d["rle"] and d["chroms"][0][0]["pieces"] == [(0, 8400, 4200, "give_up")]
        assert not sc.BY_NAME["give_up_4200_distinct_x2_k%d" % k].declared(3)["rle"]      # nothing is kept at lower 3
    r = route("hash_stream_1537_distinct_x2_k21", 2)
    assert r["handed"] and r["sb"] == 2 and [p[3] for p in r["pieces"]] == ["piece_hash", "piece_hash"]
    assert route("hash_singletons_beside_doubles_k21", 2)["handed"] is None
