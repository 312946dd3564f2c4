#!/usr/bin/env python
"""The launches and outputs of the map stage under every kind of label table, for comparing two builds of the library.

    python tools/label_launches.py OUT.json                    run (the library: SUBPHASER_HIP_LIB, else the tree's own)
    python tools/label_launches.py --compare A.json B.json     exit status 0 if the two runs agree

Per case (k, subgenomes, switches) on the 1.5 Mb genome of tests/cu_limit_cases.py, with profiling on: labels_set,
map_bins_all, map_features_cat, map_intervals, labels_hit.  Recorded: every kernel name of prof_report() with its call
count and largest grid, and the SHA-256 of every output array (equal digests: arrays equal with ==).  --compare lists
the kernels whose grids or call counts differ and the outputs whose digests differ."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SWITCHES = ("SP_MAP_ENGINE", "SP_CTAB", "SP_CTAB_FACTOR")
CASES = [(15, 3, {}), (15, 5, {}), (15, 9, {}), (13, 3, {"SP_CTAB": "1"}), (17, 3, {}), (17, 5, {}), (17, 9, {}),
         (17, 3, {"SP_CTAB": "0"})]
LIMIT = 1       # which genome of cu_limit_cases


def digest(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    return "%s %s %s" % (a.dtype, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def run(out_path):
    import numpy as np
    import cu_limit_cases as cc
    from subphaser_amd import _native
    seqs = cc.genome(LIMIT)
    ctx = _native.Context(0)
    res = {}
    try:
        ctx.genome_reset(len(seqs))
        for i, s in enumerate(seqs):
            ctx.genome_add(i, s)
        for k, S, env in CASES:
            for name in SWITCHES:
                os.environ.pop(name, None)
            os.environ.update(env)
            name = "k=%d S=%d %s" % (k, S, " ".join("%s=%s" % kv for kv in sorted(env.items())))
            keys, sg = cc.labels(LIMIT, k, S)
            ch, st, ln = cc.features(LIMIT, k)
            cat, off = cc.feature_cat(LIMIT, k)
            ctx.count(k, cc.LOWER)
            ctx.prof_reset()
            ctx.prof_enable(True)
            ctx.labels_set(keys, sg, S)
            bins, nm = ctx.map_bins_all(10000, 10_000_000)
            out = {"bins": digest(np.concatenate(bins)), "n_mapped": digest(nm)}
            out["features"] = digest(ctx.map_features_cat(cat, off))
            out["intervals"] = digest(ctx.map_intervals(ch, st, st + ln))
            out["labels_hit"] = int(ctx.labels_hit())
            rep = ctx.prof_report()
            ctx.prof_enable(False)
            ctx.prof_reset()
            res[name.strip()] = {"kernels": {kn: [int(e["calls"]), int(e["grid"])] for kn, e in sorted(rep.items())}, "outputs": out}
            print(name, out["labels_hit"], " ".join("%s:%dx%d" % (kn, c, g) for kn, (c, g) in res[name.strip()]["kernels"].items()))
    finally:
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    for case in sorted(set(a) | set(b)):
        ka, kb = a.get(case, {}).get("kernels", {}), b.get(case, {}).get("kernels", {})
        for kn in sorted(set(ka) | set(kb)):
            if ka.get(kn) != kb.get(kn):
                bad += 1
                print("%s: %s [calls, grid] %s -> %s" % (case, kn, ka.get(kn), kb.get(kn)))
        oa, ob = a.get(case, {}).get("outputs", {}), b.get(case, {}).get("outputs", {})
        for on in sorted(set(oa) | set(ob)):
            if oa.get(on) != ob.get(on):
                bad += 1
                print("%s: output %s differs" % (case, on))
    print("%d cases, %d differences" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    run(sys.argv[1])
