"""The list filter above 64 chromosomes (sps_join_wide): k > 15 and count engine 3 with 65..1024 chromosomes,
bit-exact against the CPU oracle, the dispatch between the two join kernels, the limit, the key-range view and the
CLI end to end."""
import numpy as np
import pytest

import pyoracle as po

pytestmark = pytest.mark.gpu

C_MAX = 1024
ARGS = (2.0, 1, 5, 1e9, 0.5)          # min_fold, baseline (replaced per layout), min_freq, max_freq, ratio


def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=n)].copy()


def make_genome(C, seed, n_groups=3, long_factor=50):
    """C short random chromosomes (3-10 kb) with planted repeat families: family f goes 2-4 times into the chromosomes
    of group f % n_groups (chromosome c is in group c % n_groups), so hundreds of keys are specific to a group; one
    repeat goes into every chromosome (a key with C entries); chromosome 1 is ~long_factor times longer than the rest."""
    rng = np.random.RandomState(seed)
    fams = [_rand(rng, int(rng.randint(150, 400))) for _ in range(3 * n_groups)]
    everywhere = _rand(rng, 200)
    seqs = []
    for c in range(C):
        n = int(rng.randint(3000, 10000)) * (long_factor if c == 1 else 1)
        s = _rand(rng, n) if c != 1 else np.tile(_rand(rng, n // 2), 2)     # (the long one twice over: a long list)
        n = s.size
        for f, fam in enumerate(fams):
            if f % n_groups != c % n_groups:
                continue
            for _ in range(int(rng.randint(2, 5))):
                p = int(rng.randint(0, n - fam.size))
                s[p:p + fam.size] = fam
        for _ in range(2):       # (twice: every chromosome keeps k-mers at the lower count 2)
            p = int(rng.randint(0, n - everywhere.size))
            s[p:p + everywhere.size] = everywhere
        seqs.append(s)
    return seqs


def layouts(C, seed=0):
    """name -> (sets as lists of units of chromosome ids, baseline)."""
    rng = np.random.RandomState(seed)
    out = {
        "two_units_b1": ([[[2 * i], [2 * i + 1]] for i in range(C // 2)], 1),             # fast walk, > 32 sets
        "three_units_bm1": ([[[3 * i], [3 * i + 1], [3 * i + 2]] for i in range(C // 3)], -1),
        "four_units_b2": ([[[4 * i], [4 * i + 1], [4 * i + 2], [4 * i + 3]] for i in range(C // 4)], 2),   # generic
    }
    mixed = []
    for i in range(C // 5):          # comma-joined units next to singletons
        mixed.append([[5 * i, 5 * i + 1], [5 * i + 2], [5 * i + 3]])
        mixed.append([[5 * i + 4]])
    out["joined_and_singletons_b1"] = (mixed, 1)
    # 20 non-singleton sets (screen on) of two 4-chromosome units: 160 descriptor rows, chromosomes in several sets
    screen = [[sorted(rng.choice(C, 4, replace=False).tolist()), sorted(rng.choice(C, 4, replace=False).tolist())]
              for _ in range(20)]
    out["screen_b1"] = (screen, 1)
    return out


def _load(ctx, seqs, k, lower=2, engine=0):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)
    ctx.count(k, lower, engine)


def _filter(ctx, sgs, C, baseline):
    from subphaser_amd.config import sets_to_csr
    csr = sets_to_csr(sgs, list(range(C)))
    args = (ARGS[0], baseline) + ARGS[2:]
    nu, nr, nh = ctx.filter(*csr, *args)
    keys, counts, freqs, tot = ctx.filter_fetch(nr)
    hist = np.sort(ctx.filter_hist(nh))
    return (nu, nr, nh), keys, counts, freqs, tot, hist


def _same(got, exp):
    assert got[0] == exp[0]
    for a, b in zip(got[1:], exp[1:]):
        assert a.shape == b.shape and (a == b).all()


def _layout_cases():
    cases = []
    for C in (65, 130):
        for k in (16, 21, 32):
            cases.append((C, k, None))
    for k in (16, 21, 32):
        cases.append((C_MAX, k, ["two_units_b1", "three_units_bm1", "joined_and_singletons_b1"][(k // 8) % 3]))
    return cases


@pytest.mark.parametrize("C,k,only", _layout_cases())
def test_wide_join_matches_oracle(gpu_ctx, oracle_ctx, monkeypatch, C, k, only):
    seqs = make_genome(C, seed=C + k, long_factor=50 if C < C_MAX else 10)
    _load(gpu_ctx, seqs, k)
    _load(oracle_ctx, seqs, k)
    rows = 0
    for name, (sgs, baseline) in layouts(C).items():
        if only is not None and name != only:
            continue
        exp = _filter(oracle_ctx, sgs, C, baseline)
        for generic in ("0", "1"):
            monkeypatch.setenv("SP_JOIN_GENERIC", generic)
            got = _filter(gpu_ctx, sgs, C, baseline)
            _same(got, exp)
        rows += exp[0][1]
    assert rows >= 100


def test_wide_join_dispatch(gpu_ctx, oracle_ctx):
    for C, kernel, other in ((64, "sps_join", "sps_join_wide"), (65, "sps_join_wide", "sps_join")):
        seqs = make_genome(C, seed=7, long_factor=5)
        sgs, baseline = layouts(C)["two_units_b1"]
        _load(gpu_ctx, seqs, 17)
        _load(oracle_ctx, seqs, 17)
        gpu_ctx.prof_reset()
        gpu_ctx.prof_enable(True)
        try:
            got = _filter(gpu_ctx, sgs, C, baseline)
            rep = gpu_ctx.prof_report()
        finally:
            gpu_ctx.prof_enable(False)
        labels = set(rep)
        assert kernel in labels and other not in labels, labels
        _same(got, _filter(oracle_ctx, sgs, C, baseline))


def test_wide_join_limit(gpu_ctx):
    rng = np.random.RandomState(3)
    C = C_MAX + 1
    seqs = [_rand(rng, 200) for _ in range(C)]
    _load(gpu_ctx, seqs, 17, lower=1)
    from subphaser_amd.config import sets_to_csr
    csr = sets_to_csr([[[2 * i], [2 * i + 1]] for i in range(C // 2)], list(range(C)))
    with pytest.raises(Exception, match=str(C_MAX)):
        gpu_ctx.filter(*csr, *ARGS)


def test_wide_key_range_view(gpu_ctx, oracle_ctx):
    """test_sparse_key_range_view at 70 chromosomes: cut every list at common splitters, export the pieces, filter each
    key range through sparse_view; the concatenated ranges equal the one-shot filter and the oracle."""
    from subphaser_amd.config import sets_to_csr
    C, k, lower = 70, 19, 2
    seqs = make_genome(C, seed=19, long_factor=5)
    sgs, baseline = layouts(C)["two_units_b1"]
    csr = sets_to_csr(sgs, list(range(C)))
    args = (ARGS[0], baseline) + ARGS[2:]
    _load(gpu_ctx, seqs, k, lower)
    _load(oracle_ctx, seqs, k, lower)
    nu, nr, nh = gpu_ctx.filter(*csr, *args)
    keys, counts, freqs, tot = gpu_ctx.filter_fetch(nr)
    onu, onr, onh = oracle_ctx.filter(*csr, *args)
    okeys, ocounts, ofreqs, otot = oracle_ctx.filter_fetch(onr)
    assert (nu, nr, nh) == (onu, onr, onh) and nr > 0
    assert (keys == okeys).all() and (counts == ocounts).all() and (freqs == ofreqs).all()
    lengths = gpu_ctx.lengths()
    smp = gpu_ctx.sparse_sample(1, 64)
    splitters = np.unique(smp[[21, 42]])
    bounds = [gpu_ctx.sparse_split(i, splitters) for i in range(C)]
    parts, tot_nu, tot_nh = [], 0, 0
    for r in range(len(splitters) + 1):
        bufs, pk, pc, n = [], [], [], []
        for i in range(C):
            lo, hi = int(bounds[i][r]), int(bounds[i][r + 1])
            dk, dc = gpu_ctx.dev_alloc(max(hi - lo, 1) * 8), gpu_ctx.dev_alloc(max(hi - lo, 1) * 4)
            gpu_ctx.sparse_export(i, lo, hi - lo, dk, dc)
            bufs += [dk, dc]
            pk.append(dk), pc.append(dc), n.append(hi - lo)
        gpu_ctx.sync()
        gpu_ctx.sparse_view(pk, pc, n, lengths, k, lower)
        try:
            a, b, c_ = gpu_ctx.filter(*csr, *args)
            parts.append(gpu_ctx.filter_fetch(b, sort=False))
        finally:
            gpu_ctx.sparse_view(None, None, None, None, 0, 0)
        tot_nu += a
        tot_nh += c_
        for d in bufs:
            gpu_ctx.dev_free(d)
    assert tot_nu == nu and tot_nh == nh
    assert (np.concatenate([p[0] for p in parts]) == keys).all()
    assert (np.concatenate([p[1] for p in parts]) == counts).all()
    assert (np.concatenate([p[2] for p in parts]) == freqs).all()


def test_wide_engine3_explicit(gpu_ctx, oracle_ctx):
    """Count engine 3 (k <= 15 counts as lists) takes 100 chromosomes when asked for; engine 0 keeps the byte tables."""
    C, k = 100, 13
    seqs = make_genome(C, seed=13, long_factor=5)
    sgs, baseline = layouts(C)["three_units_bm1"]
    _load(gpu_ctx, seqs, k, engine=3)
    _load(oracle_ctx, seqs, k)
    for i in range(C):
        gk, gc = gpu_ctx.dump(i)
        ok, oc = oracle_ctx.dump(i)
        assert (gk == ok).all() and (gc == oc).all(), i
    _same(_filter(gpu_ctx, sgs, C, baseline), _filter(oracle_ctx, sgs, C, baseline))
    gpu_ctx.prof_reset()
    gpu_ctx.prof_enable(True)
    try:
        _load(gpu_ctx, seqs, k, engine=0)
        _filter(gpu_ctx, sgs, C, baseline)
        labels = set(gpu_ctx.prof_report())
    finally:
        gpu_ctx.prof_enable(False)
    assert "k3_eval" in labels, labels


def test_wide_cli_k17(gpu_ctx, oracle_ctx, tmp_path):
    """`subphaser -k 17` on 32 sets x 3 subgenomes + 4 singletons (100 chromosomes) with subgenome-specific repeats:
    the same files through the GPU and through the oracle."""
    import math
    import parity_cases as pc
    from subphaser_amd import pipeline, runtime
    rng = np.random.RandomState(17)
    fams = {g: [_rand(rng, int(rng.randint(200, 500))) for _ in range(6)] for g in "ABC"}
    labels, seqs = [], {}
    for h in range(32):
        for g in "ABC":
            s = _rand(rng, int(rng.randint(20000, 40000)))
            for fam in fams[g]:
                for _ in range(int(rng.randint(3, 8))):
                    p = int(rng.randint(0, s.size - fam.size))
                    s[p:p + fam.size] = fam
            labels.append("%s%d" % (g, h + 1))
            seqs[labels[-1]] = s.tobytes().decode()
    for u in range(4):       # singletons: a copy of every family, four times
        s = _rand(rng, 20000)
        for fam in sum(fams.values(), []):
            for _ in range(4):
                p = int(rng.randint(0, s.size - fam.size))
                s[p:p + fam.size] = fam
        labels.append("U%d" % (u + 1))
        seqs[labels[-1]] = s.tobytes().decode()
    fa = tmp_path / "g.fa"
    with open(fa, "w") as f:
        for lab in labels:
            f.write(">%s\n%s\n" % (lab, seqs[lab]))
    cfg = tmp_path / "sg.config"
    cfg.write_text("".join("A%d\tB%d\tC%d\n" % (h + 1, h + 1, h + 1) for h in range(32)) +
                   "".join("U%d\n" % (u + 1) for u in range(4)))
    asg = tmp_path / "assigned.tsv"
    asg.write_text("".join("%s\t%s\n" % (lab, lab[0] if lab[0] in "ABC" else "ABC"[int(lab[1:]) % 3]) for lab in labels))
    res = {}
    old = runtime._ctx
    try:
        for tag, ctx in (("gpu", gpu_ctx), ("oracle", oracle_ctx)):
            runtime.set_context(ctx)
            out, tmpd = tmp_path / ("out_" + tag), tmp_path / ("tmp_" + tag)
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-sg_assigned", str(asg), "-k", "17", "-q", "3", "-o", str(out),
                           "-tmpdir", str(tmpd), "-disable_ltr", "-disable_circos", "-figfmt", "png",
                           "-bootstrap_seed", "1"])
            base = sorted(out.glob("k17_*.kmer.mat"))
            assert len(base) == 1
            base = str(base[0])[:-len(".kmer.mat")]
            res[tag] = {ext: open(base + ext).read() for ext in
                        (".kmer.mat", ".subgenome.bin.count", ".chrom-subgenome.tsv", ".sig.kmer-subgenome.tsv",
                         ".bin.enrich")}
    finally:
        runtime._ctx = old
    g, o = res["gpu"], res["oracle"]
    assert len(g[".kmer.mat"].split("\n")) > 100
    for ext in (".kmer.mat", ".subgenome.bin.count", ".chrom-subgenome.tsv"):
        assert g[ext] == o[ext], ext
    gs = [l.split("\t") for l in g[".sig.kmer-subgenome.tsv"].strip().split("\n")]
    os_ = [l.split("\t") for l in o[".sig.kmer-subgenome.tsv"].strip().split("\n")]
    assert gs[0] == os_[0] and len(gs) == len(os_) and len(gs) > 1
    for a, b in zip(gs[1:], os_[1:]):
        assert a[:2] == b[:2]
        for x, y in zip(a[2:], b[2:]):        # p-values and per-group means, single or comma-joined
            xs, ys = x.split(","), y.split(",")
            assert len(xs) == len(ys), (a, b)
            for u, w in zip(xs, ys):
                try:
                    fu, fw = float(u), float(w)
                except ValueError:
                    assert u == w, (a, b)
                    continue
                assert math.isclose(fu, fw, rel_tol=1e-9, abs_tol=1e-300), (a, b)
    pc._cmp_enrich_text(g[".bin.enrich"], o[".bin.enrich"], {4, 10}, {8})
