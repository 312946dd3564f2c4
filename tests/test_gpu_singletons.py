"""The list filter at k <= 15 above 1024 chromosomes (sps_filter_passengers): a few dozen set chromosomes next to
hundreds to thousands of passengers (singleton config lines, chromosomes in no set), bit-exact against the CPU oracle;
the dispatch, the automatic engine choice above 560 chromosomes, the limits and the CLI end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C_MAX = 1024
MIN_FOLD, MIN_FREQ, MAX_FREQ, RATIO = 2.0, 5, 40, 0.02


def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=n)].copy()


def _plant(rng, s, fam, copies):
    """`copies` non-overlapping copies of fam into s (one per equal share of s)."""
    share = s.size // copies
    for j in range(copies):
        p = j * share + int(rng.randint(0, share - fam.size + 1))
        s[p:p + fam.size] = fam


def make_genome(n_core, C, seed, n_groups=3):
    """n_core set chromosomes (6-10 kb) and C - n_core passengers (0.3-3 kb).  A core family goes 2-3 times into one or
    two core chromosomes of its group (chromosome c is in group c % n_groups); every passenger carries two copies of one
    family, core or passenger-only, so each of its lists holds k-mers at the lower count 2.  Two families are placed by
    hand: `lift` (tot 2 in chromosome 0, 6 with two passengers: kept by min_freq 5 only through them) and `drop` (tot 6
    in chromosomes 1 and 4, 46 with twenty passengers: dropped by max_freq 40 only through them)."""
    rng = np.random.RandomState(seed)
    core_fams = [_rand(rng, int(rng.randint(60, 140))) for _ in range(8 * n_core)]
    pass_fams = [_rand(rng, int(rng.randint(60, 140))) for _ in range(100)]
    lift, drop = _rand(rng, 90), _rand(rng, 90)
    seqs = [_rand(rng, int(rng.randint(6000, 10000))) for _ in range(n_core)]
    for f, fam in enumerate(core_fams):
        group = [c for c in range(n_core) if c % n_groups == f % n_groups]
        for c in rng.choice(group, int(rng.randint(1, 3)), replace=False):
            for _ in range(int(rng.randint(2, 4))):     # (overlaps are fine: the oracle counts what is there)
                p = int(rng.randint(0, seqs[c].size - fam.size))
                seqs[c][p:p + fam.size] = fam
    _plant(rng, seqs[0], lift, 2)
    _plant(rng, seqs[1], drop, 3)
    _plant(rng, seqs[4], drop, 3)
    for p in range(C - n_core):
        s = _rand(rng, int(rng.randint(300, 3001)))
        fam = lift if p < 2 else drop if p < 22 else (core_fams + pass_fams)[int(rng.randint(0, len(core_fams) + 100))]
        _plant(rng, s, fam, 2)
        seqs.append(s)
    return seqs


def layouts(n_core, C):
    """name -> (sets as lists of units of chromosome ids, baseline, min_fold).  Even passengers get a singleton line,
    odd ones are in no set (the C-ABI allows that)."""
    singles = [[[c]] for c in range(n_core, C, 2)]
    three = [[[3 * i], [3 * i + 1], [3 * i + 2]] for i in range(n_core // 3)]
    return {
        "b1": (three + singles, 1, MIN_FOLD),
        "bm1": (three + singles, -1, MIN_FOLD),
        "b2_generic": ([[[4 * i], [4 * i + 1], [4 * i + 2], [4 * i + 3]] for i in range(n_core // 4)] + singles, 2, MIN_FOLD),
        "joined": ([[[4 * i, 4 * i + 1], [4 * i + 2], [4 * i + 3]] for i in range(n_core // 4)] + singles, 1, MIN_FOLD),
        "fold0": (three + singles, 1, 0.0),
    }


def _load(ctx, seqs, k, lower=2, engine=0):
    ctx.genome_reset(len(seqs))
    for i, s in enumerate(seqs):
        ctx.genome_add(i, s)
    ctx.count(k, lower, engine)


def _filter(ctx, sgs, C, baseline, min_fold, max_freq=MAX_FREQ, ratio=RATIO):
    from subphaser_amd.config import sets_to_csr
    csr = sets_to_csr(sgs, list(range(C)))
    nu, nr, nh = ctx.filter(*csr, min_fold, baseline, MIN_FREQ, max_freq, ratio)
    keys, counts, freqs, tot = ctx.filter_fetch(nr)
    hist = np.sort(ctx.filter_hist(nh))
    return (nu, nr, nh), keys, counts, freqs, tot, hist


def _same(got, exp):
    assert got[0] == exp[0]
    for a, b in zip(got[1:], exp[1:]):
        assert a.shape == b.shape and (a == b).all()


CASES = [(13, 24, 1025, None), (15, 24, 1025, None), (13, 90, 1100, ("b1", "b2_generic", "fold0")),
         (14, 24, 1025, ("b1", "fold0")), (13, 30, 2000, ("bm1", "joined", "fold0")), (15, 36, 2000, ("b1", "fold0"))]


@pytest.mark.parametrize("k,n_core,C,only", CASES)
def test_passengers_match_oracle(gpu_ctx, oracle_ctx, monkeypatch, k, n_core, C, only):
    seqs = make_genome(n_core, C, seed=k * 7 + C)
    _load(gpu_ctx, seqs, k)
    _load(oracle_ctx, seqs, k)
    core = np.arange(n_core)
    for name, (sgs, baseline, min_fold) in layouts(n_core, C).items():
        if only is not None and name not in only:
            continue
        exp = _filter(oracle_ctx, sgs, C, baseline, min_fold)
        for generic in ("0", "1"):
            monkeypatch.setenv("SP_JOIN_GENERIC", generic)
            _same(_filter(gpu_ctx, sgs, C, baseline, min_fold), exp)
        counts = exp[2]
        assert exp[0][1] >= 100, name
        assert (counts[:, core].sum(axis=1) < MIN_FREQ).any(), name      # kept only through the passengers
        if min_fold == 0:
            assert (counts[:, core].sum(axis=1) == 0).any(), name      # passenger-only k-mers are candidates
            # every set a k-mer misses passes the fold test too: no set screen may drop it (ratio 0.5, most k-mers touch
            # one set)
            for generic in ("0", "1"):
                monkeypatch.setenv("SP_JOIN_GENERIC", generic)
                _same(_filter(gpu_ctx, sgs, C, baseline, min_fold, ratio=0.5),
                      _filter(oracle_ctx, sgs, C, baseline, min_fold, ratio=0.5))
        if name == "b1":
            # with max_freq open every candidate is a row: some were dropped by max_freq only through the passengers
            wide = _filter(oracle_ctx, sgs, C, baseline, min_fold, max_freq=1e18)
            _same(_filter(gpu_ctx, sgs, C, baseline, min_fold, max_freq=1e18), wide)
            t_all, t_core = wide[4].astype(np.int64), wide[2][:, core].sum(axis=1)
            assert ((t_all > MAX_FREQ) & (t_core >= MIN_FREQ) & (t_core <= MAX_FREQ)).any()


def _labels(ctx, fn):
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        out = fn()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    return out, set(rep)


def test_passengers_dispatch(gpu_ctx, oracle_ctx):
    for C in (1024, 1025):
        seqs = make_genome(24, C, seed=C)
        sgs, baseline, min_fold = layouts(24, C)["b1"]
        _load(gpu_ctx, seqs, 13)
        _load(oracle_ctx, seqs, 13)
        got, labels = _labels(gpu_ctx, lambda: _filter(gpu_ctx, sgs, C, baseline, min_fold))
        new = {lab for lab in labels if lab.startswith("sps_sg_")}
        if C == C_MAX:
            assert not new and "sps_join_wide" in labels, labels
        else:
            assert "sps_join" in labels, labels
            assert {"sps_sg_mark", "sps_sg_cand", "sps_sg_dir", "sps_sg_tot", "sps_sg_place", "sps_sg_scatter"} <= new, labels
        _same(got, _filter(oracle_ctx, sgs, C, baseline, min_fold))


def test_automatic_lists_above_560(gpu_ctx, oracle_ctx):
    """k = 15, engine 0, 600 chromosomes: counted as lists (byte tables would need 300 GiB and cannot be filtered)."""
    C = 600
    seqs = make_genome(24, C, seed=600)
    sgs, baseline, min_fold = layouts(24, C)["b1"]
    _, labels = _labels(gpu_ctx, lambda: (_load(gpu_ctx, seqs, 15), _filter(gpu_ctx, sgs, C, baseline, min_fold)))
    assert "k3_eval" not in labels and "c2_count_list" in labels and "sps_join_wide" in labels, labels
    _load(oracle_ctx, seqs, 15)
    _same(_filter(gpu_ctx, sgs, C, baseline, min_fold), _filter(oracle_ctx, sgs, C, baseline, min_fold))


def test_passengers_set_chromosome_limit(gpu_ctx):
    rng = np.random.RandomState(5)
    C = C_MAX + 2
    fam = _rand(rng, 40)
    seqs = []
    for _ in range(C):
        s = _rand(rng, 200)
        _plant(rng, s, fam, 2)
        seqs.append(s)
    _load(gpu_ctx, seqs, 15)
    from subphaser_amd.config import sets_to_csr
    sgs = [[[2 * i], [2 * i + 1]] for i in range(511)] + [[[1022], [1023], [1024]], [[1025]]]     # 1025 set chromosomes
    csr = sets_to_csr(sgs, list(range(C)))
    with pytest.raises(Exception, match="at most %d set chromosomes" % C_MAX):
        gpu_ctx.filter(*csr, MIN_FOLD, 1, MIN_FREQ, MAX_FREQ, RATIO)


def test_views_above_limit_refused(gpu_ctx):
    C = C_MAX + 1
    d = gpu_ctx.dev_alloc(1 << 12)
    try:
        with pytest.raises(Exception, match="view takes at most %d chromosomes" % C_MAX):
            gpu_ctx.filter_view([d] * C, 0, 1 << 12, np.ones(C, np.int64), 13, 2)
        with pytest.raises(Exception, match="view takes at most %d chromosomes" % C_MAX):
            gpu_ctx.sparse_view([d] * C, [d] * C, np.zeros(C, np.int64), np.ones(C, np.int64), 17, 2)
    finally:
        gpu_ctx.dev_free(d)


def test_passengers_cli_k15(gpu_ctx, oracle_ctx, tmp_path):
    """`subphaser -k 15` on 10 sets x 3 chromosomes (~20 kb) plus 1100 singleton scaffolds (1-3 kb) that each carry one
    subgenome's repeats, without -sg_assigned: the same files through the GPU and through the oracle, and the scaffolds
    land in the subgenome of their repeats."""
    import parity_cases as pc
    from subphaser_amd import pipeline, runtime
    rng = np.random.RandomState(15)
    fams = {g: [_rand(rng, int(rng.randint(80, 150))) for _ in range(4)] for g in "ABC"}
    labels, seqs, carries = [], {}, {}
    for h in range(10):
        for g in "ABC":
            s = _rand(rng, int(rng.randint(18000, 22000)))
            for fam in fams[g]:
                for _ in range(int(rng.randint(4, 8))):
                    p = int(rng.randint(0, s.size - fam.size))
                    s[p:p + fam.size] = fam
            labels.append("%s%d" % (g, h + 1))
            seqs[labels[-1]] = s
    for u in range(1100):     # three copies of three of its group's families (counts 3: kept at -lower_count 3)
        g = "ABC"[u % 3]
        s = _rand(rng, int(rng.randint(1500, 3001)))
        part = s.size // 3
        for t, j in enumerate(rng.choice(4, 3, replace=False)):
            _plant(rng, s[t * part:(t + 1) * part], fams[g][j], 3)
        labels.append("U%d" % (u + 1))
        seqs[labels[-1]] = s
        carries[labels[-1]] = g
    fa = tmp_path / "g.fa"
    with open(fa, "w") as f:
        for lab in labels:
            f.write(">%s\n%s\n" % (lab, seqs[lab].tobytes().decode()))
    cfg = tmp_path / "sg.config"
    cfg.write_text("".join("A%d\tB%d\tC%d\n" % (h + 1, h + 1, h + 1) for h in range(10)) +
                   "".join("U%d\n" % (u + 1) for u in range(1100)))
    res = {}
    old = runtime._ctx
    try:
        for tag, ctx in (("gpu", gpu_ctx), ("oracle", oracle_ctx)):
            runtime.set_context(ctx)
            out, tmpd = tmp_path / ("out_" + tag), tmp_path / ("tmp_" + tag)
            pipeline.main(["-i", str(fa), "-c", str(cfg), "-k", "15", "-q", "3", "-o", str(out), "-tmpdir", str(tmpd),
                           "-disable_ltr", "-disable_circos", "-figfmt", "png", "-replicates", "20",
                           "-bootstrap_seed", "1"])
            base = sorted(out.glob("k15_*.kmer.mat"))
            assert len(base) == 1
            base = str(base[0])[:-len(".kmer.mat")]
            res[tag] = {ext: open(base + ext).read() for ext in
                        (".kmer.mat", ".subgenome.bin.count", ".chrom-subgenome.tsv", ".bin.enrich")}
    finally:
        runtime._ctx = old
    g, o = res["gpu"], res["oracle"]
    assert len(g[".kmer.mat"].split("\n")) > 100
    assert len(g[".kmer.mat"].split("\n", 1)[0].split("\t")) >= 1130      # a column per chromosome
    for ext in (".kmer.mat", ".subgenome.bin.count", ".chrom-subgenome.tsv"):
        assert g[ext] == o[ext], ext
    pc._cmp_enrich_text(g[".bin.enrich"], o[".bin.enrich"], {4, 10}, {8})
    sg_of = dict(l.split("\t")[:2] for l in g[".chrom-subgenome.tsv"].strip().split("\n")[1:])
    name = {}
    for grp in "ABC":        # the subgenome the core chromosomes of a group went to
        votes = [sg_of[lab] for lab in labels if lab[0] == grp]
        name[grp] = max(set(votes), key=votes.count)
    assert len(set(name.values())) == 3, name
    hits = sum(sg_of[u] == name[grp] for u, grp in carries.items())
    assert hits >= 0.9 * len(carries), (hits, len(carries))


@pytest.mark.xfail(strict=True, reason="known defect of the <= 1024-chromosome list filter, kept as it is here: sps_join_blk's "
                                       "set screen takes a set a k-mer does not touch for a failed fold test, but with "
                                       "min_fold <= 0 an all-zero set passes (sps_join_wide and the passenger filter's "
                                       "phase A do without the screen then)")
def test_join_blk_screen_min_fold0(gpu_ctx, oracle_ctx):
    """k = 17, 12 chromosomes in 4 sets x 3 (sps_join_blk, set screen on), min_fold 0, ratio 1: every k-mer passes the
    fold test of every set, so every union k-mer is in the hist; the screen drops those that touch fewer sets."""
    seqs = make_genome(12, 12, seed=17)
    sgs = [[[3 * i], [3 * i + 1], [3 * i + 2]] for i in range(4)]
    _load(gpu_ctx, seqs, 17)
    _load(oracle_ctx, seqs, 17)
    exp = _filter(oracle_ctx, sgs, 12, 1, 0.0, ratio=1.0)
    assert exp[0][2] == exp[0][0]
    _same(_filter(gpu_ctx, sgs, 12, 1, 0.0, ratio=1.0), exp)
