"""GPU: the domain search (sp_domains.hip: dm_translate, dm_search, dm_pick; Context.dom_search) against the Python twin
(tests/domains_ref.py) with `==` on all six columns, and the classification of the command line.

Cases (tests/domains_cases.py): M = 1, 2, 63, 64, 65, 129, 600 (tables read from global memory) and 2048 (with 40 residues);
inner lengths 0 to 5 and 30, 31, 32; intervals at a chromosome's first and last base; N runs, IUPAC codes, lower case and
stop codons inside a domain; a delete run of 70 nodes and an insert run of 70 residues (across the lanes of the wave);
`*` transitions; equal copies (start tie, frame tie); 700 residues (eleven register stages of 64 rows); 2000 elements x 8
profiles in one call, and the same through calls of 64 entries; n = 0; every SP_EINVAL and SP_EUNSUP of the entry (the NULL
pointers through the C entry itself), each followed by a good call -- SP_ENOMEM is NOT reached: it needs a workspace the
device cannot hold.  The kernels cap no grid and work in no tunable
chunk, so there is no setter and no SP_CU_LIMIT case."""
import os

import numpy as np
import pytest

import domains_cases as dc
import domains_ref as dr
from subphaser_amd import _native

pytestmark = pytest.mark.gpu


def _load(ctx, chroms):
    ctx.genome_reset(len(chroms))
    for i, s in enumerate(chroms):
        ctx.genome_add(i, s)


@pytest.fixture(scope="module")
def laid_out():
    """the cases on two chromosomes: "planted" starts at base 0 of the first, "res700" ends on the last base of the second"""
    cases = sorted(dc.cases(), key=lambda c: (c[0] != "planted", c[0] == "res700"))
    chroms, chrom, start, end = dc.genome([c[1] for c in cases])
    assert start[0] == 0 and end[0] > 0 and end[-1] == len(chroms[chrom[-1]]) and chrom[-1] == 1
    for c, (ch, a, b) in zip(cases, zip(chrom, start, end)):
        assert chroms[ch][a:b] == c[1]
    return cases, chroms, chrom, start, end


@pytest.fixture(scope="module")
def memo():
    return {}


def test_kernel_is_the_twin_case_by_case(gpu_ctx, laid_out, memo):
    cases, chroms, chrom, start, end = laid_out
    _load(gpu_ctx, chroms)
    P = dc.profiles()
    for (name, seq, profs), ch, a, b in zip(cases, chrom, start, end):
        plist = [P[p] for p in profs]
        got = gpu_ctx.dom_search([ch], [a], [b], *dr.tables(plist))
        want = dr.search([seq], plist, memo)
        assert got.dtype == np.int32 and got.shape == (1, len(plist), 6)
        assert (got == want).all(), (name, profs, got.tolist(), want.tolist())


def test_all_cases_against_all_small_profiles_in_one_call(gpu_ctx, laid_out, memo):
    cases, chroms, chrom, start, end = laid_out
    _load(gpu_ctx, chroms)
    P = dc.profiles()
    names = ["m1", "m2", "m63", "m64", "m65", "m129", "star65", "star200", "c60", "c200", "m600"]
    plist = [P[p] for p in names]
    got = gpu_ctx.dom_search(chrom, start, end, *dr.tables(plist))
    want = dr.search([c[1] for c in cases], plist, memo)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, [(cases[i][0], names[p], got[i, p].tolist(), want[i, p].tolist()) for i, p in bad[:5]]
    res = {c[0]: dict(zip(names, want[i].tolist())) for i, c in enumerate(cases)}
    assert res["len2"]["m1"] == [dr.INT32_MIN, 0, 0, 0, 0, 0] and res["len3"]["m1"][0] > dr.INT32_MIN
    assert res["delete70"]["c200"][4:] == [1, 200] and res["insert70"]["c200"][4:] == [1, 200]
    assert res["frame_tie"]["c60"][1] == 0 and res["start_tie"]["c60"][2] == 10


def test_two_thousand_elements_by_eight_profiles(gpu_ctx, memo, monkeypatch):
    seqs, names = dc.many(2000)
    chroms, chrom, start, end = dc.genome(seqs, n_chrom=3)
    _load(gpu_ctx, chroms)
    plist = [dc.profiles()[p] for p in names]
    got = gpu_ctx.dom_search(chrom, start, end, *dr.tables(plist))
    want = dr.search(seqs, plist, memo)
    assert got.shape == (2000, 8, 6)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, [(seqs[i], names[p], got[i, p].tolist(), want[i, p].tolist()) for i, p in bad[:5]]
    assert (want[:, :, 0] == dr.INT32_MIN).any() and (want[:, :, 1] >= 3).any() and (want[:, :, 1] < 3).any()
    # the slices of Context.dom_search: 8 elements a call
    monkeypatch.setattr(_native, "DOMAINS_CALL_ENTRIES", 64)
    assert (gpu_ctx.dom_search(chrom[:300], start[:300], end[:300], *dr.tables(plist)) == want[:300]).all()


def test_empty_call_and_errors(gpu_ctx, laid_out, memo):
    cases, chroms, chrom, start, end = laid_out
    _load(gpu_ctx, chroms)
    P = dc.profiles()
    plist = [P["m5"], P["m64"]]
    tab = dr.tables(plist)
    want = dr.search([cases[0][1]], plist, memo)

    def good():
        assert (gpu_ctx.dom_search([0], [0], [end[0]], *tab) == want).all()
    z = np.zeros(0, np.int64)
    assert gpu_ctx.dom_search(z, z, z, *tab).shape == (0, 2, 6)
    good()
    n0 = len(chroms[0])
    moff, emis, trans, entry = tab

    def changed(arr, idx, val):
        a = arr.copy()
        a[idx] = val
        return a
    big = dr.tables([dr.make_profile(2049, np.zeros((2049, 22)), np.zeros((2049, 7)))])
    many = dr.tables([P["m1"]] * 4097)
    for args, msg in [(([2], [0], [5]) + tab, "chromosome 2 out of range"),
                      (([-1], [0], [5]) + tab, "chromosome -1 out of range"),
                      (([0], [-1], [5]) + tab, "outside chromosome"),
                      (([0], [0], [n0 + 1]) + tab, "outside chromosome"),
                      (([0], [6], [5]) + tab, "ends before it starts"),
                      (([0], [0], [5], np.zeros(1, np.int32), emis[:0], trans[:0], entry[:0]), "0 profiles"),
                      (([0], [0], [5], changed(moff, 1, 0), emis, trans, entry), "has 0 nodes"),
                      (([0], [0], [5], changed(moff, 0, 1), emis, trans, entry), "start at 1"),
                      (([0], [0], [5], moff, changed(emis, (0, 0), (1 << 15) + 1), trans, entry), "outside its range"),
                      (([0], [0], [5], moff, emis, changed(trans, (3, 2), 1), entry), "outside its range"),
                      (([0], [0], [5], moff, emis, trans, changed(entry, 1, 5)), "outside its range"),
                      (([0], [0], [5]) + big, "2049 nodes"),
                      (([0], [0], [5]) + many, "4097 profiles")]:
        with pytest.raises(ValueError, match=msg):
            gpu_ctx.dom_search(*args)
        good()
    # NULL pointers, through the C entry itself (Context never passes one)
    import ctypes as C
    ch, st, en = np.zeros(1, np.int32), np.zeros(1, np.int64), np.full(1, 5, np.int64)
    out = np.zeros((1, 2, 6), np.int32)
    full = [ch, st, en, moff, emis, trans, entry, out]
    for q in range(len(full)):
        ptr = [None if j == q else a.ctypes.data_as(C.c_void_p) for j, a in enumerate(full)]
        rc = gpu_ctx.L.sp_dom_search(gpu_ctx.h, 1, ptr[0], ptr[1], ptr[2], 2, ptr[3], ptr[4], ptr[5], ptr[6], ptr[7])
        assert rc == _native.SP_EINVAL and b"bad arguments" in gpu_ctx.L.sp_last_error(gpu_ctx.h), q
        good()
    assert gpu_ctx.L.sp_dom_search(None, 0, None, None, None, 2, None, None, None, None, None) == _native.SP_EINVAL
    good()
    # an interval above the limit (the chromosome has to be that long) and the last base of a chromosome
    assert gpu_ctx.dom_search([0], [n0 - 4], [n0], *tab).shape == (1, 2, 6)
    long = dr.rand_dna(__import__("random").Random(1), 65540)
    _load(gpu_ctx, [long])
    with pytest.raises(ValueError, match="65537 bases"):
        gpu_ctx.dom_search([0], [1], [65538], *tab)
    assert gpu_ctx.dom_search([0], [0], [0], *tab)[0, :, 0].tolist() == [dr.INT32_MIN] * 2
    gpu_ctx.genome_reset(0)
    with pytest.raises(ValueError, match="no genome loaded"):
        gpu_ctx.dom_search([0], [0], [5], *tab)
    _load(gpu_ctx, chroms)
    good()


def test_an_interval_at_the_length_limit(gpu_ctx):
    """65536 bases: 21845 residues in frame 0 -- i_start near the end needs all 15 bits of the start code.  The twin runs
    the one frame the domain is planted in; the device must name it over the other five."""
    import random
    rng = random.Random(8)
    prof = dr.consensus_profile(rng, dr.rand_protein(rng, 12), name="c12")
    cons = "".join(max(pe, key=pe.get) for pe, _ in prof["probs"])
    dom = dr.back_translate(rng, cons)
    seq = dr.rand_dna(rng, 65536 - 36 - 9) + dom + dr.rand_dna(rng, 9)
    _load(gpu_ctx, [seq])
    got = gpu_ctx.dom_search([0], [0], [65536], *dr.tables([prof]))[0, 0].tolist()
    i0 = (65536 - 36 - 9) // 3
    assert (65536 - 45) % 3 == got[1] and got[2:] == [i0, i0 + 11, 1, 12], got
    res = dr.translate(seq, got[1])
    assert len(res) <= 21845
    # the score is the twin's on the window around the hit (a local path does not depend on what lies outside it)
    w = dr.frame_hit(res[i0 - 20:], prof)
    assert w[0] == got[0] and w[2] == 20 + 11


# ---------------------------------------------------------------------------------------------- the command line
CLI_NAMES = ["Class_I/LTR/Ty1_copia/Ale:Ty1-INT", "Class_I/LTR/Ty1_copia/Ale:Ty1-RT",
             "Class_I/LTR/Ty3_gypsy/chromovirus/Tekay:Ty3-RT", "Class_I/LTR/Ty3_gypsy/chromovirus/Tekay:Ty3-INT"]


def planted_world(toy):
    """the toy genome with three planted LTR-RTs per chromosome (tests/ltr_cases.py): the first gets two Copia-like domains
    in its inner sequence, the second stays as it is -- a decoy --, the third two Gypsy-like ones on the reverse strand.
    Returns ({label: sequence}, elements, kinds, profiles, the .hmm text)."""
    import random

    import ltr_cases
    rng = random.Random(41)
    profs = [dr.consensus_profile(rng, dr.rand_protein(rng, 40), name=n) for n in CLI_NAMES]
    cons = ["".join(max(pe, key=pe.get) for pe, _ in p["probs"]) for p in profs]
    labels = toy["labels"]
    seqs, _, elements = ltr_cases.plant_elements({lab: str(toy["seqs"][lab]) for lab in labels}, labels, per_chrom=3)
    kinds = []
    for q, (lab, start, end, lltr, rltr) in enumerate(elements):
        kind = ("copia", "decoy", "gypsy")[q % 3]
        kinds.append(kind)
        if kind == "decoy":
            continue
        pair = cons[:2] if kind == "copia" else cons[2:]
        dom = dr.back_translate(rng, pair[0]) + dr.rand_dna(rng, 15) + dr.back_translate(rng, pair[1])
        if kind == "gypsy":
            dom = dr.revcomp(dom)
        at = start - 1 + lltr + 40
        assert at + len(dom) < end - rltr - 40
        seqs[lab] = seqs[lab][:at] + dom + seqs[lab][at + len(dom):]
    return seqs, elements, kinds, profs, dr.hmm_text(profs)


def expected_cls(seqs, labels, scn_path, hmm_path):
    """`.ltr.cls.tsv` by the twin path: the records of the `.scn`, their inner sequences searched by the twin with the
    tables the reader makes of the file, domains.py from there on.  Returns (text, {id: order})."""
    import io

    from subphaser_amd import domains, ltr
    P = domains.read_hmm(hmm_path)
    twins = [dr.make_profile(M, P.emis[a:a + M], P.trans[a:a + M], entry=e, name=n) for M, a, e, n in zip(P.M, P.moff.tolist(), P.entry.tolist(), P.names)]
    recs = ltr.read_scn(scn_path)
    ival = [domains.inner_interval(r) for r in recs]
    hits = dr.search([seqs[r.seq_id][a:b] for r, (a, b) in zip(recs, ival)], twins)
    rows = domains.classify(domains.best_domains([r.id for r in recs], [b - a for a, b in ival], hits, P))
    out = io.StringIO()
    domains.write_cls(out, rows)
    return out.getvalue(), {r[0]: r[1] for r in rows}, recs


def test_cli_denovo_with_classification(gpu_ctx, toy, tmp_path, caplog):
    """-ltr_denovo -ltr_hmm on the toy genome with planted elements.  The toy genome's own repeats make the detector
    report many more records than were planted; -ltr_maxdist 2600 (the planted LTRs start at most 2533 bases apart) keeps
    them to about two hundred, so that the twin path stays at a few seconds."""
    from test_gpu_ltrdetect import _cli
    seqs, elements, kinds, profs, text = planted_world(toy)
    hmm = tmp_path / "toy.hmm"
    hmm.write_text(text)
    extra = ["-ltr_denovo", "-ltr_maxdist", "2600", "-ltr_hmm", str(hmm)]
    base, log = _cli(gpu_ctx, toy, seqs, tmp_path / "cls", caplog, extra)
    want, order, recs = expected_cls(seqs, toy["labels"], base + ".ltr.scn", str(hmm))
    assert open(base + ".ltr.cls.tsv").read() == want
    # what was planted and found again (a planted element may come back merged with a repeat of the toy genome: most do not)
    planted = {}
    for (lab, s, e, ll, rl), k in zip(elements, kinds):
        near = [r.id for r in recs if r.seq_id == lab and abs(r.start - s) <= 20 and abs(r.end - e) <= 20]
        if len(near) == 1:
            planted[near[0]] = k
    assert len(planted) >= 12 and {"copia", "decoy", "gypsy"} == set(planted.values()), planted
    assert all((order.get(i) == "LTR") == (k != "decoy") for i, k in planted.items())
    rows = {r.split("\t")[0]: r.split("\t") for r in want.splitlines()[1:]}
    assert all(rows[i][2:4] == {"copia": ["Copia", "Ale"], "gypsy": ["Gypsy", "Tekay"]}[k] and rows[i][5] == {"copia": "+", "gypsy": "-"}[k]
               for i, k in planted.items() if k != "decoy")
    is_ltr = {r.id for r in recs if order.get(r.id) == "LTR"}
    kept = {r.split("\t")[0] for r in open(base + ".ltr.identity.tsv").read().splitlines()[1:]}
    assert kept and kept <= is_ltr and not any(i in kept for i, k in planted.items() if k == "decoy")      # (overlaps are resolved among the kept)
    assert len(open(base + ".ltr.dom.gff3").read().splitlines()) == sum(len(r[6].split()) for r in rows.values())
    assert any(m.startswith("By the device domain search, %d (" % len(is_ltr)) for m in log)
    note = [m for m in log if m.startswith("Of modules 3-4")]
    assert len(note) == 1 and "TEsorter classification" not in note[0] and "this build's own Viterbi domain search" in note[0]
    # -all_ltr: the same classes, and records without a domain stay
    base2, log2 = _cli(gpu_ctx, toy, seqs, tmp_path / "all", caplog, extra + ["-all_ltr"])
    assert open(base2 + ".ltr.cls.tsv").read() == want
    kept2 = {r.split("\t")[0] for r in open(base2 + ".ltr.identity.tsv").read().splitlines()[1:]}
    assert kept2 - is_ltr and len(kept2) > len(kept) and any(i in kept2 for i, k in planted.items() if k == "decoy")
