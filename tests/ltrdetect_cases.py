"""Hand-built inputs of the LTR detection (csrc/sp_ltrdetect.h): the smallest at which each rule can go wrong.

A case is (name, [chromosome strings], parameters of ltrdetect_ref.hsps).  Most use SMALL, a parameter set of short
distances, so that a chromosome is a few hundred bases; the chunk, flank and planted cases use the defaults.  Backgrounds
are random; where a test asserts a number of seeds, the background is drawn until it holds no repeated word at all
(`clean`).  Built once, shared, never changed."""
import random

import ltrdetect_ref as ld

SMALL = dict(L=12, X=20, dmin=50, dmax=300, maxlen=100)
DEFAULT = dict(ld.DEFAULTS)
CHUNKS = (4096, 5000, 0)         # chunk bodies every case runs at (0: the default)

_cache = {}


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def clean(rng, n, L=12):
    """random bases without a repeated word of L bases"""
    while True:
        s = rand_seq(rng, n)
        if len({s[i:i + L] for i in range(n - L + 1)}) == n - L + 1:
            return s


def other(base, step=1):
    return "ACGT"[("ACGT".index(base.upper()) + step) % 4]


def put(s, at, piece):
    assert 0 <= at and at + len(piece) <= len(s)
    return s[:at] + piece + s[at + len(piece):]


def copy(s, src, dst, n, flank=12):
    """bases [src, src + n) written at dst, the `flank` bases before and behind the copy made to differ from those of the
    source at every position: the repeat is exactly n long and no extension under X <= 20 leaves it"""
    s = put(s, dst, s[src:src + n])
    k = min(flank, src, dst - src - n)
    s = put(s, dst - k, "".join(other(c) for c in s[src - k:src]))
    k = min(flank, len(s) - dst - n, dst - src - n)
    return put(s, dst + n, "".join(other(c) for c in s[src + n:src + n + k]))


def mutate(rng, seq, sub_rate, indels):
    s = [c if rng.random() >= sub_rate else other(c, rng.randrange(1, 4)) for c in seq]
    for _ in range(indels):
        at, n = rng.randrange(10, len(s) - 10), rng.randrange(1, 10)
        if rng.random() < 0.5:
            del s[at:at + n]
        else:
            s[at:at] = [rng.choice("ACGT") for _ in range(n)]
    return "".join(s)


def _hand():
    rng = random.Random(20)
    out = []

    def add(name, seqs, par=SMALL, **over):
        out.append((name, [seqs] if isinstance(seqs, str) else list(seqs), dict(par, **over)))
    bg = lambda n: clean(rng, n)
    # an exact run of L and of L - 1
    add("run_L", copy(bg(500), 100, 300, 12))
    add("run_L-1", copy(bg(500), 100, 300, 11))
    # the distance limits
    for d in (49, 50, 300, 301):
        add("d=%d" % d, copy(bg(700), 100, 100 + d, 30))
    # a pair that starts at base 0 and ends on the last base; the same one base inside
    s = bg(240)
    add("ends", s[:40] + s[40:200] + s[:40])
    add("ends_inside", "A" + s[:40] + s[40:200] + s[:40] + "C")
    # invalid bases and case
    s = copy(bg(600), 100, 350, 80)
    add("n_inside", put(s, 390, "N"))
    add("n_at_p-1", put(copy(put(bg(600), 99, "G"), 99, 349, 31), 99, "N"))
    add("n_at_q-1", put(copy(put(bg(600), 99, "G"), 99, 349, 31), 349, "N"))
    add("iupac", put(put(s, 120, "R"), 400, "y"))
    add("lower_case", s.lower())
    add("mixed_case", "".join(c.lower() if i % 3 else c for i, c in enumerate(s)))
    # chromosomes without a word, and several chromosomes in one genome
    add("short_and_all_n", ["ACGTACGTACG", "N" * 500, "ACGTACGTACGT", s, "A"])
    # fan-out: a word with 9 valid partners keeps 8
    unit, s = rand_seq(rng, 30), ""
    for i in range(10):
        s += other(unit[-1]) + unit + rand_seq(rng, 29)
    add("fanout_9", s, dmax=1000)
    add("fanout_8", s[:9 * 60], dmax=1000)
    # the scan cap: of 34 tandem copies of 13 bases the 33rd successor of a start is not looked at, the 32nd is
    tandem = rand_seq(rng, 20) + clean(rng, 13, 4) * 34 + rand_seq(rng, 20)
    add("tandem_unseen", tandem, dmin=13 * 33, dmax=600)
    add("tandem_seen", tandem, dmin=13 * 32, dmax=600)
    add("homopolymer", rand_seq(rng, 50) + "A" * 400 + rand_seq(rng, 50))
    add("homopolymer_near", rand_seq(rng, 50) + "A" * 400 + rand_seq(rng, 50), dmin=1, dmax=40)
    # a run of mismatches that lowers the score by exactly X (the extension goes on) and by X + 2 (it stops); a seed on
    # either side of the run, so both the right and the left extension meet it
    par = dict(SMALL, dmax=600, maxlen=400)
    for n_mis in (10, 11):
        s = bg(900)
        s = copy(s, 100, 500, 200)
        s = put(s, 600, "".join(other(c) for c in s[600:600 + n_mis]))
        add("xdrop_%d" % n_mis, s, par)
        add("xdrop_%d_x0" % n_mis, s, par, X=0)
    # an HSP capped by d (three tandem copies) and one capped by maxlen
    unit = bg(150)
    add("cap_d", rand_seq(rng, 30) + unit * 3 + rand_seq(rng, 30), maxlen=400)
    s = bg(1000)
    add("cap_maxlen", copy(s, 50, 450, 300), dmax=600)
    add("cap_maxlen_left", copy(s, 50, 450, 300), dmax=600, maxlen=37)
    # p and q at every residue modulo 32
    s = rand_seq(rng, 32 * 640 + 100)
    for r in range(32):
        p = 640 * r + 64 + r
        q = p + 200 + ((7 * r + 3 - p - 200) % 32)
        assert p % 32 == r and q % 32 == (7 * r + 3) % 32
        s = copy(s, p, q, 20 + r)
    add("mod32", s)
    add("mod32_L20", s, L=20)
    add("mod32_L13", s, L=13)
    # pairs straddling the edges of chunks of 4096 and 5000 starts; d above a whole chunk
    s = rand_seq(rng, 12500)
    for p, n, q in ((4085, 40, 5385), (4990, 30, 6990), (8185, 25, 9285), (9995, 25, 11500), (100, 45, 12000)):
        s = copy(s, p, q, n)
    add("chunk_edges", s, DEFAULT)
    add("chunk_edges_small", s, SMALL, dmax=15000, maxlen=8192)
    return out


def hand_cases():
    if "hand" not in _cache:
        _cache["hand"] = _hand()
    return _cache["hand"]


def flank_case():
    """(chromosome, [(a0, a1, b0, b1)]): identical LTR pairs whose 12 flanking bases on each side differ at every position
    (flank of the right copy = flank of the left copy + 1 modulo 4), so the exact boundaries are known"""
    if "flank" not in _cache:
        rng = random.Random(21)
        s, want, at = rand_seq(rng, 26000), [], 1000
        for n, d in ((150, 1500), (400, 3000), (1000, 6000), (100, 1000)):
            a0, b0 = at, at + d
            s = put(s, b0, s[a0:a0 + n])
            s = put(s, b0 - 12, "".join(other(c) for c in s[a0 - 12:a0]))
            s = put(s, b0 + n, "".join(other(c) for c in s[a0 + n:a0 + n + 12]))
            want.append((a0, a0 + n, b0, b0 + n))
            at = b0 + n + 500
        _cache["flank"] = (s, want)
    return _cache["flank"]


PLANTED_SEQS, PLANTED_LEN, PLANTED_PER_SEQ = 3, 200_000, 14
PLANTED_REDRAWN = [0]


def planted():
    """([chromosome], [[(a0, a1, b0, b1)] per chromosome]): random sequences carrying LTR-RT-like elements -- LTRs of 120 to
    1500 bases, the right one a copy of the left with 0 to 12 % substitutions and 0 to 3 indels of 1 to 9 bases, 1000 to
    8000 bases between them.  The detector is defined to start from an exact word of L = 20 bases; a pair of LTRs that
    shares none (a short LTR at 10 % divergence often does not) is outside the definition whatever the code does, so such a
    right LTR is drawn again -- decided on the two strings alone.  PLANTED_REDRAWN counts them: 1 of 42."""
    if "planted" not in _cache:
        rng = random.Random(22)
        seqs, truth = [], []
        for _ in range(PLANTED_SEQS):
            s, els = rand_seq(rng, PLANTED_LEN), []
            slot = PLANTED_LEN // PLANTED_PER_SEQ
            for i in range(PLANTED_PER_SEQ):
                left = rand_seq(rng, rng.randrange(120, 1501))
                right = mutate(rng, left, rng.uniform(0, 0.12), rng.randrange(0, 4))
                while not {left[j:j + 20] for j in range(len(left) - 19)} & {right[j:j + 20] for j in range(len(right) - 19)}:
                    right = mutate(rng, left, rng.uniform(0, 0.12), rng.randrange(0, 4))
                    PLANTED_REDRAWN[0] += 1
                inner = rng.randrange(1000, 8001)
                a0 = i * slot + rng.randrange(50, slot - len(left) - inner - len(right) - 50)
                b0 = a0 + len(left) + inner
                s = put(put(s, a0, left), b0, right)
                els.append((a0, a0 + len(left), b0, b0 + len(right)))
            seqs.append(s)
            truth.append(els)
        _cache["planted"] = (seqs, truth)
    return _cache["planted"]


def dense_case():
    """(chromosome, parameters): 20 kb over two letters -- thousands of seeds, for the append list's capacity and for more
    seeds than one grid of the extension kernel takes in a pass"""
    if "dense" not in _cache:
        rng = random.Random(23)
        _cache["dense"] = ("".join(rng.choice("AC") for _ in range(20_000)), dict(SMALL, dmax=3000))
    return _cache["dense"]


def twin(seqs, par):
    """[(n_seeds, [hsp])] per chromosome, computed once per (case, parameters)"""
    key = ("twin", tuple(seqs), tuple(sorted(par.items())))
    if key not in _cache:
        _cache[key] = [ld.hsps(s, **par) for s in seqs]
    return _cache[key]
