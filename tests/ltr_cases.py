"""Inputs of the LTR tests: LTR pairs laid out on a toy genome for Context.ltr_align, and LTR-RTs planted into the
chromosomes of the toy allopolyploid for the command line (with the `.scn` that describes them)."""
import random

import numpy as np

import ltralign_ref as lr


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def diverge(rng, seq, subs=0, indels=0, indel_len=3):
    """a copy with `subs` substituted bases and `indels` insertions or deletions of 1..indel_len bases"""
    s = list(seq)
    for p in rng.sample(range(len(s)), min(subs, len(s))):
        s[p] = rng.choice([c for c in "ACGT" if c != s[p].upper()])
    for _ in range(indels):
        p = rng.randrange(1, max(2, len(s) - indel_len))
        n = rng.randrange(1, indel_len + 1)
        if rng.random() < 0.5 and len(s) > 4 * indel_len:
            del s[p:p + n]
        else:
            s[p:p] = list(rand_seq(rng, n))
    return "".join(s)


class Layout:
    """chromosomes grown by appending pieces; remembers the pairs it was asked to"""

    def __init__(self, n_chrom):
        self.parts = [[] for _ in range(n_chrom)]
        self.len = [0] * n_chrom
        self.pairs = []          # (name, chrom, a_start, a_len, b_start, b_len)

    def put(self, chrom, seq):
        at = self.len[chrom]
        self.parts[chrom].append(seq)
        self.len[chrom] += len(seq)
        return at

    def pair(self, name, chrom, a, b, gap=""):
        a0 = self.put(chrom, a)
        self.put(chrom, gap)
        b0 = self.put(chrom, b)
        self.pairs.append((name, chrom, a0, len(a), b0, len(b)))

    def seqs(self):
        return ["".join(p) for p in self.parts]

    def arrays(self, keep=lambda name: True):
        rows = [p for p in self.pairs if keep(p[0])]
        cols = list(zip(*[p[1:] for p in rows])) if rows else [[]] * 5
        return [p[0] for p in rows], [np.asarray(c, np.int64) for c in cols]


def kernel_cases(seed=17):
    """(sequences of three chromosomes, Layout): the smallest pairs at which the kernel can still go wrong.

    chromosome 0: LTR lengths 1, 2, 63, 64, 65, 100, 1000 with a diverged copy; lb - la of 0, +-1, +-70 (a band wider than a
    wave) and 895 / 896, 1023 / 1024 either way (just inside / outside SP_LA_MAXBAND at band 64 and at band 0); a pair with
    a run of N, one with a lower-case stretch, one of N only; a_start at every residue modulo 32; one pair at
    SP_LA_MAXLEN and one over it.  chromosome 1: 2500 short pairs at random offsets.  chromosome 2 (77 bases): a pair at
    offset 0 whose right LTR ends on the last base."""
    rng = random.Random(seed)
    lay = Layout(3)
    for n in (1, 2, 63, 64, 65, 100, 1000):
        a = rand_seq(rng, n)
        lay.pair("len%d" % n, 0, a, diverge(rng, a, subs=n // 12) if n > 2 else a, gap=rand_seq(rng, rng.randrange(0, 40)))
        lay.pair("len%d_unrelated" % n, 0, a, rand_seq(rng, n), gap=rand_seq(rng, 7))
    base = rand_seq(rng, 300)
    for delta in (1, 70):
        longer = base[:150] + rand_seq(rng, delta) + base[150:]
        lay.pair("delta+%d" % delta, 0, diverge(rng, base, subs=9), longer, gap=rand_seq(rng, 11))
        lay.pair("delta-%d" % delta, 0, longer, diverge(rng, base, subs=9), gap=rand_seq(rng, 13))
    for delta in (895, 896, 1023, 1024):
        longer = base[:30] + rand_seq(rng, delta) + base[30:60]
        lay.pair("delta+%d" % delta, 0, base[:60], longer, gap=rand_seq(rng, 3))
        lay.pair("delta-%d" % delta, 0, longer, base[:60], gap=rand_seq(rng, 5))
    a = rand_seq(rng, 200)
    lay.pair("n_run", 0, a[:60] + "N" * 45 + a[105:], diverge(rng, a, subs=6, indels=2), gap="NNNN")
    lay.pair("lower_case", 0, a[:30] + a[30:120].lower() + a[120:], diverge(rng, a, subs=6).lower(), gap=rand_seq(rng, 2))
    lay.pair("iupac", 0, a[:50] + "RYKM" + a[54:], a, gap="")
    lay.pair("all_n", 0, "N" * 40, "N" * 37, gap=rand_seq(rng, 9))
    for r in range(32):          # a_start at every residue modulo 32: pad to the residue, then a pair of 40 + r % 3 bases
        lay.put(0, rand_seq(rng, (r - lay.len[0]) % 32))
        a = rand_seq(rng, 40 + r % 3)
        lay.pair("mod32_%d" % r, 0, a, diverge(rng, a, subs=3, indels=1), gap=rand_seq(rng, r % 5))
        assert lay.pairs[-1][2] % 32 == r
    a = rand_seq(rng, lr.MAXLEN)
    lay.pair("maxlen", 0, a, diverge(rng, a, subs=400, indels=12)[:lr.MAXLEN], gap=rand_seq(rng, 21))
    lay.pair("over_maxlen", 0, a[:100], rand_seq(rng, lr.MAXLEN + 1), gap="")
    chrom1 = rand_seq(rng, 6000)
    chrom1 = chrom1[:1000] + "N" * 30 + chrom1[1030:2000] + chrom1[2000:2400].lower() + chrom1[2400:]
    lay.put(1, chrom1)
    for i in range(2500):
        la, lb = rng.randrange(3, 11), rng.randrange(3, 11)
        a0, b0 = rng.randrange(0, len(chrom1) - la), rng.randrange(0, len(chrom1) - lb)
        lay.pairs.append(("short%d" % i, 1, a0, la, b0, lb))
    a = rand_seq(rng, 30)
    lay.pair("ends", 2, a, diverge(rng, a, subs=2) + "ACG", gap=rand_seq(rng, 14))
    assert lay.len[2] == 77 and lay.pairs[-1][2] == 0 and lay.pairs[-1][4] + lay.pairs[-1][5] == 77
    return lay.seqs(), lay


_twin = {}


def twin(seqs, lay, band, keep=lambda name: True):
    """names, the five arrays and the twin's [n, 6] results for the kept pairs under `band` (computed once)"""
    names, cols = lay.arrays(keep)
    key = (id(lay), band, tuple(names))
    if key not in _twin:
        _twin[key] = lr.align_intervals(seqs, *cols, band)
    return names, cols, _twin[key]


def plant_elements(toy_seqs, labels, seed=23, per_chrom=6, max_indel_bases=12):
    """LTR-RTs written into the toy chromosomes: TSD, LTR, the chromosome's own sequence as the internal region, a diverged
    copy of the LTR (chosen substitutions, indels of at most max_indel_bases bases in all), TSD.  The `.scn` carries a similarity
    that is deliberately not the alignment's.  Returns ({label: sequence}, scn text, [(label, start, end, lltr, rltr)] 1-based)."""
    rng = random.Random(seed)
    out, lines, elements = dict(toy_seqs), ["# planted elements", "# s(ret) e(ret) l(ret) s(lLTR) e(lLTR) l(lLTR) s(rLTR) e(rLTR) l(rLTR) sim(LTRs) seq-nr chr"], []
    for nr, lab in enumerate(labels):
        s = out[lab]
        pos = 1500
        for e in range(per_chrom):
            n_ltr = rng.choice([120, 250, 333, 64])
            ltr_a = rand_seq(rng, n_ltr)
            ltr_b = diverge(rng, ltr_a, subs=rng.randrange(0, n_ltr // 8), indels=rng.randrange(0, max_indel_bases // 3 + 1), indel_len=3)
            if e == 0:
                ltr_b = ltr_a                                   # no divergence: age 0
            inner = rng.randrange(900, 2200)
            tsd = rand_seq(rng, 5)
            element = ltr_a + s[pos + 5 + n_ltr:pos + 5 + n_ltr + inner] + ltr_b
            piece = tsd + element + tsd
            s = s[:pos] + piece + s[pos + len(piece):]
            start, end = pos + 5 + 1, pos + 5 + len(element)    # 1-based, both ends included
            sim = round(100 - rng.uniform(0, 12), 1)
            lines.append("%d %d %d %d %d %d %d %d %d %s %d %s" % (start, end, len(element), start, start + n_ltr - 1, n_ltr, end - len(ltr_b) + 1,
                                                                   end, len(ltr_b), sim, nr, lab))
            elements.append((lab, start, end, n_ltr, len(ltr_b)))
            pos += len(piece) + rng.randrange(400, 2500)
        assert pos < len(out[lab]) - 500 and len(s) == len(out[lab])
        out[lab] = s
    return out, "\n".join(lines) + "\n", elements
