"""The host side of the LTR stage: LTR-RT coordinates from a `.scn`, overlap resolution, identity, insertion ages.

The reference detects LTR-RTs (ltr_finder, ltrharvest), writes them to `tmp/LTR.scn` -- its own checkpoint, which it
re-reads with LTRHarvest (LTR.py:324-331, :609-701) -- classifies them with TEsorter, maps the subgenome-specific k-mers
onto the elements, tests them for enrichment and dates the enriched ones from the similarity of their two LTRs
(LTR.py:474-606, :680-686).  Here detection and classification are not run: the stage starts from the `.scn` a user
supplies and uses every record of it, as the reference does under -all_ltr.  What this module restates is the record
(fields, derived coordinates, id), the overlap resolution for records without a classification, the age arithmetic and
the `.ltr.insert.data` / `.ltr.insert.summary` writers; the similarity is computed from the resident genome by
Context.ltr_align (csrc/sp_ltralign.h) unless -ltr_identity scn asks for the file's.

Under -ltr_denovo the `.scn` is written here instead of read: detect runs the loop -- Context.ltr_seeds / ltr_hsps give the
extended exact seeds of a chromosome (csrc/sp_ltrdetect.h), chain_hsps joins them into chains, candidates keeps the chains
that look like an LTR pair, similarity filters them by the alignment of the two LTRs -- and write_scn writes the 12 columns."""
import math
import time

import numpy as np

from ._native import LTR_ALIGN_BAND as FLAG_BAND, LTR_ALIGN_EDGE as FLAG_EDGE, LTR_ALIGN_LEN as FLAG_LEN
from .runtime import logger

LTR_BAND = 64
# detection: the values the reference passes to its detectors (LTR.py:39-41: -seed 20 -minlenltr 100 -maxlenltr 7000
# -mindistltr 1000 -maxdistltr 15000 -xdrop ... -similar 85), and the two of the chaining.  Provisional, as LTR_BAND is.
LTR_SEED, LTR_MINDIST, LTR_MAXDIST, LTR_MINLEN, LTR_MAXLEN, LTR_XDROP, LTR_SIMILAR = 20, 1000, 15000, 100, 7000, 20, 85.0
LTR_CHAIN_INDEL, LTR_CHAIN_JOIN = 32, 200
DETECT_OPTIONS = ("seed", "mindist", "maxdist", "minlen", "maxlen", "xdrop", "similar", "chain_indel", "chain_join")   # -ltr_<name>
IDENTITY_MODES = ("align", "scn")
MAX_OVL = 10


class Record:
    """One line of a `.scn` (LTRHarvestRecord, LTR.py:635-701): coordinates are 1-based, both ends included."""
    __slots__ = ("start", "end", "element_len", "lltr", "rltr", "similarity", "seq_nr", "seq_id")

    def __init__(self, fields, where=""):
        if len(fields) == 11:
            raise ValueError("{}: 11 columns: this is the raw ltrharvest format, whose 11th column is a sequence number; column 12, "
                             "the sequence id, is missing (pass the `.scn` the reference's LTR step writes, e.g. tmp/LTR.scn, or "
                             "append the id to every line)".format(where))
        if len(fields) < 12:
            raise ValueError("{}: unrecognized LTRHarvest format: {}".format(where, fields))
        # s(ret) e(ret) l(ret) s(lLTR) e(lLTR) l(lLTR) s(rLTR) e(rLTR) l(rLTR) sim seq-nr chr: the reference takes the start
        # from column 4 and the end from column 8
        self.element_len, self.start, self.lltr = int(fields[2]), int(fields[3]), int(fields[5])
        self.end, self.rltr = int(fields[7]), int(fields[8])
        self.similarity, self.seq_nr, self.seq_id = float(fields[9]), int(fields[10]), fields[11]

    @classmethod
    def from_coords(cls, seq_id, seq_nr, a0, a1, b0, b1, similarity):
        """the record of the LTRs [a0, a1) and [b0, b1), 0-based; the similarity keeps the two decimals a `.scn` holds"""
        f = [a0 + 1, b1, b1 - a0, a0 + 1, a1, a1 - a0, b0 + 1, b1, b1 - b0, "%.2f" % similarity, seq_nr, seq_id]
        return cls([str(x) for x in f])

    def columns(self):
        """the 12 columns of the record's line"""
        return [self.start, self.end, self.element_len, self.start, self.lltr_e, self.lltr, self.rltr_s, self.end, self.rltr,
                "%.2f" % self.similarity, self.seq_nr, self.seq_id]

    @property
    def lltr_e(self):
        return self.start + self.lltr - 1

    @property
    def rltr_s(self):
        return self.end - self.rltr + 1

    @property
    def key(self):
        return (self.seq_id, self.start, self.end, self.lltr_e, self.rltr_s)

    @property
    def id(self):
        return "{}:{}-{}:{}-{}".format(self.seq_id, self.start, self.end, self.lltr_e, self.rltr_s)

    def overlap(self, other):
        ovl = max(0, min(self.end, other.end) - max(self.start, other.start))
        return 100 * ovl / (min(self.element_len, other.element_len))


def read_scn(path):
    """the records of a `.scn` in file order; `#` lines (and blank ones) are skipped, a trailing `#source` column is ignored"""
    out = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            if line.startswith("#") or not line.strip():
                continue
            out.append(Record(line.strip().split(), "{}:{}".format(path, ln)))
    return out


SCN_HEADER = ("# LTR-RT candidates of the de novo detection (-ltr_denovo): chained exact seeds, no TSD or motif search\n"
              "# predictions are reported in the following way\n"
              "# s(ret) e(ret) l(ret) s(lLTR) e(lLTR) l(lLTR) s(rLTR) e(rLTR) l(rLTR) sim(LTRs) seq-nr chr\n"
              "# where:\n# s = starting position\n# e = ending position\n# l = length\n# ret = LTR-retrotransposon\n"
              "# lLTR = left LTR\n# rLTR = right LTR\n# sim = similarity\n# seq-nr = sequence number\n")


def write_scn(fout, ltrs, source="device"):
    """the comment header of ltrharvest's output as the reference's tmp/LTR.scn carries it, then the 12 columns of every
    record, 1-based and inclusive, and a `#source` column behind them, which read_scn ignores"""
    fout.write(SCN_HEADER)
    for r in ltrs:
        fout.write(" ".join(map(str, r.columns())) + " #" + source + "\n")


def chain_hsps(hsps, indel=LTR_CHAIN_INDEL, join=LTR_CHAIN_JOIN):
    """Chains of the HSPs (p0, n, d) of one chromosome, walked in ascending order: [(a0, a1, b0, b1)] in the order the chains
    were opened.  A chain keeps the hull of its left copies [a0, a1) and of its right copies [b0, b1), `end` = the largest
    p0 + n so far and the d, p0, q0 of its last HSP; it closes for good once an HSP arrives with p0 - end > join.  An HSP
    joins an open chain when |d - last d| <= indel, p0 >= last p0, p0 + d >= last q0 and p0 + n > end -- of the chains
    that qualify the one with the largest end, the earliest opened on a tie -- else it opens a chain."""
    chains, live = [], []          # a chain: [a0, a1, b0, b1, end, d, p0, q0]; live: indices of the open ones, by opening
    for p0, n, d in hsps:
        p0, n, d = int(p0), int(n), int(d)
        live = [i for i in live if p0 - chains[i][4] <= join]
        best = None
        for i in live:
            c = chains[i]
            if abs(d - c[5]) <= indel and p0 >= c[6] and p0 + d >= c[7] and p0 + n > c[4] and (best is None or c[4] > chains[best][4]):
                best = i
        if best is None:
            live.append(len(chains))
            chains.append([p0, p0 + n, p0 + d, p0 + d + n, p0 + n, d, p0, p0 + d])
        else:
            c = chains[best]
            c[1], c[3], c[4] = max(c[1], p0 + n), max(c[3], p0 + d + n), max(c[4], p0 + n)
            c[5], c[6], c[7] = d, p0, p0 + d
    return [tuple(c[:4]) for c in chains]


def candidates(chains, minlen=LTR_MINLEN, maxlen=LTR_MAXLEN, dmin=LTR_MINDIST, dmax=LTR_MAXDIST):
    """the chains that look like the two LTRs of an element: both hulls minlen..maxlen long, their starts dmin..dmax apart,
    the left one ending before the right one begins"""
    return [(a0, a1, b0, b1) for a0, a1, b0, b1 in chains
            if minlen <= a1 - a0 <= maxlen and minlen <= b1 - b0 <= maxlen and dmin <= b0 - a0 <= dmax and a1 <= b0]


def similarity(counts, similar=LTR_SIMILAR):
    """(sim per candidate or None, indices kept, number dropped as not aligned) from the int32 [n, 6] of Context.ltr_align:
    sim = 100 match / (match + mismatch + gap) -- skip columns do not count; a candidate outside the limits of the alignment
    (FLAG_BAND, FLAG_LEN) or without a counted column is dropped; one with sim >= similar is kept"""
    sims, keep, dropped = [], [], 0
    for i, row in enumerate(counts):
        m, x, g, flags = int(row[1]), int(row[2]), int(row[3]), int(row[5])
        if flags & (FLAG_BAND | FLAG_LEN) or m + x + g == 0:
            sims.append(None)
            dropped += 1
            continue
        sims.append(100 * m / (m + x + g))
        if sims[-1] >= similar:
            keep.append(i)
    return sims, keep, dropped


def detect(ctx, labels, band, opt):
    """-ltr_denovo on the resident genome, opt = {name: value} of the DETECT_OPTIONS: per chromosome the extended seeds of
    the device, chained here, and the chains that look like an LTR pair; then ONE ltr_align call for all candidates and the
    similarity filter.  (records, tallies: what was counted on the way, and the seconds of the two parts)"""
    if not 1 <= opt["minlen"] <= opt["maxlen"]:
        raise ValueError("-ltr_minlen {} is below 1 or above -ltr_maxlen {}".format(opt["minlen"], opt["maxlen"]))
    if opt["chain_indel"] < 0 or opt["chain_join"] < 0:
        raise ValueError("-ltr_chain_indel {} or -ltr_chain_join {} is below 0".format(opt["chain_indel"], opt["chain_join"]))
    t0 = time.perf_counter()
    n_seeds = n_hsps = n_chains = dropped = 0
    cands = []                     # (chromosome index, a0, a1, b0, b1)
    for ci in range(len(labels)):
        ns, nh = ctx.ltr_seeds(ci, opt["seed"], opt["xdrop"], opt["mindist"], opt["maxdist"], opt["maxlen"])
        p0, ln, d = ctx.ltr_hsps(nh)
        chains = chain_hsps(zip(p0.tolist(), ln.tolist(), d.tolist()), opt["chain_indel"], opt["chain_join"])
        n_seeds, n_hsps, n_chains = n_seeds + ns, n_hsps + nh, n_chains + len(chains)
        cands += [(ci,) + c for c in candidates(chains, opt["minlen"], opt["maxlen"], opt["mindist"], opt["maxdist"])]
    t1 = time.perf_counter()
    ltrs = []
    if cands:
        ci, a0, a1, b0, b1 = (np.array(x, np.int64) for x in zip(*cands))
        counts = np.asarray(ctx.ltr_align(ci.astype(np.int32), a0, a1 - a0, b0, b1 - b0, band))
        sims, keep, dropped = similarity(counts, opt["similar"])
        ltrs = [Record.from_coords(labels[cands[i][0]], cands[i][0], *cands[i][1:], sims[i]) for i in keep]
    return ltrs, dict(seeds=n_seeds, hsps=n_hsps, chains=n_chains, candidates=len(cands), dropped=dropped,
                      t_seeds=t1 - t0, t_align=time.perf_counter() - t1)


def resolve_overlaps(ltrs, max_ovl=MAX_OVL, completed=None):
    """resolve_overlaps (LTR.py:422-468) for records of one sequence: walking by start, of two records that overlap by more
    than max_ovl % of the shorter the longer stays (the earlier on a tie) and is what the next record is compared with; of
    two equal records the later goes.  `completed`: the keys of the records a classification calls complete (None: none is,
    as without -ltr_hmm) -- when exactly one of the two is complete, it stays whatever the lengths.  What is returned is
    set(ltrs) - set(discards) with the reference's equality -- the key (seq_id, start, end, lltr_e, rltr_s) -- so a
    discarded record takes every record of its key with it.  Order: (start, end, lltr_e, rltr_s) (the reference leaves
    equal starts in set order)."""
    done = completed or ()
    last, discards = None, set()
    for ltr in sorted(ltrs, key=lambda x: x.start):
        if last is not None:
            if ltr.key == last.key:
                discard = ltr
            elif ltr.overlap(last) > max_ovl:
                if (ltr.key in done) != (last.key in done):
                    discard = last if ltr.key in done else ltr
                else:
                    discard = last if ltr.element_len > last.element_len else ltr
            else:
                last = ltr
                continue
            discards.add(discard.key)
            if discard.key == ltr.key:
                continue
        last = ltr
    seen, kept = set(discards), []
    for ltr in ltrs:
        if ltr.key not in seen:
            seen.add(ltr.key)
            kept.append(ltr)
    return sorted(kept, key=lambda x: (x.start, x.end, x.lltr_e, x.rltr_s))


def group_resolve_overlaps(ltrs, completed=None):
    """group_resolve_overlaps (LTR.py:415-420): runs of consecutive records of one sequence, each resolved on its own"""
    out, i = [], 0
    while i < len(ltrs):
        j = i
        while j < len(ltrs) and ltrs[j].seq_id == ltrs[i].seq_id:
            j += 1
        out += resolve_overlaps(ltrs[i:j], completed=completed)
        i = j
    return out


def estimate_age(div, mu):
    """estimate_age (LTR.py:680-686, JC69) of a divergence, in years"""
    if div >= 0.75:
        dist = div
    else:
        dist = -3 / 4 * math.log(1 - 4 * div / 3)
    return dist / (mu * 2)


def ltr_intervals(ltrs):
    """0-based (a_start, a_len, b_start, b_len) of the two LTRs of every record"""
    a0 = np.array([r.start - 1 for r in ltrs], np.int64)
    la = np.array([r.lltr for r in ltrs], np.int64)
    lb = np.array([r.rltr for r in ltrs], np.int64)
    b0 = np.array([r.end - r.rltr for r in ltrs], np.int64)
    return a0, la, b0, lb


def divergences(ltrs, counts, mode):
    """(div list, number of elements that fell back to the file's similarity).  counts: int32 [n, 6] of Context.ltr_align or
    None.  align: mismatch / (match + mismatch) -- gap and skip columns carry no substitution information; an element
    without a substitution column or one that was not aligned takes 1 - similarity / 100, which is what scn takes for all."""
    divs, fell = [], 0
    for i, r in enumerate(ltrs):
        if mode == "align" and counts is not None:
            m, x, flags = int(counts[i][1]), int(counts[i][2]), int(counts[i][5])
            if m + x > 0 and not flags & (FLAG_BAND | FLAG_LEN):
                divs.append(x / (m + x))
                continue
            fell += 1
        divs.append(1 - r.similarity / 100)
    return divs, fell


def write_identity(fout, ltrs, counts, divs, ages):
    fout.write("\t".join(["#id", "similarity", "score", "match", "mismatch", "gap", "skip", "flags", "div", "age"]) + "\n")
    for i, r in enumerate(ltrs):
        cc = ["NA"] * 6 if counts is None else [str(int(x)) for x in counts[i]]
        fout.write("\t".join([r.id, str(r.similarity)] + cc + [str(divs[i]), str(ages[i])]) + "\n")


def write_insert_data(fout, ltrs, ages, d_enriched, d_exchange, exclude_exchanges=False, non_specific=False):
    """`.ltr.insert.data` as plot_insert_age writes it (LTR.py:474-511; `shared` is empty): ({sg: [age in Myr]}, enriched
    records, number excluded as potential exchanges)"""
    fout.write("\t".join(["ltr", "sg", "age"]) + "\n")
    d_data, enriched, excluded = {}, [], 0
    for ltr, age in zip(ltrs, ages):
        if ltr.id in d_enriched:
            sg = d_enriched[ltr.id]
            enriched.append(ltr)
            if exclude_exchanges and d_exchange.get(ltr.id) == "yes":
                excluded += 1
                continue
        elif non_specific:
            sg = "non-specific"
        else:
            continue
        age = age / 1e6
        fout.write("\t".join(map(str, [ltr.id, sg, age])) + "\n")
        d_data.setdefault(sg, []).append(age)
    return d_data, enriched, excluded


def summary_ltr_time(d_data, fout):
    """`.ltr.insert.summary` and the two log lines of summary_ltr_time (LTR.py:568-606): {sg: "median (95% CI)"}"""
    fout.write("# Summary of LTR insertion age (million years)\n")
    fout.write("\t".join(["#subgenome", "mean", "median", "standard_deviation", "75%-CI", "95%-CI", "99%-CI"]) + "\n")
    d_info, xages, medians, lo95, hi95 = {}, [], [], [], []
    for sg, ages in sorted(d_data.items()):
        xages += ages
        ages = np.array(ages)
        median = np.median(ages)
        medians.append(median)
        t2_5, t97_5 = np.percentile(ages, 2.5), np.percentile(ages, 97.5)
        lo95.append(t2_5)
        hi95.append(t97_5)
        ci95 = "{:.3f}-{:.3f}".format(abs(t2_5), t97_5)
        ci99 = "{:.3f}-{:.3f}".format(abs(np.percentile(ages, 0.5)), np.percentile(ages, 99.5))
        ci75 = "{:.3f}-{:.3f}".format(np.percentile(ages, 12.5), np.percentile(ages, 87.5))
        median = "{:.3f}".format(median)
        fout.write("\t".join([sg, "{:.3f}".format(ages.mean()), median, "{:.3f}".format(np.std(ages)), ci75, ci95, ci99]) + "\n")
        d_info[sg] = "{} ({})".format(median, ci95)
    logger.info("Summary of overall LTR insertion age (million years):")
    logger.info("\tmedian: {:.3f}\t95% CI (percentile-based): {:.3f}-{:.3f}".format(
        np.median(xages), abs(np.percentile(xages, 2.5)), np.percentile(xages, 97.5)))
    logger.info("A rough estimation of the divergence–hybridization period: {:.3f}-{:.3f} ({:.3f})".format(
        np.mean(hi95), np.mean(lo95), np.mean(medians)))
    return d_info


def _density(x, grid):
    """Gaussian kernel density with R's default bandwidth (bw.nrd0), what geom_line(stat = "density") draws"""
    x = np.asarray(x, float)
    sd, iqr = (x.std(ddof=1) if x.size > 1 else 0.0), np.subtract(*np.percentile(x, [75, 25]))
    lo = min(sd, iqr / 1.34) or sd or abs(x[0]) or 1.0
    bw = 0.9 * lo * x.size ** -0.2
    z = (grid[:, None] - x[None, :]) / bw
    return np.exp(-0.5 * z * z).sum(axis=1) / (x.size * bw * math.sqrt(2 * math.pi))


def plot(d_data, d_info, density_fig, histo_fig, sg_colors=None):
    """`.ltr.insert.density.<figfmt>` and `.ltr.insert.histo.<figfmt>`: the two ggplot figures of plot_insert_age, drawn with
    matplotlib (age density per subgenome; stacked histogram of 30 bins), annotated with the summary"""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    sgs = sorted(d_data)
    cycle = plt.rcParams["axes.prop_cycle"].by_key()["color"]
    colors = [(sg_colors or {}).get(sg, cycle[i % len(cycle)]) for i, sg in enumerate(sgs)]
    text = "Summary: median (95% CI)\n" + "".join("{}: {}\n".format(sg, info) for sg, info in sorted(d_info.items()))
    allx = np.concatenate([np.asarray(d_data[sg], float) for sg in sgs])
    span = (allx.max() - allx.min()) or 1.0
    grid = np.linspace(allx.min() - 0.1 * span, allx.max() + 0.1 * span, 512)
    for kind, path in (("density", density_fig), ("histo", histo_fig)):
        fig, ax = plt.subplots(figsize=(7, 7))
        if kind == "density":
            for sg, c in zip(sgs, colors):
                ax.plot(grid, _density(d_data[sg], grid), color=c, lw=2, label=sg)
            ax.set_ylabel("Density")
        else:
            ax.hist([d_data[sg] for sg in sgs], bins=30, stacked=True, color=colors, label=sgs)
            ax.set_ylabel("Frequence")
        ax.set_xlabel("LTR insertion age (million years)")
        ax.text(0.97, 0.97, text, transform=ax.transAxes, ha="right", va="top")
        ax.legend(loc="center right", frameon=False)
        fig.savefig(path, dpi=300)
        plt.close(fig)
