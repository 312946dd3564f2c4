"""LTR-RT classification from protein domains: the profiles, the hits of the device search, TEsorter's rules restated.

The reference classifies the inner sequences of its LTR-RTs with TEsorter: hmmscan of their six-frame translation against
REXdb, the best hit per domain, and a rule table from domains to order / superfamily / clade (LTR.py:378-401).  Neither
HMMER nor a profile database exists here, so the SEARCH is this build's own: a local Viterbi alignment in integer
arithmetic, one hit per (frame, profile), defined in csrc/sp_domains.h and run on the device (Context.dom_search).  It is
not hmmscan: there is no length model, no multi-hit loop, no E-value and no posterior probability, the background is the
codon composition of translated random DNA and not HMMER's Swiss-Prot composition, and the two thresholds below are
provisional -- our bits are not HMMER's envelope bits.  What follows the search -- names, filters, coordinates, the
`.dom.gff3` lines and the classifier -- restates TEsorter (subphaser/api/TEsorter/app.py) as it is, quirks included:

  read_hmm       a HMMER3 ASCII file (REXdb's `.hmm` as TEsorter ships it, or any other) -> integer tables
  parse_name     parse_hmmname for rexdb: gene, clade, domain; full clade name
  best_domains   the best profile per (element, domain) by score per node, and TEsorter's coverage and score filters
  coordinates    hmm2best's nucleotide coordinates (app.py:970-990)
  write_gff      `.ltr.dom.gff3`
  classify       Classifier.classify / identify_rexdb / _parse_rexdb (app.py:460-547) -> rows of `.ltr.cls.tsv`
Not here: the domain peptides (`.dom.faa`), TEsorter's pass 2 (blast), the trees from domain alignments."""
import math
import re
from collections import Counter

import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY"
SCALE = 256                    # SP_DM_SCALE: scores are integers in units of 1/256 bit
NEG = -(1 << 20)               # SP_DM_NEG: a `*` of the file
EMAX = 1 << 15                 # SP_DM_EMAX
STOP_COST = 2048               # SP_DM_STOPCOST: a stop codon costs 8 bits in every node
COLS, COL_X, COL_STOP = 22, 20, 21
MAX_M, MAX_LEN, MAX_P = 2048, 65536, 4096      # SP_DM_MAXM, SP_DM_MAXLEN, SP_DM_MAXP
MIN_COV, MIN_SCORE = 20.0, 0.5                 # TEsorter's mincov and minscore (hmm2best)
# -ltr_dom_prefilter without a value: the threshold of the ungapped prefilter in bits.  PROVISIONAL, set by a rule
# (profiles/domains_notes.md): the smallest whole number of bits, of the 8..30 swept, at which at most 2 % of the (frame,
# profile) pairs of random DNA pass (1.02 % at 8), on assumed profiles and synthetic DNA -- no REXdb, no calibration, no
# comparison with hmmscan
PREFILTER_BITS = 8
# codons per amino acid of the standard code: the background is codons / 61.  PROVISIONAL: the composition of translated
# random DNA, not HMMER's Swiss-Prot composition
CODONS = dict(zip(AA, (4, 2, 2, 2, 2, 4, 2, 3, 2, 6, 1, 2, 4, 2, 6, 6, 4, 4, 1, 2)))
BACKGROUND = {a: CODONS[a] / 61.0 for a in AA}
LN2 = math.log(2.0)


def trans_score(v):
    """a transition -ln p of the file -> 1/256 bit"""
    return NEG if v is None else int(math.floor(-v * SCALE / LN2 + 0.5))


def emis_score(v, a):
    """a match emission -ln p of residue a -> its log-odds against the background, 1/256 bit"""
    return NEG if v is None else int(math.floor((-v / LN2 - math.log2(BACKGROUND[a])) * SCALE + 0.5))


def entry_score(M):
    """HMMER's uniform local entry 2 / (M (M + 1))"""
    return int(math.floor(math.log2(2.0 / (M * (M + 1))) * SCALE + 0.5))


class Profiles:
    """The profiles of a file: names, M per profile, and the tables Context.dom_search takes"""

    def __init__(self, names, emis, trans):
        self.names = list(names)
        self.M = [len(e) for e in emis]
        self.moff = np.concatenate(([0], np.cumsum(self.M))).astype(np.int32)
        self.emis = np.concatenate(emis).astype(np.int32).reshape(-1, COLS) if emis else np.zeros((0, COLS), np.int32)
        self.trans = np.concatenate(trans).astype(np.int32).reshape(-1, 7) if trans else np.zeros((0, 7), np.int32)
        self.entry = np.array([entry_score(m) for m in self.M], np.int32)

    def __len__(self):
        return len(self.names)

    def tables(self):
        return self.moff, self.emis, self.trans, self.entry


def _values(tokens, n, where, what):
    if len(tokens) < n:
        raise ValueError("{}: expected {} ({} values), found {}".format(where, what, n, len(tokens)))
    out = []
    for t in tokens[:n]:
        if t == "*":
            out.append(None)
            continue
        try:
            v = float(t)
        except ValueError:
            raise ValueError("{}: expected {} ({} numbers or `*`), found `{}`".format(where, what, n, t)) from None
        if not math.isfinite(v):
            raise ValueError("{}: expected {} (finite numbers or `*`), found `{}`".format(where, what, t))
        out.append(v)
    return out


def read_hmm(path):
    """The profiles of a HMMER3 ASCII file (any number, each ended by `//`): NAME, LENG and ALPH (amino) of the header, the
    match emissions and the transitions of nodes 1..M.  Node 0, the insert emissions, COMPO and every other header line are
    skipped.  Values are -ln p, `*` is p = 0.  ValueError names the file, the line and what was expected."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    pos = [0]

    def where():
        return "{}:{}".format(path, pos[0])

    def take(what):
        if pos[0] >= len(lines):
            raise ValueError("{}:{}: the file ends where {} was expected".format(path, len(lines) + 1, what))
        pos[0] += 1
        return lines[pos[0] - 1]

    names, emis, trans = [], [], []
    while pos[0] < len(lines):
        if not lines[pos[0]].strip():
            pos[0] += 1
            continue
        first = take("a profile")
        if not first.startswith("HMMER3/"):
            raise ValueError("{}: expected the first line of a profile (`HMMER3/...`), found `{}`".format(where(), first[:40]))
        name, M, alph = None, None, None
        while True:
            line = take("the `HMM` line of the profile")
            tag = line.split(None, 1)
            if not tag:
                continue
            if tag[0] == "HMM":
                break
            if tag[0] == "//":
                raise ValueError("{}: expected the `HMM` line before the end of the profile".format(where()))
            val = tag[1].strip() if len(tag) > 1 else ""
            if tag[0] == "NAME":
                name = val
            elif tag[0] == "LENG":
                try:
                    M = int(val)
                except ValueError:
                    raise ValueError("{}: expected `LENG <integer>`, found `{}`".format(where(), line.strip())) from None
            elif tag[0] == "ALPH":
                alph = val.lower()
        if not name:
            raise ValueError("{}: expected a `NAME` line before the `HMM` line".format(where()))
        if M is None or M < 1:
            raise ValueError("{}: profile {}: expected a `LENG` line with a length of 1 at least before the `HMM` line".format(where(), name))
        if alph != "amino":
            raise ValueError("{}: profile {}: expected `ALPH  amino`, found `{}`".format(where(), name, alph))
        if line.split()[1:] != list(AA):
            raise ValueError("{}: profile {}: expected the 20 letters `{}` on the `HMM` line".format(where(), name, " ".join(AA)))
        take("the transition header line")
        line = take("node 0")
        if line.split()[:1] == ["COMPO"]:
            line = take("node 0")
        _values(line.split(), 20, where(), "the insert emissions of node 0")
        _values(take("the transitions of node 0").split(), 7, where(), "the transitions of node 0")
        e, t = np.zeros((M, COLS), np.int64), np.zeros((M, 7), np.int64)
        for k in range(1, M + 1):
            tok = take("the match line of node {}".format(k)).split()
            if tok[:1] != [str(k)]:
                raise ValueError("{}: profile {}: expected the match line of node {} of {}, found `{}`".format(where(), name, k, M, " ".join(tok[:2])))
            vals = _values(tok[1:], 20, where(), "the match emissions of node {}".format(k))
            e[k - 1, :20] = [emis_score(v, a) for v, a in zip(vals, AA)]
            e[k - 1, COL_X], e[k - 1, COL_STOP] = 0, -STOP_COST
            _values(take("the insert line of node {}".format(k)).split(), 20, where(), "the insert emissions of node {}".format(k))
            vals = _values(take("the transition line of node {}".format(k)).split(), 7, where(), "the transitions of node {}".format(k))
            t[k - 1] = [trans_score(v) for v in vals]
        if e[:, :20].max() > EMAX or e[:, :20].min() < NEG or t.max() > 0 or t.min() < NEG:
            raise ValueError("{}: profile {}: expected probabilities (-ln p >= 0, scores within 2^20 of 0); a value is outside".format(where(), name))
        end = take("the `//` that ends profile {}".format(name))
        if end.strip() != "//":
            raise ValueError("{}: profile {}: expected `//` after node {}, found `{}`".format(where(), name, M, end.strip()[:40]))
        names.append(name)
        emis.append(e)
        trans.append(t)
    if not names:
        raise ValueError("{}:1: expected a profile (`HMMER3/...`), the file holds none".format(path))
    return Profiles(names, emis, trans)


# ------------------------------------------------------------------------------------------------ names
def parse_name(name):
    """(gene, clade, domain, full clade name) of a profile: parse_hmmname for rexdb -- `Class_I/LTR/Ty3_gypsy/chromovirus/
    Tekay:Ty3-RT` is gene Ty3-RT, clade Tekay, domain RT (aRH counts as RH and TPase as INT, _hmm2best), full name the part
    in front of the colon (what LTRgffLine.name carries to the classifier).  A name without a colon is its own gene, clade
    and domain."""
    if ":" not in name:
        return name, name, name, name
    full, gene = name.split(":")[0], name.split(":")[1]
    parts = gene.split("-")
    domain = parts[1] if len(parts) > 1 else gene
    domain = {"aRH": "RH", "TPase": "INT"}.get(domain, domain)
    return gene, full.split("/")[-1], domain, full


# ------------------------------------------------------------------------------------------------ hits
class Domain:
    """one line of `.ltr.dom.gff3`"""
    __slots__ = ("element", "seqid", "start", "end", "score", "strand", "frame", "profile", "gene", "clade", "full", "coverage", "raw", "pidx", "hit")

    def attributes(self):
        return "ID={}|{};Name={}-{};gene={};clade={};coverage={};score={}".format(
            format_gff_id(self.element), self.profile, self.clade, self.gene, self.gene, self.clade, self.coverage, self.score)

    def columns(self):
        return [self.seqid, "subphaser_amd", "CDS", self.start, self.end, self.score, self.strand, self.frame, self.attributes()]


def format_gff_id(s):
    return re.sub(r"[;=\|]", "_", s)


def coordinates(element_id, frame, i_start, i_end, n):
    """hmm2best's nucleotide coordinates (app.py:970-990) of residues i_start..i_end (0-based, inclusive) of frame 0..5 of
    an inner sequence of n bases: (seqid, start, end, strand, frame 0..2), 1-based and inclusive.  As in TEsorter the
    offset added is the first number of the element's id -- the start of the ELEMENT, not of its inner sequence, so the
    coordinates lie lltr - 1 bases left of the domain; the order of an element's domains, which is all the classifier
    reads, is not affected."""
    env_start, env_end = i_start + 1, i_end + 1
    if frame < 3:
        strand, fr = "+", frame
        a, b = (env_start - 1) * 3 + fr + 1, env_end * 3 + fr
    else:
        strand, fr = "-", frame - 3
        a, b = n - (env_end * 3 + fr) + 1, n - ((env_start - 1) * 3 + fr)
    seqid = element_id
    m = re.compile(r"(\S+?):(\d+)[\.\-]+(\d+)").match(element_id)
    if m:
        seqid, line_start = m.group(1), int(m.group(2))
        a, b = line_start + a - 1, line_start + b - 1
    return seqid, a, b, strand, fr


def best_domains(ids, lengths, hits, profiles, min_cov=MIN_COV, min_score=MIN_SCORE):
    """The lines of `.ltr.dom.gff3` from the hits of Context.dom_search (int32 [n, P, 6]) of n elements (ids; lengths of
    their inner sequences).  Per (element, domain) the profile with the largest score per node wins -- s1 M2 > s2 M1 in
    integers, the lower profile on a tie.  This is this build's rule: TEsorter's replacement in file order with its
    overlap clause and its rounding to two decimals is not reproduced.  Then TEsorter's filters: coverage 100 (k_end -
    k_start + 1) / M >= min_cov, and score per node >= min_score bits, i.e. score >= min_score 256 M; both compared in
    integers, against the right side rounded up.  No E-value and no probability: there are no calibrated
    statistics.  Sorted as hmm2best sorts: (sequence, element id, start)."""
    parsed = [parse_name(n) for n in profiles.names]
    out = []
    hits = np.asarray(hits)
    for e, eid in enumerate(ids):
        best = {}
        for p in range(len(profiles)):
            s = int(hits[e, p, 0])
            if s == -(1 << 31):
                continue
            dom = parsed[p][2]
            if dom not in best or s * profiles.M[best[dom]] > int(hits[e, best[dom], 0]) * profiles.M[p]:
                best[dom] = p
        for dom, p in best.items():
            s, frame, i0, i1, k0, k1 = (int(x) for x in hits[e, p])
            M = profiles.M[p]
            if 100 * (k1 - k0 + 1) < math.ceil(min_cov * M) or s < math.ceil(min_score * SCALE * M):
                continue
            d = Domain()
            d.element, d.profile, d.raw = eid, profiles.names[p], s
            d.pidx, d.hit = p, (frame, i0, i1)      # the profile's index and (frame 0..5, i_start, i_end): what the domain trees align
            d.seqid, d.start, d.end, d.strand, d.frame = coordinates(eid, frame, i0, i1, int(lengths[e]))
            d.score = round(s / float(SCALE * M), 2)
            d.coverage = round(1e2 * (k1 - k0 + 1) / M, 1)
            _, d.clade, d.gene, d.full = parsed[p]
            out.append(d)
    out.sort(key=lambda d: (d.seqid, d.element, d.start))
    return out


def write_gff(fout, domains):
    for d in domains:
        fout.write("\t".join(map(str, d.columns())) + "\n")


# ------------------------------------------------------------------------------------------------ the classifier
CLS_HEADER = ["#TE", "Order", "Superfamily", "Clade", "Complete", "Strand", "Domains"]
PERFECT = {("LTR", "Copia"): ["GAG", "PROT", "INT", "RT", "RH"],
           ("LTR", "Gypsy"): ["GAG", "PROT", "RT", "RH", "INT"],
           ("LTR", "Bel-Pao"): ["GAG", "PROT", "RT", "RH", "INT"]}


def parse_rexdb(clade):
    """_parse_rexdb: (order, superfamily) of a full clade name.  A name of no known class is ('Unknown', 'unknown'): the
    reference fails there (its warning names an undefined variable)."""
    if clade.startswith("Class_I/LTR/Ty1_copia"):
        return "LTR", "Copia"
    if clade.startswith("Class_I/LTR/Ty3_gypsy"):
        return "LTR", "Gypsy"
    if clade.startswith("Class_I/LTR/"):
        parts = clade.split("/")[1:3]
    elif clade.startswith("Class_I/"):
        parts = clade.split("/")[1:3]
    elif clade.startswith("Class_II/"):
        parts = clade.split("/")[2:4]
    elif clade.startswith("NA"):
        return "LTR", "Retrovirus"
    else:
        return "Unknown", "unknown"
    return (parts[0], parts[1]) if len(parts) == 2 else (parts[0], "unknown")


def identify(genes, clades):
    """identify_rexdb on the genes and FULL clade names of an element's domains in order: (order, superfamily, clade,
    complete).  The clade that occurs most often names the element when it is the only one or occurs more than once AND
    the first clade seen is more frequent than the second seen (counts[0] > counts[1]: insertion order, the reference's
    quirk); otherwise `mixture`, and superfamily and order become `mixture` when they differ among the domains."""
    count = Counter(clades)
    counts = list(count.values())
    top = max(count, key=lambda x: count[x])
    order, superfamily = parse_rexdb(top)
    if len(count) == 1 or (count[top] > 1 and counts[0] > counts[1]):
        top = top.split("/")[-1]
    else:
        top = "mixture"
        if len(Counter(parse_rexdb(c)[1] for c in clades)) > 1:
            superfamily = "mixture"
            if len(Counter(parse_rexdb(c)[0] for c in clades)) > 1:
                order = "mixture"
    if (order, superfamily) in PERFECT:
        ordered = PERFECT[(order, superfamily)]
        complete = "yes" if [g for g in genes if g in set(ordered)] == ordered else "no"
    else:
        complete = "unknown"
    if superfamily not in ("Copia", "Gypsy") or top.startswith("Ty"):
        top = "unknown"
    return order, superfamily, top, complete


def classify(domains):
    """Classifier.classify on the lines of `.ltr.dom.gff3` in file order: rows [id, order, superfamily, clade, complete,
    strand, domains].  Lines of one element are consecutive; `?` is the strand of an element whose domains lie on both, and
    the domains of a `-` element are read from its last line to its first (the Domains column too: the reference reverses
    the list in place before it prints it)."""
    rows, i = [], 0
    while i < len(domains):
        j = i
        while j < len(domains) and domains[j].element == domains[i].element:
            j += 1
        rc = list(domains[i:j])
        i = j
        strands = set(d.strand for d in rc)
        strand = "?" if len(strands) > 1 else rc[0].strand
        if strand == "-":
            rc.reverse()
        order, superfamily, clade, complete = identify([d.gene for d in rc], [d.full for d in rc])
        rows.append([format_gff_id(rc[0].element), order, superfamily, clade, complete, strand, " ".join("{}|{}".format(d.gene, d.clade) for d in rc)])
    return rows


def write_cls(fout, rows):
    fout.write("\t".join(CLS_HEADER) + "\n")
    for r in rows:
        fout.write("\t".join(r) + "\n")


def inner_interval(r):
    """the inner sequence of a record as get_int_seq cuts it (LTR.py:698): seq[lltr_e:rltr_s], 0-based and half-open -- the
    1-based lltr_e and rltr_s used as 0-based slice bounds, so it starts behind the last base of the left LTR and ends ON
    the first base of the right one"""
    return r.lltr_e, max(r.lltr_e, r.rltr_s)
