"""The domain trees of the LTR stage (-ltr_domtree): host side.

The reference ends its module 3 in one tree per Copia / Gypsy (LTR.LTRtree, LTR.py:144-233): the domain peptides of
TEsorter's `.cls.pep`, concat_domains keeps the elements with all of -ltr_domains, mafft aligns each domain, catAln
concatenates, trimal trims, iqtree or FastTree builds the tree, nw_reroot roots it.  None of these programs is part of this
build, so the trees here are defined by their own arithmetic and were never compared with mafft, trimal or iqtree:
  alignment  every element's domain is aligned to ONE profile per domain (the common profile: the winner of that domain
             for the most selected elements -- REXdb has one profile per (clade, domain), and match columns of different
             profiles are not comparable) by the Viterbi path of csrc/sp_domalign.h; a row is the residues on the
             profile's match nodes, `-` elsewhere.  Inserted residues appear in no column.
  trimming   a column stays when at least -ltr_tree_occupancy percent of the rows hold a residue (integers).
  distance   Kimura's protein distance of the share of differing columns, in the fixed point of ltrtree.UNIT.
  tree       neighbour joining (Context.nj_tree), midpoint rooting, newick and figure of ltrtree.py, unchanged.
The device answers four calls (Context.dom_align, dom_peptide, aln_pairs, nj_tree); everything here lies between them."""
import math
import re
from collections import Counter

import numpy as np

from . import ltrtree

PAD = 32                 # residues either side of an element's own hit that its window takes; provisional
OCCUPANCY = 50           # -ltr_tree_occupancy: percent of rows with a residue a column needs; provisional
OVERLAP = 20             # -ltr_tree_overlap: columns two rows must share for a distance of their own; provisional
DOMAINS = ("INT", "RT", "RH")      # the reference's -ltr_domains
CATEGORIES = (("LTR", "Copia"), ("LTR", "Gypsy"))
MAX_WIN = 8192           # SP_DA_MAXWIN
MAX_N = 4096             # SP_DA_MAXN, SP_LT_MAXN
MAX_C = 8192             # SP_DA_MAXC
LETTERS = "ACDEFGHIKLMNPQRSTVWYX*"
GAP = 255
P_CAP = 0.75
D_CAP = 2130444828       # kimura_units at p = 0.75: floor(-ln(0.1375) * 2^30 + 0.5) < 2^31, what Context.nj_tree takes


def fmt_cls(*args):
    """TEsorter's fmt_cls: the parts that are not `unknown`, each once, joined by `/`"""
    values = []
    for a in args:
        if a == "unknown" or a in values:
            continue
        values.append(a)
    return "/".join(values)


def format_id_for_iqtree(name):
    return re.sub(r"[^\w]+", "_", name)


def peptide(codes):
    return "".join(LETTERS[int(c)] for c in codes)


def write_pep(fout, domains, rows, peptides):
    """`.ltr.cls.pep`: per line of `.ltr.dom.gff3` (domains.Domain) one record in the shape TEsorter gives `.cls.pep`
    (app.py:326-339): >{id}#{Order/Superfamily/Clade}#{gene}|{clade} {the gff attributes}.  rows: those of `.ltr.cls.tsv`."""
    from .domains import format_gff_id
    d_class = {r[0]: r for r in rows}
    for d, pep in zip(domains, peptides):
        rid = format_gff_id(d.element)
        r = d_class[rid]
        fout.write(">{}#{}#{}|{} {}\n{}\n".format(rid.split("#")[0], fmt_cls(r[1], r[2], r[3]), d.gene, d.clade, d.attributes(), pep))


def select(candidates, elem_domains, classes, order, superfamily, wanted):
    """The candidates (ids, in order) of one category that have every wanted domain.  elem_domains: {id: {domain: Domain}},
    classes: {id: (order, superfamily)}.  Returns (selected ids, {domain: number of the category's candidates with it})."""
    mine = [c for c in candidates if classes.get(c) == (order, superfamily)]
    counts = {dom: sum(dom in elem_domains.get(c, {}) for c in mine) for dom in wanted}
    return [c for c in mine if all(dom in elem_domains.get(c, {}) for dom in wanted)], counts


def common_profile(winners):
    """the profile index that wins for the most elements, the lowest index on a tie"""
    count = Counter(int(w) for w in winners)
    top = max(count.values())
    return min(p for p, n in count.items() if n == top)


def window(i_start, i_end, n_res, pad=PAD):
    """[i_start - pad, i_end + pad] clipped to the frame's residues 0 .. n_res - 1"""
    return max(0, int(i_start) - pad), min(int(n_res) - 1, int(i_end) + pad)


def n_residues(n_bases, frame):
    """sp_dm_nres: residues of frame 0..5 of an interval"""
    o = frame % 3
    return 0 if n_bases < o else (n_bases - o) // 3


def row_string(col, i0, codes):
    """the match-column row of one item: col from Context.dom_align (frame indices or -1), codes the residues of the window
    that starts at frame index i0 (Context.dom_peptide)"""
    return "".join("-" if c < 0 else LETTERS[int(codes[int(c) - i0])] for c in col)


def cat_rows(ids, blocks, unique=True):
    """catAln on aligned blocks: blocks[d][q] is the row of element q in domain d.  Returns (description, [(id, row)] kept,
    number dropped): with `unique` a row equal to an earlier one is dropped."""
    lens = [len(b[0]) if b else 0 for b in blocks]
    description = "genes:{} sites:{} blocks:{}".format(len(lens), sum(lens), lens)
    seen, kept, dropped = set(), [], 0
    for q, name in enumerate(ids):
        row = "".join(b[q] for b in blocks)
        if unique and row in seen:
            dropped += 1
            continue
        seen.add(row)
        kept.append((name, row))
    return description, kept, dropped


def write_aln(fout, records, description):
    for name, row in records:
        fout.write(">{} {}\n{}\n".format(name, description, row))


def encode(rows):
    """uint8 [N, C] for Context.aln_pairs: 0..19 the residues, 20 X, 21 stop, 255 the gap"""
    table = np.full(256, GAP, np.uint8)
    for code, letter in enumerate(LETTERS):
        table[ord(letter)] = code
    return table[np.frombuffer("".join(rows).encode("ascii"), np.uint8)].reshape(len(rows), -1)


def trim_columns(rows, occupancy=OCCUPANCY):
    """indices of the columns that stay: 100 * residues >= occupancy * rows, in integers; a residue is one of the 20 letters
    (X, stop and the gap are none, as in the comparison)"""
    codes = encode(rows)
    residues = (codes < 20).sum(axis=0).astype(np.int64)
    return np.flatnonzero(100 * residues >= int(occupancy) * len(rows)).tolist()


def trim(rows, occupancy=OCCUPANCY):
    keep = trim_columns(rows, occupancy)
    return ["".join(r[c] for c in keep) for r in rows]


def kimura_units(same, both, overlap=OVERLAP):
    """The fixed-point Kimura protein distance of (same, both) pairs, int64 of their shape: p = (both - same) / both, capped
    at 0.75, and p = 0.75 when both is below `overlap` or 0;  D = floor(-ln(1 - p - p^2 / 5) * 2^30 + 0.5).  The cap keeps
    D <= D_CAP = 2130444828 < 2^31."""
    same, both = np.asarray(same, np.int64), np.asarray(both, np.int64)
    if (same < 0).any() or (same > both).any():
        raise ValueError("kimura_units: a pair with same < 0 or same > both")
    out = np.empty(same.shape, np.int64)
    for idx in np.ndindex(*same.shape):
        s, b = int(same[idx]), int(both[idx])
        p = P_CAP if b == 0 or b < overlap else min(P_CAP, (b - s) / b)
        out[idx] = int(math.floor(-math.log(1.0 - p - p * p / 5.0) * ltrtree.UNIT + 0.5))
    return out


def distance_matrix(same, both, overlap=OVERLAP):
    """the N x N input of nj_tree: kimura_units of every pair, the diagonal zero; only the distinct (same, both) pairs are
    evaluated"""
    same, both = np.asarray(same, np.int64), np.asarray(both, np.int64)
    width = int(both.max(initial=0)) + 1
    uniq, inv = np.unique(same * width + both, return_inverse=True)
    D = kimura_units(uniq // width, uniq % width, overlap)[inv].reshape(same.shape)
    np.fill_diagonal(D, 0)
    return np.ascontiguousarray(D, np.int64)


REQUIRED = ("dom_align", "dom_peptide", "aln_pairs", "nj_tree")


def peptides_of(ctx, chrom, start, end, frame, i0, i1):
    """the letters of the windows, one string per item"""
    if not len(chrom):
        return []
    pep, poff = ctx.dom_peptide(chrom, start, end, frame, i0, i1)
    return [peptide(pep[int(poff[q]):int(poff[q + 1])]) for q in range(len(chrom))]


def align_category(ctx, selected, elem_domains, where, wanted, profiles, pad=PAD):
    """The aligned blocks of one category.  selected: ids; elem_domains[id][domain]: a domains.Domain with pidx (its profile)
    and hit = (frame, i_start, i_end); where[id] = (chromosome index, start, end) of the inner sequence.  Returns (ids that
    stay, blocks [domain][element] of row strings, {domain: common profile index}, ids left out for their window)."""
    common = {dom: common_profile([elem_domains[e][dom].pidx for e in selected]) for dom in wanted}
    items, out = [], []
    for e in selected:
        c, a, b = where[e]
        wins = []
        for dom in wanted:
            f, i_s, i_e = elem_domains[e][dom].hit
            wins.append((f,) + window(i_s, i_e, n_residues(b - a, f), pad))
        if any(i1 - i0 + 1 > MAX_WIN for _, i0, i1 in wins):
            out.append(e)
            continue
        items.append((e, c, a, b, wins))
    if not items:
        return [], [[] for _ in wanted], common, out
    cols = {k: [] for k in ("chrom", "start", "end", "frame", "i0", "i1", "prof")}
    for e, c, a, b, wins in items:
        for dom, (f, i0, i1) in zip(wanted, wins):
            for k, v in zip(cols, (c, a, b, f, i0, i1, common[dom])):
                cols[k].append(v)
    arr = {k: np.array(v, np.int64) for k, v in cols.items()}
    place = (arr["chrom"].astype(np.int32), arr["start"], arr["end"], arr["frame"].astype(np.int32), arr["i0"].astype(np.int32), arr["i1"].astype(np.int32))
    hit, col, coff = ctx.dom_align(*place, arr["prof"].astype(np.int32), *profiles.tables())
    pep, poff = ctx.dom_peptide(*place)
    blocks = [[] for _ in wanted]
    for q in range(len(arr["chrom"])):
        d = q % len(wanted)
        blocks[d].append(row_string(col[int(coff[q]):int(coff[q + 1])].tolist(), int(arr["i0"][q]), pep[int(poff[q]):int(poff[q + 1])]))
    return [it[0] for it in items], blocks, common, out
