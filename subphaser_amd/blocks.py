"""Homoeologous blocks: the host side of the anchor vote of csrc/sp_blocks.hip.

The reference aligns every pair of homoeologous chromosomes with minimap2 / unimap (Blocks.run_align, Blocks.py:7-56) and
keeps the primary alignments of alen >= -min_block as the links of the innermost ring (Circos.paf2blocks,
Circos.py:654-682).  Here the device votes per window of A for a window of B (definition in csrc/sp_blocks.h); this
module has the pair list of run_align, the walk that chains called windows into blocks, the two text outputs and a
figure.  Everything is integers; tests/blocks_ref.py is the twin of the walk.
"""
import itertools

import numpy as np

from .runtime import logger

# bin and votes: 10000 / 3 were the first choice; on the wheat-like synthetic genome they call 59 % of the windows and cover
# 48 % of a chromosome, 50000 / 5 cover 99.7 % in 40 times fewer blocks (profiles/blocks_notes.md)
BLOCK_K, BLOCK_SAMPLE, BLOCK_BIN, BLOCK_VOTES, BLOCK_GAP, MIN_BLOCK = 21, 4, 50000, 5, 5, 100000
# circos' chromosome colour names, one per config line, cycled (what paf2blocks takes by default)
LINK_COLORS = ["chr{}".format(c) for c in list(range(1, 23)) + ["X", "Y"]]
HEADER = "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tstrand\twindows\tanchors\n"


def pair_list(sgs):
    """Per config line the ordered chromosome pairs Blocks.run_align aligns: combinations(units, 2), then product of
    their chromosomes; a pair seen before (on this line or an earlier one) is left out."""
    seen, groups = set(), []
    for line in sgs:
        group = []
        for u1, u2 in itertools.combinations(line, 2):
            for pair in itertools.product(u1, u2):
                if pair in seen:
                    continue
                seen.add(pair)
                group.append(pair)
        groups.append(group)
    return groups


def walk(win_b, opp, votes, len_a, len_b, bin_size, min_votes=BLOCK_VOTES, max_gap=BLOCK_GAP, min_block=MIN_BLOCK):
    """Chain the called windows of A (votes >= min_votes), ascending, into blocks.  A window joins the open block when it
    has the same opp, dA = wa - wa_last <= max_gap + 1 and |dB - dA| <= max_gap (dB = wb - wb_last, or wb_last - wb for
    opp = 1); else the block closes and the window opens the next.  Returns the blocks with end1 - start1 >= min_block as
    (start1, end1, start2, end2, strand, windows, anchors), by start1."""
    win_b, opp, votes = np.asarray(win_b, np.int64), np.asarray(opp, np.int64), np.asarray(votes, np.int64)
    called = np.flatnonzero((votes >= min_votes) & (win_b >= 0))
    if called.size == 0:
        return []
    wa, wb, o, v = called, win_b[called], opp[called], votes[called]
    dA = np.diff(wa)
    dB = np.where(o[1:] == 1, wb[:-1] - wb[1:], wb[1:] - wb[:-1])
    joins = (o[1:] == o[:-1]) & (dA <= max_gap + 1) & (np.abs(dB - dA) <= max_gap)
    first = np.concatenate(([0], np.flatnonzero(~joins) + 1))
    last = np.concatenate((first[1:], [called.size])) - 1
    out = []
    for i, j in zip(first.tolist(), last.tolist()):
        s1, e1 = int(wa[i]) * bin_size, min((int(wa[j]) + 1) * bin_size, len_a)
        if e1 - s1 < min_block:
            continue
        seg = wb[i:j + 1]
        out.append((s1, e1, int(seg.min()) * bin_size, min((int(seg.max()) + 1) * bin_size, len_b), "-" if o[i] else "+",
                    j - i + 1, int(v[i:j + 1].sum())))
    return out


def write_tsv(fout, pair_blocks):
    """`blocks.tsv`: pair_blocks = [(chrom1, chrom2, blocks)] in pair order, blocks by start1"""
    fout.write(HEADER)
    for c1, c2, blocks in pair_blocks:
        for s1, e1, s2, e2, strand, n_win, n_anch in blocks:
            fout.write("\t".join(map(str, (c1, s1, e1, c2, s2, e2, strand, n_win, n_anch))) + "\n")


def write_links(fout, groups, colors=None):
    """`block_link.txt` as Circos.paf2blocks writes it: per config line its blocks sorted by size (end1 - start1,
    ascending, stable), `chr1 start1 end1 chr2 start2 end2 color=<c>`.  groups = [[(chrom1, chrom2, blocks)]] per line."""
    colors = colors or LINK_COLORS
    for i, group in enumerate(groups):
        rows = [(c1, b[0], b[1], c2, b[2], b[3]) for c1, c2, blocks in group for b in blocks]
        for row in sorted(rows, key=lambda r: r[2] - r[1]):
            fout.write(" ".join(map(str, row)) + " color={}\n".format(colors[i % len(colors)]))


def run(ctx, groups, labels, lengths, block_k=BLOCK_K, block_sample=BLOCK_SAMPLE, bin_size=BLOCK_BIN, min_votes=BLOCK_VOTES,
        max_gap=BLOCK_GAP, min_block=MIN_BLOCK):
    """Index, vote and walk every pair of `groups` (pair_list's result) on the device context: [[(chrom1, chrom2,
    blocks)]] per config line.  The indexes of a line's chromosomes are built when first needed and released after the
    line unless a later line uses the chromosome again."""
    where = {lab: i for i, lab in enumerate(labels)}
    last_use = {}
    for gi, group in enumerate(groups):
        for pair in group:
            for c in pair:
                last_use[c] = gi
    have, out = set(), []
    tot_pairs = tot_blocks = tot_cov = 0
    for gi, group in enumerate(groups):
        res = []
        for c1, c2 in group:
            for c in (c1, c2):
                if c not in have:
                    ctx.blocks_index(where[c], block_k, block_sample)
                    have.add(c)
            a, b = where[c1], where[c2]
            win_b, opp, votes, _total, n_anchors = ctx.blocks_pair(a, b, block_k, block_sample, bin_size)
            blocks = walk(win_b, opp, votes, lengths[a], lengths[b], bin_size, min_votes, max_gap, min_block)
            covered = sum(b_[1] - b_[0] for b_ in blocks)
            logger.info("blocks {} - {}: {} anchors, {} called windows, {} blocks, {} bp ({:.1%}) of {} covered".format(
                c1, c2, n_anchors, int((votes >= min_votes).sum()), len(blocks), covered, covered / max(1, lengths[a]), c1))
            res.append((c1, c2, blocks))
            tot_pairs, tot_blocks, tot_cov = tot_pairs + 1, tot_blocks + len(blocks), tot_cov + covered
        out.append(res)
        for c in [c for c in have if last_use.get(c, -1) <= gi]:
            ctx.blocks_release(where[c])
            have.discard(c)
    logger.info("blocks: {} pairs, {} blocks, {} bp covered".format(tot_pairs, tot_blocks, tot_cov))
    return out


def plot(outfig, groups, lengths_by_name, chrom_colors=None, inverted="#d62728", forward="#7f7f7f"):
    """One row per config line: its chromosomes as bars (in `chrom_colors[name]`, grey otherwise) stacked top to bottom
    in the order of their first appearance, the blocks as ribbons between NEIGHBOURING bars, inverted blocks in a second
    colour.  Raises ImportError without matplotlib (the caller warns)."""
    from matplotlib import pyplot as plt
    from matplotlib.patches import Polygon, Rectangle
    plt.switch_backend("agg")
    rows = [g for g in groups if g]
    n = max(1, len(rows))
    fig, axes = plt.subplots(n, 1, figsize=(10, 2.2 * n + 0.6), squeeze=False)
    for ax, group in zip(axes[:, 0], rows):
        order = []
        for c1, c2, _ in group:
            for c in (c1, c2):
                if c not in order:
                    order.append(c)
        y = {c: len(order) - 1 - i for i, c in enumerate(order)}
        longest = max(lengths_by_name[c] for c in order)
        for c in order:
            ax.add_patch(Rectangle((0, y[c] - 0.08), lengths_by_name[c], 0.16, color=(chrom_colors or {}).get(c, "#444444"), lw=0))
            ax.text(-0.01 * longest, y[c], c, ha="right", va="center", fontsize=8)
        for c1, c2, blocks in group:
            if abs(y[c1] - y[c2]) != 1:
                continue
            up, lo = (c1, c2) if y[c1] > y[c2] else (c2, c1)
            for s1, e1, s2, e2, strand, _, _ in blocks:
                (us, ue), (ls, le) = ((s1, e1), (s2, e2)) if up == c1 else ((s2, e2), (s1, e1))
                if strand == "-":
                    ls, le = le, ls
                ax.add_patch(Polygon([(us, y[up] - 0.08), (ue, y[up] - 0.08), (le, y[lo] + 0.08), (ls, y[lo] + 0.08)], closed=True,
                                     color=inverted if strand == "-" else forward, alpha=0.5, lw=0))
        ax.set_xlim(-0.08 * longest, 1.02 * longest)
        ax.set_ylim(-0.5, len(order) - 0.5)
        ax.set_yticks([])
        for side in ("left", "right", "top"):
            ax.spines[side].set_visible(False)
    fig.savefig(outfig, bbox_inches="tight", dpi=200)
    plt.close(fig)
