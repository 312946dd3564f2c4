"""The LTR-RT tree of the LTR stage (-ltr_tree): host side.

The reference builds its trees (LTR.LTRtree, __main__.py:622-638) from TEsorter's domain peptides with mafft, trimal and
iqtree or FastTree, roots them with nw_reroot and draws them with ggtree -- one tree per Copia / Gypsy.  None of these tools
and no HMM database is part of this build, so the tree here is a different object, defined by its own arithmetic
(csrc/sp_ltrtree.h): bottom-s MinHash sketches of the elements' canonical k-mers on the resident genome, the Mash distance
of every pair in fixed point, and neighbour joining on that integer matrix.  It is ONE tree over all subgenome-specific
elements (there is no classification), coloured by subgenome.  It is not a protein-domain tree, and it was never compared
with iqtree or FastTree.  Above roughly 25-30 % divergence at k = 13 two elements share no hash and the distance saturates:
unrelated families are joined in no meaningful order; only the clades of similar elements carry information.

The device answers three calls (Context.ltr_sketch, ltr_sketch_pairs, nj_tree); everything here is what lies between and
behind them: the distance units, the branch lengths of the join records, the midpoint rooting and the newick text, the
`.ltr.tree.map` and the figure."""
import math
import random

import numpy as np

TREE_K = 13              # provisional: judged on synthetic families only
TREE_SKETCH = 1024       # provisional, as above
SUBSAMPLE = 1000         # the reference's -subsample
MAX_LEN = 65536          # SP_LT_MAXLEN
MAX_N = 4096             # SP_LT_MAXN
MIN_SEQS = 4             # the reference's rule (nseq < 4: no tree)
UNIT = 1 << 30           # fixed-point units of one substitution per site


def mash_units(shared, denom, k, s):
    """The fixed-point Mash distance of (shared, denom) pairs, int64 of their shape:
        j = shared / denom, with shared = 0 counted as half a shared hash;  d = -ln(2 j / (1 + j)) / k;
        D = floor(d * 2^30 + 0.5);  denom = 0 (two empty sketches) gives the distance of shared = 0, denom = s.
    D < 2^31 for every allowed k and s: the smallest j is 0.5 / denom with denom <= s <= 4096, so 2 j / (1 + j) >= 2 / 8193,
    -ln of it is at most ln(4096.5) < 8.32, and with k >= 9 d < 0.925: D < 0.925 * 2^30 + 1 < 2^31.  j = 1 gives D = 0."""
    shared, denom = np.asarray(shared, np.int64), np.asarray(denom, np.int64)
    if not (9 <= int(k) <= 31 and 16 <= int(s) <= 4096):
        raise ValueError("mash_units: k = {} or s = {} outside 9..31 / 16..4096".format(k, s))
    if (shared < 0).any() or (shared > denom).any() or (denom > s).any():
        raise ValueError("mash_units: a pair with shared < 0, shared > denom or denom > s")
    out = np.empty(shared.shape, np.int64)
    for idx in np.ndindex(*shared.shape):
        sh, dn = int(shared[idx]), int(denom[idx])
        if dn == 0:
            sh, dn = 0, int(s)
        j = (sh if sh else 0.5) / dn
        out[idx] = int(math.floor(-math.log(2.0 * j / (1.0 + j)) / k * UNIT + 0.5))
    return out


def distance_matrix(shared, denom, k, s):
    """the N x N input of nj_tree: mash_units of every pair, the diagonal zero.  Only the distinct (shared, denom) pairs
    are evaluated."""
    shared, denom = np.asarray(shared, np.int64), np.asarray(denom, np.int64)
    code = shared * (int(s) + 1) + denom
    uniq, inv = np.unique(code, return_inverse=True)
    vals = mash_units(uniq // (int(s) + 1), uniq % (int(s) + 1), k, s)
    D = vals[inv].reshape(shared.shape)
    np.fill_diagonal(D, 0)
    return np.ascontiguousarray(D, np.int64)


def branch_lengths(records):
    """[(l_i, l_j)] in matrix units (fp64) of the N - 1 join records (i, j, D, R_i, R_j): with n live slots before the join,
    l_i = D / 2 + (R_i - R_j) / (2 (n - 2)) and l_j = D - l_i; the last record (n = 2) is one edge of length D, given as (D, 0)."""
    records = [tuple(int(x) for x in r) for r in np.asarray(records).tolist()]
    N, out = len(records) + 1, []
    for t, (_, _, d, ri, rj) in enumerate(records):
        n = N - t
        if n == 2:
            out.append((float(d), 0.0))
        else:
            li = d / 2.0 + (ri - rj) / (2.0 * (n - 2))
            out.append((li, d - li))
    return out


def unrooted_edges(records):
    """The unrooted tree of the records: [(u, v, length in matrix units)] -- leaves 0 .. N - 1, the node of join t is N + t;
    the last record joins the two nodes left by one edge.  Lengths are raw (they may be negative)."""
    recs = np.asarray(records).tolist()
    N = len(recs) + 1
    node = list(range(N))
    edges = []
    for t, ((i, j, *_), (li, lj)) in enumerate(zip(recs, branch_lengths(recs))):
        i, j = int(i), int(j)
        if t == N - 2:
            edges.append((node[i], node[j], li))
        else:
            edges += [(N + t, node[i], li), (N + t, node[j], lj)]
            node[i] = N + t
    return edges


def splits(edges, n_leaves):
    """{frozenset of the leaves on the side without leaf 0: length} over the edges of an unrooted tree; two edges with the
    same split (a node of degree 2) add up"""
    adj = {}
    for u, v, w in edges:
        adj.setdefault(u, []).append((v, w))
        adj.setdefault(v, []).append((u, w))
    out, below = {}, {}
    order, parent = [0], {0: (None, 0.0)}
    for u in order:                      # breadth first from leaf 0
        for v, w in adj.get(u, ()):
            if v not in parent:
                parent[v] = (u, w)
                order.append(v)
    for u in reversed(order):
        s = {u} if u < n_leaves else set()
        for v, _ in adj.get(u, ()):
            if parent.get(v, (None,))[0] == u:
                s |= below[v]
        below[u] = s
        if parent[u][0] is not None:
            key = frozenset(s)
            out[key] = out.get(key, 0.0) + parent[u][1]
    return out


def midpoint_root(edges, n_leaves):
    """Roots an unrooted tree (lengths >= 0) at the midpoint of its longest leaf-to-leaf path -- this build's own rule, not
    nw_reroot's: a = the leaf farthest from leaf 0, b = the leaf farthest from a (the lowest leaf on ties); the root lies
    half the path's length from a, as a new node on the edge that holds the point (walking from b: the first edge whose
    end nearer to a is not beyond the point; when that end is an inner node exactly at the point, it is the root).  Returns (root, children: {node: [(child, length)]}); children are ordered by their smallest leaf."""
    adj = {}
    for u, v, w in edges:
        adj.setdefault(u, []).append((v, w))
        adj.setdefault(v, []).append((u, w))

    def walk(src):
        dist, par, order = {src: 0.0}, {src: None}, [src]
        for u in order:
            for v, w in adj.get(u, ()):
                if v not in dist:
                    dist[v], par[v] = dist[u] + w, u
                    order.append(v)
        return dist, par

    def farthest(dist):
        best = None
        for leaf in range(n_leaves):
            if leaf in dist and (best is None or dist[leaf] > dist[best]):
                best = leaf
        return best
    a = farthest(walk(0)[0])
    dist, par = walk(a)
    b = farthest(dist)
    half, u = dist[b] / 2.0, b
    while par[u] is not None and dist[par[u]] > half:
        u = par[u]
    p = par[u]                           # the edge (p, u) holds the point: dist[p] <= half <= dist[u]
    if p is None:                        # a single leaf
        root, cut = u, None
    elif dist[p] == half and p >= n_leaves:
        root, cut = p, None              # on an inner node
    else:
        root = max(max(x, y) for x, y, _ in edges) + 1
        cut = (p, u, half - dist[p], dist[u] - half)
    if cut:
        p, u, wp, wu = cut
        adj[p] = [(v, w) for v, w in adj[p] if v != u]
        adj[u] = [(v, w) for v, w in adj[u] if v != p]
        adj[root] = [(p, wp), (u, wu)]
        adj[p].append((root, wp))
        adj[u].append((root, wu))
    children, low, order, parent = {}, {}, [root], {root: None}
    for x in order:
        for v, w in adj.get(x, ()):
            if v not in parent:
                parent[v] = x
                children.setdefault(x, []).append((v, w))
                order.append(v)
    for x in reversed(order):
        low[x] = min(([x] if x < n_leaves else []) + [low[v] for v, _ in children.get(x, ())])
    for x in children:
        children[x].sort(key=lambda c: low[c[0]])
    return root, children


def quote(label):
    """a newick label: as it is when it holds none of the format's characters, else in single quotes"""
    label = str(label)
    if label and not any(ch in label for ch in " \t()[]':;,"):
        return label
    return "'" + label.replace("'", "''") + "'"


def newick(root, children, labels, scale=1.0 / UNIT):
    """the newick text of a rooted tree; lengths times `scale`, written with 6 significant digits"""
    out, stack = [], [(root, None, 0)]
    # iterative: a caterpillar of 4096 leaves is deeper than Python's recursion limit
    while stack:
        node, w, state = stack.pop()
        kids = children.get(node, [])
        if state == 0 and kids:
            out.append("(")
            stack.append((node, w, 1))
            for q, (v, wv) in enumerate(reversed(kids)):
                if q:
                    stack.append((None, None, 2))
                stack.append((v, wv, 0))
            continue
        if state == 2:
            out.append(",")
            continue
        if state == 1:
            out.append(")")
        else:
            out.append(quote(labels[node]))
        if w is not None:
            out.append(":{:.6g}".format(w * scale))
    # the commas were pushed between the children in reverse: the pops give child, comma, child, ...
    return "".join(out) + ";"


def tree_text(records, labels):
    """newick of the midpoint-rooted tree of the join records; negative lengths are written as 0"""
    N = len(labels)
    if N == 1:
        return quote(labels[0]) + ";"
    edges = [(u, v, max(w, 0.0)) for u, v, w in unrooted_edges(records)]
    root, children = midpoint_root(edges, N)
    return newick(root, children, labels)


def choose(n_eligible, limit, seed):
    """indices of the elements that stay when more than `limit` are eligible: a seeded choice without replacement, in
    input order"""
    if n_eligible <= limit:
        return list(range(n_eligible))
    return sorted(random.Random(seed).sample(range(n_eligible), limit))


def build(ctx, chrom, start, end, k, s):
    """records int64 [N - 1, 5] of the tree over the elements, and the three timings (sketch, pairs, joins) in seconds"""
    import time
    t0 = time.perf_counter()
    sketch, length = ctx.ltr_sketch(chrom, start, end, k, s)
    t1 = time.perf_counter()
    shared, denom = ctx.ltr_sketch_pairs(sketch, length)
    t2 = time.perf_counter()
    D = distance_matrix(shared, denom, k, s)
    t3 = time.perf_counter()
    records = np.asarray(ctx.nj_tree(D), np.int64)
    return records, (t1 - t0, t2 - t1, time.perf_counter() - t3)


def write_map(fout, labels, sgs, clades=None):
    """`.ltr.tree.map`: the reference's columns label, Clade, Subgenome; Clade is `unknown` unless the elements were classified
    (-ltr_hmm: `clades`, one per label)"""
    fout.write("\t".join(["label", "Clade", "Subgenome"]) + "\n")
    for q, (lab, sg) in enumerate(zip(labels, sgs)):
        fout.write("\t".join([str(lab), "unknown" if clades is None else str(clades[q]), str(sg)]) + "\n")


def plot(path, records, sgs, sg_colors=None):
    """A circular cladogram (no branch lengths) of the midpoint-rooted tree, the branches coloured by subgenome: a branch
    whose leaves all belong to one subgenome takes its colour, the others are grey."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    N = len(sgs)
    edges = [(u, v, max(w, 0.0)) for u, v, w in unrooted_edges(records)]
    root, children = midpoint_root(edges, N)
    names = sorted(set(sgs))
    if not sg_colors:
        cyc = plt.rcParams["axes.prop_cycle"].by_key()["color"]
        sg_colors = {sg: cyc[i % len(cyc)] for i, sg in enumerate(names)}
    order, depth = [root], {root: 0}
    for x in order:
        for v, _ in children.get(x, ()):
            depth[v] = depth[x] + 1
            order.append(v)
    height, angle, kind, nleaf = {}, {}, {}, 0
    stack, leaves = [root], []
    while stack:                         # leaves in newick order
        x = stack.pop()
        if x < N:
            leaves.append(x)
        stack += [v for v, _ in reversed(children.get(x, []))]
    for q, x in enumerate(leaves):
        angle[x] = 2 * math.pi * q / max(len(leaves), 1)
    for x in reversed(order):
        kids = [v for v, _ in children.get(x, ())]
        if x < N:
            height[x], kind[x] = 0, sgs[x]
        else:
            height[x] = 1 + max(height[v] for v in kids)
            angle[x] = sum(angle[v] for v in kids) / len(kids)
            ks = {kind[v] for v in kids}
            kind[x] = ks.pop() if len(ks) == 1 else None
    top = max(height[root], 1)
    radius = {x: (top - height[x]) / top for x in order}
    fig = plt.figure(figsize=(8, 8))
    ax = fig.add_subplot(111, projection="polar")
    for x in order:
        for v, _ in children.get(x, ()):
            col = sg_colors.get(kind[v], "grey") if kind[v] is not None else "grey"
            arc = np.linspace(angle[x], angle[v], 16)
            ax.plot(arc, np.full(arc.shape, radius[x]), color=col, lw=0.6)
            ax.plot([angle[v], angle[v]], [radius[x], radius[v]], color=col, lw=0.6)
    for sg in names:
        ax.plot([], [], color=sg_colors.get(sg, "grey"), label=sg)
    ax.legend(loc="upper right", fontsize=8, frameon=False)
    ax.set_axis_off()
    fig.savefig(path, dpi=200, bbox_inches="tight")
    plt.close(fig)
