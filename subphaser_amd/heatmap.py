"""Host side of the clustered k-mer heatmap (Cluster.heatmap; the reference's Jellyfish.py:524-609 hands the same sample
to R's heatmap.2): the sample, the linkage form of the device's merges, leaf orders and dendrogram lines.  numpy only.

A linkage Z is scipy's: (n - 1) x 4 rows (id a < id b, height, leaves), ids below n are leaves, id n + i is the cluster
row i made, rows ascending in height.  Every walk over a tree here is iterative: 10 000 leaves in a chain-shaped tree
must not depend on the interpreter's recursion limit."""
import numpy as np


def sample_rows(M_good, size, seed):
    """`size` of M_good row numbers without replacement, ascending; all of them when M_good <= size"""
    if M_good <= size:
        return np.arange(M_good, dtype=np.int64)
    return np.sort(np.random.RandomState(seed).choice(M_good, size, replace=False)).astype(np.int64)


def to_linkage(merges, P):
    """The nearest-neighbour chain's merges ((P - 1) x 4: slot x, slot y, height, size; unsorted, raw slot ids, as
    Context.hclust_complete and csrc/sp_hclust.h define them) as scipy's linkage: a stable sort by height, then a
    union-find pass that replaces each slot by the cluster it belongs to by then, the lower id first.  Equals
    scipy.cluster.hierarchy.linkage(condensed, "complete") for the same distances."""
    merges = np.asarray(merges, np.float64).reshape(P - 1, 4)
    Z = merges[np.argsort(merges[:, 2], kind="stable")].copy()
    parent = np.arange(2 * P - 1, dtype=np.int64)
    size = np.ones(2 * P - 1, np.int64)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    for i in range(P - 1):
        a, b = find(int(Z[i, 0])), find(int(Z[i, 1]))
        if a > b:
            a, b = b, a
        new = P + i
        parent[a] = parent[b] = new
        size[new] = size[a] + size[b]
        Z[i, 0], Z[i, 1], Z[i, 3] = a, b, size[new]
    return Z


def _children(Z):
    return Z[:, 0].astype(np.int64).tolist(), Z[:, 1].astype(np.int64).tolist()


def _walk(left, right, n, first_is_left=None):
    """leaf order of the tree: at node i the left child first, or the right one where first_is_left[i] is False"""
    if n == 1:
        return np.zeros(1, np.int64)
    out, stack = [], [2 * n - 2]
    while stack:
        node = stack.pop()
        if node < n:
            out.append(node)
            continue
        i = node - n
        a, b = left[i], right[i]
        if first_is_left is not None and not first_is_left[i]:
            a, b = b, a
        stack.append(b)
        stack.append(a)
    return np.array(out, np.int64)


def leaves(Z):
    """leaf ids from left to right: scipy.cluster.hierarchy.leaves_list(Z)"""
    Z = np.asarray(Z, np.float64)
    left, right = _children(Z)
    return _walk(left, right, len(Z) + 1)


def reorder(Z, weights):
    """Leaf order after R's reorder(as.dendrogram(h), weights) (agglo.FUN = sum), which heatmap.2 applies with the row
    means: at every node the child with the smaller sum of leaf weights goes first, the left child on ties."""
    Z = np.asarray(Z, np.float64)
    n = len(Z) + 1
    left, right = _children(Z)
    w = np.zeros(2 * n - 1)
    w[:n] = np.asarray(weights, np.float64)
    first_is_left = [True] * (n - 1)
    for i in range(n - 1):          # children come before their parent in a linkage
        a, b = left[i], right[i]
        first_is_left[i] = bool(w[a] <= w[b])
        w[n + i] = w[a] + w[b]
    return _walk(left, right, n, first_is_left)


def dendrogram_segments(Z, order):
    """The dendrogram as line coordinates for a plot whose leaves sit at 0, 1, 2 ... in `order` (a leaf order of this
    tree: leaves() or reorder()): returns (xs, ys), each (n - 1) x 4 -- node i is the polyline
    (x_a, h_a) - (x_a, h_i) - (x_b, h_i) - (x_b, h_b) over its children a and b; leaves have height 0."""
    Z = np.asarray(Z, np.float64)
    n = len(Z) + 1
    left, right = _children(Z)
    pos, height = np.zeros(2 * n - 1), np.zeros(2 * n - 1)
    pos[np.asarray(order, np.int64)] = np.arange(n)
    xs, ys = np.empty((n - 1, 4)), np.empty((n - 1, 4))
    for i in range(n - 1):
        a, b, h = left[i], right[i], Z[i, 2]
        xs[i] = (pos[a], pos[a], pos[b], pos[b])
        ys[i] = (height[a], h, h, height[b])
        pos[n + i], height[n + i] = 0.5 * (pos[a] + pos[b]), h
    return xs, ys


def zscale_columns(x):
    """the R script's z.scale over the chromosomes of every k-mer: x is N x C (k-mer rows); returns C x N,
    z[c, j] = (x[j, c] - mean_j) / sqrt(var_j), the sample variance (ddof = 1)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    sd = np.sqrt(x.var(axis=1, ddof=1, keepdims=True))
    return np.ascontiguousarray(((x - mean) / sd).T)


def color_levels(colors, n=100):
    """n RGB levels interpolated through 2 or 3 colours (the R script's colorpanel); any other count is an error"""
    from matplotlib.colors import to_rgb
    if isinstance(colors, str):
        colors = colors.split(",")
    check_colors(colors)
    rgb = np.array([to_rgb(c) for c in colors])
    at = np.linspace(0.0, 1.0, len(rgb))
    t = np.linspace(0.0, 1.0, n)
    return np.stack([np.interp(t, at, rgb[:, j]) for j in range(3)], axis=1)


def check_colors(colors):
    if isinstance(colors, str):
        colors = colors.split(",")
    if len(colors) not in (2, 3):
        raise ValueError("heatmap_colors must be 2 or 3 colours (low, [mid,] high), got {}: {}".format(len(colors), list(colors)))
    return list(colors)


def plot(outfig, z, row_Z, col_Z, chrom_order, kmer_order, chrs, chrom_colors, kmer_colors, heatmap_colors):
    """The figure: the k-mer dendrogram on top, the chromosome dendrogram on the left, side strips of subgenome colours,
    the image of z (chromosome rows, each scaled to mean 0 and sd 1 as heatmap.2's scale="row" does) in 100 colour
    levels, chromosome labels, a colour key.  Returns False when matplotlib is missing."""
    try:
        from matplotlib import pyplot as plt
        from matplotlib.colors import ListedColormap, to_rgb
    except ImportError:
        return False
    plt.switch_backend("agg")
    C, N = z.shape
    img = z[np.ix_(chrom_order, kmer_order)]
    with np.errstate(all="ignore"):
        sd = img.std(axis=1, ddof=1, keepdims=True)
        img = (img - img.mean(axis=1, keepdims=True)) / np.where(sd > 0, sd, 1.0)
    lim = float(np.nanmax(np.abs(img))) if img.size else 1.0
    lim = lim if np.isfinite(lim) and lim > 0 else 1.0
    cmap = ListedColormap(color_levels(heatmap_colors, 100))
    fig = plt.figure(figsize=(10, 8), dpi=300)
    gs = fig.add_gridspec(3, 3, width_ratios=[1.2, 0.15, 8], height_ratios=[1.5, 0.15, 8], wspace=0.01, hspace=0.01,
                          left=0.03, right=0.88, top=0.97, bottom=0.03)
    ax = fig.add_subplot(gs[2, 2])
    im = ax.imshow(img, aspect="auto", interpolation="nearest", cmap=cmap, vmin=-lim, vmax=lim,
                   extent=(-0.5, N - 0.5, C - 0.5, -0.5))
    ax.set_xticks([])
    ax.yaxis.tick_right()
    ax.set_yticks(np.arange(C))
    base = plt.rcParams["font.size"]
    ax.set_yticklabels([chrs[i] for i in chrom_order], fontsize=base * min(1.5, 30.0 / C))
    top = fig.add_subplot(gs[0, 2], sharex=ax)
    xs, ys = dendrogram_segments(col_Z, kmer_order)
    if N <= 2000:
        top.plot(xs.T, ys.T, color="black", lw=0.5)
    else:       # thousands of four-point lines as ONE collection
        from matplotlib.collections import LineCollection
        top.add_collection(LineCollection(np.stack([xs, ys], axis=2), colors="black", linewidths=0.3))
        top.set_ylim(0, float(ys.max()) * 1.02 if ys.size and ys.max() > 0 else 1.0)
    top.set_xlim(-0.5, N - 0.5)
    top.axis("off")
    lft = fig.add_subplot(gs[2, 0], sharey=ax)
    xs, ys = dendrogram_segments(row_Z, chrom_order)
    lft.plot(ys.T, xs.T, color="black", lw=0.5)
    lft.set_xlim(float(ys.max()) * 1.02 if ys.size and ys.max() > 0 else 1.0, 0)
    lft.set_ylim(C - 0.5, -0.5)
    lft.axis("off")
    strip_c = fig.add_subplot(gs[2, 1], sharey=ax)
    strip_c.imshow(np.array([to_rgb(chrom_colors[i]) for i in chrom_order])[:, None, :], aspect="auto",
                   interpolation="nearest", extent=(0, 1, C - 0.5, -0.5))
    strip_c.axis("off")
    strip_k = fig.add_subplot(gs[1, 2], sharex=ax)
    strip_k.imshow(np.array([to_rgb(kmer_colors[j]) for j in kmer_order])[None, :, :], aspect="auto",
                   interpolation="nearest", extent=(-0.5, N - 0.5, 1, 0))
    strip_k.axis("off")
    key = fig.add_axes([0.03, 0.86, 0.09, 0.03])
    fig.colorbar(im, cax=key, orientation="horizontal")
    key.set_title("Row Z-score", fontsize=base * 0.7)
    key.tick_params(labelsize=base * 0.6)
    fig.savefig(outfig, dpi=300)
    plt.close(fig)
    return True
