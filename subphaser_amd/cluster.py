"""Chromosome -> subgenome assignment and subgenome-specific k-mer test ("next" row f-1).

The reference's Cluster.py is the unchanged CONSUMER of the `.kmer.mat` matrix
(BASELINE.json north_star).  This module only re-states the part that
produces the input of the second half of the hot path:
  Cluster.__init__/fit/sort_subgenomes/assign_subgenomes (Cluster.py:17-47, 114-143)
  Cluster.output_kmers / _output_kmers                    (Cluster.py:151-194)
so that an end-to-end run is self-contained.  KMeans is delegated to
scikit-learn exactly like the reference; the bootstrap's k-means fits can also
run on the device (bootstrap_engine="device": csrc/sp_kboot.hip).  The k-mer PCA
(Cluster.pca, Cluster.py:48-75: `.kmer_pca` coordinates and figure) is scikit-learn's
full-solver PCA restated on the C x C Gram matrix of the Z-scores: the passes over the
k-mers run on the device from the integer rows (csrc/sp_kpca.hip) or in numpy, the
eigen-decomposition on the host.  The clustered heatmap (Cluster.heatmap, Jellyfish.py:524-609) takes its two
complete-linkage dendrograms from the device (csrc/sp_hclust.hip) or from scipy and draws the figure with matplotlib
(subphaser_amd/heatmap.py).  The per-k-mer Student t-test is vectorised over the
M x C matrix instead of looped through a process pool.
"""
import os
import sys
from collections import OrderedDict

import numpy as np

from . import _native
from . import kmer as kmerlib
from .runtime import logger
from .seqs import KmerLabels
from ._native import write_chunks


def load_matrix(datafile):
    """`.kmer.mat` reader with the contract of the reference's Data.py:6-21."""
    colnames, rownames, data = [], [], []
    with open(datafile) as fh:
        for i, line in enumerate(fh):
            t = line.strip().split()
            if i == 0:
                colnames = t[1:]
                continue
            rownames.append(t[0])
            data.append(list(map(float, t[1:])))
    return colnames, rownames, np.array(data, np.float64).reshape(len(rownames), len(colnames))


def relabel_by_chromosome_order(chrs, raw_labels):
    """Cluster ids renumbered 0, 1, 2 ... in the order in which they first occur when the chromosomes are
    walked in sorted-name order (what the reference's sort_subgenomes produces, Cluster.py:119-127), as
    array operations: the first position of every id in the name-sorted label vector ranks the ids."""
    raw = np.asarray(raw_labels)
    if raw.size != len(chrs):
        raise ValueError("{} labels for {} chromosomes".format(raw.size, len(chrs)))
    by_name = np.argsort(np.asarray(chrs, dtype=object), kind="stable")
    ids, first, inverse = np.unique(raw[by_name], return_index=True, return_inverse=True)
    rank_of_id = np.empty(ids.size, np.int64)
    rank_of_id[np.argsort(first, kind="stable")] = np.arange(ids.size)
    out = np.empty(raw.size, np.int64)
    out[by_name] = rank_of_id[inverse]
    return out


class Cluster:
    """Chromosome -> subgenome assignment (k-means on the Z-normalised matrix, or the `-sg_assigned` table),
    bootstrap support and the subgenome-specific k-mer test."""

    def __init__(self, data, n_clusters, sg_prefix="SG", sg_assigned={}, re_assign=True, bootstrap=False,
                 replicates=1000, jackknife=80, seed=None, bootstrap_engine="sklearn", **kargs):
        """data: path of a `.kmer.mat` file or a FilteredMatrix (jellyfish.filter result).
        bootstrap_engine: "sklearn" (the loop of scikit-learn fits) or "device" (Context.kmeans_bootstrap: up to
        KBOOT_MAX_POINTS chromosomes in KBOOT_MAX_CLUSTERS clusters, the scikit-learn loop beyond)."""
        if bootstrap_engine not in BOOTSTRAP_ENGINES:
            raise ValueError("bootstrap_engine must be one of {}".format(BOOTSTRAP_ENGINES))
        self.bootstrap_engine = bootstrap_engine
        if isinstance(data, str):
            self.chrs, kmers, self.raw_data = load_matrix(data)
            self.k = len(kmers[0]) if kmers else 0
            self.keys = kmerlib.encode_many(kmers)
        else:
            self.chrs, self.raw_data, self.keys, self.k = list(data.labels), data.freqs, data.keys, data.k
            # the integer matrix behind the frequencies: lets the k-mer test run on the device (sp_kmer_ttest)
            self._counts, self._lengths = getattr(data, "counts", None), getattr(data, "lengths", None)
            self._ctx = getattr(data, "ctx", None)
            self._counts_dev = getattr(data, "counts_dev", None)
        self.sg_prefix, self.seed = sg_prefix, seed
        self.n_clusters = len(set(sg_assigned.values())) if sg_assigned else n_clusters
        if sg_assigned:
            logger.info("Skip k-means clustering")
            given = [sg_assigned[c] for c in self.chrs]
            if re_assign:
                self._name(relabel_by_chromosome_order(self.chrs, given))
            else:
                self.d_sg, self.sg_names = sg_assigned, sorted(set(sg_assigned.values()))
                self.labels = relabel_by_chromosome_order(self.chrs, given)
        else:
            self._name(relabel_by_chromosome_order(self.chrs, self._kmeans(self.zscores()).labels_))
        self.d_bs = self.bootstrap(replicates, jackknife) if bootstrap and replicates and replicates > 0 \
            else {c: "NA" for c in self.chrs}

    # chromosomes x k-mers, every k-mer column Z-normalised (Cluster.py:24-26, 78-82)
    def zscores(self, freqs=None):
        x = (self.raw_data if freqs is None else freqs).T
        with np.errstate(all="ignore"):
            return (x - x.mean(axis=0)) / x.std(axis=0)

    normalize_data = staticmethod(lambda data, axis=0: (data - data.mean(axis=axis)) / data.std(axis=axis))

    def _kmeans(self, points):
        from sklearn.cluster import KMeans
        return KMeans(n_clusters=self.n_clusters, random_state=self.seed).fit(points)

    def _name(self, labels):
        width = len(str(self.n_clusters))
        self.labels = np.asarray(labels, np.int64)
        names = ["{}{:0>{}d}".format(self.sg_prefix, int(l) + 1, width) for l in self.labels]
        self.d_sg = OrderedDict(zip(self.chrs, names))
        self.sg_names = sorted(set(names))

    def bootstrap(self, replicates=1000, jackknife=80):
        """Support of every chromosome's assignment: share of `replicates` k-means runs, each on `replicates`
        k-mers drawn with replacement (the reference resamples n_samples=replicates and ignores the jackknife
        size it computes, Cluster.py:85-90), that give the chromosome the same renumbered cluster id."""
        logger.info("Performing bootstrap of {} replicates, with each replicate resampling {}% data "
                    "with replacement".format(replicates, jackknife))
        z = self.zscores()                                   # C x M
        rng = np.random.RandomState(self.seed)
        M = z.shape[1]
        R = int(replicates)
        entry = self._device_bootstrap(z) if self.bootstrap_engine == "device" else None
        if entry is not None:
            # the columns exactly as the loop below draws them: a given seed resamples the same k-mers under both engines
            cols = np.array([rng.randint(0, M, size=R) for _ in range(R)], np.int64).reshape(R, R)
            seed = self.seed if self.seed is not None else int.from_bytes(os.urandom(8), "little")
            raw, _ = entry(z, cols, self.n_clusters, seed)
            reps = np.array([relabel_by_chromosome_order(self.chrs, r) for r in raw], np.int64).reshape(R, len(self.chrs))
        else:
            reps = np.empty((R, len(self.chrs)), np.int64)
            for i in range(R):
                cols = rng.randint(0, M, size=R)
                reps[i] = relabel_by_chromosome_order(self.chrs, self._kmeans(z[:, cols]).labels_)
        self.bootstrap_labels = reps                         # R x C, renumbered by chromosome order
        agree = (reps == self.labels[None, :]).sum(axis=0)
        self._bootstrap_scores(reps)
        return {c: int(100 * a / replicates) for c, a in zip(self.chrs, agree.tolist())}

    def _device_bootstrap(self, z):
        """Context.kmeans_bootstrap when the device engine applies, else None (one log line says why)"""
        entry = getattr(getattr(self, "_ctx", None), "kmeans_bootstrap", None)
        C, K = z.shape[0], self.n_clusters
        if entry is None:
            why = "no device context with the k-means bootstrap"
        elif C > _native.KBOOT_MAX_POINTS or K > _native.KBOOT_MAX_CLUSTERS:
            why = "{} chromosomes in {} clusters (the device engine takes up to {} in {})".format(
                C, K, _native.KBOOT_MAX_POINTS, _native.KBOOT_MAX_CLUSTERS)
        elif K > C:
            why = "{} clusters for {} chromosomes".format(K, C)
        else:
            if not np.isfinite(z).all():
                raise ValueError("Input contains NaN or infinity: the Z-normalised matrix of the bootstrap")
            return entry
        logger.info("bootstrap_engine=device: {}; using scikit-learn".format(why))
        return None

    def _bootstrap_scores(self, reps):
        """the reference's log line (Cluster.py:108-111): every replicate's labels against the assignment"""
        from sklearn import metrics
        truth = self.labels
        # most replicates repeat a few label vectors: one pair of scores per distinct vector, weighted by its count
        # (a millisecond per score otherwise: as long as the fits themselves at 1000 replicates)
        uniq, counts = np.unique(reps, axis=0, return_counts=True)
        w = counts / float(len(reps))
        self.mean_adjusted_rand_score = float(np.dot(w, [metrics.adjusted_rand_score(truth, r) for r in uniq]))
        self.mean_v_measure_score = float(np.dot(w, [metrics.v_measure_score(truth, r) for r in uniq]))
        logger.info("Bootstrap: mean Adjusted Rand-Index: {:.4f}; mean V-measure score: {:.4f}".format(
            self.mean_adjusted_rand_score, self.mean_v_measure_score))

    def pca(self, outfig=None, outtsv=None, n_components=2, colors=None, defer=False):
        """The reference's k-mer PCA (Cluster.py:48-75) with the arithmetic of PCA(svd_solver="full"): the Gram matrix
        G = Z Z^T of the C x M Z-scores, eigh(G) with the eigenvalues descending, scores U sqrt(w), every component
        given the sign of its largest-|v| k-mer (v = u^T Z: scikit-learn's svd_flip), percent = 100 w / sum(w), then the
        per-component Z-normalisation of the scores.  n = min(max(2, n_components), C) components are kept.
        The two passes over the k-mers run on the device when the matrix came with a context that has the entries, the
        integer counts and lengths, and C <= KPCA_MAX_CHROM (staged rows are read in place); in numpy on zscores()
        otherwise (one log line says which).  A k-mer whose Z-scores are not finite raises ValueError, as scikit-learn
        would.  Keeps pca_scores [C, n], pca_percent [n] and pca_engine ("device" / "numpy").
        outtsv: `#PC1=..%` line, header, one row per chromosome in matrix order, floats written with repr.
        outfig: the reference's scatter (one colour per subgenome; `colors`: a list or a comma-separated string of
        colours, matplotlib's cycle otherwise); skipped with a warning when matplotlib is missing.
        defer=True: the figure is not drawn; returns write() that draws it later (the CLI's main-thread writer queue)."""
        C = len(self.chrs)
        ctx = getattr(self, "_ctx", None)
        gram_entry, sign_entry = getattr(ctx, "kmer_pca_gram", None), getattr(ctx, "kmer_pca_signs", None)
        counts, lengths = getattr(self, "_counts", None), getattr(self, "_lengths", None)
        if gram_entry is None or sign_entry is None:
            why = "no device context with the k-mer PCA"
        elif counts is None or lengths is None:
            why = "no integer counts behind the matrix"
        elif C > _native.KPCA_MAX_CHROM:
            why = "{} chromosomes (the device takes up to {})".format(C, _native.KPCA_MAX_CHROM)
        else:
            why = None
        n = min(max(2, int(n_components)), C)
        if why is None:
            rows = getattr(self, "_counts_dev", None) or counts
            logger.info("k-mer PCA: {} k-mers x {} chromosomes on the device{}".format(
                len(self.raw_data), C, " (staged rows)" if rows is not counts else ""))
            G, n_bad = gram_entry(rows, lengths)
            sign_vals = lambda U: sign_entry(rows, lengths, U)[1]
            self.pca_engine = "device"
        else:
            logger.info("k-mer PCA: {}; using numpy".format(why))
            z = self.zscores()
            n_bad = int((~np.isfinite(z)).any(axis=0).sum())
            G = z @ z.T if not n_bad else None
            def sign_vals(U):
                v = U.T @ z
                return v[np.arange(v.shape[0]), np.argmax(np.abs(v), axis=1)]
            self.pca_engine = "numpy"
        if n_bad:
            raise ValueError("Input contains NaN or infinity: {} k-mers of the PCA have no finite Z-score "
                             "(the same frequency on every chromosome)".format(n_bad))
        w, V = np.linalg.eigh(G)
        w, V = w[::-1], V[:, ::-1]
        U = np.ascontiguousarray(V[:, :n])
        sign = np.where(np.asarray(sign_vals(U)) < 0, -1.0, 1.0)
        scores = U * np.sqrt(np.maximum(w[:n], 0.0)) * sign
        self.pca_percent = 100 * w[:n] / w.sum()
        with np.errstate(all="ignore"):
            self.pca_scores = self.normalize_data(scores, axis=0)
        if outtsv is not None:
            with open(outtsv, "w") as fout:
                fout.write("#" + "\t".join("PC{}={}%".format(j + 1, repr(float(p))) for j, p in enumerate(self.pca_percent)) + "\n")
                fout.write("\t".join(["#chrom", "subgenome"] + ["PC{}".format(j + 1) for j in range(n)]) + "\n")
                for c, row in zip(self.chrs, self.pca_scores.tolist()):
                    fout.write("\t".join([c, self.d_sg[c]] + [repr(v) for v in row]) + "\n")
        scores, percent = self.pca_scores, self.pca_percent
        chrs, d_sg, labels = list(self.chrs), dict(self.d_sg), self.labels.tolist()

        def write():
            if outfig is not None:
                plot_pca(outfig, scores, percent, chrs, d_sg, labels, colors)
        if defer:
            return write
        write()

    def heatmap(self, kmer_labels, outfig=None, outtsv=None, size=10000, colors=None,
                heatmap_colors=("green", "black", "red"), defer=False):
        """The reference's clustered heatmap of the matrix (Jellyfish.py:524-609, drawn there by R's heatmap.2): `size`
        k-mers sampled without replacement with the seed of the run, each Z-scaled over the chromosomes with the sample
        variance (the R script's z.scale: ddof = 1, not zscores()), complete-linkage dendrograms under the Euclidean
        distance over the k-mers (N points x C) and over the chromosomes (C points x N).  k-mers whose variance is 0 or not
        finite are left out of the pool before sampling (R fails on them; one log line counts them).
        The two linkages come from Context.hclust_complete (csrc/sp_hclust.hip) when the matrix came with a context that
        has it and both point counts are within HCLUST_MAX_POINTS, from scipy's pdist + linkage otherwise (one log line
        says which; heatmap_engine is "device" or "scipy").  Both follow the same procedure, so they agree whenever the
        distances hold no ties that rounding separates.
        Chromosomes are ordered as heatmap.2 orders them: reorder() by the chromosome's mean Z over the sample.  The
        k-mers keep the linkage's own leaf order: every k-mer's mean Z is 0 by construction, so R's reordering of that
        axis sorts rounding noise, and it is not imitated.
        Keeps heatmap_rows (the sampled rows of the matrix, ascending), heatmap_z [C, N], heatmap_row_linkage
        (chromosomes), heatmap_col_linkage (k-mers), heatmap_chrom_order and heatmap_kmer_order.  Fewer than 2 chromosomes
        or usable k-mers: one log line, heatmap_engine None, nothing written.
        kmer_labels: output_kmers' KmerLabels (or None): the subgenome a sampled k-mer is significant for, `NA` without.
        outtsv: `#kmer<TAB>subgenome<TAB>chromosomes in dendrogram order`, then the sampled k-mers in dendrogram order with
        their Z-scores written with repr.  outfig: dendrograms, side strips of subgenome colours (`colors`, or
        matplotlib's cycle; white for NA), the image scaled per chromosome row in 100 levels through the 2 or 3
        heatmap_colors (any other count: ValueError), a colour key; skipped with a warning when matplotlib is missing.
        defer=True: the figure is not drawn; returns write() that draws it later."""
        from . import heatmap as hm
        heatmap_colors = hm.check_colors(heatmap_colors)
        X = self.raw_data
        M, C = X.shape
        self.heatmap_engine = None
        with np.errstate(all="ignore"):
            var = X.var(axis=1, ddof=1) if C > 1 else np.zeros(M)
        good = np.flatnonzero(np.isfinite(var) & (var > 0))
        logger.info("heatmap: {} of {} k-mers left out of the sample pool (the same frequency on every chromosome, "
                    "or not finite)".format(M - good.size, M))
        if C < 2 or good.size < 2:
            logger.info("heatmap skipped: {} chromosomes, {} usable k-mers (2 of each at least)".format(C, good.size))
            return None
        rows = good[hm.sample_rows(good.size, int(size), self.seed)]
        z = hm.zscale_columns(X[rows])                       # C x N
        N = len(rows)
        entry = getattr(getattr(self, "_ctx", None), "hclust_complete", None)
        if entry is None:
            why = "no device context with the clustering entry"
        elif max(N, C) > _native.HCLUST_MAX_POINTS:
            why = "{} k-mers x {} chromosomes (the device takes up to {} points)".format(N, C, _native.HCLUST_MAX_POINTS)
        else:
            why = None
        if why is None:
            logger.info("heatmap: complete linkage of {} k-mers and of {} chromosomes on the device".format(N, C))
            link = lambda pts: hm.to_linkage(entry(pts), len(pts))
            self.heatmap_engine = "device"
        else:
            logger.info("heatmap: {}; using scipy".format(why))
            from scipy.cluster.hierarchy import linkage
            from scipy.spatial.distance import pdist
            link = lambda pts: linkage(pdist(pts), "complete")
            self.heatmap_engine = "scipy"
        try:
            col_Z = link(np.ascontiguousarray(z.T))
            row_Z = link(z)
        except BaseException:
            self.heatmap_engine = None
            raise
        chrom_order = hm.reorder(row_Z, z.mean(axis=1))
        kmer_order = hm.leaves(col_Z)
        self.heatmap_rows, self.heatmap_z = rows, z
        self.heatmap_row_linkage, self.heatmap_col_linkage = row_Z, col_Z
        self.heatmap_chrom_order, self.heatmap_kmer_order = chrom_order, kmer_order
        # the subgenome every sampled k-mer is significant for: -1 = none
        sg = np.full(N, -1, np.int64)
        sg_names = list(getattr(kmer_labels, "sg_names", []))
        if kmer_labels is not None and len(kmer_labels.keys):
            lk = np.asarray(kmer_labels.keys)
            by_key = np.argsort(lk, kind="stable")
            canon = kmerlib.canonical(self.keys[rows], self.k)
            at = np.minimum(np.searchsorted(lk[by_key], canon), len(lk) - 1)
            hit = lk[by_key][at] == canon
            sg[hit] = np.asarray(kmer_labels.sg_idx)[by_key][at][hit]
        self.heatmap_kmer_sg = [sg_names[i] if i >= 0 else "NA" for i in sg.tolist()]
        chrs, kmer_sg = list(self.chrs), self.heatmap_kmer_sg
        if outtsv is not None:
            kmers = kmerlib.decode_many(self.keys[rows], self.k)
            zt = z[chrom_order].T.tolist()                   # N x C, chromosomes in dendrogram order
            with open(outtsv, "w") as fout:
                fout.write("\t".join(["#kmer", "subgenome"] + [chrs[i] for i in chrom_order.tolist()]) + "\n")
                for j in kmer_order.tolist():
                    fout.write("\t".join([kmers[j], kmer_sg[j]] + [repr(v) for v in zt[j]]) + "\n")
        all_sg = sorted(set(self.d_sg.values()) | set(sg_names))
        chrom_sg = [all_sg.index(self.d_sg[c]) for c in chrs]
        kmer_sgi = [all_sg.index(s) if s != "NA" else -1 for s in kmer_sg]

        def write():
            if outfig is None:
                return
            try:
                from matplotlib import pyplot as plt
            except ImportError:
                logger.warning("matplotlib missing: skipping " + outfig)
                return
            pal = colors.split(",") if isinstance(colors, str) else colors
            if not pal:
                pal = plt.rcParams["axes.prop_cycle"].by_key()["color"]
            hm.plot(outfig, z, row_Z, col_Z, chrom_order, kmer_order, chrs, [pal[i % len(pal)] for i in chrom_sg],
                    [pal[i % len(pal)] if i >= 0 else "white" for i in kmer_sgi], heatmap_colors)
        if defer:
            return write
        write()

    def output_subgenomes(self, fout=sys.stdout):
        fout.write("#chrom\tsubgenome\tbootstrap\n")
        for c in sorted(self.d_sg, key=lambda x: self.d_sg[x]):      # stable: by subgenome, input order inside
            fout.write("{}\t{}\t{}\n".format(c, self.d_sg[c], self.d_bs[c]))

    def output_kmers(self, fout=sys.stdout, max_pval=0.05, ncpu=4, method="map", test_method="ttest_ind", defer=False):
        """Student t-test (pooled variance, two-sided; or the `test_method` given) between the highest-mean and the
        second-highest-mean subgenome groups of every k-mer; keeps p <= max_pval.
        Returns KmerLabels (array form of the reference's d_ksg dict).
        defer=True: nothing is written; returns (KmerLabels, write) where write(fout) produces the same text later
        (the CLI runs it on a writer thread while the mapping stage uses the labels)."""
        if test_method not in TEST_METHODS:
            raise ValueError("test_method must be one of {}".format(TEST_METHODS))
        sgs = sorted(set(self.d_sg.values()))
        groups = [[i for i, c in enumerate(self.chrs) if self.d_sg[c] == sg] for sg in sgs]
        X = self.raw_data
        M = X.shape[0]
        ctx = getattr(self, "_ctx", None)
        staged = getattr(self, "_counts_dev", None)      # rows already on the device (the CLI stages them early)
        call, why = self._device_kmer_test(ctx, M, groups, test_method)
        if why:
            logger.info("k-mer test ({}) on the host: {}".format(test_method, why))
        if call is None:
            self._release_staged(ctx, staged)           # the numpy code reads the host matrix
            top, second, pvals, means = numpy_kmer_test(X, groups, test_method)
        else:
            # device path: a thread per k-mer; the numpy code is the same test for matrices that only exist as a
            # `.kmer.mat` file or behind a context without the kernel
            try:
                top, second, pvals, means = call(staged if staged else self._counts, self._lengths, groups)[:4]
            finally:
                self._release_staged(ctx, staged)       # M x C x 4 bytes of HBM nobody reads again
        return self._write_kmers(fout, sgs, top, pvals, means, max_pval, defer)

    def _device_kmer_test(self, ctx, M, groups, test_method):
        """(call, None) when a device engine of KMER_ENGINES applies -- call(rows, lengths, groups) returns (top, second,
        pvals, means[, stat]) -- else (None, why): the reason for the log, None where the method stays silent"""
        engines = KMER_ENGINES[test_method]
        have = [e for e in engines if getattr(ctx, e[0], None) is not None]
        if not have:
            says = engines[0][3]
            return None, says if isinstance(says, str) else None
        fits = [e for e in have if e[2](groups) is None]
        # the first the context has whose sizes fit; else the widest it has, whose size rule is the reason
        attr, extra, size_rule, says = fits[0] if fits else have[-1]
        entry = getattr(ctx, attr)
        if getattr(self, "_counts", None) is None or self._lengths is None:
            why = "the matrix has no integer counts and lengths"
        elif not M:
            why = "no k-mers"
        else:
            why = size_rule(groups)
        if why is None:
            return (lambda rows, lengths, groups: entry(rows, lengths, groups, *extra)), None
        return None, why if says else None

    def _release_staged(self, ctx, staged):
        if staged and hasattr(ctx, "release_rows"):
            ctx.release_rows()
            self._counts_dev = None

    def _write_kmers(self, fout, sgs, top, pvals, means, max_pval, defer=False):
        with np.errstate(invalid="ignore"):
            keep = np.flatnonzero(~(pvals > max_pval))      # `if pvalue > max_pval: continue` keeps NaN
        kkeys, ktop, kp, kmeans, k = self.keys[keep], top[keep], pvals[keep], means[keep], self.k

        def fmt(lo, hi):
            kmers = kmerlib.decode_many(kkeys[lo:hi], k)
            return "".join("\t".join([km, sgs[t], repr(p), ",".join(map(repr, mv))]) + "\n"
                           for km, t, p, mv in zip(kmers, ktop[lo:hi].tolist(), kp[lo:hi].tolist(), kmeans[lo:hi].tolist()))
        def write(fout):
            print("\t".join(["#kmer", "subgenome", "p_value", "ratios"]), file=fout)
            fout.flush() if hasattr(fout, "flush") else None
            if len(kkeys) and _native.text_sig_kmers(fout, kkeys, k, ktop, sgs, kp, kmeans):
                return      # formatted by threads of this process (write_chunks below serves non-file objects, in this process)
            write_chunks(fout, len(kkeys), fmt)

        canon = kmerlib.canonical(self.keys[keep], self.k)
        labels = KmerLabels(canon, top[keep].astype(np.uint8), sgs, self.k)
        if defer:
            return labels, write
        write(fout)
        return labels


def plot_pca(outfig, scores, percent, chrs, d_sg, labels, colors=None):
    """Same figure as Cluster.py:56-75 (visualisation; optional)."""
    try:
        from matplotlib import pyplot as plt
    except ImportError:
        logger.warning("matplotlib missing: skipping " + outfig)
        return
    plt.switch_backend("agg")
    if isinstance(colors, str):
        colors = colors.split(",")
    if not colors:
        colors = plt.rcParams["axes.prop_cycle"].by_key()["color"]
    d_coord = {}
    for x, y, c, l in zip(scores[:, 0].tolist(), scores[:, 1].tolist(), chrs, labels):
        xs, ys, _ = d_coord.setdefault(d_sg[c], ([], [], colors[int(l) % len(colors)]))
        xs.append(x)
        ys.append(y)
    fig = plt.figure(figsize=(7, 7), dpi=300, tight_layout=True)
    for sg, (xs, ys, col) in sorted(d_coord.items()):
        plt.scatter(xs, ys, c=col, marker="o", label=sg)
    plt.axhline(0, ls="--", c="grey")
    plt.axvline(0, ls="--", c="grey")
    plt.xlabel("PC1 ({:.1f}%)".format(percent[0]), fontsize=18)
    plt.ylabel("PC2 ({:.1f}%)".format(percent[1]), fontsize=18, ha="center", va="center")
    plt.legend(fontsize=18)
    plt.tick_params(labelsize=15)
    plt.savefig(outfig, bbox_inches="tight", dpi=300)
    plt.close(fig)


TEST_METHODS = ("ttest_ind", "kruskal", "wilcoxon", "mannwhitneyu")
BOOTSTRAP_ENGINES = ("sklearn", "device")
TTEST_MAX_GROUP = 64     # SP_TT_MAXG in csrc/sp_enrich.hip
TTEST_WIDE_MAX_GROUP = 65536     # SP_TT_WIDE_MAX in csrc/sp_ttest.h


def _groups_upto(limit):
    def rule(groups):
        biggest = max(len(g) for g in groups)
        if biggest > limit():
            return "a subgenome of {} chromosomes (the device engine takes up to {})".format(biggest, limit())
    return rule


def _wilcoxon_sizes(groups):
    sizes = sorted({len(g) for g in groups})
    if len(sizes) > 1:
        return "subgenomes of {} chromosomes (the paired test needs one size)".format(", ".join(map(str, sizes)))
    if sizes[0] < 2 or sizes[0] > _native.WILCOXON_MAX_GROUP:
        return "subgenomes of {} chromosomes (the device engine takes 2 to {})".format(sizes[0], _native.WILCOXON_MAX_GROUP)


# test_method -> its device engines, the first the context has whose size rule passes is taken: (Context attribute,
# arguments behind the group lists, size rule: groups -> None or why not, what the log says -- a string: every reason,
# this one for a context without the entry; True: every reason but that one; False: nothing).  When no size rule
# passes, the last engine the context has gives the reason.
#   ttest_ind     k7_ttest keeps a group's values in registers, up to TTEST_MAX_GROUP chromosomes (csrc/sp_enrich.hip);
#                 scaffold-level runs with larger groups, up to TTEST_WIDE_MAX_GROUP, take k7_ttest_wide*
#   rank-sum      k7_ranktest ranks the two chosen groups in LDS, up to RANKTEST_MAX_GROUP each (csrc/sp_ranktest.hip);
#                 larger groups, up to RANKTEST_WIDE_MAX_GROUP, take k7_ranktest_wide, a workgroup per k-mer
#                 (csrc/sp_rankwide.hip)
#   wilcoxon      k7_wilcoxon: every subgenome has the same number of chromosomes, 2 .. WILCOXON_MAX_GROUP
#                 (csrc/sp_wilcoxon.hip); unequal sizes reach scipy, which raises
KMER_ENGINES = {
    "ttest_ind": [("kmer_ttest", (), _groups_upto(lambda: TTEST_MAX_GROUP), False),
                  ("kmer_ttest_wide", (), _groups_upto(lambda: TTEST_WIDE_MAX_GROUP), False)],
    "wilcoxon": [("kmer_wilcoxon", (), _wilcoxon_sizes, True)],
}
for _m in _native.RANKTEST_METHODS:
    KMER_ENGINES[_m] = [("kmer_ranktest", (_m,), _groups_upto(lambda: _native.RANKTEST_MAX_GROUP),
                         "no device context with the rank-sum tests"),
                        ("kmer_ranktest_wide", (_m,), _groups_upto(lambda: _native.RANKTEST_WIDE_MAX_GROUP),
                         "no device context with the rank-sum tests")]


def numpy_kmer_test(X, groups, test_method="ttest_ind"):
    """Cluster.output_kmers' test in numpy on the M x C fp64 matrix (matrices without a context, the other
    `-test_method`s): (top, second, pvals, means [M, n_groups])."""
    from scipy import special
    M, G = X.shape[0], len(groups)
    means = np.stack([X[:, g].mean(axis=1) for g in groups], axis=1) if M else np.zeros((0, G))
    # the reference orders groups by -sum/len (Cluster.py:182); ties keep SG-name order (stable)
    keyv = np.stack([-(X[:, g].sum(axis=1) / len(g)) for g in groups], axis=1) if M else means
    order = np.argsort(keyv, axis=1, kind="stable")
    top, second = order[:, 0], (order[:, 1] if G > 1 else order[:, 0])
    pvals = np.ones(M)
    for a in range(G):
        for b in range(G):
            if a == b:
                continue
            sel = np.flatnonzero((top == a) & (second == b))
            if sel.size and test_method == "ttest_ind":
                pvals[sel] = _ttest_ind(X[np.ix_(sel, groups[a])], X[np.ix_(sel, groups[b])], special)
            elif sel.size:      # the other scipy tests the reference accepts (Cluster.py:178-194), row by row
                pvals[sel] = _scipy_rows(test_method, X[np.ix_(sel, groups[a])], X[np.ix_(sel, groups[b])])
    return top, second, pvals, means


def _kruskal_rows(a, b):
    """scipy.stats.kruskal(a[i], b[i]).pvalue for every row, in array form (same operations in the same order as
    scipy's: average ranks, tie correction 1 - sum(t^3 - t) / (N^3 - N), H = 12 / (N (N + 1)) * sum(R_j^2 / n_j)
    - 3 (N + 1), chi-square survival function with one degree of freedom); rows whose values are all identical --
    where scipy raises "All numbers are identical" -- get p = 1 like the row-wise wrapper below gives them."""
    from scipy import special, stats as st
    n1, n2 = a.shape[1], b.shape[1]
    N = float(n1 + n2)
    x = np.concatenate([a, b], axis=1)
    ranked = st.rankdata(x, axis=1)
    srt = np.sort(ranked, axis=1)
    first = np.concatenate([np.ones((x.shape[0], 1), bool), srt[:, 1:] != srt[:, :-1]], axis=1)
    # size of the tie group every element belongs to: distance between consecutive group starts
    idx = np.where(first, np.arange(x.shape[1])[None, :], 0)
    start = np.maximum.accumulate(idx, axis=1)
    nxt = np.where(first, np.arange(x.shape[1])[None, :], x.shape[1])
    end = np.minimum.accumulate(nxt[:, ::-1], axis=1)[:, ::-1]       # start of the NEXT group at or after this element
    end = np.concatenate([end[:, 1:], np.full((x.shape[0], 1), x.shape[1])], axis=1)
    end = np.where(first, end, 0)        # count every group once, at its first element
    cnt = np.where(first, (end - start).astype(np.float64), 0.0)
    ties = 1.0 - (cnt ** 3 - cnt).sum(axis=1) / (N ** 3 - N) if N >= 2 else np.ones(x.shape[0])
    ssbn = ranked[:, :n1].sum(axis=1) ** 2 / n1 + ranked[:, n1:].sum(axis=1) ** 2 / n2
    with np.errstate(all="ignore"):
        h = (12.0 / (N * (N + 1)) * ssbn - 3 * (N + 1)) / ties
        p = special.chdtrc(1, h)
    return np.where(ties == 0, 1.0, p)


def _wilcoxon_rows(a, b):
    """scipy.stats.wilcoxon(a[i], b[i]).pvalue for every row.  scipy (>= 1.13) picks the method per call: exact when the
    differences hold no ties and no zeros; with ties or zeros and at most 13 pairs an EXACT PERMUTATION TEST over all
    2^n sign assignments (3 ms per call: two hours for the 2.2 M rows of a wheat-like run); the normal approximation
    otherwise.  Here the rows are split the same way: scipy's own `axis` form for the exact and the asymptotic rows,
    and for the permutation rows the null distribution of r_plus = all subset sums of the ranks of |d| (zeros rank 0:
    they only duplicate subsets), one matrix product per block of rows; p = 2 min(#(null <= obs), #(null >= obs)) / 2^n
    with scipy's tolerance, clipped at 1.  Sums of half-integers are exact in floating point, so the p-values are
    scipy's bit for bit (tests/test_abi_and_host.py)."""
    from scipy import stats as st
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    M, n = a.shape
    out = np.ones(M)
    if M == 0 or n == 0:
        return out
    d = a - b
    nz = d != 0
    ad = np.where(nz, np.abs(d), np.inf)              # zeros are dropped ("wilcox"): rank them last, out of the way
    srt = np.sort(ad, axis=1)
    tied = ((srt[:, 1:] == srt[:, :-1]) & np.isfinite(srt[:, 1:])).any(axis=1)
    exact = ~tied & nz.all(axis=1) & (n <= 50)
    perm = ~exact & (n <= 13)
    asym = ~exact & ~perm
    if exact.any():
        out[exact] = st.wilcoxon(a[exact], b[exact], axis=1, method="exact")[1]
    if asym.any():
        out[asym] = st.wilcoxon(a[asym], b[asym], axis=1, method="asymptotic")[1]
    if perm.any():
        rows = np.flatnonzero(perm)
        ranks = np.where(nz[rows], st.rankdata(ad[rows], axis=1), 0.0)
        obs = np.where(d[rows] > 0, ranks, 0.0).sum(axis=1)
        pat = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)      # [2^n, n]
        gamma = np.abs(np.finfo(np.float64).eps * 100 * obs)
        step = max(1, (1 << 22) >> n)                 # ~32 MB of null values per block
        for lo in range(0, rows.size, step):
            sl = slice(lo, lo + step)
            null = ranks[sl] @ pat.T
            le = (null <= (obs[sl] + gamma[sl])[:, None]).sum(axis=1)
            ge = (null >= (obs[sl] - gamma[sl])[:, None]).sum(axis=1)
            out[rows[sl]] = np.clip(np.minimum(le, ge) / float(1 << n) * 2, 0, 1)
    return out


# scipy releases whose per-call method rules the array forms below restate (wilcoxon: exact for n <= 50 without ties
# or zeros, permutation for n <= 13, else asymptotic -- scipy 1.13; mannwhitneyu: exact unless both samples exceed 8
# values or any value is tied) and whose `axis=` / `method=` keywords they rely on.  Checked against the row-wise
# calls of 1.15 (tests/test_abi_and_host.py); any other release takes the row-wise loop (advisor r04).
_SCIPY_ARRAY_RANGE = ((1, 13), (1, 17))


def _scipy_array_ok(version=None):
    if version is None:
        import scipy
        version = scipy.__version__
    try:
        v = tuple(int(x) for x in version.split(".")[:2])
    except ValueError:
        return False
    return _SCIPY_ARRAY_RANGE[0] <= v < _SCIPY_ARRAY_RANGE[1]


def _scipy_rows(name, a, b):
    """p-value of scipy.stats.<name>(a[i], b[i]) for every row (the reference calls the test per k-mer).
    mannwhitneyu: scipy's own axis argument, the rows split by the method a row-wise call picks (millions of rows in seconds); kruskal: the array form
    above (equal to the row-wise call, tests/test_abi_and_host.py); wilcoxon: _wilcoxon_rows; groups of unequal size
    (scipy raises for every row) fall through to the row-wise loop, which reports scipy's error."""
    from scipy import stats as st
    if not _scipy_array_ok():
        name_array = None        # an unvalidated scipy release: its own row-wise calls decide (slow, but its answers)
    else:
        name_array = name
    if a.shape[0] and name_array == "mannwhitneyu":
        # method="auto" decides per CALL: exact unless both samples exceed 8 values or ANY value is tied -- so the rows
        # are split by what a row-wise call would have chosen for each of them
        n1, n2 = a.shape[1], b.shape[1]
        xs = np.sort(np.concatenate([a, b], axis=1), axis=1)
        tied = (xs[:, 1:] == xs[:, :-1]).any(axis=1)
        exact = ~tied if not (n1 > 8 and n2 > 8) else np.zeros(a.shape[0], bool)
        out = np.empty(a.shape[0])
        if exact.any():
            out[exact] = st.mannwhitneyu(a[exact], b[exact], axis=1, method="exact")[1]
        if (~exact).any():
            out[~exact] = st.mannwhitneyu(a[~exact], b[~exact], axis=1, method="asymptotic")[1]
        return out
    if a.shape[0] and name_array == "kruskal":
        return _kruskal_rows(np.asarray(a, np.float64), np.asarray(b, np.float64))
    if a.shape[0] and name_array == "wilcoxon" and a.shape[1] == b.shape[1] and a.shape[1] >= 2:      # (one pair: scipy's permutation branch raises)
        return _wilcoxon_rows(a, b)
    test = getattr(st, name)
    out = np.empty(a.shape[0])
    for i in range(a.shape[0]):
        try:
            out[i] = test(a[i], b[i])[1]
        except ValueError as e:
            if "identical" in str(e) or "zero" in str(e):     # all values equal: no evidence of a difference
                out[i] = 1.0
            else:
                raise
    return out


def _ttest_ind(a, b, special):
    """Row-wise scipy.stats.ttest_ind(a, b) (equal_var=True, two-sided) p-values."""
    n1, n2 = a.shape[1], b.shape[1]
    with np.errstate(all="ignore"):
        v1 = a.var(axis=1, ddof=1) if n1 > 1 else np.zeros(a.shape[0])
        v2 = b.var(axis=1, ddof=1) if n2 > 1 else np.zeros(a.shape[0])
        df = n1 + n2 - 2.0
        svar = ((n1 - 1) * v1 + (n2 - 1) * v2) / df if df > 0 else np.full(a.shape[0], np.nan)
        denom = np.sqrt(svar * (1.0 / n1 + 1.0 / n2))
        t = (a.mean(axis=1) - b.mean(axis=1)) / denom
        return 2.0 * special.stdtr(df, -np.abs(t))
