"""The differential filter over per-chromosome (key, count) lists, written from its specification (the comment block of
sp_filter in include/subphaser_hip.h) in plain Python and numpy.  TEST INFRASTRUCTURE ONLY.

  union            the chromosome x k-mer matrix of the lists
  decide_row       the decision for one k-mer: Python int and float only (int / int is the correctly rounded fp64
                   quotient, which is the defined behaviour)
  decide_pairs_vec the same decision in numpy float64 for sets of two single-chromosome units (million-row inputs)
  margin           the exact relative distance of a set from its fold threshold (classifies test inputs, decides nothing)
  filter           what sp_filter + sp_filter_fetch + sp_filter_hist return

sgs: list of sets, each a list of units, each a list of chromosome indices."""
from fractions import Fraction

import numpy as np


def union(lists):
    """lists: per chromosome (ascending uint64 keys, uint32 counts) -> keys (ascending), M x C uint32 matrix."""
    C = len(lists)
    parts = [np.asarray(k, np.uint64) for k, _ in lists]
    keys = np.unique(np.concatenate(parts)) if C else np.empty(0, np.uint64)
    mat = np.zeros((len(keys), C), np.uint32)
    for c, (k, v) in enumerate(lists):
        if len(k):
            mat[np.searchsorted(keys, np.asarray(k, np.uint64)), c] = np.asarray(v, np.uint32)
    return keys, mat


def _unit_sums(counts_row, lengths, sg):
    return [(sum(int(counts_row[c]) for c in unit), sum(int(lengths[c]) for c in unit)) for unit in sg]


def set_passes(counts_row, lengths, sg, min_fold, baseline):
    """The fold test of one set of two or more units."""
    f = [num / den for num, den in _unit_sums(counts_row, lengths, sg)]
    order = sorted(range(len(f)), key=lambda u: (-f[u], u))       # descending, ties in unit order
    f = [f[u] for u in order]
    return 1.0 * f[0] / (f[baseline] + 1e-20) >= min_fold


def fold_pass(counts_row, lengths, sgs, min_fold, baseline, ratio):
    """is_hist of one k-mer: enough of the sets of two or more units pass the fold test."""
    include = n_multi = 0
    for sg in sgs:
        if len(sg) == 1:
            continue
        n_multi += 1
        if set_passes(counts_row, lengths, sg, min_fold, baseline):
            include += 1
    return not (include / n_multi < ratio)


def decide_row(counts_row, lengths, sgs, min_fold, baseline, min_freq, max_freq, ratio, is_hist=None):
    """-> (is_hist, is_row) of one k-mer (is_hist: a fold_pass answer the caller kept)."""
    if is_hist is None:
        is_hist = fold_pass(counts_row, lengths, sgs, min_fold, baseline, ratio)
    if not is_hist:
        return False, False
    tot = float(sum(int(x) for x in counts_row))
    return True, not (tot < min_freq or tot > max_freq)


def decide_pairs_vec(counts, lengths, sgs, min_fold, baseline, min_freq, max_freq, ratio):
    """decide_row for every row of `counts` (M x C) at once: sets of two single-chromosome units (and singleton sets,
    which are skipped), baseline 1 or -1 -- the second unit frequency is the baseline either way."""
    assert baseline in (1, -1)
    counts = np.asarray(counts)
    cols = np.ascontiguousarray(counts.T)      # (a column per chromosome, contiguous)
    include = np.zeros(len(counts), np.int64)
    n_multi = 0
    for sg in sgs:
        if len(sg) == 1:
            continue
        assert len(sg) == 2 and len(sg[0]) == 1 and len(sg[1]) == 1, sg
        n_multi += 1
        a = cols[sg[0][0]].astype(np.float64) / np.float64(int(lengths[sg[0][0]]))
        b = cols[sg[1][0]].astype(np.float64) / np.float64(int(lengths[sg[1][0]]))
        hi, lo = np.maximum(a, b), np.minimum(a, b)
        include += (1.0 * hi / (lo + 1e-20) >= min_fold)
    is_hist = ~(include.astype(np.float64) / np.float64(n_multi) < ratio)
    tot = counts.sum(axis=1, dtype=np.uint64).astype(np.float64)
    is_row = is_hist & ~((tot < min_freq) | (tot > max_freq))
    return is_hist, is_row


def margin(counts_row, lengths, sg, min_fold, baseline):
    """hi / (lo * min_fold) - 1 as an exact Fraction (without the 1e-20); None when lo == 0."""
    f = [Fraction(num, den) for num, den in _unit_sums(counts_row, lengths, sg)]
    order = sorted(range(len(f)), key=lambda u: (-f[u], u))
    f = [f[u] for u in order]
    hi, lo = f[0], f[baseline]
    if lo == 0:
        return None
    return hi / (lo * Fraction(min_fold)) - 1


def filter(lists, lengths, sgs, min_fold=2, baseline=1, min_freq=200, max_freq=1e9, ratio=1, vec=False, memo=None,
           joined=None):
    """-> n_union, keys, counts, tot, hist (ascending), freqs: the differential rows in ascending key order,
    freqs = counts / lengths in fp64.  vec: decide with decide_pairs_vec instead of row by row.  memo: a dict that
    keeps fold_pass's answers per distinct count row, for callers that filter the same rows under several key sets or
    frequency bounds (one dict per lengths, sgs, min_fold, baseline and ratio)."""
    keys, mat = union(lists)
    args = (min_fold, baseline, min_freq, max_freq, ratio)
    if vec:
        is_hist, is_row = decide_pairs_vec(mat, lengths, sgs, *args)
    else:
        is_hist = np.zeros(len(keys), bool)
        is_row = np.zeros(len(keys), bool)
        rows = mat.tolist()
        for i, row in enumerate(rows):
            if memo is None:
                is_hist[i], is_row[i] = decide_row(row, lengths, sgs, *args)
                continue
            t = tuple(row)
            if t not in memo:
                memo[t] = fold_pass(row, lengths, sgs, min_fold, baseline, ratio)
            is_hist[i], is_row[i] = decide_row(row, lengths, sgs, *args, is_hist=memo[t])
    tot_all = mat.sum(axis=1, dtype=np.uint64)
    counts = mat[is_row]
    freqs = counts.astype(np.float64) / np.asarray(lengths, np.int64).astype(np.float64)[None, :]
    return len(keys), keys[is_row], counts, tot_all[is_row], np.sort(tot_all[is_hist]), freqs
