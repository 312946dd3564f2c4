"""Positional reference of the four map modes (bins, windows, features, intervals): plain numpy over the label of
every k-mer start, no project kernel and no C oracle.  The oracle (oracle/sp_oracle.c, tests/oracle_ctx.py) computes a
start's chunk and a slot's chunk with the same closed forms as the kernels; here the chunks are cut and walked one by
one, the way the modelled project cuts them, and a row is whatever the positions say it is.

    hits       label and key index of the canonical k-mer at every start
    bins       [rows, S] counts, row = start // bin + (index of the chunk the start was met in)
    windows    [rows, S] counts, row = (seg_start + start // bin * bin) // window
    ranges     [n, S] counts of the starts s with a <= s and s + k <= e (features and intervals), by cumulative sums
"""
import numpy as np

from subphaser_amd import kmer as km
from test_gpu_map_runs import _keys_by_position      # (canonical key per start of an ACGT-only sequence)

_A = ord("A")


def hits(seq, k, keys, lab):
    """(label, key index) of every start s in [0, L - k]: -1 / -1 where the window holds a byte that is not ACGT (after
    upper-casing) or its canonical k-mer is not in `keys` (sorted, canonical)."""
    a = np.frombuffer(bytes(seq), np.uint8) if isinstance(seq, (bytes, bytearray, str)) else np.asarray(seq, np.uint8)
    n = a.size - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    up = np.where((a >= 97) & (a <= 122), a - 32, a).astype(np.uint8)
    bad = ~np.isin(up, np.frombuffer(b"ACGT", np.uint8))
    cb = np.concatenate(([0], np.cumsum(bad)))
    valid = (cb[k:k + n] - cb[:n]) == 0                                   # no bad byte in [s, s + k)
    key = _keys_by_position(np.where(bad, _A, up).astype(np.uint8), k)    # (a bad byte reads as A: masked below)
    assert key.size == n
    keys = np.asarray(keys, np.uint64)
    assert keys.size and (keys[1:] > keys[:-1]).all() and (km.canonical(keys, k) == keys).all()
    pos = np.minimum(np.searchsorted(keys, key), keys.size - 1)
    found = valid & (keys[pos] == key)
    idx = np.where(found, pos, -1).astype(np.int64)
    return np.where(found, np.asarray(lab, np.int64)[pos], -1), idx


def chunks(L, k, W):
    """the pieces a sequence of L bases is mapped in: one per multiple i of W below L, the bases [i - (k - 1), i + W)
    clipped to the sequence; W = 0: the sequence itself"""
    if W == 0:
        return [(0, L)]
    return [(max(0, i - (k - 1)), min(i + W, L)) for i in range(0, L, W)]


def n_rows(L, k, bin_size, W):
    """The size of a bins table is a convention of the interface, not a property of the positions: a row per bin of the
    sequence (an empty one counts as one base) plus a row per multiple of W up to L + k - 1, the furthest a chunk index
    could be pushed by the k - 1 bases of overlap.  bins() checks that every hit lands below it."""
    L1 = max(L, 1)
    return len(range(0, L1, bin_size)) + (len(range(0, L1 + k, W)) if W else 1)


def bins(lab_at, L, k, S, bin_size, W):
    """[n_rows, S] int64: every chunk walked, every k-mer that fits inside it dropped into row start // bin + j"""
    out = np.zeros((n_rows(L, k, bin_size, W), S), np.int64)
    seen = np.zeros(lab_at.size, np.int64)
    for j, (a, b) in enumerate(chunks(L, k, W)):
        if b - a < k:
            continue
        s = np.arange(a, b - k + 1)
        seen[s] += 1
        s = s[lab_at[s] >= 0]
        rows = s // bin_size + j
        assert rows.size == 0 or rows.max() < out.shape[0]
        np.add.at(out, (rows, lab_at[s]), 1)
    assert W == 0 or W < k or (seen == 1).all()      # chunks of at least k bases meet every start exactly once
    return out


def windows(lab_at, S, bin_size, window_size, rows, seg_start=0):
    """[rows, S] int64 from positions alone: the bin a start lies in, then the window that bin's first base lies in"""
    out = np.zeros((rows, S), np.int64)
    s = np.flatnonzero(lab_at >= 0)
    r = (seg_start + s // bin_size * bin_size) // window_size
    assert r.size == 0 or r.max() < rows
    np.add.at(out, (r, lab_at[s]), 1)
    return out


def window_rows(L, window_size):
    return -(-L // window_size) + 1


def ranges(lab_at, k, S, a, e):
    """([n, S] int64 counts of the hits with a[i] <= s and s + k <= e[i], mask of the starts inside some range)"""
    n = lab_at.size
    cum = np.zeros((n + 1, S), np.int64)
    for g in range(S):
        cum[1:, g] = np.cumsum(lab_at == g)
    a, e = np.asarray(a, np.int64), np.asarray(e, np.int64)
    lo, hi = np.minimum(a, n), np.clip(e - k + 1, 0, n)
    hi = np.maximum(hi, lo)
    cover = np.zeros(n + 1, np.int64)
    np.add.at(cover, lo, 1)
    np.add.at(cover, hi, -1)
    return cum[hi] - cum[lo], np.cumsum(cover)[:n] > 0


def totals(lab_at, idx_at, counted=None):
    """(n_mapped, labels_hit) of the starts in `counted` (default: all): the hits, and the distinct keys among them"""
    m = lab_at >= 0
    if counted is not None:
        m &= counted
    return int(m.sum()), np.unique(idx_at[m])
