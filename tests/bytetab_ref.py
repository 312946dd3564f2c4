"""Plain reference for the byte-table wire format (include/subphaser_hip.h, sp_tables_bind ff.): one byte per
dense slot holding the raw count saturated at 255, plus an overflow list of (absolute slot, exact count) pairs,
ascending slot, for every count >= 255.  numpy only, exact integer arithmetic, nothing of the library imported:
TEST INFRASTRUCTURE ONLY -- what sp_table_merge / sp_table_lengths / sp_table_overflow are compared with."""
import numpy as np

SAT = 255
BUCKET = 1 << 15      # the merge kernel ranks its pairs per bucket of 2^15 LOCAL slots


def encode(exact_u32, slot_base=0):
    """exact counts of slots [slot_base, slot_base + n) -> (bytes uint8[n], pairs uint32[m, 2])"""
    exact = np.asarray(exact_u32)
    assert exact.ndim == 1 and (exact.size == 0 or (int(exact.min()) >= 0 and int(exact.max()) < 1 << 32))
    assert 0 <= slot_base and slot_base + exact.size <= 1 << 32
    exact = exact.astype(np.uint64)
    big = np.flatnonzero(exact >= SAT)
    pairs = np.empty((big.size, 2), np.uint32)
    pairs[:, 0] = (big + int(slot_base)).astype(np.uint32)
    pairs[:, 1] = exact[big].astype(np.uint32)
    return np.minimum(exact, SAT).astype(np.uint8), pairs


def decode(bytes_u8, pairs, slot_base, n):
    """exact counts (uint32[n]) of a byte slice; `pairs` may cover more than [slot_base, slot_base + n)"""
    b = np.asarray(bytes_u8, np.uint8)
    assert b.shape == (n,)
    out = b.astype(np.uint32)
    p = np.asarray(pairs, np.uint32).reshape(-1, 2)
    loc = p[:, 0].astype(np.int64) - int(slot_base)
    ok = (loc >= 0) & (loc < n)
    loc, val = loc[ok], p[ok, 1]
    assert np.unique(loc).size == loc.size, "a slot has two overflow pairs"
    assert (val >= SAT).all(), "an overflow pair below 255"
    assert (b[loc] == SAT).all(), "an overflow pair on an unsaturated byte"
    assert loc.size == int((b == SAT).sum()), "a saturated byte without its pair"
    out[loc] = val
    return out


def add(a, b):
    """exact sum of two exact tables (uint64)"""
    return np.asarray(a).astype(np.uint64) + np.asarray(b).astype(np.uint64)


def merge(a, b, slot_base=0):
    """what sp_table_merge leaves behind: a + b on exact uint64 counts, re-encoded -> (bytes, pairs)"""
    return encode(add(a, b), slot_base)


def lengths(exact, lower):
    """(sum, number) of the counts >= max(1, lower)"""
    e = np.asarray(exact).astype(np.uint64)
    keep = e >= max(1, int(lower))
    return int(e[keep].sum()), int(keep.sum())


def pairs_per_bucket(pairs, slot_base, n):
    """number of pairs in every bucket of 2^15 local slots of the slice"""
    p = np.asarray(pairs, np.uint32).reshape(-1, 2)
    loc = p[:, 0].astype(np.int64) - int(slot_base)
    assert ((loc >= 0) & (loc < n)).all()
    return np.bincount(loc // BUCKET, minlength=(n + BUCKET - 1) // BUCKET)


# ---------------------------------------------------------------------------------------------------------------
# Inputs for the merge tests: two exact tables whose sum has one crowded bucket (more than 96 pairs: the merge ranks
# such a bucket through a bitmap, fewer by brute force), one lightly filled bucket and one empty bucket, as far as
# the slice has buckets for them.
def _plant(rng, A, B, where):
    """Every class of summands, in turn, at the local slots `where`."""
    for j, i in enumerate(where):
        c = j % 8
        if c == 0:      # both below 255, the sum reaches it
            a = int(rng.randint(128, 255)); b = int(rng.randint(255 - a, 255))
        elif c == 1:    # exactly 254: the largest sum that stays in the byte
            a = int(rng.randint(0, 255)); b = 254 - a
        elif c == 2:    # exactly 255: the smallest sum that leaves it
            a = int(rng.randint(1, 255)); b = 255 - a
        elif c == 3:    # dst saturated (exactly 255 now and then), src in the byte or absent
            a = int(rng.choice([255, 256, 300, 4000])); b = int(rng.choice([0, 1, 254]))
        elif c == 4:    # src saturated
            a = int(rng.choice([0, 7, 254])); b = int(rng.choice([255, 257, 65535]))
        elif c == 5:    # both saturated
            a = int(rng.randint(255, 3000)); b = int(rng.randint(255, 3000))
        elif c == 6:    # beyond 16 bits, one side
            a = int(rng.randint(65536, 5_000_000)); b = int(rng.randint(0, 255))
        else:           # beyond 16 bits, both sides
            a = int(rng.randint(65536, 1 << 30)); b = int(rng.randint(65536, 1 << 30))
        A[i], B[i] = a, b


def make_summands(seed, slot_base, n):
    """(A, B, info): exact uint32 tables of slots [slot_base, slot_base + n).  info names the local buckets that
    were given many / few / no slots with a sum >= 255 (None where the slice is too short for one) and the local
    offset of the first absolute 2^15 boundary inside the slice."""
    rng = np.random.RandomState(seed)
    A = (rng.randint(0, 31, size=n) * (rng.rand(n) < 0.5)).astype(np.uint32)
    B = (rng.randint(0, 31, size=n) * (rng.rand(n) < 0.5)).astype(np.uint32)
    info = dict(crowded=None, light=None, empty=None, boundary=None)
    nb = (n + BUCKET - 1) // BUCKET
    if n == 0:
        return A, B, info
    if n < 1024:         # too short for a crowded bucket: every class once, as far as the slots go
        _plant(rng, A, B, rng.permutation(n)[:8])
        return A, B, info
    # the crowded bucket is the one the first absolute bucket boundary cuts (bucket 0), planted on both sides of
    # the cut; an aligned slice has no such cut, its bucket 0 is planted around its middle
    cut = BUCKET - slot_base % BUCKET if slot_base % BUCKET else BUCKET // 2
    if slot_base % BUCKET:
        info["boundary"] = cut
    lo = np.arange(max(0, cut - 600), cut)
    hi = np.arange(cut, min(cut + 600, BUCKET, n))
    where = np.concatenate([rng.permutation(lo)[:300], rng.permutation(hi)[:300]])
    _plant(rng, A, B, rng.permutation(where))
    info["crowded"] = 0
    if nb >= 2:          # the last (possibly ragged) bucket: a few dozen pairs
        first = (nb - 1) * BUCKET
        _plant(rng, A, B, first + rng.permutation(n - first)[:40])
        info["light"] = nb - 1
    if nb >= 3:
        info["empty"] = 1
    return A, B, info


def with_outside(pairs, slot_base, n, seed, space=1 << 29):
    """The same list as part of a whole-table list: ascending pairs below and above the slice around it."""
    rng = np.random.RandomState(seed)
    out = []
    for lo, hi in ((0, slot_base), (slot_base + n, space)):
        m = min(50, max(0, hi - lo))
        s = np.unique(rng.randint(lo, hi, size=m)) if m else np.zeros(0, np.int64)
        out.append(np.stack([s, rng.randint(255, 100000, size=s.size)], axis=1).astype(np.uint32).reshape(-1, 2))
    return np.ascontiguousarray(np.concatenate([out[0], np.asarray(pairs, np.uint32).reshape(-1, 2), out[1]]))
