"""Seeded inputs of the homoeologous-block tests (CPU and GPU): sequences as str, built once and shared."""
import numpy as np

_B = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
_cache = {}


def rand_seq(rng, n):
    return _B[rng.randint(0, 4, size=n)].tobytes().decode()


def revcomp(s):
    return s.translate(_COMP)[::-1]


def mutate(rng, s, rate):
    a = np.frombuffer(s.encode(), np.uint8).copy()
    m = rng.random_sample(a.size) < rate
    cur = np.searchsorted(_B, a[m])
    a[m] = _B[(cur + rng.randint(1, 4, size=int(m.sum()))) % 4]
    return a.tobytes().decode()


def _put(s, at, text):
    return s[:at] + text + s[at + len(text):]


def edges():
    """Two related sequences of 4211 and 3917 bases (no multiple of 16 or 32): B is A without its bases 1000..1293, with
    2 % substitutions; N runs across a 32-start unit boundary (2040..2055 crosses 2048) and across the window boundaries
    of bin = 64 (..2048) and bin = 1000 (2990..3010); a lower-case stretch, IUPAC codes; and both sequences end in the
    same 40 unmutated bases, so the very last start of either is a valid, shared k-mer for every kb <= 31."""
    if "edges" not in _cache:
        rng = np.random.RandomState(101)
        a = rand_seq(rng, 4211)
        b = mutate(rng, a[:1000] + a[1294:4171], 0.02) + a[4171:]
        a = _put(a, 2040, "N" * 16)
        a = _put(a, 2990, "N" * 20)
        a = _put(a, 500, a[500:760].lower())
        a = _put(a, 3333, "R")
        a = _put(a, 31, "n")          # the first 32-start unit has one valid start fewer than it has bases
        b = _put(b, 1017, "NNNNN")
        b = _put(b, 2500, b[2500:2600].lower())
        b = _put(b, 64, "Y")
        _cache["edges"] = (a, b)
    return _cache["edges"]


PLANTED = dict(inv=(5300, 13300), dup_src=16000, dup_dst=22000, dup_len=4000, ins_at=30000, ins_len=5000)


def planted(seed=5):
    """A: 40 137 random bases.  B: A with 5 % substitutions, A[5300:13300] inverted in place, B[16000:20000] copied over
    B[22000:26000] (the second copy; both copies' k-mers stop being single-copy in B) and 5000 unrelated bases inserted
    at 30000."""
    key = ("planted", seed)
    if key not in _cache:
        rng = np.random.RandomState(seed)
        a = rand_seq(rng, 40137)
        b = mutate(rng, a, 0.05)
        i0, i1 = PLANTED["inv"]
        b = _put(b, i0, revcomp(b[i0:i1]))
        s, d, n = PLANTED["dup_src"], PLANTED["dup_dst"], PLANTED["dup_len"]
        b = _put(b, d, b[s:s + n])
        at = PLANTED["ins_at"]
        b = b[:at] + rand_seq(rng, PLANTED["ins_len"]) + b[at:]
        _cache[key] = (a, b)
    return _cache[key]


def worst():
    """(A, the same 20 011 bases again, the same cut into 64-base pieces and shuffled)"""
    if "worst" not in _cache:
        rng = np.random.RandomState(77)
        a = rand_seq(rng, 20011)
        pieces = [a[i:i + 64] for i in range(0, len(a), 64)]
        order = rng.permutation(len(pieces))
        _cache["worst"] = (a, a, "".join(pieces[i] for i in order))
    return _cache["worst"]


def unrelated():
    if "unrelated" not in _cache:
        rng = np.random.RandomState(9)
        _cache["unrelated"] = (rand_seq(rng, 3001), rand_seq(rng, 2777))
    return _cache["unrelated"]


def trio():
    """three chromosomes of one backbone: 3 % substitutions each, the third with an inverted middle"""
    if "trio" not in _cache:
        rng = np.random.RandomState(31)
        base = rand_seq(rng, 6029)
        c0, c1, c2 = mutate(rng, base, 0.03), mutate(rng, base[:5500], 0.03), mutate(rng, base[300:], 0.03)
        c2 = _put(c2, 2000, revcomp(c2[2000:3500]))
        _cache["trio"] = (c0, c1, c2)
    return _cache["trio"]


def check_planted(blocks, bin_size):
    """the inversion is one `-` block whose ends lie within one bin of the planted ones; no block reaches into the second
    copy of the duplicated segment by more than the window that straddles its edge"""
    i0, i1 = PLANTED["inv"]
    minus = [b for b in blocks if b[4] == "-"]
    assert len(minus) == 1
    s1, e1, s2, e2 = minus[0][:4]
    assert abs(s1 - i0) <= bin_size and abs(e1 - i1) <= bin_size and abs(s2 - i0) <= bin_size and abs(e2 - i1) <= bin_size
    d0 = PLANTED["dup_dst"]
    d1 = d0 + PLANTED["dup_len"]
    for b in blocks:
        assert b[3] <= d0 + bin_size or b[2] >= d1 - bin_size, b
    assert len([b for b in blocks if b[4] == "+"]) >= 3
