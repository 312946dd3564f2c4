"""The byte-table exchange primitives of the multi-GPU path at k <= 15 -- sp_table_overflow, sp_table_merge,
sp_table_lengths, sp_filter_view on a slot range, sp_count_range -- each against a plain reference
(tests/bytetab_ref.py: numpy, exact integers) or the CPU oracle, one process, no collectives.  dist.py cuts the
slot space into 64-slot aligned ranges, so the slices these primitives see start at bases that are NOT multiples
of the 2^15-slot bucket the overflow lists are built in.  Every comparison is bit-exact."""
import numpy as np
import pytest

import bytetab_ref as ref
import pyoracle as po

pytestmark = pytest.mark.gpu

B = ref.BUCKET
GUARD = 64             # sentinel bytes behind every uploaded table: nothing may be written past a slice
FILL8, FILL32 = 0xA5, 0xEEEEEEEE


class _Dev:
    """device buffers of one test, freed behind it"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.dev_alloc(max(int(nbytes), 16))
        self.ptrs.append(p)
        return p

    def put_bytes(self, b):
        """a table slice followed by GUARD sentinel bytes"""
        b = np.asarray(b, np.uint8)
        p = self.alloc(b.size + GUARD)
        self.ctx.host_to_dev(p, np.concatenate([b, np.full(GUARD, FILL8, np.uint8)]))
        return p

    def get_bytes(self, p, n):
        a = self.ctx.dev_to_host(p, n + GUARD)
        assert (a[n:] == FILL8).all(), "bytes behind the slice were written"
        return a[:n]

    def put_pairs(self, pairs):
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        p = self.alloc(8 * len(pairs))
        if len(pairs):
            self.ctx.host_to_dev(p, pairs)
        return p, len(pairs)

    def new_list(self, cap):
        """an output list of `cap` pairs (+ one guard pair), filled with a sentinel"""
        p = self.alloc(8 * (cap + 1))
        self.ctx.host_to_dev(p, np.full((cap + 1, 2), FILL32, np.uint32))
        return p

    def get_list(self, p, m, cap):
        a = self.ctx.dev_to_host(p, 8 * (cap + 1)).view(np.uint32).reshape(-1, 2)
        assert (a[m:] == FILL32).all(), "pairs behind the returned count were written"
        return a[:m]

    def free_all(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


@pytest.fixture
def dev(gpu_ctx):
    d = _Dev(gpu_ctx)
    yield d
    d.free_all()


def _check_list(got, exp, what):
    """a merged overflow list against the reference's; the order is stated on its own: sp_ovf_lookup (k3_eval / k3_slow /
    kx_merge / k3_emit) binary-searches these lists, an unsorted one silently turns exact counts into 255"""
    assert len(got) == len(exp), (what, len(got), len(exp))
    slots = got[:, 0].astype(np.int64)
    assert np.all(np.diff(slots) > 0), \
        "%s: the merged overflow list is not ascending (first descent at pair %d: slot %d -> %d)" % (
            what, int(np.flatnonzero(np.diff(slots) <= 0)[0]), *slots[np.flatnonzero(np.diff(slots) <= 0)[0]:][:2])
    assert (got == exp).all(), "%s: merged pairs differ from the reference" % what


# ------------------------------------------------------------------------------------------------------ a. merge
MERGE_CASES = [
    pytest.param(0, 3 * B, True, id="aligned-3-buckets"),
    pytest.param(64, B, False, id="base64-one-bucket-straddles-32768"),
    pytest.param(11184832, 2 * B + 4160, True, id="k13-rank1-of-3-ragged-end"),
    pytest.param((1 << 29) - (B + 64), B + 64, False, id="top-of-k15-slot-space"),
    pytest.param(32767, 1, True, id="one-slot"),
    pytest.param(64, 0, False, id="no-slot"),
]


@pytest.mark.parametrize("slot_base,n,whole_lists", MERGE_CASES)
def test_table_merge_vs_reference(gpu_ctx, dev, slot_base, n, whole_lists):
    """dst += src at aligned and unaligned bases: returned count, dst bytes, merged pairs and their order.
    whole_lists: the input lists cover the whole table (what dist.py passes) instead of the range only."""
    A, Bt, info = ref.make_summands(20 + n % 7, slot_base, n)
    ba, pa = ref.encode(A, slot_base)
    bb, pb = ref.encode(Bt, slot_base)
    if whole_lists:
        pa, pb = ref.with_outside(pa, slot_base, n, 1), ref.with_outside(pb, slot_base, n, 2)
    exp_bytes, exp_pairs = ref.merge(A, Bt, slot_base)
    # the case must not quietly degenerate: stated on the reference, before any GPU call.  (A slice of one / two
    # buckets has no room for a light / an empty bucket next to the crowded one; the generator says which exist.)
    per = ref.pairs_per_bucket(exp_pairs, slot_base, n)
    loc = exp_pairs[:, 0].astype(np.int64) - slot_base
    if n >= B:
        assert info["crowded"] is not None and per[info["crowded"]] > 96
        if slot_base % B:
            cut, inb = info["boundary"], loc // B == info["crowded"]
            assert cut == B - slot_base % B
            assert (inb & (loc < cut)).sum() >= 30 and (inb & (loc >= cut)).sum() >= 30
        tot, sa, sb = ref.add(A, Bt), A >= 255, Bt >= 255
        assert (~sa & ~sb & (tot >= 255)).any() and (tot == 254).any() and (tot == 255).any()
        assert (sa ^ sb).any() and (sa & sb).any() and (tot > 65535).any()
    if len(per) >= 2:
        assert any(1 <= c <= 96 for c in per)
    if len(per) >= 3:
        assert (per == 0).any()
    d_a, d_b = dev.put_bytes(ba), dev.put_bytes(bb)
    (d_pa, n_pa), (d_pb, n_pb) = dev.put_pairs(pa), dev.put_pairs(pb)
    cap = len(exp_pairs) + 5
    d_out = dev.new_list(cap)
    m = gpu_ctx.table_merge(d_a, d_pa, n_pa, d_b, d_pb, n_pb, slot_base, n, d_out, cap)
    assert m == len(exp_pairs)
    assert (dev.get_bytes(d_a, n) == exp_bytes).all()
    assert (dev.get_bytes(d_b, n) == bb).all()                   # src is read only
    _check_list(dev.get_list(d_out, m, cap), exp_pairs, "base %d, n %d" % (slot_base, n))
    if n_pa:
        assert (gpu_ctx.dev_to_host(d_pa, 8 * n_pa).view(np.uint32).reshape(-1, 2) == pa).all()


# ----------------------------------------------------------------------------------------- b. chains and lengths
@pytest.mark.parametrize("slot_base,n", [pytest.param(11184832, 2 * B + 4160, id="k13-rank1-of-3"),
                                         pytest.param(0, 2 * B, id="aligned")])
def test_table_merge_chain_and_lengths(gpu_ctx, dev, slot_base, n):
    """((A += B) += C): the list the first merge wrote is dst's list of the second, dst is written in place both
    times; then sp_table_lengths on the result with a list that covers more than the range."""
    A, Bt, _ = ref.make_summands(31, slot_base, n)
    C1, C2, _ = ref.make_summands(32, slot_base, n)
    Cc = np.maximum(C1, C2)                                       # a third summand, crowded in the same bucket
    exact = ref.add(ref.add(A, Bt), Cc)
    assert int(exact.max()) < 1 << 32
    exp_bytes, exp_pairs = ref.encode(exact, slot_base)
    assert ref.pairs_per_bucket(exp_pairs, slot_base, n)[0] > 96
    enc = [ref.encode(t, slot_base) for t in (A, Bt, Cc)]
    d_t = [dev.put_bytes(b) for b, _ in enc]
    d_p = [dev.put_pairs(ref.with_outside(p, slot_base, n, 40 + i) if i != 1 else p) for i, (_, p) in enumerate(enc)]
    cap = len(exp_pairs) + 8
    d_o1, d_o2 = dev.new_list(cap), dev.new_list(cap)
    m1 = gpu_ctx.table_merge(d_t[0], d_p[0][0], d_p[0][1], d_t[1], d_p[1][0], d_p[1][1], slot_base, n, d_o1, cap)
    _check_list(dev.get_list(d_o1, m1, cap), ref.merge(A, Bt, slot_base)[1], "first link")
    m2 = gpu_ctx.table_merge(d_t[0], d_o1, m1, d_t[2], d_p[2][0], d_p[2][1], slot_base, n, d_o2, cap)
    assert (dev.get_bytes(d_t[0], n) == exp_bytes).all()
    got = dev.get_list(d_o2, m2, cap)
    _check_list(got, exp_pairs, "second link")
    assert (ref.decode(dev.get_bytes(d_t[0], n), got, slot_base, n) == exact).all()
    d_more, n_more = dev.put_pairs(ref.with_outside(exp_pairs, slot_base, n, 50))
    assert n_more > len(exp_pairs)
    for lower in (1, 3, 255, 256, 70000):
        assert gpu_ctx.table_lengths(d_t[0], d_more, n_more, slot_base, n, lower) == ref.lengths(exact, lower), lower
        assert gpu_ctx.table_lengths(d_t[0], d_o2, m2, slot_base, n, lower) == ref.lengths(exact, lower), lower
    # a table without any saturated slot and without a list
    small = np.minimum(A, 200).astype(np.uint32)
    d_s = dev.put_bytes(ref.encode(small, slot_base)[0])
    assert gpu_ctx.table_lengths(d_s, 0, 0, slot_base, n, 3) == ref.lengths(small, 3)
    assert gpu_ctx.table_lengths(d_s, 0, 0, slot_base, 0, 1) == (0, 0)


# ------------------------------------------------------------------------------------------------- c. capacity
def test_table_merge_capacity(gpu_ctx, dev):
    """One pair too few is an ordinary error (the kernel guards every write with pos < cap) whose message carries
    the number needed; from fresh inputs with exactly that capacity the merge succeeds."""
    slot_base, n = 64, B
    A, Bt, _ = ref.make_summands(41, slot_base, n)
    (ba, pa), (bb, pb) = ref.encode(A, slot_base), ref.encode(Bt, slot_base)
    exp_bytes, exp_pairs = ref.merge(A, Bt, slot_base)
    need = len(exp_pairs)
    assert need > 96
    d_b, (d_pa, n_pa), (d_pb, n_pb) = dev.put_bytes(bb), dev.put_pairs(pa), dev.put_pairs(pb)
    d_a, d_out = dev.put_bytes(ba), dev.new_list(need - 1)
    with pytest.raises(MemoryError) as e:
        gpu_ctx.table_merge(d_a, d_pa, n_pa, d_b, d_pb, n_pb, slot_base, n, d_out, need - 1)
    assert ("%d overflow pairs" % need) in str(e.value) and ("capacity %d" % (need - 1)) in str(e.value)
    dev.get_bytes(d_a, n), dev.get_bytes(d_b, n)                  # (guards intact)
    a = gpu_ctx.dev_to_host(d_out, 8 * need).view(np.uint32).reshape(-1, 2)
    assert (a[need - 1:] == FILL32).all()                         # nothing behind the capacity
    d_a, d_out = dev.put_bytes(ba), dev.new_list(need)            # fresh inputs, the exact capacity
    m = gpu_ctx.table_merge(d_a, d_pa, n_pa, d_b, d_pb, n_pb, slot_base, n, d_out, need)
    assert m == need and (dev.get_bytes(d_a, n) == exp_bytes).all()
    _check_list(dev.get_list(d_out, m, need), exp_pairs, "exact capacity")
    # no saturated result: no list needed at all
    lo_a, lo_b = np.minimum(A, 100).astype(np.uint32), np.minimum(Bt, 100).astype(np.uint32)
    d_a, d_b2 = dev.put_bytes(lo_a.astype(np.uint8)), dev.put_bytes(lo_b.astype(np.uint8))
    assert gpu_ctx.table_merge(d_a, 0, 0, d_b2, 0, 0, slot_base, n, 0, 0) == 0
    assert (dev.get_bytes(d_a, n) == (lo_a + lo_b).astype(np.uint8)).all()


# -------------------------------------------------------------------- d / e. slot-range filter at non-zero bases
K, LOWER, NCHROM = 9, 1, 6
FILTERS = (
    ([[[0], [1]], [[2], [3]], [[4], [5]]], dict(min_fold=2, baseline=1, min_freq=1, max_freq=1e12, ratio=1)),
    ([[[0], [1]], [[2], [3]], [[4], [5]]], dict(min_fold=1.5, baseline=-1, min_freq=1, max_freq=1e12, ratio=0.6)),
    ([[[0], [1], [2]], [[3], [4, 5]]], dict(min_fold=2, baseline=1, min_freq=10, max_freq=1e12, ratio=0.5)),
    ([[[0, 4], [1, 5]], [[2], [3]]], dict(min_fold=2.0000001, baseline=-1, min_freq=1, max_freq=1e12, ratio=1)),
)


def _dumps_of(tabs, keys_all, lo, hi):
    """per chromosome the (keys ascending, counts) of the slots [lo, hi) with a count >= LOWER"""
    out = []
    for t in tabs:
        nz = np.flatnonzero(t[lo:hi] >= LOWER) + lo
        kk = keys_all[nz]
        o = np.argsort(kk, kind="stable")
        out.append((kk[o], t[nz][o].astype(np.uint32)))
    return out


@pytest.fixture(scope="module")
def view_case():
    """Hand-made exact tables at k = 9 (2^17 slots, 6 chromosomes), as test_filter_near_threshold_screen builds them:
    near-equal lengths and rows (2m, m), (3m, 2m), +-1 whose fold lands within 1e-9 .. 1e-3 of the threshold on both
    sides.  About 1.5 % of the slots carry such a row with m up to 2^20 (saturated bytes: the overflow lists decide),
    another 1 % one with m < 40 (decided from the bytes).  The whole-table oracle results are computed once."""
    from subphaser_amd import kmer as km
    n = km.dense_slots(K)
    rng = np.random.RandomState(177)
    base = 1_000_000_007
    lengths = np.array([base, base + 1, base + 1000, base - 3, 2 * base + 1, 2 * base - 1], np.int64)
    tabs = np.zeros((NCHROM, n), np.uint32)
    occ = rng.rand(NCHROM, n) < 0.5
    tabs[occ] = rng.randint(1, 50, size=int(occ.sum())).astype(np.uint32)
    rows = [(i, int(rng.randint(1, 1 << 20))) for i in range(0, n, 67)] + [(i, int(rng.randint(1, 40))) for i in range(5, n, 97)]
    for j, (i, m) in enumerate(rows):
        a, b = [(2 * m, m), (2 * m + 1, m), (2 * m - 1, m), (3 * m, 2 * m), (3 * m + 1, 2 * m), (4 * m, 2 * m + 1)][j % 6]
        tabs[0, i], tabs[1, i] = a, b
        tabs[2, i], tabs[3, i] = b, a
        tabs[4, i], tabs[5, i] = 2 * a, 2 * b
    sat = (tabs >= 255).any(axis=0).mean()
    assert 0.01 <= sat <= 0.02, sat
    keys_all = km.keys_of_slots(np.arange(n, dtype=np.uint64), K)
    whole = [po.filter_dumps(_dumps_of(tabs, keys_all, 0, n), sgs, list(range(NCHROM)), lengths=lengths, **kw)
             for sgs, kw in FILTERS]
    for w in whole:
        assert len(w.keys) > 0 and len(w.hist) > len(w.keys) // 2
    return dict(n=n, tabs=tabs, lengths=lengths, keys_all=keys_all, whole=whole)


def _dummy_count(ctx):
    """sp_filter_view wants a context that counted with the same k (any genome)"""
    ctx.genome_reset(NCHROM)
    for c in range(NCHROM):
        ctx.genome_add(c, b"ACGTACGTACGT")
    ctx.count(K, LOWER, 1)


def _filter_range(ctx, vc, d_ptrs, d_ovf, n_ovf, lo, hi, lengths, tabs, which):
    """sp_filter_view on [lo, hi) + sp_filter + sp_filter_fetch for the filters `which`, each compared with the oracle
    on the dumps restricted to the keys whose slot lies in the range; returns the rows per filter"""
    from subphaser_amd.config import sets_to_csr
    labels = list(range(NCHROM))
    dumps = _dumps_of(tabs, vc["keys_all"], lo, hi)
    out = {}
    for f in which:
        sgs, kw = FILTERS[f]
        exp = po.filter_dumps(dumps, sgs, labels, lengths=lengths, **kw)
        ctx.filter_view(d_ptrs, lo, hi - lo, lengths, K, LOWER, d_ovf, n_ovf)
        try:
            nu, nr, nh = ctx.filter(*sets_to_csr(sgs, labels), kw["min_fold"], kw["baseline"], kw["min_freq"],
                                    kw["max_freq"], kw["ratio"])
            keys, counts, freqs, tot = ctx.filter_fetch(nr)
        finally:
            ctx.filter_view(None, 0, 0, None, 0, 0)
        rows_ok = (nu, nr, nh) == (exp.n_union, len(exp.keys), len(exp.hist)) and (keys == exp.keys).all() and \
            (counts == exp.counts).all() and (tot == exp.tot).all()
        out[f] = dict(ok=rows_ok, n=(nu, nr, nh), exp_n=(exp.n_union, len(exp.keys), len(exp.hist)), keys=keys, counts=counts)
    return out


def _ranges(n, world):
    chunk = (n + 64 * world - 1) // (64 * world) * 64          # dist.py's range layout
    return [(r * chunk, min((r + 1) * chunk, n)) for r in range(world) if r * chunk < n]


def _upload_whole(dev, tabs):
    """whole byte tables and whole overflow lists of every chromosome"""
    d_tabs, d_ovf, n_ovf, pairs = [], [], [], []
    for t in tabs:
        b, p = ref.encode(t, 0)
        d_tabs.append(dev.put_bytes(b))
        dp, m = dev.put_pairs(p)
        d_ovf.append(dp), n_ovf.append(m), pairs.append(p)
    return d_tabs, d_ovf, n_ovf, pairs


def _range_lists(dev, pairs, lo, hi):
    """the overflow lists cut down to the pairs of [lo, hi)"""
    d_ovf, n_ovf = [], []
    for p in pairs:
        q = p[(p[:, 0] >= lo) & (p[:, 0] < hi)]
        dp, m = dev.put_pairs(q)
        d_ovf.append(dp), n_ovf.append(m)
    return d_ovf, n_ovf


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_filter_view_slot_ranges(gpu_ctx, dev, view_case, world):
    """The table cut into dist.py's ranges of `world` ranks (64-slot aligned, the last one short): every range equals
    the oracle on its keys, and the ranges together equal the whole table.  Table pointers are base pointer +
    slot_base; the lists are whole-chromosome lists and range-only lists in turn."""
    vc = view_case
    n, tabs, lengths = vc["n"], vc["tabs"], vc["lengths"]
    rng_ = _ranges(n, world)
    assert rng_[0][0] == 0 and rng_[-1][1] == n and all(a[1] == b[0] for a, b in zip(rng_, rng_[1:]))
    assert world == 1 or 0 < rng_[-1][1] - rng_[-1][0] <= rng_[0][1] - rng_[0][0]
    _dummy_count(gpu_ctx)
    d_tabs, d_ovf, n_ovf, pairs = _upload_whole(dev, tabs)
    which = range(len(FILTERS))
    parts = []
    for r, (lo, hi) in enumerate(rng_):
        o, no = (d_ovf, n_ovf) if r % 2 == 0 else _range_lists(dev, pairs, lo, hi)
        res = _filter_range(gpu_ctx, vc, [p + lo for p in d_tabs], o, no, lo, hi, lengths, tabs, which)
        for f in which:
            assert res[f]["ok"], (world, r, lo, hi, f, res[f]["n"], res[f]["exp_n"])
        parts.append(res)
    for f in which:
        w = vc["whole"][f]
        assert tuple(sum(p[f]["n"][i] for p in parts) for i in range(3)) == (w.n_union, len(w.keys), len(w.hist))
        keys = np.concatenate([p[f]["keys"] for p in parts])
        counts = np.concatenate([p[f]["counts"] for p in parts])
        o = np.argsort(keys, kind="stable")
        assert (keys[o] == w.keys).all() and (counts[o] == w.counts).all()


@pytest.mark.parametrize("lo,nview", [(4160, B + 1000 + 7), ((1 << 17) - 64, 37), (64 * 1000, 15), (B - 64, 64 + 16 + 9)])
def test_filter_view_ragged_range(gpu_ctx, dev, view_case, lo, nview):
    """Ranges whose length is no multiple of 16 (the byte-wise staging of a ragged end) at non-zero bases."""
    vc = view_case
    _dummy_count(gpu_ctx)
    d_tabs, d_ovf, n_ovf, pairs = _upload_whole(dev, vc["tabs"])
    for o, no in ((d_ovf, n_ovf), _range_lists(dev, pairs, lo, lo + nview)):
        res = _filter_range(gpu_ctx, vc, [p + lo for p in d_tabs], o, no, lo, lo + nview, vc["lengths"], vc["tabs"], (0, 3))
        for f, r in res.items():
            assert r["ok"], (lo, nview, f, r["n"], r["exp_n"])
    assert nview < 100 or res[0]["n"][1] > 0


def test_merge_then_filter(gpu_ctx, dev, view_case):
    """dist.py's sequence without processes: every chromosome arrives in 2-3 summand pieces, the pieces are merged on
    the device per slot range of 3 ranks (range 1 starts at slot 43712, not a multiple of 2^15), sp_table_lengths
    gives the lengths, sp_filter_view + sp_filter run over the merged bytes and merged lists."""
    vc = view_case
    n, tabs = vc["n"], vc["tabs"]
    rng = np.random.RandomState(61)
    pieces = []                                  # per chromosome 2-3 exact tables that add up to tabs[c]
    for c in range(NCHROM):
        rest, ps = tabs[c].astype(np.int64), []
        for _ in range(1 + c % 2):
            p = (rng.rand(n) * (rest + 1)).astype(np.int64)
            p = np.where(rng.rand(n) < 0.2, rest * (rng.rand(n) < 0.5), np.minimum(p, rest))   # all / nothing now and then
            ps.append(p.astype(np.uint32))
            rest = rest - p
        ps.append(rest.astype(np.uint32))
        assert 2 <= len(ps) <= 3 and (sum(x.astype(np.int64) for x in ps) == tabs[c]).all()
        pieces.append(ps)
    ranges = _ranges(n, 3)
    assert ranges[1][0] % B != 0 and ranges[1][0] % 64 == 0
    _dummy_count(gpu_ctx)
    # what every rank holds after the exchange: the pieces' byte tables and their whole-table overflow lists
    d_piece = []
    for ps in pieces:
        enc = [ref.encode(p, 0) for p in ps]
        d_piece.append([(dev.put_bytes(b),) + dev.put_pairs(q) for b, q in enc])
    lens = np.zeros(NCHROM, np.int64)
    unsorted, merged = [], []
    for r, (lo, hi) in enumerate(ranges):
        d_tabs, d_ovf, n_ovf = [], [], []
        for c in range(NCHROM):
            exp_bytes, exp_pairs = ref.encode(tabs[c][lo:hi], lo)
            if r == 1:      # the unaligned range has a crowded bucket that the absolute boundary at 65536 cuts
                per = ref.pairs_per_bucket(exp_pairs, lo, hi - lo)
                assert per[0] > 96 and (exp_pairs[:, 0] < 65536).sum() >= 30 and \
                    ((exp_pairs[:, 0] >= 65536) & (exp_pairs[:, 0] < lo + B)).sum() >= 30
            cap = len(exp_pairs) + 4
            # dst is a copy of the first piece's slice (the filter wants 16-byte aligned tables), src the others' in place
            d_dst = dev.put_bytes(ref.encode(pieces[c][0][lo:hi], lo)[0])
            d_lst, n_lst = d_piece[c][0][1], d_piece[c][0][2]
            for pi in range(1, len(pieces[c])):
                d_out = dev.new_list(cap)
                m = gpu_ctx.table_merge(d_dst, d_lst, n_lst, d_piece[c][pi][0] + lo, d_piece[c][pi][1], d_piece[c][pi][2],
                                        lo, hi - lo, d_out, cap)
                d_lst, n_lst = d_out, m
            got = dev.get_list(d_lst, n_lst, cap)
            assert n_lst == len(exp_pairs) and (dev.get_bytes(d_dst, hi - lo) == exp_bytes).all()
            if not np.all(np.diff(got[:, 0].astype(np.int64)) > 0):
                unsorted.append((r, c))
            else:
                assert (got == exp_pairs).all()
            s, m = gpu_ctx.table_lengths(d_dst, d_lst, n_lst, lo, hi - lo, LOWER)
            if (r, c) not in unsorted:
                assert (s, m) == ref.lengths(tabs[c][lo:hi], LOWER)
            lens[c] += ref.lengths(tabs[c][lo:hi], LOWER)[0]
            d_tabs.append(d_dst), d_ovf.append(d_lst), n_ovf.append(n_lst)
        merged.append((d_tabs, d_ovf, n_ovf))
    assert lens.tolist() == [ref.lengths(t, LOWER)[0] for t in tabs]
    # the filter twice: with the lengths just computed (dist.py's sequence), and with the hand-made near-equal lengths
    # under which the saturated rows sit on the fold threshold and come out as rows -- counts read from the merged lists
    from subphaser_amd import kmer as km
    results = []
    for lengths, which in ((lens, (0, 1)), (vc["lengths"], (0, 3))):
        parts = [_filter_range(gpu_ctx, vc, d_tabs, d_ovf, n_ovf, lo, hi, lengths, tabs, which)
                 for (lo, hi), (d_tabs, d_ovf, n_ovf) in zip(ranges, merged)]
        results.append((lengths, which, parts))
    bad_rows = [(li, r, f, x["n"], x["exp_n"]) for li, (_, _, parts) in enumerate(results) for r, p in enumerate(parts)
                for f, x in p.items() if not x["ok"]]
    assert not unsorted, "merged overflow lists are not ascending for (range, chromosome) %s; the filter's rows %s" % (
        unsorted, "differ from the oracle's: (lengths, range, filter, got, expected) %s" % bad_rows if bad_rows
        else "equal the oracle's all the same")
    assert not bad_rows, bad_rows
    for li, (lengths, which, parts) in enumerate(results):
        for f in which:
            sgs, kw = FILTERS[f]
            w = vc["whole"][f] if li else po.filter_dumps(_dumps_of(tabs, vc["keys_all"], 0, n), sgs, list(range(NCHROM)),
                                                          lengths=lengths, **kw)
            keys = np.concatenate([p[f]["keys"] for p in parts])
            o = np.argsort(keys, kind="stable")
            assert len(w.keys) > 0 and (keys[o] == w.keys).all()
            assert (np.concatenate([p[f]["counts"] for p in parts])[o] == w.counts).all()
            if li:      # rows whose counts came out of the merged lists of the unaligned range were part of the comparison
                big = (w.counts >= 255).any(axis=1)
                sl = km.slots_of_keys(w.keys[big], K).astype(np.int64)
                assert ((sl >= ranges[1][0]) & (sl < ranges[1][1])).sum() > 96


# -------------------------------------------------------------------------------- f. sp_count_range, bound tables
def _rand_seq(rng, n, p_other=0.001, lower=0.1):
    a = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=n)].copy()
    a[rng.random_sample(n) < lower] |= 0x20
    m = rng.random_sample(n) < p_other
    a[m] = np.frombuffer(b"NRYKMSWnx-", np.uint8)[rng.randint(0, 10, size=int(m.sum()))]
    return a


@pytest.fixture(scope="module")
def three_chroms():
    """three chromosomes of a few hundred kb, every one with counts above 255, one with a repeat family (hundreds of
    saturated slots); raw oracle counts as exact tables at k = 11"""
    from subphaser_amd import kmer as km
    rng = np.random.RandomState(29)
    k = 11
    s0 = _rand_seq(rng, 300_000)
    s0[1000:4000] = ord("A")
    s1 = _rand_seq(rng, 450_000)
    fam = _rand_seq(rng, 600, 0, 0)
    for p in 10_000 + 1000 * rng.permutation(430)[:400]:        # 400 copies that do not overlap: ~590 slots at 400
        s1[p:p + 600] = fam
    s2 = _rand_seq(rng, 200_001)
    s2[50_000:58_000] = np.frombuffer(b"ACGTTGCA" * 1000, np.uint8)
    seqs, exact, raw = [s0, s1, s2], [], []
    n = km.dense_slots(k)
    for s in seqs:
        keys, cnts = po.count(s, k, 1, nthreads=4)
        t = np.zeros(n, np.uint32)
        t[km.slots_of_keys(keys, k).astype(np.int64)] = cnts
        exact.append(t), raw.append((keys, cnts))
    assert all((t >= 255).any() for t in exact) and int((exact[1] >= 255).sum()) >= 300
    return dict(k=k, n=n, seqs=seqs, exact=exact, raw=raw)


@pytest.mark.parametrize("engine", [1, 2])
def test_count_range_bound_tables(gpu_ctx, dev, three_chroms, engine):
    """sp_count_range(0, 1) then (1, 3) into caller-bound tables: the first call leaves the tables of chromosomes 1-2
    alone, afterwards bytes and sp_table_overflow lists of all three are the oracle's counts in the wire format."""
    tc = three_chroms
    k, n, lower = tc["k"], tc["n"], 3
    d8 = [dev.alloc(n) for _ in range(3)]
    sentinel = np.full(n, FILL8, np.uint8)
    for p in d8:
        gpu_ctx.host_to_dev(p, sentinel)
    gpu_ctx.genome_reset(3)
    try:
        for c in range(3):
            gpu_ctx.tables_bind(c, d8[c])
            gpu_ctx.genome_add(c, tc["seqs"][c])

        def check(c):
            exp_bytes, exp_pairs = ref.encode(tc["exact"][c], 0)
            assert (gpu_ctx.dev_to_host(d8[c], n) == exp_bytes).all(), c
            m = gpu_ctx.table_overflow(c)
            assert m == len(exp_pairs) and m > 0, (c, m, len(exp_pairs))
            d_ov = dev.new_list(m)
            assert gpu_ctx.table_overflow(c, d_ov, m) == m
            gpu_ctx.sync()
            got = dev.get_list(d_ov, m, m)
            assert np.all(np.diff(got[:, 0].astype(np.int64)) > 0), "overflow list of chromosome %d is not ascending" % c
            assert (got == exp_pairs).all(), c

        gpu_ctx.count_range(k, lower, engine, 0, 1)
        check(0)
        for c in (1, 2):
            assert (gpu_ctx.dev_to_host(d8[c], n) == FILL8).all(), "count_range(0, 1) wrote the table of chromosome %d" % c
        gpu_ctx.count_range(k, lower, engine, 1, 3)
        for c in range(3):
            check(c)
        with pytest.raises(ValueError):
            gpu_ctx.table_overflow(1, dev.new_list(1), 1)          # capacity below the number of pairs
        lens = gpu_ctx.lengths()
        for c in range(3):
            keys, cnts = tc["raw"][c]
            keep = cnts >= lower
            assert int(lens[c]) == int(cnts[keep].astype(np.int64).sum()) == ref.lengths(tc["exact"][c], lower)[0]
            gk, gc = gpu_ctx.dump(c)
            assert (gk == keys[keep]).all() and (gc == cnts[keep]).all()
    finally:
        for c in range(3):
            gpu_ctx.tables_bind(c, None)
