"""The plain byte-table reference (tests/bytetab_ref.py) and the CPU twin of the table exchange
(tests/oracle_ctx.py, what the gloo tests of dist.py run on) check each other on host buffers: the GPU tests of
tests/test_gpu_table_exchange.py then compare sp_table_merge / sp_table_lengths with the reference alone."""
import numpy as np
import pytest

import bytetab_ref as ref
from oracle_ctx import OracleDistContext

B = ref.BUCKET
SHAPES = [(0, 3 * B), (64, B), (11184832, 2 * B + 4160), ((1 << 29) - (B + 64), B + 64), (32767, 1), (64, 0)]


def _ptr(a):
    return a.ctypes.data if a.size else 0


@pytest.mark.parametrize("slot_base,n", SHAPES)
def test_encode_decode_roundtrip(slot_base, n):
    A, _, _ = ref.make_summands(1, slot_base, n)
    b, p = ref.encode(A, slot_base)
    assert b.dtype == np.uint8 and p.dtype == np.uint32 and p.shape == (int((A >= 255).sum()), 2)
    assert (b == np.minimum(A, 255)).all()
    assert (np.diff(p[:, 0].astype(np.int64)) > 0).all() and (p[:, 1] >= 255).all()
    assert (p[:, 0].astype(np.int64) - slot_base == np.flatnonzero(A >= 255)).all()
    assert (ref.decode(b, p, slot_base, n) == A).all()
    whole = ref.with_outside(p, slot_base, n, 5)
    assert (np.diff(whole[:, 0].astype(np.int64)) > 0).all() and len(whole) >= len(p)
    assert (ref.decode(b, whole, slot_base, n) == A).all()        # a list may cover more than the range


def test_decode_rejects_inconsistent_tables():
    b, p = ref.encode(np.array([3, 255, 900, 0], np.uint32), 64)
    with pytest.raises(AssertionError):
        ref.decode(b, p[:1], 64, 4)                               # a saturated byte without its pair
    with pytest.raises(AssertionError):
        ref.decode(np.array([3, 255, 254, 0], np.uint8), p, 64, 4)   # a pair on an unsaturated byte


@pytest.mark.parametrize("slot_base,n", SHAPES)
def test_summands_cover_what_they_promise(slot_base, n):
    """The generated inputs do have the crowded / light / empty buckets and the summand classes they name."""
    A, Bt, info = ref.make_summands(3, slot_base, n)
    tot = ref.add(A, Bt)
    _, pairs = ref.merge(A, Bt, slot_base)
    per = ref.pairs_per_bucket(pairs, slot_base, n)
    if n >= 1024:
        assert per[info["crowded"]] > 96
        sat_a, sat_b = A >= 255, Bt >= 255
        assert (~sat_a & ~sat_b & (tot >= 255)).any() and (tot == 254).any() and (tot == 255).any()
        assert (sat_a & ~sat_b).any() and (~sat_a & sat_b).any() and (sat_a & sat_b).any() and (tot > 65535).any()
    if info["boundary"] is not None:
        loc = pairs[:, 0].astype(np.int64) - slot_base
        in_b = loc // B == info["crowded"]
        assert (in_b & (loc < info["boundary"])).sum() > 30 and (in_b & (loc >= info["boundary"])).sum() > 30
    if info["light"] is not None:
        assert 1 <= per[info["light"]] <= 96
    if info["empty"] is not None:
        assert per[info["empty"]] == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("slot_base,n", SHAPES)
def test_twin_merge_and_lengths_equal_reference(seed, slot_base, n):
    A, Bt, _ = ref.make_summands(seed, slot_base, n)
    ba, pa = ref.encode(A, slot_base)
    bb, pb = ref.encode(Bt, slot_base)
    if seed % 2:                                                  # whole-table input lists
        pa, pb = ref.with_outside(pa, slot_base, n, seed + 10), ref.with_outside(pb, slot_base, n, seed + 20)
    exp_bytes, exp_pairs = ref.merge(A, Bt, slot_base)
    cap = len(exp_pairs) + 3
    out = np.full((cap, 2), 0xEEEEEEEE, np.uint32)
    dst, src = ba.copy(), bb.copy()
    ctx = OracleDistContext()
    m = ctx.table_merge(_ptr(dst), _ptr(pa), len(pa), _ptr(src), _ptr(pb), len(pb), slot_base, n, _ptr(out), cap)
    assert m == len(exp_pairs)
    assert (dst == exp_bytes).all() and (src == bb).all()
    assert (out[:m] == exp_pairs).all() and (out[m:] == 0xEEEEEEEE).all()
    assert (ref.decode(dst, out[:m], slot_base, n) == ref.add(A, Bt)).all()
    more = ref.with_outside(out[:m], slot_base, n, seed + 30)
    for lower in (0, 1, 3, 255, 256, 70000):
        assert ctx.table_lengths(_ptr(dst), _ptr(more), len(more), slot_base, n, lower) == \
            ref.lengths(ref.add(A, Bt), lower), lower


def test_twin_merge_capacity():
    A, Bt, _ = ref.make_summands(4, 64, B)
    ba, pa = ref.encode(A, 64)
    bb, pb = ref.encode(Bt, 64)
    need = len(ref.merge(A, Bt, 64)[1])
    out = np.zeros((need, 2), np.uint32)
    with pytest.raises(MemoryError):
        OracleDistContext().table_merge(_ptr(ba), _ptr(pa), len(pa), _ptr(bb), _ptr(pb), len(pb), 64, B, _ptr(out),
                                        need - 1)
