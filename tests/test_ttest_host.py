"""The bit-exact pieces of the wide k-mer t-test (subphaser_amd/csrc/sp_ttest.h), checked on the host.

tests/ttest_host_check.cpp is compiled against the header with the host C++ compiler (-ffp-contract=off, as the library is
built).  It must reproduce np.sum bit for bit through the streaming pairwise accumulator -- every length in 1..1100 and
the lengths around 4096, 8192 and 65536, magnitudes from 1e-9 to 1e3, one all-positive and one signed vector per length --
and its sp_tt_pvalue(df, t) must lie within the tolerances of tests/hp_reference.py of mpmath's regularised incomplete
beta for 400 values of t at each df in {1, 2, 3, 10, 127, 129, 1000, 4094, 16382, 65534, 200000}."""
import struct

import mpmath as mp
import numpy as np
import pytest

import host_check
import hp_reference as hr

SIZES = list(range(1, 1101)) + [4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536]
DFS = [1, 2, 3, 10, 127, 129, 1000, 4094, 16382, 65534, 200000]
# 400 per df: |t| over ten decades up to 60 (well beyond, at the larger df, p is so far below the doubles that mpmath's series
# gives up), and evenly from 0 (p = 1) to 45, where p has left the doubles at the larger df
TS = np.concatenate([np.geomspace(1e-8, 60.0, 200), np.linspace(0.0, 45.0, 200)])


def _p_mp(df, t):
    """I_x(df / 2, 1 / 2), x = df / (df + t^2), rounded to fp64 (hp_reference.ttest_p_mp for a given t)"""
    with mp.workdps(hr.DPS):
        tt = mp.mpf(float(t)) ** 2
        return hr.to_f64(mp.betainc(mp.mpf(df) / 2, mp.mpf(1) / 2, 0, df / (df + tt), regularized=True))


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ttest_host")
    rng = np.random.RandomState(65536)
    blob = [struct.pack("=q", 2 * len(SIZES))]
    for n in SIZES:
        for signed in (False, True):
            a = 10.0 ** rng.uniform(-9, 3, size=n)
            if signed:
                a *= rng.choice([-1.0, 1.0], size=n)
            a = np.ascontiguousarray(a, np.float64)
            blob += [struct.pack("=qd", n, float(np.sum(a))), a.tobytes()]
    pairs = np.array([(df, t) for df in DFS for t in TS], np.float64)
    blob += [struct.pack("=q", len(pairs)), pairs.tobytes()]
    data = tmp / "vectors.bin"
    data.write_bytes(b"".join(blob))
    r = host_check.run(tmp, "ttest_host_check", [data], flags=["-ffp-contract=off"], libs=["-lm"])
    return r, pairs


def test_streaming_sum_is_numpys(host_run):
    r, _ = host_run
    lines = r.stdout.splitlines()
    head = [l for l in lines if not l.startswith("P ")]
    print("\n".join(head[:40]))
    assert r.returncode == 0, "\n".join(head[:40])
    sums = [l for l in lines if l.startswith("SUMS ")][0].split()
    assert int(sums[1]) == 2 * len(SIZES) and int(sums[2]) == 0
    depth = [l for l in lines if l.startswith("DEPTH ")][0].split()
    assert int(depth[1]) <= int(depth[3])


def test_pvalue_against_mpmath(host_run):
    r, pairs = host_run
    got = np.array([[float(v) for v in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("P ")])
    assert got.shape == (len(pairs), 3) and (got[:, :2] == pairs).all()
    ref = np.array([_p_mp(df, t) for df, t in pairs])
    ok = hr.tail_ok(got[:, 2], ref)
    for df in DFS:
        m = pairs[:, 0] == df
        mid = m & (ref >= hr.TINY) & (ref <= 0.5)
        print("df = %6d: %3d of %d outside, worst relative error %.2e" % (
            df, int((~ok[m]).sum()), int(m.sum()),
            float((np.abs(got[mid, 2] - ref[mid]) / ref[mid]).max()) if mid.any() else 0.0))
    assert ok.all(), [(pairs[i, 0], pairs[i, 1], got[i, 2], ref[i]) for i in np.nonzero(~ok)[0][:8]]
    # the set reaches what it is meant to: p = 1, the complement branch, far tails, denormals and 0
    assert (ref == 1.0).any() and ((ref > 0.5) & (ref < 1)).any() and ((ref > 0) & (ref < 1e-280)).any()
    assert ((ref > 0) & (ref < 2.2250738585072014e-308)).any() and (ref == 0).any()
