"""The plan and the thresholds of the k = 16..32 count chain (subphaser_amd/csrc/sp_s3plan.h), checked on the host.

tests/s3plan_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP types) and
compares s3_make_plan at every k = 16..32 with hand-worked values -- B2 = 8 up to k = 17 and 9 above, R1 = 32 at k = 21,
R2 = 31 / 33 on the two sides of the 64-bit residuals, 45 at k = 32, never 32 or 64 (so the all-ones EMPTY marker of the hash
tables is never a residual) -- and s3_split_bits with the split widths worked out by hand at the bucket sizes the hand-made
chromosomes use.  It then prints every threshold; they must equal the literals the routing model of tests/s3_cases.py is
written with, so a threshold that moves without the cases fails here, on the CPU."""
import host_check
import s3_cases as sc


def test_s3_plan_and_thresholds_match_the_cases(tmp_path):
    r = host_check.run(tmp_path, "s3plan_host_check")
    assert host_check.ok_count(r) > 200
    shown = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) == 2 and f[0].startswith("S3"):
            shown[f[0]] = int(f[1])
    assert shown == sc.LIT
    for k in range(16, 33):
        for n in (2049, 3074, 4097, 6000, 65536, 1 << 19, (1 << 22) + 1):
            assert sc.split_bits(n, sc.Plan(k).R2) == {2049: 1, 3074: 2, 4097: 2, 6000: 3, 65536: 6, 1 << 19: 8, (1 << 22) + 1: 8}[n]
