"""The choice and sizing of the label table of sp_labels_set (subphaser_amd/csrc/sp_labelplan.h), checked on the host.

tests/labelplan_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP
types) and compares the plan with values worked out by hand from its rules: which of the six kinds (direct, compact,
label bytes at k <= 15; quad, pair hash, per-k-mer hash at k > 15) a (k, n, S) and the three switches SP_MAP_ENGINE,
SP_CTAB, SP_CTAB_FACTOR lead to, on both sides of every threshold -- the 64 MiB of the direct table, bb against sb and
27, 3 / 7 subgenomes, k = 5 --, the bucket bits, the bytes of the buckets and of the overflow table, the hash capacity,
the k = 31 / 32 tables as they are today, the fallback of a full overflow table; over a sweep of (k, n, S, switches)
that the sizes are powers of two, that a bucket table's tag fits its field and that the fallback is the plan of
SP_CTAB=0; and how the switches are read from the environment.  The same program is built and run once more with
-fsanitize=address,undefined."""
import pytest

import host_check


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_label_plan_matches_the_hand_worked_values(tmp_path, flags):
    assert host_check.ok_count(host_check.run(tmp_path, "labelplan_host_check", flags=flags)) > 100000
