"""The host-clean part of the k-mer tests' shared driver (subphaser_amd/csrc/sp_ktlayout.h), checked on the host.

tests/kmertest_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP
types).  The workspace layout on a null base at M = 1 and 129, C = 6, G = 1, 2, 3, rows on the host or on the device, with
and without a statistic and an extra array of the entry's own: every array starts at a 256-byte multiple, the arrays
follow one another without overlap, the total is the end of the last array, rows on the device take no room, and the sizing
and the placing pass hand out the same offsets.  The group check's verdicts on hand-made lists."""
import host_check


def test_kmertest_layout_and_group_check(tmp_path):
    assert host_check.ok_count(host_check.run(tmp_path, "kmertest_host_check")) > 1500
