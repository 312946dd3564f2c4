"""The host planning of the list filter's join (subphaser_amd/csrc/sp_listplan.h), checked on the host.

tests/listplan_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP
types) and compares the plan with values worked out by hand from its rules: the range plan (bits, rb, shift, R,
per_range) at k = 32 / 31 / 24 / 17 / 16 with a handful of k-mers -- `key >> 64` is no shift: the k32_join fuzz case --,
in list mode, at the cap of 2^23 ranges and on both sides of the 64-list limit of sps_join_blk, with the ranges covering
the key space every time; the row-cap policy; the fast walk's descriptors and each way the walk is switched off; the
set masks and when the screen is off; the wide kernel's set CSR; the passenger path's renumbering."""
import host_check


def test_list_plan_matches_the_hand_worked_values(tmp_path):
    assert host_check.ok_count(host_check.run(tmp_path, "listplan_host_check")) > 300
