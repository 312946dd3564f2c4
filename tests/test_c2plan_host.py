"""The host planning of the k <= 15 partition chain (subphaser_amd/csrc/sp_c2plan.h), checked on the host.

tests/c2plan_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP
types) and compares it with values worked out by hand from its rules: the plan at 2^17, 2^18, 2^28 and 2^29 slots and
the table sizes it refuses (2^16, 2^30, no power of two); the sizing of a 20-Mb chromosome at 2^29 slots in estimate
and exact mode and under each override, of chromosomes of 1 to 32769 bases at 2^17 slots (shorter than one stripe, one
stripe more, one sampled stripe more) and on both sides of the two slack clamps; the workspace layout's offsets for
those, that its arrays are 256-byte aligned, in order and without overlap or hole, that the cursors of level 1 take
1024 lines whatever the fan-out, and that the per-chromosome and the batched use see the same offsets; the lane-fit
rule, the negative budget included."""
import host_check


def test_c2_plan_matches_the_hand_worked_values(tmp_path):
    assert host_check.ok_count(host_check.run(tmp_path, "c2plan_host_check")) > 300
