"""The two-counters-per-word arithmetic of c2_count16's write-out (subphaser_amd/csrc/sp_swar.h), checked on the host.

tests/swar_host_check.cpp is compiled against the header with the host C++ compiler and compares every helper with the
slot-by-slot definition: both halves of a word over {0, 1, lower-1, lower, lower+1, 254, 255, 256, 0x7FFF, 0x8000,
0xFFFF} crossed with each other, all 2^16 values of one half against each of those in the other half, for `lower` in
{1, 2, 3, 254, 255, 256, 0x7FFF, 0x8000}; 0x8001 and 70000 must be left to the per-slot code (SP_SWAR_MAX_LOWER)."""
import host_check


def test_swar_helpers_match_the_per_slot_definition(tmp_path):
    assert host_check.ok_count(host_check.run(tmp_path, "swar_host_check")) > 8 * 11 * 2 * 65536
