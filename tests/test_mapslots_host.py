"""The integer rules of the map stage's walk modes (subphaser_amd/csrc/sp_mapslots.h), checked on the host.

tests/mapslots_host_check.cpp is compiled against the header with the host C++ compiler alone.  Every reference in it is a
loop over single starts or single bits, never the closed form under test.
  bins      k = 15 | 17, bins 1 .. 10 000, chunks 0 | 40 | 1000 | 5000, lengths of a few thousand bases at and one off a multiple of
            the bin, the chunk and the unit (and three bins of a whole range of MAP_RANGE starts and more: only those make
            the one-slot shortcut true).  Every valid start's slot is bin + chunk and lies below map_nslots_host; the
            map_slot_end pieces of every unit tile it, each piece is the starts of one slot and ends where the slot does;
            per range, the one-slot shortcut holds exactly when the range has one slot, and wherever map_params_of chooses
            the LDS histogram, (slot - slot_lo) * S + S <= MAP_LDS_ENTRIES for every start of the range, S = 1 .. 7.  Those
            geometries lie far from the LDS rule's edge, so for every S the smallest bin that gets the histogram and the
            next one are checked as well, with and without chunks (a rule with + 1 in place of + 3 fails there).
  stack     map_chunk_of_slot gives the forward chunk for every slot map_slot produces at those geometries.
  features  random offset lists with empty features, features shorter than k and features of several units: bit j of
            map_unit_fit is "the k-mer at s0 + j lies inside one feature" by a scan from the front; the cursor
            map_feat_locate, fed every start in order and then a random subset in order, agrees and names the same feature.
  planes    map_plane_mask against a decode per bit for labels 1 .. 7; map_span for every 0 <= a, b <= 64."""
import pytest

import host_check


@pytest.mark.parametrize("what,at_least", [("bins", 10 ** 7), ("stack", 10 ** 6), ("features", 10 ** 5), ("planes", 65 * 65 + 7 * 2000)])
def test_map_arithmetic(tmp_path, what, at_least):
    assert host_check.ok_count(host_check.run(tmp_path, "mapslots_host_check", [what])) >= at_least
