"""The hash functions of the map stage (subphaser_amd/csrc/sp_maphash.h), checked on the host.

tests/maphash_host_check.cpp is compiled against the header with the host C++ compiler.  Its reference is the family the
filter had before the 24-bit one (multiplies of 32 x 32 bits), copied into the program verbatim.
  mix        map_ct_mix on 24-bit multiplies gives the bits of the 32-bit form: every x for kb = 2..16 (and a bijection
             there), 2^20 random x for each of kb = 17..24; kb > 24 keeps the 32-bit form.
  probe K    10^5 random k-mers, inserted as k4_pair_filter inserts them, are found from both strands through map_bloom,
             with and without core addressing; the chain form of the rolled walk (map_chain_start24 + map_quad_probes24: cores a, b, c
             of consecutive pairs, the carried hash) gives the word and the bits of the generic form for every pair of 25 000 quads of a
             random sequence and of its reverse complement.
  quality K  the filter model the family was chosen on, fixed seed: the canonical (k-1)-mers of 36 random "repeat"
             sequences are the label set, the unlabelled (k-1)-mers at every second start of a random sequence (1.97 M
             starts) the probes, the filter has the size sp_map_filter_build would choose (2^24 bits at k = 15).  Repeats
             of 60 kb at k = 15 and 13; at k = 11 there are only 524 800 canonical 10-mers, and 36 x 4 kb label the same
             quarter of them as 36 x 60 kb do of the 12-mers at k = 13.  The 24-bit family's false positives per pair are
             at most the old family's, its word-load variance / mean at most 1.05 times the old family's (sampling slack
             on ~5 x 10^5 words).  Measured (old -> new): k = 15 0.0757 -> 0.0582 and 1.99 -> 1.82, k = 13 0.2378 -> 0.1771
             and 6.14 -> 5.90, k = 11 0.2520 -> 0.1970 and 6.42 -> 6.30 (profiles/map_hash_notes.md)."""
import pytest

import host_check


def test_table_mix_keeps_its_bits(tmp_path):
    n = sum(1 << kb for kb in range(2, 17))
    assert host_check.ok_count(host_check.run(tmp_path, "maphash_host_check", ["mix"])) >= 3 * n + 2 * 8 * (1 << 20)


@pytest.mark.parametrize("k", (5, 6, 8, 11, 13, 14, 15))
def test_no_false_negatives_and_chain_equals_generic(tmp_path, k):
    # per mode 2 x 10^5 insert checks + 4 x 10^5 probes; 2 x 25 000 quads x 2 checks
    assert host_check.ok_count(host_check.run(tmp_path, "maphash_host_check", ["probe", k])) >= 2 * 600000 + 100000


@pytest.mark.parametrize("k", (15, 13, 11))
def test_filter_quality_against_the_old_family(tmp_path, k):
    r = host_check.run(tmp_path, "maphash_host_check", ["quality", k])
    assert host_check.ok_count(r) >= 4
