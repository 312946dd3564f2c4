"""The parse of the SP_CU_LIMIT switch (subphaser_amd/csrc/sp_culimit.h), checked on the host.

tests/culimit_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP
types): unset, empty, garbage (signs, white space, trailing text, fractions, hexadecimal), 0, negative, the device's own
count and anything above it -- a value that would wrap a 32-bit integer included -- leave the count alone; every integer
1 <= n < count replaces it."""
import host_check


def test_cu_limit_parse(tmp_path):
    assert host_check.ok_count(host_check.run(tmp_path, "culimit_host_check")) > 600
