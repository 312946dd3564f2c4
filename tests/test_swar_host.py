"""The two-counters-per-word arithmetic of c2_count16's write-out (subphaser_amd/csrc/sp_swar.h), checked on the host.

tests/swar_host_check.cpp is compiled against the header with the host C++ compiler and compares every helper with the
slot-by-slot definition: both halves of a word over {0, 1, lower-1, lower, lower+1, 254, 255, 256, 0x7FFF, 0x8000,
0xFFFF} crossed with each other, all 2^16 values of one half against each of those in the other half, for `lower` in
{1, 2, 3, 254, 255, 256, 0x7FFF, 0x8000}; 0x8001 and 70000 must be left to the per-slot code (SP_SWAR_MAX_LOWER)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_swar_helpers_match_the_per_slot_definition(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++ or $CXX) on PATH")
    exe = tmp_path / "swar_host_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "subphaser_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "swar_host_check.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK" and int(last[1]) > 8 * 11 * 2 * 65536
