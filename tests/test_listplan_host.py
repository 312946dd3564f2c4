"""The host planning of the list filter's join (subphaser_amd/csrc/sp_listplan.h), checked on the host.

tests/listplan_host_check.cpp is compiled against the header with the host C++ compiler alone (the header uses no HIP
types) and compares the plan with values worked out by hand from its rules: the range plan (bits, rb, shift, R,
per_range) at k = 32 / 31 / 24 / 17 / 16 with a handful of k-mers -- `key >> 64` is no shift: the k32_join fuzz case --,
in list mode, at the cap of 2^23 ranges and on both sides of the 64-list limit of sps_join_blk, with the ranges covering
the key space every time; the row-cap policy; the fast walk's descriptors and each way the walk is switched off; the
set masks and when the screen is off; the wide kernel's set CSR; the passenger path's renumbering."""
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


def test_list_plan_matches_the_hand_worked_values(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++ or $CXX) on PATH")
    exe = tmp_path / "listplan_host_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "subphaser_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "listplan_host_check.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK" and int(last[1]) > 300
