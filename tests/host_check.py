"""Builds and runs the stand-alone host checks (tests/*_host_check.cpp): programs with their own main() that include a
header of subphaser_amd/csrc, compiled with the host C++ compiler alone and run on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def run(tmp, name, args=(), flags=(), libs=()):
    """Compile tests/<name>.cpp into `tmp` (-std=c++17 -O1 -Wall -Werror -I csrc, plus `flags` and `libs`) and run it
    with `args`, 300 s at most: the finished process, stderr folded into its text stdout.  Skips without a compiler."""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++ or $CXX) on PATH")
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", *flags, "-Wall", "-Werror", "-I", os.path.join(ROOT, "subphaser_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", name + ".cpp"), *libs])
    return subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def ok_count(r):
    """the number of checks of a program that ends with "OK <checks>"; it must have exited with status 0"""
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK"
    return int(last[1])
