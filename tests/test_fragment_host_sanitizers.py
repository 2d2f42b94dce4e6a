"""The fragment step's host twin under AddressSanitizer and
UndefinedBehaviorSanitizer (CPU only): tests/cpp/fragment_check.cpp, a
stand-alone program, drives gevws_fragment_records (gev_amd/csrc/
gevws_fragment_host.cpp, the rule of gevws_fragment.hpp) over random and edge
record lists into heap blocks of exactly the contract's sizes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_fragment_check_asan_ubsan(tmp_path):
    exe = tmp_path / "fragment_check"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "fragment_check.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_fragment_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "fragment_check ok" in r.stdout, r.stdout + r.stderr
