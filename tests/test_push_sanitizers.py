"""The push pass's record rule under AddressSanitizer and
UndefinedBehaviorSanitizer (CPU only): tests/cpp/push_fuzz.cpp, a stand-alone
program, drives gevws_push_check (gev_amd/csrc/gevws_push_host.cpp, the rule of
gevws_push.hpp) over mutated and random record lists, each at the end of a heap
block of exactly its size."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_push_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "push_fuzz"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "push_fuzz.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_push_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "push_fuzz ok" in r.stdout, r.stdout + r.stderr
