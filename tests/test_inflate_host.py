"""The DEFLATE decode core as the host sees it, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/inflate_fuzz.cpp, a stand-alone program
that runs mutated and random streams through gev_amd/csrc/gevws_inflate_core.hpp
and gevws_inflate_raw.  Malformed streams meet this build before the device's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_inflate_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "inflate_fuzz"
    r = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "inflate_fuzz.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "inflate_fuzz ok" in r.stdout, r.stdout + r.stderr
