"""The outbound compressor as the host sees it: gevws_deflate_raw, the twin of
the device's deflate step (one core, gev_amd/csrc/gevws_deflate_core.hpp).

Round trips through zlib's raw inflate with the window the message was
compressed for (zlib rejects a distance beyond 2^N, which pins the distance
limit) and through gevws_inflate_raw; the bound; the size conditions of the
corpus kinds; and tests/cpp/deflate_fuzz.cpp, a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer.  The sizes against zlib level
1 Z_FIXED are printed (pytest -s): the algorithm is deterministic, DESIGN 5.7
records that line, and later changes are judged against it."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import gev_amd
from tests._inflate_corpus import sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
TAIL = b"\x00\x00\xff\xff"
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 70000,
         300000)


def _zlib_accepts(n: int) -> bool:
    try:
        zlib.decompressobj(-n).decompress(b"\x00" + TAIL)
        return True
    except (zlib.error, ValueError):
        return False


# zlib's raw inflate takes window_bits 8 here if it can be opened with it; else the check starts at 9
WBITS = (0,) + tuple(range(8 if _zlib_accepts(8) else 9, 16))


def _zfixed(data: bytes, level: int = 1, strategy: int = zlib.Z_FIXED) -> int:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return len(c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)) - 4


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(0xDEF1A7E)
    return [(n, kind, sample(rng, n, kind)) for n in SIZES for kind in range(4)]


def test_zlib_pins_the_distance_limit():
    """The check the round trips rest on: zlib's raw inflate refuses a stream
    whose distances pass its window."""
    data = sample(np.random.default_rng(5), 70000, 0)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    s = c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)
    for n in (9, 12):
        with pytest.raises(zlib.error):
            zlib.decompressobj(-n).decompress(s)


def test_round_trip_every_window(corpus):
    for n, kind, data in corpus:
        for wb in WBITS:
            p = gev_amd.deflate_raw(data, wb)
            assert len(p) <= gev_amd.deflate_bound(n), (n, kind, wb)
            assert zlib.decompressobj(-(wb or 15)).decompress(p + TAIL) == data, (n, kind, wb)
            st, back = gev_amd.inflate_raw(p, n + 1)
            assert st == gev_amd.MSG_OK and back == data, (n, kind, wb)
    assert gev_amd.deflate_raw(b"") == b"\x00"


def test_window_bits_limit_the_distance():
    """A period longer than the window: nothing of it may be referenced, and
    zlib's inflate with that window takes the result."""
    rng = np.random.default_rng(11)
    period = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    data = period * 12
    sizes = {}
    for wb in (8, 9, 10, 11, 12, 13, 15):
        p = gev_amd.deflate_raw(data, wb)
        if wb in WBITS:
            assert zlib.decompressobj(-wb).decompress(p + TAIL) == data
        assert gev_amd.inflate_raw(p, len(data))[1] == data
        sizes[wb] = len(p)
    assert sizes[11] > len(data) and sizes[12] < len(data) // 4, sizes  # 2 048 < 3 000 <= 4 096


def test_bound():
    for n in list(range(0, 10000, 7)) + [2 ** 16, 2 ** 20 + 1, 2 ** 32 - 1]:
        b = gev_amd.deflate_bound(n)
        assert n < b <= n + n // 512 + 16, n
    rng = np.random.default_rng(3)
    for n in (1, 100, 2559, 2560, 4096, 4097, 8192, 8193, 50000):  # random bytes: stored blocks, within the bound
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert n < len(gev_amd.deflate_raw(data)) <= gev_amd.deflate_bound(n), n


def test_size_conditions_and_recorded_sizes(corpus):
    tot = {k: [0, 0, 0] for k in range(4)}
    for n, kind, data in corpus:
        c = len(gev_amd.deflate_raw(data))
        assert c <= gev_amd.deflate_bound(n)
        if n >= 4096:
            if kind in (2, 3):
                assert c < n // 8, (n, kind, c)
            if kind == 0:
                assert c < n, (n, kind, c)
            tot[kind][0] += n
            tot[kind][1] += c
            tot[kind][2] += _zfixed(data)
    for kind, (n, c, z) in tot.items():
        print(f"deflate sizes, kind {kind}, n >= 4096: plain {n}  ours {c} ({c / n:.4f})  "
              f"zlib-1 Z_FIXED {z} ({z / n:.4f})  ours/zlib {c / z:.3f}")


def test_errors():
    with pytest.raises(RuntimeError):
        gev_amd.deflate_raw(b"abc", 7)
    with pytest.raises(RuntimeError):
        gev_amd.deflate_raw(b"abc", 16)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_deflate_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "deflate_fuzz"
    r = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "deflate_fuzz.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_deflate_host.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "deflate_fuzz ok" in r.stdout, r.stdout + r.stderr
