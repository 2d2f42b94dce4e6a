"""The outbound compressor with GEVWS_DEFLATE_DYNAMIC as the host sees it:
gevws_deflate_raw_flags, the twin of the device's deflate step with that flag
(one core, gev_amd/csrc/gevws_deflate_core.hpp).

The corpus is that of tests/test_deflate_host.py (same seed, sizes, kinds,
windows).  Round trips through zlib's raw inflate with the message's window
and through gevws_inflate_raw; never longer than without the flag; a dynamic
block is really sent; the size conditions per kind; the edge messages the
decoders are strict about; flags 0 unchanged; and
tests/cpp/deflate_dynamic_fuzz.cpp under AddressSanitizer and
UndefinedBehaviorSanitizer.  The sizes against zlib level 1 (default strategy
and Z_FIXED) are printed (pytest -s): DESIGN 5.7 records that line, and later
matcher changes are judged against it."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import gev_amd
from tests._inflate_corpus import sample
from tests.test_deflate_host import ROOT, SAN, SIZES, TAIL, WBITS, _zfixed

DYN = gev_amd.DEFLATE_DYNAMIC


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(0xDEF1A7E)
    return [(n, kind, sample(rng, n, kind)) for n in SIZES for kind in range(4)]


@pytest.fixture(scope="module")
def sizes(corpus):
    """[(n, kind, fixed-mode length, dynamic-mode length)], computed once."""
    return [(n, kind, len(gev_amd.deflate_raw(d)), len(gev_amd.deflate_raw(d, 0, DYN))) for n, kind, d in corpus]


def btype(p: bytes) -> int:
    """BTYPE of the payload's first block: bits 1 and 2 (bit 0 is BFINAL)."""
    return (p[0] >> 1) & 3


def both_decoders(data: bytes, wb: int = 0) -> bytes:
    p = gev_amd.deflate_raw(data, wb, DYN)
    assert len(p) <= gev_amd.deflate_bound(len(data))
    assert zlib.decompressobj(-(wb or 15)).decompress(p + TAIL) == data
    st, back = gev_amd.inflate_raw(p, len(data) + 1)
    assert st == gev_amd.MSG_OK and back == data
    return p


def test_round_trip_every_window(corpus):
    for n, kind, data in corpus:
        for wb in WBITS:
            p = gev_amd.deflate_raw(data, wb, DYN)
            assert len(p) <= gev_amd.deflate_bound(n), (n, kind, wb)
            assert zlib.decompressobj(-(wb or 15)).decompress(p + TAIL) == data, (n, kind, wb)
            st, back = gev_amd.inflate_raw(p, n + 1)
            assert st == gev_amd.MSG_OK and back == data, (n, kind, wb)
    assert gev_amd.deflate_raw(b"", 0, DYN) == b"\x00"


def test_never_longer_than_fixed(sizes):
    for n, kind, f, d in sizes:
        assert d <= f, (n, kind, f, d)


def test_a_dynamic_block_is_really_sent(corpus):
    sent = [n for n, kind, data in corpus if kind == 0 and n and btype(gev_amd.deflate_raw(data, 0, DYN)) == 2]
    assert sent, "no text message begins with a BTYPE 10 block"
    for n, kind, data in corpus:  # and never without the flag
        if n:
            assert btype(gev_amd.deflate_raw(data)) in (0, 1), (n, kind)


def test_size_conditions_and_recorded_sizes(corpus, sizes):
    tot = {k: [0, 0, 0, 0, 0] for k in range(4)}
    for (n, kind, data), (_, _, f, d) in zip(corpus, sizes):
        if n >= 4096:
            t = tot[kind]
            t[0] += n
            t[1] += f
            t[2] += d
            t[3] += _zfixed(data, 1, zlib.Z_DEFAULT_STRATEGY)
            t[4] += _zfixed(data)
    for kind, (n, f, d, z, zf) in tot.items():
        print(f"deflate sizes, dynamic, kind {kind}, n >= 4096: plain {n}  fixed {f}  dynamic {d} ({d / f:.4f} x fixed)  "
              f"zlib-1 default {z} (ours/zlib {d / z:.3f})  zlib-1 Z_FIXED {zf} (ours/zlib {d / zf:.3f})")
    assert tot[0][2] <= 0.75 * tot[0][1], tot[0]  # text
    assert tot[3][2] <= 0.90 * tot[3][1], tot[3]  # short periods
    assert tot[1][2] <= tot[1][1] and tot[2][2] <= tot[2][1], (tot[1], tot[2])  # random, long runs


def de_bruijn(k: int, n: int) -> bytes:
    """The de Bruijn sequence B(k, n): every n-gram over k values exactly once (cyclically)."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(seq)


def edge_messages():
    """[(name, bytes)], also the GPU test's edge batch.  "4 096 bytes without a
    repeated 4-gram over 3 values" cannot exist (3^4 = 81 four-grams), so the
    case is split: B(3, 4), 84 bytes over 3 values without a repeated 4-gram
    (its 3-grams repeat, so it may have matches), and 4 096 bytes of B(16, 3)
    over 16 values: no 3-gram repeats, so the run has no match at all."""
    rng = np.random.default_rng(0xED6E)
    fib = [1, 1]
    while fib[-1] < 987:
        fib.append(fib[-1] + fib[-2])
    fibs = np.repeat(np.arange(len(fib), dtype=np.uint8) * 11 + 40, fib)
    rng.shuffle(fibs)
    b3 = de_bruijn(3, 4)
    b16 = de_bruijn(16, 3)
    return [
        ("a", b"a"),
        ("ab", b"ab"),
        ("one byte x 4096", b"\x5a" * 4096),
        ("256 distinct", bytes(range(256))),
        ("B(3,4)", bytes(65 + x for x in b3 + b3[:3])),
        ("B(16,3)", bytes(48 + 3 * x for x in b16)[:4096]),
        ("one match", bytes(range(40, 240)) + bytes(range(90, 100))),
        ("fibonacci", fibs.tobytes()),
        ("last run of 1", sample(rng, 4097, 0)),
        ("last run of 2", sample(rng, 4098, 0)),
        ("last run of 3", sample(rng, 8195, 0)),
    ]


def dyn_header(p: bytes):
    """(HLIT, HDIST, HCLEN) of a payload whose first block is dynamic."""
    v = int.from_bytes(p[:4], "little")
    return 257 + ((v >> 3) & 31), 1 + ((v >> 8) & 31), 4 + ((v >> 13) & 15)


def test_edge_messages():
    got = {}
    for name, data in edge_messages():
        for wb in (0, 9):
            got[name] = both_decoders(data, wb)
        assert len(got[name]) <= len(gev_amd.deflate_raw(data)), name
    assert btype(got["256 distinct"]) == 0  # no match, all lengths 8: stored wins
    assert btype(got["B(3,4)"]) == 2
    # no match: one distance code of one bit, HDIST 1; sixteen values: four bits a byte
    assert btype(got["B(16,3)"]) == 2 and dyn_header(got["B(16,3)"])[1] == 1
    assert len(got["B(16,3)"]) < 4096 // 2 + 64
    assert btype(got["fibonacci"]) == 2
    assert btype(got["one byte x 4096"]) in (1, 2)


def test_flags_zero_is_unchanged(corpus):
    for n, kind, data in corpus:
        if n > 70000:
            continue
        cap = gev_amd.deflate_bound(n)
        out = ctypes.create_string_buffer(cap)
        ln = ctypes.c_uint64(0)
        assert gev_amd.lib.gevws_deflate_raw(ctypes.c_char_p(data), n, 0, out, cap, ctypes.byref(ln)) == gev_amd.OK
        assert gev_amd.deflate_raw(data) == gev_amd.deflate_raw(data, flags=0) == out.raw[:ln.value], (n, kind)
    for flags in (1, 4, 3, 6, 1 << 31):  # (1 is a flag of the device call only)
        with pytest.raises(RuntimeError):
            gev_amd.deflate_raw(b"abc", 0, flags)
    with pytest.raises(RuntimeError):
        gev_amd.deflate_raw(b"abc", 7, DYN)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_deflate_dynamic_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "deflate_dynamic_fuzz"
    r = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "deflate_dynamic_fuzz.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_deflate_host.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "deflate_dynamic_fuzz ok" in r.stdout, r.stdout + r.stderr
