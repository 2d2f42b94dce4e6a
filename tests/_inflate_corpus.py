"""Streams for the inflate tests: what zlib's compressor makes of a few kinds
of data, and bit-flipped, truncated and random variants of them.  A stream
here is a message payload: raw DEFLATE ended by Z_SYNC_FLUSH with the four
tail bytes 00 00 ff ff stripped (RFC 7692 section 7.2.1)."""
from __future__ import annotations

import zlib

import numpy as np

from tests._inflate_model import TAIL

LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    s = c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)
    assert s.endswith(TAIL)
    return s[:-4]


def zlib_inflate(payload: bytes):
    """(raised, bytes) of zlib's raw inflate fed payload + TAIL."""
    d = zlib.decompressobj(-15)
    try:
        return False, d.decompress(payload + TAIL)
    except zlib.error:
        return True, b""


def sample(rng, n: int, kind: int) -> bytes:
    """n bytes: 0 text-like, 1 random, 2 long runs, 3 short period."""
    if kind == 0:
        words = [b"frame", b"socket", b"deflate", b"window", "größe".encode(), "€uro".encode(), b"ping", b" ", b"\n"]
        b = b"".join(words[int(i)] for i in rng.integers(0, len(words), n // 3 + 2))
    elif kind == 1:
        b = rng.integers(0, 256, n + 1, dtype=np.uint8).tobytes()
    elif kind == 2:
        b = b"".join(bytes([int(rng.integers(97, 123))]) * int(rng.integers(1, 400)) for _ in range(n // 50 + 2))
    else:
        period = bytes(rng.integers(97, 123, int(rng.integers(1, 9)), dtype=np.uint8))
        b = period * (n // len(period) + 2)
    return (b * (n // max(len(b), 1) + 1))[:n]


def valid_streams(rng, sizes=(0, 1, 2, 17, 300, 2000)):
    """(payload, data) for every level x strategy x kind over a few sizes."""
    out = []
    for level in LEVELS:
        for strategy in STRATEGIES:
            for kind in range(4):
                n = int(rng.choice(sizes))
                data = sample(rng, n, kind)
                out.append((deflate(data, level, strategy), data))
    return out


def mutate(rng, payload: bytes) -> bytes:
    """One of: a single bit flip, a few bit flips, a truncation, a byte
    overwritten, random bytes."""
    b = bytearray(payload)
    how = int(rng.integers(0, 5))
    if how == 4 or not b:
        return rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
    if how == 0:
        i = int(rng.integers(0, 8 * len(b)))
        b[i >> 3] ^= 1 << (i & 7)
    elif how == 1:
        for _ in range(int(rng.integers(2, 6))):
            i = int(rng.integers(0, 8 * min(len(b), 24)))  # the block header is where the rules are
            b[i >> 3] ^= 1 << (i & 7)
    elif how == 2:
        del b[int(rng.integers(0, len(b))):]
    else:
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    return bytes(b)


def malformed_streams(rng, count: int, max_len: int = 300):
    """`count` mutations of small valid streams (most no longer valid)."""
    seeds = [p for p, _ in valid_streams(rng, sizes=(1, 17, 120, 300)) if 0 < len(p) <= max_len]
    return [mutate(rng, seeds[int(rng.integers(0, len(seeds)))]) for _ in range(count)]
