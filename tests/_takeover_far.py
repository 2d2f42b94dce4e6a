"""Takeover slots of connections that have been open for a long time: the
inputs of the relocated-slot tests (tests/test_deflate_takeover_host.py,
tests/test_inflate_takeover_host.py and their GPU twins).

A relocated slot is a real slot whose `total` has been raised by a shift S and
nothing else: S a multiple of 65 536 for the deflate slot (the ring index
i & 32767 and the 16-bit table positions stay valid), of 32 768 for the inflate
slot.  The slot it starts from is old enough to be indifferent to its absolute
position: total >= 70 000, so the ring is full and the 16-bit positions have
wrapped once.  include/gevws.h makes the behaviour of such a slot a function of
total mod 65 536 (mod 32 768), so the same call on the relocated slot must give
the same bytes and leave the same slot with `total` larger by exactly S."""
from __future__ import annotations

import zlib

import numpy as np

from tests import _inflate_corpus as ic

WIN = 32768
U_DEF, U_INF = 65536, 32768
MSG = 100_003                       # longer than either unit: one message spans a boundary from any residue
DEF_CTX = 64 + WIN + 8192
KINDS = ("text", "random", "runs", "period", "tiled")


class DefSlot:
    """The deflate step's context slot (include/gevws.h): a 64-byte head --
    uint64 total, zeros --, the ring image, 4 096 table entries of 16 bits."""

    def __init__(self, image):
        self.image = bytes(image)
        assert len(self.image) == DEF_CTX

    @property
    def total(self) -> int:
        return int.from_bytes(self.image[:8], "little")

    @property
    def head_rest(self) -> bytes:
        return self.image[8:64]

    @property
    def ring(self) -> bytes:
        return self.image[64:64 + WIN]

    @property
    def table(self) -> bytes:
        return self.image[64 + WIN:]

    def relocated(self, shift: int) -> bytearray:
        assert shift % U_DEF == 0 and 0 <= self.total + shift < 1 << 64
        return bytearray((self.total + shift).to_bytes(8, "little") + self.image[8:])


def assert_def_translated(far, near, shift: int, tag=""):
    """The slot `far` is the slot `near` with total larger by exactly `shift`."""
    far, near = DefSlot(far), DefSlot(near)
    assert far.total == near.total + shift, (tag, far.total, near.total, shift)
    assert far.ring == near.ring, (tag, "ring")
    assert far.table == near.table, (tag, "table")
    assert far.head_rest == near.head_rest == bytes(56), (tag, "head")


def history_messages(rng):
    """The chain that makes a slot old: 70 001 bytes after the third message
    (the `odd` base), 131 055 = 2 * 65 536 - 17 after the fifth (the `edge` base:
    a 17-byte message ends on a multiple of both units)."""
    msgs = [ic.sample(rng, n, kind) for n, kind in ((30000, 0), (25000, 2), (15001, 3), (40000, 1), (21054, 0))]
    assert sum(map(len, msgs[:3])) == 70001 and sum(map(len, msgs)) == 2 * U_DEF - 17
    return msgs


def message(rng, history: bytes, kind: str, n: int = MSG) -> bytes:
    """n bytes that find matches in the history: they begin with 300 bytes from
    450 back (in reach of the smallest window the tests use, 2^9), then
    text-like, random, long runs, a short period, or a random block of 7 919
    bytes over and over (matches at one distance everywhere, across any
    boundary inside the message)."""
    k = KINDS.index(kind)
    if k < 4:
        body = ic.sample(rng, n, k)
    else:
        block = ic.sample(rng, 7919, 1)
        body = (block * (n // 7919 + 1))[:n]
    head = history[-450:-150]
    return (head + body)[:n] if n >= 2 * len(head) else body


def shift_below(total: int, unit: int, boundary: int) -> int:
    """The largest shift that leaves total' below `boundary`: a message longer
    than `unit` then crosses it."""
    return (boundary - 1 - total) // unit * unit


def shift_onto(total: int, unit: int, boundary: int) -> int:
    """total' = boundary + total mod unit: on the boundary, rounded to the unit."""
    return boundary - total // unit * unit


def far_cases(total: int, unit: int, msg_len: int = MSG):
    """[(name, S)]: where the issue wants total' = total + S to land.  The
    straddles are asserted, so a test over these cannot pass vacuously."""
    assert total >= 70000 and msg_len > unit
    cases = [("below 2^31", shift_below(total, unit, 1 << 31)), ("below 2^32", shift_below(total, unit, 1 << 32)),
             ("on 2^32", shift_onto(total, unit, 1 << 32)), ("above 2^32", (1 << 32) + 3 * unit),
             ("near 2^48", shift_below(total, unit, 1 << 48)), ("near 2^62", shift_below(total, unit, 1 << 62))]
    for (name, s), b in zip(cases, (31, 32, None, None, 48, 62)):
        assert s > 0 and s % unit == 0, name
        if b is not None:                                    # the next message crosses 2^b
            assert total + s < 1 << b < total + s + msg_len, (name, total + s)
    t = total + cases[2][1]
    assert 1 << 32 <= t < (1 << 32) + unit and (t & 0xFFFFFFFF) < WIN    # a 32-bit `total` would read "young"
    assert total + cases[3][1] > (1 << 32) + unit
    return cases


def edge_cases(total: int, unit: int):
    """[(name, S)] for the `edge` base: total' = 2^b - 17, so a 17-byte message
    ends on 2^b exactly and an empty one and the next one start there."""
    assert (total + 17) % unit == 0
    cases = [(f"2^{b} - 17", shift_below(total, unit, 1 << b)) for b in (31, 32, 48, 62)]
    for (name, s), b in zip(cases, (31, 32, 48, 62)):
        assert s % unit == 0 and total + s + 17 == 1 << b, name
    return cases


def peer_chain(history: bytes, msgs, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY):
    """What a peer whose compressor holds `history` sends next: the payloads of
    `msgs` from one zlib compressor with the last 32 768 history bytes as its
    dictionary, a sync flush per message, the tail removed."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, history[-WIN:])
    out = []
    for m in msgs:
        s = c.compress(m) + c.flush(zlib.Z_SYNC_FLUSH)
        assert s.endswith(ic.TAIL)
        out.append(s[:-4])
    return out


def rng_of(seed: int):
    return np.random.default_rng(seed)
