"""The inflate step's verdict rules (gevws_inflate_async, include/gevws.h) in
plain Python: raw DEFLATE (RFC 1951) read bit by bit, byte-serial output.

    inflate(payload, limit) -> (status, bytes produced)

`payload` is a message's compressed payload; the stream S is payload + TAIL.
A block that ends with BFINAL set ends the message; so does one that ends with
less than a whole byte of S unread (unless the bits left already spell block
type 3, which zlib rejects at once).  Running out of S anywhere else, a
distance beyond the bytes produced and everything zlib's inflate rejects are
ERR_DEFLATE; the byte after `limit` bytes of output is ERR_TOO_BIG.

Pinned against zlib by tests/test_inflate_model.py; where they disagree zlib
wins.  Slow: meant for streams of a few hundred bytes."""
from __future__ import annotations

OK, ERR_UTF8, ERR_DEFLATE, ERR_TOO_BIG = 0, 6, 7, 8
TAIL = b"\x00\x00\xff\xff"

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CODE_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Fail(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, s: bytes):
        self.s, self.pos, self.n = s, 0, 8 * len(s)

    def left(self) -> int:
        return self.n - self.pos

    def bit(self) -> int:
        if self.pos >= self.n:
            raise _Fail(ERR_DEFLATE)
        b = (self.s[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, k: int) -> int:
        return sum(self.bit() << i for i in range(k))

    def peek(self, k: int) -> int:
        return sum(((self.s[(self.pos + i) >> 3] >> ((self.pos + i) & 7)) & 1) << i for i in range(k))


def _build(lens, strict: bool):
    """The canonical code of `lens` as {(length, code): symbol}, under zlib's
    inflate_table rules: over-subscribed fails; incomplete fails unless there
    is no code at all or a single one-bit code (never for the code-length code)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    used = [l for l in range(1, 16) if count[l]]
    if not used:
        if strict:
            raise _Fail(ERR_DEFLATE)
        return {}
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise _Fail(ERR_DEFLATE)
    if left > 0 and (strict or max(used) != 1):
        raise _Fail(ERR_DEFLATE)
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + (count[l - 1] if l > 1 else 0)) << 1
        nxt[l] = code
    table = {}
    for sym, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def _decode(br: _Bits, table) -> int:
    code = 0
    for l in range(1, 16):
        code = (code << 1) | br.bit()
        if (l, code) in table:
            return table[(l, code)]
    raise _Fail(ERR_DEFLATE)  # no code of an incomplete set


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _build([5] * 32, False))
    return _FIXED


def inflate(payload: bytes, limit: int = 1 << 32):
    br = _Bits(bytes(payload) + TAIL)
    out = bytearray()

    def put(c):
        if len(out) >= limit:
            raise _Fail(ERR_TOO_BIG)
        out.append(c)

    try:
        while True:
            last, btype = br.bit(), br.bits(2)
            if btype == 3:
                raise _Fail(ERR_DEFLATE)
            if btype == 0:
                br.pos = (br.pos + 7) & ~7
                n, nn = br.bits(16), br.bits(16)
                if n != nn ^ 0xFFFF:
                    raise _Fail(ERR_DEFLATE)
                for _ in range(n):
                    put(br.bits(8))
            else:
                if btype == 1:
                    lit, dist = _fixed()
                else:
                    nlen, ndist, ncode = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
                    if nlen > 286 or ndist > 30:
                        raise _Fail(ERR_DEFLATE)
                    cl = [0] * 19
                    for i in range(ncode):
                        cl[CODE_ORDER[i]] = br.bits(3)
                    ctab = _build(cl, True)
                    lens = []
                    while len(lens) < nlen + ndist:
                        s = _decode(br, ctab)
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise _Fail(ERR_DEFLATE)
                            val, rep = lens[-1], 3 + br.bits(2)
                        elif s == 17:
                            val, rep = 0, 3 + br.bits(3)
                        else:
                            val, rep = 0, 11 + br.bits(7)
                        if len(lens) + rep > nlen + ndist:
                            raise _Fail(ERR_DEFLATE)
                        lens += [val] * rep
                    if lens[256] == 0:
                        raise _Fail(ERR_DEFLATE)
                    lit, dist = _build(lens[:nlen], False), _build(lens[nlen:], False)
                while True:
                    s = _decode(br, lit)
                    if s < 256:
                        put(s)
                        continue
                    if s == 256:
                        break
                    s -= 257
                    if s >= 29:
                        raise _Fail(ERR_DEFLATE)
                    length = LEN_BASE[s] + br.bits(LEN_EXTRA[s])
                    d = _decode(br, dist)
                    if d >= 30:
                        raise _Fail(ERR_DEFLATE)
                    back = DIST_BASE[d] + br.bits(DIST_EXTRA[d])
                    if back > len(out):
                        raise _Fail(ERR_DEFLATE)
                    for _ in range(length):
                        put(out[-back])
            if last:
                break
            if br.left() < 8:
                if br.left() >= 3 and (br.peek(3) >> 1) == 3:
                    raise _Fail(ERR_DEFLATE)
                break
    except _Fail as f:
        return f.status, bytes(out)
    return OK, bytes(out)
