"""Session tests of the message chain: the peer's view of a whole connection.

However a connection's byte stream is cut into passes, at any byte, the peer
must receive the same thing: what a host-side reading of RFC 6455 / RFC 7692
and include/gevws.h says a server sends for that stream.  This file holds the
host side of that check -- a traffic generator, a cutter, the expected peer
view (host_walk / walk), a peer-side parser and checker, a reference host
server for the CPU self-test, and the driver that feeds a session through the
device chain pass by pass.  It is deliberately not a composition of the
tests/_*_model.py step models: those mirror the kernels' tables, this is what
a client sees.  No torch at import time (the drivers import it when called)."""
from __future__ import annotations

import codecs
import functools
import zlib
from collections import Counter
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import ws_oracle as wo

T, B, C, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
RSV1 = 4
TAIL = b"\x00\x00\xff\xff"
# conn_ext bits (include/gevws.h: GEVWS_EXT_DEFLATE, _CLIENT_TAKEOVER, _SERVER_TAKEOVER)
D, CT, ST = 1, 2, 4
LIMIT = 1 << 20       # the inflate limit and the carry limit of a session: every message stays below both
ROOM_NONE = 0xFFFFFFFF
SKIP_SENDER = 1       # GEVWS_ROOMS_SKIP_SENDER


class CheckError(AssertionError):
    """What the peer-side checker raises: the bytes a socket was sent are not
    what the connection's stream asks for."""


# ---------------------------------------------------------------------------- the expected peer view
def walk(frames, deflate: bool, limit: int, client_takeover: bool = False):
    """What a host that walks a connection's received frames (wo.decode_stream's)
    sends, as (frame index, kind, x): ("ctl", reply wire bytes) / ("echo",
    message bytes) / ("fail", close code); nothing behind a close or a failure.

    The frame checks are RFC 6455's in the order include/gevws.h lists them
    (RSV, reserved opcode, control frame fragmented or over 125 bytes,
    continuation without a message, a new message inside one: 1002); a plain
    text message fails with 1007 at the frame that holds a byte no UTF-8
    sequence can continue with, or at its FIN frame when that ends inside a
    sequence (section 8.1, fail fast); a compressed message is inflated at its
    FIN frame (RFC 7692 section 7.2.2: the tail 00 00 ff ff appended), against
    the connection's history when the client keeps its context."""
    parts, compressed, text, utf8 = None, False, False, None
    z = zlib.decompressobj(-15) if client_takeover else None
    for i, f in enumerate(frames):
        h = f.header
        op = h.opcode
        ctl = bool(op & 8)
        bad_rsv = (h.rsv & 3 or (h.rsv & 4 and (ctl or op == 0))) if deflate else h.rsv
        if bad_rsv or op in (3, 4, 5, 6, 7, 11, 12, 13, 14, 15) or (ctl and (not h.fin or h.length > 125)):
            yield i, "fail", 1002
            return
        if ctl:
            reply, shutdown = wo.on_message(h, f.payload, wo.HANDLER_NONE)
            yield i, "ctl", reply
            if shutdown:
                return
            continue
        if (op == 0) == (parts is None):      # a continuation of nothing, or a new message inside one
            yield i, "fail", 1002
            return
        if op:
            parts, compressed, text = [], bool(h.rsv & 4), op == 1
            utf8 = codecs.getincrementaldecoder("utf-8")("strict") if text and not compressed else None
        parts.append(f.payload)
        if utf8 is not None:
            try:
                utf8.decode(f.payload, bool(h.fin))
            except UnicodeDecodeError:
                yield i, "fail", 1007
                return
        if not h.fin:
            continue
        data, parts = b"".join(parts), None
        if compressed:
            try:
                data = (z or zlib.decompressobj(-15)).decompress(data + TAIL)
            except zlib.error:
                yield i, "fail", 1007
                return
            if len(data) > limit:
                yield i, "fail", 1009
                return
            if text and not wo.utf8_valid(data):
                yield i, "fail", 1007
                return
        yield i, "echo", data


def host_walk(stream: bytes, deflate: bool, limit: int, client_takeover: bool = False):
    """walk over a connection's received bytes, without the frame indices."""
    return [(k, x) for _, k, x in walk(wo.decode_stream(stream).frames, deflate, limit, client_takeover)]


# ---------------------------------------------------------------------------- traffic
def comp(data: bytes, co=None) -> bytes:
    """One message's permessage-deflate payload: a sync flush without its tail."""
    co = co or zlib.compressobj(6, zlib.DEFLATED, -15)
    return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]


WORDS = ("the quick brown fox jumps over the lazy dog; zwölf Boxkämpfer jagen Viktor quer über den Sylter Deich; "
         "€uro und 𝄞-Schlüssel; ").encode()


@dataclass
class Conn:
    """One connection of a session: its negotiated extension, the bytes a
    masked client sends over its life, and what the peer view needs of them."""
    ext: int
    window_bits: int
    heavy: str = ""
    events: List[Tuple[str, bytes]] = field(default_factory=list)   # ("text" | "binary" | "ping" | "pong" | "close" | "raw", payload)
    wire: bytes = b""
    # filled by finish():
    frames: list = field(default_factory=list)        # wo.decode_stream's
    items: list = field(default_factory=list)         # walk's (frame, kind, x)
    dead_at: Optional[int] = None                     # the frame that shuts the connection down
    info: list = field(default_factory=list)          # per frame: (open_after, compressed message, plain text)
    cut_here: List[int] = field(default_factory=list)  # offsets a cutting of three passes or more must use

    def finish(self) -> "Conn":
        res = wo.decode_stream(self.wire)
        assert res.status == wo.OK and res.consumed == len(self.wire)    # decode statuses < 0 are the host's
        self.frames = res.frames
        self.items = list(walk(self.frames, bool(self.ext & D), LIMIT, bool(self.ext & CT)))
        self.dead_at = None
        if self.items and (self.items[-1][1] == "fail" or
                           (self.items[-1][1] == "ctl" and self.frames[self.items[-1][0]].header.opcode == CLOSE)):
            self.dead_at = self.items[-1][0]
        self.info, is_open, compressed, text = [], False, False, False
        for f in self.frames:
            h = f.header
            if not h.opcode & 8:
                if h.opcode:
                    compressed, text = bool(h.rsv & 4) and bool(self.ext & D), h.opcode == 1
                is_open = not h.fin
            self.info.append((is_open, compressed, text and not compressed))
        return self

    def frame_end(self, i: int) -> int:
        f = self.frames[i]
        return f.stream_pos + f.header_len + f.header.length

    def fed_frames(self, offset: int) -> int:
        """The frames that are whole within the first `offset` bytes, up to and including the one that shuts the
        connection down."""
        n = 0
        while n < len(self.frames) and self.frame_end(n) <= offset:
            n += 1
            if self.dead_at is not None and n == self.dead_at + 1:
                break
        return n

    def expected(self):
        return [(k, x) for _, k, x in self.items]


class Builder:
    """A masked client: random keys, random fragment edges, all three length forms."""

    def __init__(self, rng, ext: int = 0, window_bits: int = 0, heavy: str = ""):
        self.rng, self.c = rng, Conn(ext, window_bits, heavy)
        self.co = zlib.compressobj(6, zlib.DEFLATED, -15) if ext & CT else None
        self.parts: List[bytes] = []

    def key(self) -> bytes:
        return bytes(self.rng.integers(0, 256, 4, dtype=np.uint8))

    def frame(self, payload: bytes, op: int, fin: bool = True, rsv: int = 0, len_form=None) -> "Builder":
        self.parts.append(wo.encode_frame(payload, op, fin, rsv, True, self.key(), len_form))
        return self

    def mark(self, back: int = 0) -> "Builder":
        """A pass boundary here (`back` bytes before), in every cutting with room for it."""
        self.c.cut_here.append(sum(len(p) for p in self.parts) - back)
        return self

    def ctl(self, op: int, payload: bytes = b"", fin: bool = True) -> "Builder":
        self.c.events.append(({PING: "ping", PONG: "pong", CLOSE: "close"}[op], payload))
        return self.frame(payload, op, fin)

    def close(self, code: int = 1000, reason: bytes = b"") -> "Builder":
        return self.ctl(CLOSE, code.to_bytes(2, "big") + reason)

    def message(self, data: bytes, op: int = T, frags=1, compress: Optional[bool] = None, between: Sequence = (),
                payload: Optional[bytes] = None, len_form=None) -> "Builder":
        """A message of `frags` fragments (an int: random edges; a list: those
        edges of the payload), compressed on a deflate connection unless
        compress is False; between: control frames (op, payload) dealt over the
        gaps between the fragments; payload: the wire payload when it is not
        the honest compression of data."""
        self.c.events.append(("text" if op == T else "binary", data))
        if compress is None:
            compress = bool(self.c.ext & D)
        if payload is None:
            payload = comp(data, self.co) if compress else data
        if isinstance(frags, int):
            k = min(frags - 1, len(payload))
            edges = sorted(int(x) for x in self.rng.integers(0, len(payload) + 1, k))
        else:
            edges = list(frags)
        edges = [0, *edges, len(payload)]
        n = len(edges) - 1
        for i in range(n):
            self.frame(payload[edges[i]:edges[i + 1]], op if i == 0 else C, i == n - 1,
                       RSV1 if compress and i == 0 else 0, len_form)
            for j, (cop, cp) in enumerate(between):
                if n > 1 and j % (n - 1) == i and i < n - 1:
                    self.ctl(cop, cp)
        return self

    def done(self) -> Conn:
        self.c.wire = b"".join(self.parts)
        return self.c.finish()


def text_of(rng, n: int, random_share: float = 0.0) -> bytes:
    """n bytes of valid UTF-8: the pangrams, with runs of random letters among them."""
    out, size = [], 0
    while size < n:
        if rng.random() < random_share:
            s = bytes(rng.integers(0x61, 0x7B, int(rng.integers(50, 400)), dtype=np.uint8))
        else:
            a = int(rng.integers(0, 40))
            s = WORDS[a:] if wo.utf8_valid(WORDS[a:]) else WORDS
        out.append(s)
        size += len(s)
    data = b"".join(out)[:n]
    while not wo.utf8_valid(data):
        data = data[:-1]
    return data + b"." * (n - len(data))


def clip(text: bytes, a: int, b: Optional[int] = None) -> bytes:
    """text[a:b], without the halves of characters the slice cuts."""
    return text[a:b].decode("utf-8", "ignore").encode()


def noise(rng, n: int) -> bytes:
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


CLASSES = ((0, 0), (D, 0), (D | CT, 0), (D | ST, 10), (D | ST, 12), (D | ST, 15), (D | CT | ST, 15))


def light_conn(rng, ext: int, wb: int) -> Conn:
    b = Builder(rng, ext, wb)
    for _ in range(int(rng.integers(1, 4))):
        k = rng.random()
        n = int(rng.integers(0, 201))
        data = text_of(rng, n, 0.3) if rng.random() < 0.7 else noise(rng, n)
        op = T if wo.utf8_valid(data) and rng.random() < 0.8 else B
        between = [(PING, b"p%d" % n)] if k < 0.15 else ([(PONG, b"")] if k < 0.2 else [])
        b.message(data, op, 1 + int(rng.random() < 0.3) + bool(between), compress=bool(ext & D) and rng.random() < 0.7,
                  between=between, len_form=16 if k > 0.9 else None)
        if 0.2 <= k < 0.3:
            b.ctl(PING if k < 0.25 else PONG, bytes(rng.integers(0x20, 0x7F, int(rng.integers(0, 126)), dtype=np.uint8)))
    if rng.random() < 0.05:
        b.close(1000, b"bye").message(b"behind the close", T)
    return b.done()


def heavy_conns(rng) -> List[Conn]:
    """About twenty connections that hold, between them, every class and every
    case the session test names; each is named by what it is for."""
    pings = lambda n, tag: [(PING if i % 3 else PONG, b"%s %d" % (tag, i)) for i in range(n)]  # noqa: E731
    out = []

    def new(name, cls=0):
        b = Builder(rng, *CLASSES[cls], heavy=name)
        out.append(b)
        return b

    # plain
    new("plain: one 70 000-byte frame, the 64-bit length form").message(b"short", T).message(
        noise(rng, 70000), B).message(b"", B).message(text_of(rng, 300), T, 3)
    new("plain: a text of 80 000 bytes in 9 fragments, pings and pongs between").message(
        text_of(rng, 80000), T, 9, between=pings(8, b"in the text")).message(b"", T).message(
        text_of(rng, 40000), T, 7, len_form=64)
    bad = text_of(rng, 600)
    new("plain: a text failing UTF-8 in the middle of a fragment").message(text_of(rng, 500), T, 2).message(
        bad[:300] + b"\xff" + bad[300:], T, [100, 500], between=[(PING, b"before the bad byte"), (PING, b"behind it")]
    ).message(b"never answered", T)
    new("plain: a close between two fragments, frames behind it").message(text_of(rng, 2000), T, 2).frame(
        text_of(rng, 3000), T, False).mark().ctl(PING, b"answered").close(1000, b"bye").frame(
        text_of(rng, 2000), C, True).mark(1000).message(b"behind the close", T).ctl(PING, b"unanswered")
    new("plain: a fragmented ping inside an open message").message(b"fine", T).frame(noise(rng, 5000), B, False).ctl(
        PING, b"whole").ctl(PING, b"half", fin=False).frame(b"", C, True)
    new("plain: a 126-byte ping").message(text_of(rng, 100), T).ctl(PING, b"x" * 125).ctl(PING, b"y" * 126).message(
        b"late", T)
    new("plain: RSV1 without the extension").message(b"fine", T, 2).frame(comp(b"not negotiated"), T, True, RSV1)
    new("plain: empty fragments, a message of nothing but them").message(noise(rng, 4000), B, [0, 0, 2000, 4000]).frame(
        b"", T, False).ctl(PONG, b"between nothing").frame(b"", C, False).frame(b"", C, True).message(b"after", T)
    # deflate, no takeover
    new("deflate: a compressed text of 90 000 bytes in 8 fragments, pings between", 1).message(
        text_of(rng, 90000, 0.5), T, 8, between=pings(7, b"z")).message(b"", T).message(
        text_of(rng, 700), T, compress=False).message(noise(rng, 30000), B, 3)
    new("deflate: a compressed text that inflates to invalid UTF-8", 1).message(text_of(rng, 900), T).message(
        text_of(rng, 2000) + b"\xc3\x28" + text_of(rng, 2000), T, 4, between=[(PING, b"answered"), (PING, b"too")]
    ).message(b"never answered", T)
    broken = comp(text_of(rng, 20000, 0.5)) + b"\x12\x34\x56\x78"   # a stored block whose LEN is not ~NLEN
    new("deflate: a compressed message that does not inflate", 1).message(text_of(rng, 50), T).message(
        b"", T, 5, payload=broken, between=[(PING, b"answered")]).ctl(PING, b"unanswered")
    new("deflate: RSV1 on a continuation frame", 1).message(text_of(rng, 3000), T, 2).frame(
        comp(b"first")[:2], T, False, RSV1).ctl(PING, b"answered").frame(comp(b"first")[2:], C, True, RSV1)
    new("deflate: a ping between two fragments whose message ends much later", 1).frame(b"", PONG).message(
        text_of(rng, 60000, 0.6), B, [10, 20000, 20001, 40000], between=[(PING, b"early"), (PONG, b"")]).close(1001)
    # the client keeps its context
    history = text_of(rng, 3000, 0.4)
    new("client takeover: 75 000 bytes in fragments, then messages out of its history", 2).message(
        history, T).message(text_of(rng, 75000, 0.5), T, 7, between=pings(3, b"ct")).message(
        clip(history, 500, 2500), T).message(b"plain, outside the window", T, compress=False).message(
        clip(history, 1000), T, 2).message(b"", T).message(clip(history, 0, 1500) + b"!", B)
    new("client takeover: history, then a close with frames behind it", 2).message(history, T, 3).message(
        clip(history, 100, 2900), T, 2, between=[(PING, b"pi")]).close(1000).message(history, T)
    # the server keeps its context: window bits 10, 12, 15
    for cls, big in ((3, 70000), (4, 80000), (5, 100000)):
        rep = text_of(rng, 2500, 0.4)
        new("server takeover, %d window bits: %d bytes, then replies out of the window" % (CLASSES[cls][1], big),
            cls).message(rep, T).message(rep, T, 2).message(text_of(rng, big, 0.5), T, 7, between=pings(4, b"st")
                                                              ).message(clip(rep, 300), T).message(b"", T).message(rep, B)
    rep = text_of(rng, 2000, 0.4)
    new("server takeover, 12 window bits: a failed message never enters the window", 4).message(rep, T).message(
        clip(rep, 0, 1000) + b"\xff" + clip(rep, 1000), T, 3).message(rep, T)
    # both
    new("both takeovers: 85 000 bytes, both windows wrap", 6).message(rep, T).message(
        text_of(rng, 85000, 0.5), T, 9, between=pings(5, b"both")).message(rep, T).message(clip(rep, 700), T, 2)
    new("both takeovers: a close, and messages behind it that no window may see", 6).message(rep, T).message(
        rep, T, 2).close(1000, b"done").message(rep, T).message(rep, T)
    return [b.done() for b in out]


def echo_traffic(seed: int, n_conns: int = 320) -> List[Conn]:
    """The echo session's connections: the heavy ones spread over the batch
    (one of them its last: behind the 256-lane edge of the per-connection
    kernels), light ones of every class between them."""
    rng = np.random.default_rng(seed)
    heavy = heavy_conns(rng)
    slots = sorted(int(x) for x in rng.choice(n_conns - 1, len(heavy) - 1, replace=False)) + [n_conns - 1]
    conns: List[Optional[Conn]] = [None] * n_conns
    for s, h in zip(slots, heavy):
        conns[s] = h
    for c in range(n_conns):
        if conns[c] is None:
            conns[c] = light_conn(rng, *CLASSES[int(rng.integers(0, len(CLASSES)))])
    assert sum(len(c.wire) for c in conns) <= 3 << 19     # 1.5 MiB of wire at the most
    return conns


# ---------------------------------------------------------------------------- cutting
CUT_CLASSES = ("header", "extlen", "mask", "payload0", "utf8", "compressed", "edge", "between")


def cut_classes(conn: Conn, off: int) -> set:
    """What a pass boundary at byte `off` of the connection's stream cuts; only
    frames the connection is fed while it lives count."""
    live = len(conn.frames) if conn.dead_at is None else conn.dead_at + 1
    out = set()
    for i in range(live):
        f = conn.frames[i]
        s, hl, n = f.stream_pos, f.header_len, f.header.length
        if off < s:
            break
        if off == s and off > 0:
            out.add("edge")
            if i and conn.info[i - 1][0]:
                out.add("between")          # the message of the frames before is still open
                if conn.info[i - 1][1]:
                    out.add("between, compressed")
        if off >= s + hl + n:
            continue
        rel = off - s
        ext = hl - 6                        # masked: 2 + extended length + 4
        if rel == 1:
            out.add("header")
        elif 2 < rel < 2 + ext:
            out.add("extlen")
        elif 2 + ext < rel < hl:
            out.add("mask")
        elif rel == hl and n:
            out.add("payload0")
        elif rel > hl:
            _, compressed, plain_text = conn.info[i]
            if not f.header.opcode & 8 and compressed:
                out.add("compressed")
            if not f.header.opcode & 8 and plain_text and f.payload[rel - hl] & 0xC0 == 0x80:
                out.add("utf8")
    return out


def cut_sites(conn: Conn) -> Dict[str, List[int]]:
    """Some offsets of every class this connection has."""
    live = len(conn.frames) if conn.dead_at is None else conn.dead_at + 1
    sites: Dict[str, List[int]] = {k: [] for k in (*CUT_CLASSES, "between, compressed")}
    for i in range(live):
        f = conn.frames[i]
        s, hl, n = f.stream_pos, f.header_len, f.header.length
        cand = [s, s + 1, s + 3, s + hl - 2, s + hl]
        if n > 1:
            cand.append(s + hl + n // 2)
            p = f.payload
            cand += [s + hl + j for j in range(1, min(n, 256)) if p[j] & 0xC0 == 0x80][:1]
        for off in cand:
            for k in cut_classes(conn, off):
                sites[k].append(off)
    return sites


def make_cuts(conns: Sequence[Conn], passes: int, seed: int):
    """Per connection the sorted byte offsets at which passes 1 .. passes - 1
    start (a duplicate: an idle pass), and how many cuts of each class there
    are.  A connection's own marks (Conn.cut_here) come first: the close between
    two fragments is cut so that the open message's first fragment, the close
    and the message's end fall into three passes.  Random offsets, and on every heavy connection forced ones: one class
    after the other, and on every third a cut between two fragments doubled, so
    that the open message waits through an idle pass."""
    rng = np.random.default_rng(seed)
    cuts, classes, turn, heavy = [], Counter(), 0, 0
    pick = lambda s: s[int(rng.integers(0, len(s)))]  # noqa: E731
    for conn in conns:
        n, k = len(conn.wire), passes - 1
        mine = [int(x) for x in rng.integers(0, n + 1, k)] if n else [0] * k
        if conn.heavy and k:
            sites = cut_sites(conn)
            forced = []
            for _ in range(min(k, 2)):
                for step in range(len(CUT_CLASSES)):     # the next class this connection has a site of
                    s = sites[CUT_CLASSES[(turn + step) % len(CUT_CLASSES)]]
                    if s:
                        forced.append(pick(s))
                        turn += step + 1
                        break
            doubled = sites["between, compressed"] or sites["between"]
            if k >= 2 and heavy % 3 == 2 and doubled:
                forced = [pick(doubled)] * 2
            if k >= len(conn.cut_here) > 0:
                forced = list(conn.cut_here)
            heavy += 1
            mine[:len(forced)] = forced
        mine.sort()
        cuts.append(mine)
        for off in mine:
            classes.update(cut_classes(conn, off) & set(CUT_CLASSES))
    return cuts, classes


def pass_ends(cuts: List[int], passes: int, total: int) -> List[int]:
    return [*cuts, total][:passes] if passes > 1 else [total]


def predicted_carries(conns: Sequence[Conn], cuts, passes: int) -> Counter:
    """What the carry must hold after some pass, from the cuts alone: an open
    plain message, an open compressed one, one on a client-takeover connection,
    one that waits through a pass without bytes."""
    seen = Counter()
    for conn, mine in zip(conns, cuts):
        ends = pass_ends(mine, passes, len(conn.wire))
        for p, e in enumerate(ends[:-1]):
            n = conn.fed_frames(e)
            if n == 0 or (conn.dead_at is not None and n > conn.dead_at):
                continue
            is_open, compressed, _ = conn.info[n - 1]
            if not is_open:
                continue
            seen["compressed" if compressed else "plain"] += 1
            if compressed and conn.ext & CT:
                seen["compressed, client takeover"] += 1
            if compressed and ends[p + 1] == e:
                seen["compressed, across an idle pass"] += 1
    return seen


# ---------------------------------------------------------------------------- the peer's side
def parse_wire(wire: bytes):
    """The frames of what a socket was sent.  (The oracle, as the reference,
    reads no header from fewer than 6 buffered bytes: three bare close frames
    behind the wire let it read a short last frame, and are dropped again.)"""
    got = wo.decode_stream(wire + b"\x88\x00" * 3)
    frames = [f for f in got.frames if f.stream_pos < len(wire)]
    if got.status != wo.OK or sum(f.header_len + f.header.length for f in frames) != len(wire):
        raise CheckError("the bytes sent are not whole frames")
    return frames


def replies_of(frames, F: Optional[int], deflate: bool):
    """Parsed frames as replies: [("ctl", opcode, payload) | ("msg", rsv of the
    first frame, [payloads])], with the framing rules checked on the way: nothing
    masked, control frames whole and outside a reply's fragments, RSV1 on a
    first fragment only and only with permessage-deflate, the fragment pattern
    of the limit F, nothing behind a close frame."""
    out, cur, closed = [], None, False
    for f in frames:
        h = f.header
        if closed:
            raise CheckError("a frame behind a close frame")
        if h.masked:
            raise CheckError("a server frame is masked")
        if h.opcode & 8:
            if cur is not None:
                raise CheckError("a control frame between a reply's fragments")
            if not h.fin or h.rsv or h.length > 125 or h.opcode not in (CLOSE, PING, PONG):
                raise CheckError("a malformed control frame")
            out.append(("ctl", h.opcode, f.payload))
            closed = h.opcode == CLOSE
            continue
        if cur is None:
            if h.opcode not in (T, B) or h.rsv & ~RSV1 or (h.rsv and not deflate):
                raise CheckError("a first fragment with opcode %d, rsv %d (deflate: %s)" % (h.opcode, h.rsv, deflate))
            cur = [h.rsv, []]
        elif h.opcode != C or h.rsv:
            raise CheckError("opcode %d, rsv %d on a continuation: RSV1 belongs on the first fragment" % (h.opcode, h.rsv))
        cur[1].append(f.payload)
        if h.fin:
            parts = cur[1]
            total = sum(len(p) for p in parts)
            if F is None and len(parts) != 1:
                raise CheckError("a reply in %d fragments without a limit" % len(parts))
            if F is not None and (len(parts) != max(1, -(-total // F)) or any(len(p) != F for p in parts[:-1])
                                  or len(parts[-1]) > F):
                raise CheckError("fragment pattern: %s under the limit %d" % ([len(p) for p in parts], F))
            out.append(("msg", cur[0], parts))
            cur = None
    if cur is not None:
        raise CheckError("a reply without its FIN frame")
    return out


def check_replies(wire: bytes, want: Sequence[Tuple[str, object]], F: Optional[int], deflate: bool,
                  takes_deflate: bool, z=None, tally: Optional[Counter] = None) -> None:
    """What a socket was sent over a connection's life against the expected
    peer view `want` (walk's kinds).  deflate: the connection negotiated
    permessage-deflate; takes_deflate: its data replies are compressed; z: the
    peer's persistent decompressor when the server keeps its context."""
    got = replies_of(parse_wire(wire), F, deflate)
    tally = Counter() if tally is None else tally
    for i, (g, (kind, x)) in enumerate(zip(got, want)):
        if (g[0] == "msg") != (kind == "echo"):
            raise CheckError("reply %d: a %s frame where %s is due" % (i, g[0], kind))
        if kind == "ctl":
            w = wo.decode_stream(x + b"\x88\x00" * 3).frames[0]
            if (g[1], g[2]) != (w.header.opcode, w.payload):
                raise CheckError("reply %d: the control reply differs" % i)
            tally[{PONG: "pong", PING: "ping for pong", CLOSE: "close reply"}[g[1]]] += 1
        elif kind == "fail":
            if (g[1], g[2]) != (CLOSE, int(x).to_bytes(2, "big")):
                raise CheckError("reply %d: the failure close differs, %d is due" % (i, x))
            tally[str(x)] += 1
        else:
            data = b"".join(g[2])
            if not takes_deflate:
                if g[1] or data != x:
                    raise CheckError("reply %d: the echo's bytes differ (%d bytes due)" % (i, len(x)))
                tally["echo plain"] += 1
                continue
            if g[1] != RSV1:
                raise CheckError("reply %d: an uncompressed reply on a connection that takes deflate" % i)
            try:
                back = (z or zlib.decompressobj(-15)).decompress(data + TAIL)
            except zlib.error:
                back = None
            if back != x:
                raise CheckError("reply %d: the echo does not inflate to the message (%d bytes due)" % (i, len(x)))
            tally["echo deflated"] += 1
            if z is not None and x:
                try:
                    alone = zlib.decompressobj(-15).decompress(data + TAIL)
                except zlib.error:
                    alone = None
                tally["needs the window"] += alone != x
    if len(got) != len(want):
        raise CheckError("%d replies where %d are due" % (len(got), len(want)))


def check_echo_conn(conn: Conn, wire: bytes, F: Optional[int], tally: Optional[Counter] = None) -> None:
    z = zlib.decompressobj(-15) if conn.ext & ST else None
    check_replies(wire, conn.expected(), F, bool(conn.ext & D), bool(conn.ext & D), z, tally)


# ---------------------------------------------------------------------------- a reference host server
def encode_replies(want, F: Optional[int], takes_deflate: bool, window_bits: int = 0, co=None) -> List[bytes]:
    """Wire bytes a correct server could send for walk's items, one element a
    reply: control replies and failure closes whole, data replies text frames
    of at most F payload bytes, compressed with zlib (co: the server's
    persistent compressor) when the connection takes deflate."""
    out = []
    for kind, x in want:
        if kind == "ctl":
            out.append(x)
        elif kind == "fail":
            out.append(wo.encode_frame(int(x).to_bytes(2, "big"), CLOSE, True, 0, False))
        else:
            payload = x
            if takes_deflate:
                payload = comp(x, co or zlib.compressobj(6, zlib.DEFLATED, -(window_bits or 15)))
            step = F or max(len(payload), 1)
            parts = [payload[i:i + step] for i in range(0, len(payload), step)] or [b""]
            out.append(b"".join(wo.encode_frame(p, T if i == 0 else C, i == len(parts) - 1,
                                                RSV1 if takes_deflate and i == 0 else 0, False)
                                for i, p in enumerate(parts)))
    return out


def reference_echo_server(conn: Conn, F: Optional[int]) -> List[bytes]:
    co = zlib.compressobj(6, zlib.DEFLATED, -(conn.window_bits or 15)) if conn.ext & ST else None
    return encode_replies(conn.expected(), F, bool(conn.ext & D), conn.window_bits, co)


# ---------------------------------------------------------------------------- the broadcast session
@dataclass
class BroadcastCase:
    conns: List[Conn]
    cuts: list
    passes: int
    n_rooms: int
    rooms0: np.ndarray              # uint32 [n_conns]
    changes: List[np.ndarray]       # per pass, applied behind it: int64 [k, 2]


def broadcast_traffic(seed: int, n_conns: int = 300, n_rooms: int = 7, passes: int = 4) -> BroadcastCase:
    rng = np.random.default_rng(seed)
    classes = ((0, 0), (D, 0), (D, 0), (D | ST, 12))
    conns = []
    closers = set(int(x) for x in rng.choice(n_conns, 3, replace=False))
    big = set(int(x) for x in rng.choice([c for c in range(n_conns) if c not in closers], 2, replace=False))
    for c in range(n_conns):
        b = Builder(rng, *classes[int(rng.integers(0, len(classes)))])
        for _ in range(int(rng.integers(0, 4))):
            data = text_of(rng, int(rng.integers(0, 120)), 0.3)
            b.message(data, T, 1 + int(rng.random() < 0.3), compress=bool(b.c.ext & D) and rng.random() < 0.6,
                      between=[(PING, b"pi")] if rng.random() < 0.2 else [])
            if rng.random() < 0.15:
                b.ctl(PONG if rng.random() < 0.3 else PING, b"between messages")
        if c in big:
            b.message(text_of(rng, 40000, 0.5), T, 4, between=[(PING, b"in the big one")])
        if c in closers:
            b.c.heavy = "closes"
            if c == min(closers):
                b.message(b"ok \xff not", T).message(b"behind the failure", T)
            else:
                b.message(b"last words", T).close(1000, b"bye").message(b"behind the close", T)
            for _ in range(3):      # a long tail nobody reads: the connection ends in an early pass
                b.message(text_of(rng, 1500), T)
        conns.append(b.done())
    rooms0 = rng.integers(0, n_rooms, n_conns).astype(np.uint32)
    rooms0[rng.choice(n_conns, 25, replace=False)] = ROOM_NONE
    for c in closers | big:
        rooms0[c] = c % n_rooms
    cuts, _ = make_cuts(conns, passes, seed ^ 0x5A5A)
    # join / move / leave records behind every pass but the last.  A host names no connection it has closed -- but
    # in the pass that closes one a join for it may still be under way, and the close must win
    others = np.array([c for c in range(n_conns) if c not in closers])
    changes = []
    for p in range(passes):
        k = 20 if p < passes - 1 else 0
        who = rng.choice(others, k)
        if k:
            who[-3:] = who[:3]                      # some connections are named twice: the last record wins
        room = rng.integers(0, n_rooms + 2, k).astype(np.int64)
        room[room >= n_rooms] = ROOM_NONE
        recs = [(int(a), int(b)) for a, b in zip(who, room)]
        for c in closers:
            ends = pass_ends(cuts[c], passes, len(conns[c].wire))
            if conns[c].fed_frames(ends[p]) > conns[c].dead_at and (p == 0 or conns[c].fed_frames(ends[p - 1])
                                                                    <= conns[c].dead_at) and k:
                recs.insert(len(recs) // 2, (c, (c + 1) % n_rooms))
        changes.append(np.array(recs, np.int64).reshape(-1, 2))
    return BroadcastCase(conns, cuts, passes, n_rooms, rooms0, changes)


def takes_deflate_broadcast(ext: int) -> bool:
    # gevws.h, "Recipient kind": deflate with GEVWS_EXT_DEFLATE and without GEVWS_EXT_SERVER_TAKEOVER, else plain
    return bool(ext & D) and not ext & ST


def broadcast_view(case: BroadcastCase, flags: int):
    """Per pass and recipient the expected replies (walk's kinds), and the room
    table behind every pass, from the contract of gevws_reply_rooms_async /
    gevws_room_plan_async / gevws_rooms_update_async in include/gevws.h."""
    n = len(case.conns)
    room = case.rooms0.copy()
    alive = [True] * n
    # a message belongs to the pass in which its FIN frame is whole: the pass whose end first reaches the frame's end
    ends = [pass_ends(case.cuts[c], case.passes, len(case.conns[c].wire)) for c in range(n)]
    views, tables = [], []
    for p in range(case.passes):
        mine: List[List] = [[] for _ in range(n)]
        for c, conn in enumerate(case.conns):
            if not alive[c]:
                continue
            lo = conn.fed_frames(ends[c][p - 1]) if p else 0
            hi = conn.fed_frames(ends[c][p])
            mine[c] = [(k, x) for i, k, x in conn.items if lo <= i < hi]
        view: List[List] = [[] for _ in range(n)]
        for r in range(n):
            if not alive[r]:
                continue                     # the host feeds a shut-down connection nothing, and update took it out
            if room[r] != ROOM_NONE:
                # "Order": first every publication of its room's members in frame order (sender order, then stream
                # order; r's own left out under GEVWS_ROOMS_SKIP_SENDER) ...
                for s in np.flatnonzero(room == room[r]):
                    if flags & SKIP_SENDER and s == r:
                        continue
                    # "Publishing": a frame that ends a delivered message (no control reply, up to the cut)
                    view[r] += [(k, x) for k, x in mine[int(s)] if k == "echo"]
            # "... then its own control replies in frame order.  The close reply of a cut is therefore the last
            # thing r is sent."  A GEVWS_ROOM_NONE connection "is sent only its own control replies".
            view[r] += [(k, x) for k, x in mine[r] if k != "echo"]
        views.append(view)
        # gevws_rooms_update_async: the changes in list order, the last one of a connection wins; a connection the
        # pass shut down ends in GEVWS_ROOM_NONE, "a close beats a join in the same call"
        for who, g in case.changes[p]:
            room[int(who)] = g
        for c, conn in enumerate(case.conns):
            if alive[c] and conn.dead_at is not None and conn.fed_frames(ends[c][p]) > conn.dead_at:
                alive[c] = False
            if not alive[c]:
                room[c] = ROOM_NONE
        tables.append(room.copy())
    return views, tables


def check_broadcast_conn(case: BroadcastCase, views, r: int, sent_per_pass: Sequence[bytes], F: Optional[int],
                         tally: Optional[Counter] = None) -> None:
    """Recipient r's bytes of every pass against its view of that pass (no
    window crosses a broadcast: every compressed reply inflates alone)."""
    ext = case.conns[r].ext
    for p, wire in enumerate(sent_per_pass):
        try:
            check_replies(bytes(wire), views[p][r], F, bool(ext & D), takes_deflate_broadcast(ext), None, tally)
        except CheckError as e:
            raise CheckError("pass %d, recipient %d: %s" % (p, r, e)) from None


def reference_broadcast_server(case: BroadcastCase, flags: int, F: Optional[int]):
    """sent[p][r]: the reply list (encode_replies) a correct host server sends recipient r in pass p."""
    views, _ = broadcast_view(case, flags)
    return [[encode_replies(v, F, takes_deflate_broadcast(case.conns[r].ext)) for r, v in enumerate(view)]
            for view in views]


# ---------------------------------------------------------------------------- the session driver
@dataclass
class SessionRun:
    """What a session left behind: per pass and connection the bytes of the
    send plan (conn_bytes) and of the gather (host_sends), the carry records
    behind every pass, and the state at its end."""
    sent: List[List[bytes]] = field(default_factory=list)       # [pass][conn]
    gathered: List[List[bytes]] = field(default_factory=list)   # [pass][conn]
    carries: List[np.ndarray] = field(default_factory=list)     # CARRY_DTYPE [n_conns] behind each pass
    carry_used: List[int] = field(default_factory=list)
    shutdown_pass: Dict[int, int] = field(default_factory=dict)
    consumed: List[int] = field(default_factory=list)           # stream bytes the decode took, per connection
    leftover: List[bytes] = field(default_factory=list)
    cuts: Optional[list] = None
    state: Optional[np.ndarray] = None
    inf_ctx: Optional[np.ndarray] = None
    def_ctx: Optional[np.ndarray] = None
    room_tables: list = field(default_factory=list)             # the broadcast: conn_room behind every pass

    def wire(self, c: int) -> bytes:
        return b"".join(s[c] for s in self.sent)


def all_conn_bytes(res) -> List[bytes]:
    """Responses.conn_bytes for every connection, with one copy of the wires
    and the plan: a connection's plan entries' segments in order."""
    wires = [w.cpu().numpy() for w in (res.echo.plain_wire, res.echo.def_wire, res.ctl_wire)]
    send = res.send_host()
    out = []
    for cs in res.conn_send_host():
        first, count = int(cs["first"]), int(cs["count"])
        out.append(b"".join(wires[int(e["wire"])][int(e["off"]): int(e["off"]) + int(e["len"])].tobytes()
                            for e in send[first: first + count]))
    return out


def run_session(engine, conns: Sequence[Conn], cuts, passes: int, F: Optional[int] = None, rooms=None,
                changes=None, rooms_flags: int = 0, deflate_flags: int = 0) -> SessionRun:
    """The wiring DESIGN section 8 item 8 describes, on the device, pass by
    pass: every connection's buffer is its leftover bytes and the next slice of
    its stream; decode -> messages -> inflate -> join(carry) -> respond (or
    broadcast, with Rooms.update between the passes), gathered; the bytes the
    decode did not consume wait for the next pass; a connection with
    CTL_SHUTDOWN is fed nothing afterwards."""
    import torch

    import gev_amd
    from tests._helpers import gpu_decode, pack_streams
    from tests._messages_model import _dev
    dev = torch.device("cuda", engine.device)
    n = len(conns)
    ext = _dev(np.array([c.ext for c in conns], np.uint8), dev, 1)
    wb = _dev(np.array([c.window_bits for c in conns], np.uint8), dev, 1)
    state = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
    inf_ctx = torch.zeros((n, gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev)
    def_ctx = torch.zeros((n, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    carry = gev_amd.Carry(engine, n, LIMIT, compressed=True)
    ends = [pass_ends(cuts[c], passes, len(conns[c].wire)) for c in range(n)]
    run = SessionRun(consumed=[0] * n, leftover=[b""] * n, cuts=cuts)
    pos = [0] * n
    for p in range(passes):
        bufs = []
        for c in range(n):
            if c in run.shutdown_pass:
                bufs.append(b"")
                continue
            bufs.append(run.leftover[c] + conns[c].wire[pos[c]: ends[c][p]])
            pos[c] = ends[c][p]
        batch = gpu_decode(engine, *pack_streams(bufs), aux_slots=n)
        co = batch.conn_out_host()
        assert not (co["status"] < 0).any()          # decode statuses < 0 are the host's, and no stream here has one
        for c in range(n):
            if c not in run.shutdown_pass:
                k = int(co["consumed"][c])
                run.consumed[c] += k
                run.leftover[c] = bufs[c][k:]
        msgs = engine.messages(batch, state, conn_ext=ext)
        inf = engine.inflate(batch, msgs, LIMIT, state, conn_ext=ext, contexts=inf_ctx, carry=carry)
        bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL, carry=carry)
        if rooms is None:
            res = engine.respond(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, wb, contexts=def_ctx,
                                 flags=deflate_flags, gather=True, max_fragment_bytes=F)
        else:
            res = engine.broadcast(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, rooms, window_bits=wb,
                                   flags=deflate_flags, rooms_flags=rooms_flags, gather=True, max_fragment_bytes=F)
            rooms = rooms.update(engine, changes[p] if len(changes[p]) else None, closed=res)
            run.room_tables.append(rooms.host())
        sent = all_conn_bytes(res)
        for c in range(0, n, 37):                    # the library's own reading of the plan, on a sample
            assert res.conn_bytes(c) == sent[c], (p, c)
        run.sent.append(sent)
        run.gathered.append([bytes(m) for m in res.host_sends()])
        flags = res.conn_send_host()["flags"]
        for c in np.flatnonzero(flags & gev_amd.CTL_SHUTDOWN):
            run.shutdown_pass.setdefault(int(c), p)
        run.carries.append(carry.records_host().copy())
        run.carry_used.append(carry.used)
    run.state = state.cpu().numpy()
    run.inf_ctx = inf_ctx.cpu().numpy()
    run.def_ctx = def_ctx.cpu().numpy()
    return run


LEAD_FILL = 0xA5
LEAD_FILLED = 1 << 20


def lead_header(length: int) -> bytes:
    """An unmasked FIN frame's header, the reserved opcode 0x3, the 64-bit length form."""
    return bytes([0x83, 127]) + length.to_bytes(8, "big")


@dataclass
class FarRun:
    """run_far_session's result; connection 0 is the leading one everywhere."""
    sent: List[bytes]                   # [conn]: the bytes of the send plan
    gathered: List[bytes]               # [conn]: the bytes of the gather
    conn_flags: np.ndarray              # the plan's flags per connection
    decode_summary: np.ndarray
    payload_off: np.ndarray             # per frame record
    first_frame: np.ndarray             # per connection
    aux_off: int
    bodies_in_place: np.ndarray         # BODY_DTYPE, the join without JOIN_ALL
    bodies_copied: np.ndarray           # ... and with it
    body_bytes: List[Tuple[bytes, bytes]]   # per message: (in place, copied)
    seconds: float


def run_far_session(engine, conns: Sequence[Conn], lead: int, F: Optional[int] = None,
                    deflate_flags: int = 0) -> FarRun:
    """One pass of run_session's chain behind a payload arena larger than 4 GiB:
    connection 0 holds one unmasked frame of `lead` payload bytes with a
    reserved opcode (a protocol error: it is sent a 1002 close and nothing
    else), so every payload offset of `conns` behind it, and the aux region
    at the arena's end, lie `lead` bytes up.  The input is assembled on the
    device: the frame's payload is whatever the allocation holds but for its
    first MiB, LEAD_FILL -- where an offset cut to 32 bits would land.

    decode -> messages -> inflate -> join -> respond, gathered, as run_session
    with one pass and without a carry (nothing spans passes; the calls are then
    their NULL-carry forms bit for bit), the capacities those of the session
    without the leading frame.  The join runs twice, without GEVWS_JOIN_ALL
    first: the reply step takes copied bodies only (include/gevws.h), so the
    bodies left in place in the far arena are read back here instead."""
    import time

    import torch

    import gev_amd
    from tests._messages_model import _dev
    t0 = time.perf_counter()
    dev = torch.device("cuda", engine.device)
    n = len(conns) + 1
    rest = np.frombuffer(b"".join(c.wire for c in conns), np.uint8)
    head = lead_header(lead)
    in_bytes = len(head) + lead + rest.size
    d_in = torch.empty(in_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
    d_in[: len(head)] = torch.from_numpy(np.frombuffer(head, np.uint8).copy()).to(dev)
    d_in[len(head): len(head) + LEAD_FILLED] = LEAD_FILL
    d_in[len(head) + lead: in_bytes] = torch.from_numpy(rest.copy()).to(dev)
    d_in[in_bytes:] = 0
    lens = np.array([len(head) + lead] + [len(c.wire) for c in conns], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    n_frames = 1 + sum(len(c.frames) for c in conns)
    lead16 = (lead + 15) // 16 * 16
    near_cap = int(rest.size) + 16 * n_frames + 64
    batch = engine.decode(d_in, in_bytes, torch.from_numpy(np.stack([offs, lens], 1)).to(dev), n,
                          max_frames=n_frames, payload_cap=lead16 + near_cap, aux_slots=n)
    del d_in
    co = batch.conn_out_host()
    assert not (co["status"] < 0).any() and int(co["consumed"][0]) == int(lens[0])
    ds = batch.summary_host().copy()
    ext = _dev(np.array([0] + [c.ext for c in conns], np.uint8), dev, 1)
    wb = _dev(np.array([0] + [c.window_bits for c in conns], np.uint8), dev, 1)
    state = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
    inf_ctx = torch.zeros((n, gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev)
    def_ctx = torch.zeros((n, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    msgs = engine.messages(batch, state, conn_ext=ext)
    nm = int(msgs.summary_host()["frames"])
    inf = engine.inflate(batch, msgs, LIMIT, state, out_cap=4 * near_cap + 16 * nm, conn_ext=ext, contexts=inf_ctx)
    join_cap = (int(inf.summary_host()["payload_bytes"]) + 15) // 16 * 16 + near_cap
    in_place = engine.join(batch, msgs, inf, flags=0, out_cap=join_cap)
    bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL, out_cap=join_cap)
    b0, b1 = in_place.bodies_host().copy(), bodies.bodies_host().copy()
    o0, o1 = in_place.out.cpu().numpy(), bodies.out.cpu().numpy()
    far = batch.payload[lead16: lead16 + near_cap].cpu().numpy()
    body_bytes = []
    for r0, r1 in zip(b0, b1):
        pair = []
        for r, out in ((r0, o0), (r1, o1)):
            off, k, fl = int(r["off"]), int(r["length"]), int(r["flags"])
            if not fl & gev_amd.BODY_WHOLE:
                pair.append(b"")
            elif fl & (gev_amd.BODY_JOINED | gev_amd.BODY_INFLATED):
                pair.append(out[off: off + k].tobytes())
            else:
                assert off >= lead16
                pair.append(far[off - lead16: off - lead16 + k].tobytes())
        body_bytes.append(tuple(pair))
    res = engine.respond(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, wb, contexts=def_ctx,
                         flags=deflate_flags, gather=True, max_fragment_bytes=F)
    sent = all_conn_bytes(res)
    for c in range(0, n, 37):
        assert res.conn_bytes(c) == sent[c], c
    aux_cap = gev_amd._abi.AUX_SLOT * batch.aux_slots
    return FarRun(sent=sent, gathered=[bytes(m) for m in res.host_sends()],
                  conn_flags=res.conn_send_host()["flags"].copy(), decode_summary=ds,
                  payload_off=batch.frames_host()["payload_off"].astype(np.uint64),
                  first_frame=co["first_frame"].astype(np.int64),
                  aux_off=(batch.payload.numel() - 16 - aux_cap) // 16 * 16, bodies_in_place=b0, bodies_copied=b1,
                  body_bytes=body_bytes, seconds=time.perf_counter() - t0)


def observed_carries(run: SessionRun, conns: Sequence[Conn], cuts, passes: int) -> Counter:
    """predicted_carries' counts, read from the carry records the run left behind each pass."""
    OPEN, COMPRESSED = 1, 4     # GEVWS_CARRY_OPEN, GEVWS_CARRY_COMPRESSED
    seen = Counter()
    for p, recs in enumerate(run.carries[:-1]):
        for c in np.flatnonzero(recs["flags"] & OPEN):
            c = int(c)
            if c in run.shutdown_pass and run.shutdown_pass[c] <= p:
                continue
            compressed = bool(int(recs["flags"][c]) & COMPRESSED)
            seen["compressed" if compressed else "plain"] += 1
            if compressed and conns[c].ext & CT:
                seen["compressed, client takeover"] += 1
            ends = pass_ends(cuts[c], passes, len(conns[c].wire))
            if compressed and ends[p + 1] == ends[p] and int(run.carries[p + 1]["flags"][c]) & OPEN:
                seen["compressed, across an idle pass"] += 1
    return seen


# ---------------------------------------------------------------------------- the cases of the two session tests
ECHO_SEED, BROADCAST_SEED = 0x5E5510, 0x5E5B0C
CUTTINGS = ((1, None), (3, None), (7, None), (4, 1000))     # (passes, max_fragment_bytes)
REPLY_KINDS = ("echo plain", "echo deflated", "pong", "ping for pong", "close reply", "1002", "1007")
CARRY_KINDS = ("plain", "compressed", "compressed, client takeover", "compressed, across an idle pass")


@functools.lru_cache(maxsize=None)
def echo_conns() -> List[Conn]:
    return echo_traffic(ECHO_SEED)


@functools.lru_cache(maxsize=None)
def echo_cuts(passes: int):
    """(cuts, classes) of the echo session's cutting into `passes` passes."""
    return make_cuts(echo_conns(), passes, ECHO_SEED + passes)


@functools.lru_cache(maxsize=None)
def broadcast_case() -> BroadcastCase:
    return broadcast_traffic(BROADCAST_SEED)
