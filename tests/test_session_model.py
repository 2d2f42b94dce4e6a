"""The session tests' checker, pinned on the CPU (tests/_session.py).

The peer-side checker accepts what the reference host server sends for the
echo and the broadcast session, and rejects that output with one thing wrong
in it; and the traffic and the cuttings the GPU tests use hold what those
tests are for, so the choice of inputs is validated here and not discovered on
the card."""
import zlib
from collections import Counter

import numpy as np
import pytest

from oracle import ws_oracle as wo
from tests import _session as s
from tests._session import CLOSE, PING, PONG, D, CT, ST, CheckError

F_TEST = 1000


def frames_of(wire: bytes):
    """A reply's wire bytes, one element a frame."""
    return [wire[f.stream_pos: f.stream_pos + f.header_len + f.header.length] for f in s.parse_wire(wire)]


def find(pred, F=None):
    """The first connection (index, Conn, its reference replies) with pred(conn, replies)."""
    for c, conn in enumerate(s.echo_conns()):
        replies = s.reference_echo_server(conn, F)
        if pred(conn, replies):
            return c, conn, replies
    raise AssertionError("the traffic holds no such connection")


def kinds(conn):
    return [k for k, _ in conn.expected()]


def check(conn, replies, F=None, tally=None):
    s.check_echo_conn(conn, b"".join(replies), F, tally)


# ---------------------------------------------------------------------------- the checker accepts a correct server
@pytest.mark.parametrize("F", (None, F_TEST))
def test_accepts_the_reference_echo_server(F):
    tally, checked = Counter(), 0
    for conn in s.echo_conns():
        check(conn, s.reference_echo_server(conn, F), F, tally)
        checked += 1
    assert checked == len(s.echo_conns()) == 320          # no connection is left out
    assert all(tally[k] > 0 for k in s.REPLY_KINDS), tally
    assert tally["needs the window"] > 0                  # a takeover reply that an empty window does not inflate


@pytest.mark.parametrize("flags,F", ((0, None), (s.SKIP_SENDER, F_TEST)))
def test_accepts_the_reference_broadcast_server(flags, F):
    case = s.broadcast_case()
    views, tables = s.broadcast_view(case, flags)
    sent = s.reference_broadcast_server(case, flags, F)
    tally = Counter()
    for r in range(len(case.conns)):
        s.check_broadcast_conn(case, views, r, [b"".join(sent[p][r]) for p in range(case.passes)], F, tally)
    assert all(tally[k] > 0 for k in ("echo plain", "echo deflated", "pong", "ping for pong", "close reply", "1007"))


# ---------------------------------------------------------------------------- ... and rejects one with a defect
def test_rejects_a_dropped_pong():
    _, conn, replies = find(lambda c, r: "echo" in kinds(c) and any(
        k == "ctl" and x[0] == 0x80 | PONG for k, x in c.expected()))
    i = next(i for i, (k, x) in enumerate(conn.expected()) if k == "ctl" and x[0] == 0x80 | PONG)
    with pytest.raises(CheckError, match="is due|the control reply differs|replies where"):
        check(conn, replies[:i] + replies[i + 1:])


def test_rejects_two_replies_swapped():
    _, conn, replies = find(lambda c, r: len(set(r)) >= 2 and c.dead_at is None)
    i = next(i for i in range(len(replies) - 1) if replies[i] != replies[i + 1])
    swapped = replies[:i] + [replies[i + 1], replies[i]] + replies[i + 2:]
    with pytest.raises(CheckError, match="reply %d: " % i):
        check(conn, swapped)


@pytest.mark.parametrize("ext,what", ((0, "the echo's bytes differ"), (D, "does not inflate to the message")))
def test_rejects_a_flipped_payload_byte(ext, what):
    _, conn, replies = find(lambda c, r: c.ext == ext and any(k == "echo" and len(x) > 20 for k, x in c.expected()))
    i = next(i for i, (k, x) in enumerate(conn.expected()) if k == "echo" and len(x) > 20)
    bad = bytearray(replies[i])
    bad[-3] ^= 0x10
    with pytest.raises(CheckError, match="reply %d: .*%s" % (i, what)):
        check(conn, replies[:i] + [bytes(bad)] + replies[i + 1:])


def test_rejects_a_missing_and_a_wrong_failure_close():
    for code, other in ((1002, 1007), (1007, 1002)):
        _, conn, replies = find(lambda c, r: c.expected() and c.expected()[-1] == ("fail", code))
        with pytest.raises(CheckError, match="%d replies where %d are due" % (len(replies) - 1, len(replies))):
            check(conn, replies[:-1])
        wrong = wo.encode_frame(other.to_bytes(2, "big"), CLOSE, True, 0, False)
        with pytest.raises(CheckError, match="the failure close differs, %d is due" % code):
            check(conn, replies[:-1] + [wrong])


def test_rejects_a_frame_behind_a_close():
    for last in ("ctl", "fail"):
        _, conn, replies = find(lambda c, r: c.dead_at is not None and kinds(c)[-1] == last)
        with pytest.raises(CheckError, match="a frame behind a close frame"):
            check(conn, replies + [wo.encode_frame(b"late", PONG, True, 0, False)])


def test_takeover_reply_against_another_window():
    """A server-takeover connection's second reply compressed against a window
    the peer does not hold (here: one that saw a message the peer was never
    sent, as a window that took in a stripped message would) is rejected.  The
    same reply compressed against an empty window is a legal stream -- RFC 7692
    lets a sender use less history than it may, and the peer's decompressor
    holds a superset -- so the checker must accept it; what notices it is the
    count of replies that need the window, which the session tests assert."""
    _, conn, replies = find(lambda c, r: c.ext == D | ST and c.window_bits == 15 and c.heavy and kinds(c).count("echo") >= 3)
    echoes = [x for k, x in conn.expected() if k == "echo"]
    idx = [i for i, (k, _) in enumerate(conn.expected()) if k == "echo"]
    second = echoes[1]
    assert second and second == echoes[0]                      # a repeat: its honest reply is all history
    alone = s.comp(second, zlib.compressobj(6, zlib.DEFLATED, -conn.window_bits))
    assert len(replies[idx[1]]) < len(alone) // 4
    # the honest reply does not inflate in an empty window (_inflate_takeover.empty_window_differs' test)
    honest = s.parse_wire(replies[idx[1]])[0].payload
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(honest + s.TAIL)
    base = Counter()
    check(conn, replies, None, base)
    # (a) against an empty window: accepted, and one reply fewer needs the window
    tally = Counter()
    legal = replies[:idx[1]] + [wo.encode_frame(alone, 1, True, 4, False)] + replies[idx[1] + 1:]
    check(conn, legal, None, tally)
    assert tally["needs the window"] == base["needs the window"] - 1
    # (b) against a window that holds a phantom message in the first one's place: rejected
    co = zlib.compressobj(6, zlib.DEFLATED, -conn.window_bits)
    s.comp(bytes(reversed(echoes[0])), co)
    phantom = wo.encode_frame(s.comp(second, co), 1, True, 4, False)
    with pytest.raises(CheckError, match="reply %d: the echo does not inflate to the message" % idx[1]):
        check(conn, replies[:idx[1]] + [phantom] + replies[idx[1] + 1:])


def fragmented(F):
    """A deflate connection with a reply of three fragments or more under F."""
    c, conn, replies = find(lambda c, r: c.ext & D and any(len(frames_of(x)) >= 3 for x in r), F)
    i = next(i for i, x in enumerate(replies) if len(frames_of(x)) >= 3)
    return conn, replies, i, frames_of(replies[i])


def test_rejects_rsv1_on_a_continuation():
    conn, replies, i, fr = fragmented(F_TEST)
    fr[1] = bytes([fr[1][0] | 0x40]) + fr[1][1:]
    with pytest.raises(CheckError, match="on a continuation"):
        check(conn, replies[:i] + [b"".join(fr)] + replies[i + 1:], F_TEST)


def test_rejects_a_fragment_longer_than_the_limit():
    conn, replies, i, fr = fragmented(F_TEST)
    parts = [f.payload for f in s.parse_wire(replies[i])]
    parts[0], parts[1] = parts[0] + parts[1][:1], parts[1][1:]     # F + 1 bytes, then F - 1
    wire = b"".join(wo.encode_frame(p, 1 if k == 0 else 0, k == len(parts) - 1, 4 if k == 0 else 0, False)
                    for k, p in enumerate(parts))
    with pytest.raises(CheckError, match="fragment pattern"):
        check(conn, replies[:i] + [wire] + replies[i + 1:], F_TEST)
    with pytest.raises(CheckError, match="without a limit"):       # and fragments where no limit was asked for
        check(conn, replies, None)


def test_rejects_a_control_frame_between_two_fragments():
    conn, replies, i, fr = fragmented(F_TEST)
    fr.insert(1, wo.encode_frame(b"between", PONG, True, 0, False))
    with pytest.raises(CheckError, match="a control frame between a reply's fragments"):
        check(conn, replies[:i] + [b"".join(fr)] + replies[i + 1:], F_TEST)


def test_rejects_rsv1_without_deflate_and_masked_frames():
    _, conn, replies = find(lambda c, r: c.ext == 0 and kinds(c) and kinds(c)[0] == "echo" and len(c.expected()[0][1]) < 100)
    data = conn.expected()[0][1]
    with pytest.raises(CheckError, match="rsv 4"):
        check(conn, [wo.encode_frame(data, 1, True, 4, False)] + replies[1:])
    with pytest.raises(CheckError, match="masked"):
        check(conn, [wo.encode_frame(data, 1, True, 0, True, b"\x00\x00\x00\x00")] + replies[1:])


def test_rejects_a_broadcast_to_a_non_member_and_one_missing():
    case = s.broadcast_case()
    views, tables = s.broadcast_view(case, 0)
    sent = s.reference_broadcast_server(case, 0, None)
    p, member = next((p, r) for p in range(case.passes) for r in range(len(case.conns))
                     if sum(k == "echo" for k, _ in views[p][r]) >= 2 and not case.conns[r].ext)
    i = next(i for i, (k, _) in enumerate(views[p][member]) if k == "echo")
    outsider = next(r for r in range(len(case.conns)) if case.rooms0[r] == s.ROOM_NONE and not case.conns[r].ext
                    and all(r != int(w) for ch in case.changes for w, _ in ch))
    wires = lambda r, mine: [b"".join(mine if q == p else sent[q][r]) for q in range(case.passes)]  # noqa: E731
    with pytest.raises(CheckError, match="pass %d, recipient %d: " % (p, outsider)):
        s.check_broadcast_conn(case, views, outsider, wires(outsider, [sent[p][member][i]] + sent[p][outsider]), None)
    with pytest.raises(CheckError, match="pass %d, recipient %d: " % (p, member)):
        s.check_broadcast_conn(case, views, member, wires(member, sent[p][member][:i] + sent[p][member][i + 1:]), None)
    # ... and the publications of a room in another order
    j = next(j for j in range(i + 1, len(views[p][member])) if views[p][member][j][0] == "echo"
             and views[p][member][j] != views[p][member][i])
    mine = list(sent[p][member])
    mine[i], mine[j] = mine[j], mine[i]
    with pytest.raises(CheckError, match="pass %d, recipient %d: reply %d" % (p, member, i)):
        s.check_broadcast_conn(case, views, member, wires(member, mine), None)


# ---------------------------------------------------------------------------- the inputs the GPU tests use
def test_echo_traffic_holds_its_cases():
    conns = s.echo_conns()
    heavy = [c for c in conns if c.heavy]
    assert len(conns) == 320 and conns[-1].heavy and len(heavy) >= 20
    assert {(c.ext, c.window_bits) for c in heavy} == set(s.CLASSES) == {(c.ext, c.window_bits) for c in conns}
    assert sum(len(c.wire) for c in conns) <= 3 << 19
    echoes = [x for c in heavy for k, x in c.expected() if k == "echo"]
    assert sum(70000 <= len(x) <= 100000 for x in echoes) >= 8 and b"" in echoes
    assert all(len(x) < s.LIMIT for x in echoes)
    assert any(f.header_len == 14 and f.header.length > 0xFFFF for c in heavy for f in c.frames)
    assert {f.header_len for c in conns for f in c.frames} >= {6, 8, 14}
    # a message in 7 fragments or more with pings and pongs between them
    many = [c for c in heavy if sum(not f.header.opcode & 8 for f in c.frames) >= 7
            and {PING, PONG} <= {f.header.opcode for f in c.frames}]
    assert len(many) >= 4
    ends = Counter((k, x) for c in heavy if c.dead_at is not None for k, x in c.expected()[-1:] if k == "fail")
    assert ends[("fail", 1002)] >= 4 and ends[("fail", 1007)] >= 4
    behind = [c for c in heavy if c.dead_at is not None and c.dead_at + 1 < len(c.frames)]
    assert len(behind) >= 8                                   # frames behind a close or a failure
    assert any(c.ext & CT and c.dead_at is not None for c in heavy)
    # a client that keeps its context sends messages that an empty window does not inflate
    needs = 0
    for c in heavy:
        parts = []
        for i, f in enumerate(c.frames[: len(c.frames) if c.dead_at is None else c.dead_at]):
            if f.header.opcode & 8 or not c.ext & CT:
                continue
            parts = [f.payload] if f.header.opcode else parts + [f.payload]
            if f.header.fin and c.info[i][1]:
                want = next(x for j, k, x in c.items if j == i)
                try:
                    needs += zlib.decompressobj(-15).decompress(b"".join(parts) + s.TAIL) != want
                except zlib.error:
                    needs += 1
    assert needs >= 4


@pytest.mark.parametrize("passes", [p for p, _ in s.CUTTINGS if p > 1])
def test_every_cutting_opens_every_carry(passes):
    conns = s.echo_conns()
    cuts, _ = s.echo_cuts(passes)
    assert all(len(m) == passes - 1 and m == sorted(m) and 0 <= m[0] and m[-1] <= len(c.wire)
               for m, c in zip(cuts, conns))
    seen = s.predicted_carries(conns, cuts, passes)
    assert all(seen[k] > 0 for k in s.CARRY_KINDS), seen
    assert any(len(set(m)) < len(m) for m in cuts)            # a pass without bytes


def test_the_cuttings_cut_everywhere():
    classes = Counter()
    for passes, _ in s.CUTTINGS:
        classes.update(s.echo_cuts(passes)[1])
    assert all(classes[k] > 0 for k in s.CUT_CLASSES), classes


def test_broadcast_traffic_holds_its_cases():
    case = s.broadcast_case()
    n = len(case.conns)
    assert n == 300 and case.n_rooms == 7 and case.passes == 4
    assert {c.ext for c in case.conns} == {0, D, D | ST}
    assert np.count_nonzero(case.rooms0 == s.ROOM_NONE) >= 10
    closers = [c for c in range(n) if case.conns[c].dead_at is not None]
    assert len(closers) == 3 and sorted(kinds(case.conns[c])[-1] for c in closers) == ["ctl", "ctl", "fail"]
    assert sum(len(x) == 40000 for c in case.conns for k, x in c.expected() if k == "echo") == 2
    assert 55 <= sum(len(ch) for ch in case.changes) <= 70
    assert any(len(set(int(w) for w, _ in ch)) < len(ch) for ch in case.changes)      # a connection named twice
    joined = [int(w) for ch in case.changes for w, _ in ch if int(w) in closers]
    assert joined                                             # a join in the pass that closes the connection
    for flags in (0, s.SKIP_SENDER):
        views, tables = s.broadcast_view(case, flags)
        assert all(tables[-1][c] == s.ROOM_NONE for c in closers)
        # rooms with plain, deflate and server-takeover members that are sent a publication
        got = {case.conns[r].ext for p in range(case.passes) for r in range(n)
               if any(k == "echo" for k, _ in views[p][r])}
        assert got == {0, D, D | ST}
    seen = s.predicted_carries(case.conns, case.cuts, case.passes)
    assert seen["plain"] > 0 and seen["compressed"] > 0
