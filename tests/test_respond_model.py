"""Pins tests/_respond_model.py (the control step's and the send plan's
contracts) on the CPU: every control reply against oracle.ws_oracle.on_message /
handle_close, and the cut kinds, the close codes, the flag, the stripped bodies
and the plan order by hand-derived cases."""
import numpy as np

from oracle import ws_oracle as wo
from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm

T, B, C, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
NO = rm.NO_FRAME


def control(conns, flags=0, state=None, inflated_status=None, **kw):
    d = mm.Decoded(conns)
    t = rm.tables_of(d, state, inflated_status)
    want = rm.control_model(d.frames, d.conn_out, d.n_decoded, d.arena, t["msg_of"], t["messages"], t["conn_msg"],
                            t["bodies"], flags, **kw)
    return d, t, want


def wire_of(op: int, payload: bytes) -> bytes:
    return wo.frame_to_bytes(*wo.new_frame(op, True, payload))


def cuts_of(want):
    return [(int(r["cut_frame"]), int(r["close_code"]), int(r["flags"])) for r in want["conn_ctl"]]


CLOSE_PAYLOADS = [
    b"", b"\x03", (1000).to_bytes(2, "big"), (1000).to_bytes(2, "big") + b"bye", (999).to_bytes(2, "big") + b"x",
    (1005).to_bytes(2, "big"), (1006).to_bytes(2, "big") + b"r", (1015).to_bytes(2, "big"), (1004).to_bytes(2, "big"),
    (1012).to_bytes(2, "big"), (2999).to_bytes(2, "big"), (3000).to_bytes(2, "big") + "grüß".encode(),
    (4999).to_bytes(2, "big"), (1001).to_bytes(2, "big") + b"\xc3\x28", (1000).to_bytes(2, "big") + b"\xed\xa0\x80",
    (1000).to_bytes(2, "big") + b"r" * 123, (1011).to_bytes(2, "big") + b"\xf0\x9f\x98\x80" * 30,
    (0).to_bytes(2, "big"), (65535).to_bytes(2, "big") + b"z",
]


def test_every_control_reply_is_the_oracles():
    """One connection per close payload, pings and pongs before it: each reply
    of the model == HandlerWrap.OnMessage's bytes for that frame."""
    conns = []
    for i, p in enumerate(CLOSE_PAYLOADS):
        conns.append([(1, 0, PING, b"p%d" % i), (1, 0, PONG, b""), (1, 0, PING, bytes(range(125))), (1, 0, CLOSE, p),
                      (1, 0, PING, b"behind the close")])
    d, t, want = control(conns)
    assert len(want["replies"]) == 4 * len(conns) and want["summary"]["errors"] == len(conns)
    for f, c, op, payload in want["replies"]:
        h = wo.Header(fin=True, opcode=int(d.frames["opcode"][f]), length=int(d.frames["length"][f]))
        off = int(d.frames["payload_off"][f])
        reply, shutdown = wo.on_message(h, d.arena[off: off + h.length].tobytes(), wo.HANDLER_NONE)
        assert wire_of(op, payload) == reply, (f, c)
        assert shutdown == (op == 8) and f <= int(want["conn_ctl"]["cut_frame"][c])
        if op == 8:
            assert reply == wo.handle_close(h, CLOSE_PAYLOADS[c]) and f == 5 * c + 3
    # the records say the same: a payload reply points at the frame's slot, a close body at its aux slot
    ctl = want["ctl"]
    assert np.all(ctl["fin"] == 1) and not ctl["rsv"].any() and not ctl["masked"].any()
    slots = [k for k in range(len(ctl)) if ctl["opcode"][k] == 8 and ctl["length"][k]]
    assert [int(ctl["payload_off"][k]) for k in slots] == [rm.AUX_SLOT * i for i in range(len(slots))]
    assert want["summary"]["payload_bytes"] == len(slots) == len(CLOSE_PAYLOADS) - 1
    assert all(fl == rm.SHUTDOWN and code == 0 for _, code, fl in cuts_of(want))


def test_the_flag_drops_the_ping_for_a_pong():
    conns = [[(1, 0, PONG, b"a"), (1, 0, PING, b"b"), (1, 0, PONG, b"")]]
    _, _, want = control(conns)
    assert [(f, op) for f, _, op, _ in want["replies"]] == [(0, 9), (1, 10), (2, 9)]
    _, _, want = control(conns, flags=rm.NO_PING_FOR_PONG)
    assert [(f, op, p) for f, _, op, p in want["replies"]] == [(1, 10, b"b")]
    assert list(want["ctl_of"]) == [-1, 0, -1] and cuts_of(want) == [(NO, 0, 0)]


def test_cut_kinds_and_close_codes():
    good = (1, 0, B, b"good")
    conns = [
        [good, (1, 0, CLOSE, b""), good],                        # 0 (a) bare close, a message behind it
        [good, (1, 4, B, b"rsv")],                               # 1 (b) ERR_RSV
        [good, (1, 0, 5, b"")],                                  # 2 (b) ERR_OPCODE
        [good, (0, 0, PING, b"")],                               # 3 (b) ERR_CONTROL
        [good, (1, 0, C, b"")],                                  # 4 (b) ERR_CONTINUATION
        [good, (0, 0, T, b"a"), (1, 0, T, b"b")],                # 5 (b) ERR_INTERLEAVE
        [good, (0, 0, T, b"ok"), (1, 0, C, b"\xff"), good],      # 6 (b) ERR_UTF8
        [good, (1, 0, B, b"broken"), (1, 0, PING, b""), good],   # 7 (c) a failed inflate
        [(1, 0, B, b"too big"), good],                           # 8 (c) over max_message_bytes
        [good, (1, 4, CLOSE, b"")],                              # 9 a close frame that fails a check: (b) wins
        [good, (1, 0, PING, b"only")],                           # 10 no cut
    ]
    # messages 0-1, 2, 3, 4, 5, 6-7, 8-9 belong to connections 0-6: connection 7's are 10-12, connection 8's 13-14
    d, t, want = control(conns, inflated_status={11: rm.ERR_DEFLATE, 13: rm.ERR_TOO_BIG})
    first = [int(x) for x in d.conn_out["first_frame"]]
    S, F = rm.SHUTDOWN, rm.SHUTDOWN | rm.FAILED
    assert cuts_of(want) == [
        (first[0] + 1, 0, S), (first[1] + 1, 1002, F), (first[2] + 1, 1002, F), (first[3] + 1, 1002, F),
        (first[4] + 1, 1002, F), (first[5] + 2, 1002, F), (first[6] + 2, 1007, F), (first[7] + 1, 1007, F),
        (first[8], 1009, F), (first[9] + 1, 1002, F), (NO, 0, 0)]
    assert want["summary"] == dict(frames=11, payload_bytes=9, payload_len=0, errors=10, status=0)
    # one reply per cut, the failure close a 2-byte body; the ping behind connection 7's cut gets nothing
    per = {c: rm.conn_replies(want, c) for c in range(len(conns))}
    assert per[0] == [(first[0] + 1, 8, b"")] and per[10] == [(first[10] + 1, 10, b"only")]
    for c, code in ((1, 1002), (5, 1002), (6, 1007), (7, 1007), (8, 1009), (9, 1002)):
        assert per[c] == [(cuts_of(want)[c][0], 8, code.to_bytes(2, "big"))], c
    # bodies: before the cut kept, the failed message left as it is, behind the cut CLOSED
    b, w = t["bodies"], want["bodies"]
    status = [int(x) for x in w["status"]]
    m_of = lambda c: int(t["conn_msg"]["first_message"][c])  # noqa: E731
    assert status[m_of(0)] == 0 and status[m_of(0) + 1] == rm.ERR_CLOSED and not int(w["flags"][m_of(0) + 1])
    assert status[m_of(6) + 1] == mm.ERR_UTF8                      # the failed message itself
    assert status[m_of(7) + 1] == rm.ERR_DEFLATE and status[m_of(7) + 2] == rm.ERR_CLOSED
    assert status[m_of(8)] == rm.ERR_TOO_BIG and status[m_of(8) + 1] == rm.ERR_CLOSED
    closed = np.flatnonzero(w["status"] == rm.ERR_CLOSED)
    assert list(closed) == [m_of(0) + 1, m_of(7) + 2, m_of(8) + 1]
    assert not w["off"][closed].any() and not w["length"][closed].any() and np.all(w["conn"][closed] == b["conn"][closed])
    keep = np.setdiff1d(np.arange(len(w)), closed)
    assert w[keep].tobytes() == b[keep].tobytes()
    # msg_end: the last data frame of every message with END
    assert int(want["msg_end"][m_of(5) + 1]) == NO                 # left open by the interleave error
    assert int(want["msg_end"][m_of(6) + 1]) == NO                 # a UTF-8 failure has no END
    assert int(want["msg_end"][m_of(7) + 2]) == first[7] + 3      # behind the cut, and still the message's end


def test_close_inside_a_fragmented_message_and_quiet_connections():
    st = np.zeros(5, mm.MSG_STATE_DTYPE)
    st[2]["failed"] = mm.ERR_OPCODE
    conns = [
        [(0, 0, T, b"he"), (1, 0, PING, b"mid"), (1, 0, CLOSE, (1000).to_bytes(2, "big")), (1, 0, C, b"llo")],
        [(0, 0, B, b"ab"), (1, 0, PING, b"between"), (1, 0, C, b"cd"), (1, 0, PING, b"behind the FIN")],
        [(1, 0, PING, b"comes in failed")],
        (mm.ERR_LEN_MSB, [(1, 0, PING, b"before the bad header")]),
        [],
    ]
    d, t, want = control(conns, state=st)
    assert cuts_of(want) == [(2, 0, rm.SHUTDOWN), (NO, 0, 0), (NO, 0, 0), (NO, 0, 0), (NO, 0, 0)]
    assert [(f, c, op) for f, c, op, _ in want["replies"]] == [(1, 0, 10), (2, 0, 8), (5, 1, 10), (7, 1, 10)]
    assert list(want["ctl_of"]) == [-1, 0, 1, -1, -1, 2, -1, 3, -1, -1]
    # the message around the close ends behind it: stripped; connection 1's keeps its body
    assert [int(x) for x in want["bodies"]["status"]] == [rm.ERR_CLOSED, 0]
    assert [int(x) for x in want["msg_end"]] == [3, 6]
    assert want["summary"] == dict(frames=4, payload_bytes=1, payload_len=0, errors=1, status=0)


def test_gates_capacity_and_malformed_tables():
    conns = [[(1, 0, B, b"m"), (1, 0, CLOSE, b"\x03\xe8")], [(1, 0, B, b"m"), (1, 4, B, b"")]]
    d, t, want = control(conns, aux_cap=2 * rm.AUX_SLOT)
    assert want["summary"]["status"] == 0 and want["summary"]["payload_bytes"] == 2
    _, _, short = control(conns, aux_cap=2 * rm.AUX_SLOT - 1)
    assert short["summary"] == dict(frames=2, payload_bytes=2, payload_len=0, errors=2, status=rm.ERR_CAPACITY)
    assert short["ctl"] is None and short["bodies"] is None
    for kw in (dict(msg_status=-2), dict(join_status=-2)):
        _, _, g = control(conns, **kw)
        assert g["summary"] == rm.zero_summary() and g["ctl"] is None
    args = lambda tt: (d.frames, d.conn_out, d.n_decoded, d.arena, tt["msg_of"], tt["messages"], tt["conn_msg"],  # noqa: E731
                       tt["bodies"])
    bad = dict(t, msg_of=t["msg_of"].copy())
    bad["msg_of"][0] = 2
    assert rm.control_model(*args(bad))["summary"] == dict(rm.zero_summary(), errors=1, status=rm.ERR_INVALID)
    bad["msg_of"][2] = -2
    assert rm.control_model(*args(bad))["summary"]["errors"] == 2
    bad = dict(t, conn_msg=t["conn_msg"].copy())
    bad["conn_msg"]["error_frame"][1] = 1   # connection 0's frame
    assert rm.control_model(*args(bad))["summary"] == dict(rm.zero_summary(), errors=1, status=rm.ERR_INVALID)
    assert rm.control_model(d.frames, d.conn_out, 0, d.arena, t["msg_of"], t["messages"], t["conn_msg"],
                            t["bodies"])["summary"] == rm.zero_summary()


def test_plan_order():
    """A pong stands before the reply to the message whose fragments surround
    the ping; each connection's entries are one run, wires mixed."""
    conns = [
        [(0, 0, B, b"ab"), (1, 0, PING, b"mid"), (1, 0, C, b"cd"), (1, 0, PING, b"after"), (1, 0, B, b"second")],
        [(1, 0, T, b"deflate connection"), (1, 0, CLOSE, b""), (1, 0, T, b"behind")],
        [],
        [(1, 0, B, b"x"), (1, 1, B, b"fails")],
    ]
    d, t, ctl = control(conns)
    ext = np.array([0, 1, 0, 0], np.uint8)
    rep = jm.reply_model(ctl["bodies"], jm.HANDLER_ECHO_BINARY, ext, None, 4)
    assert list(rep["reply_of"]) == [0, 1, 0, -1, 2]
    # wire offsets as three encodes would give them: (header 2 bytes + payload) back to back
    sizes = [[2 + int(x) for x in rep["plain"]["payload_len"]], [2 + 7],
             [2 + int(x) for x in ctl["ctl"]["payload_len"]]]
    wires = [(np.concatenate([[0], np.cumsum(s)[:-1]]).astype(np.uint64), len(s), int(sum(s))) for s in sizes]
    plan = rm.plan_model(d.n_decoded, d.conn_out, t["msg_of"], ctl["msg_end"], rep["reply_of"], 5, ext, ctl["ctl_of"],
                         ctl["conn_ctl"], wires)
    send = plan["send"]
    assert [(int(e["frame"]), int(e["conn"]), int(e["wire"])) for e in send] == [
        (1, 0, 2), (2, 0, 0), (3, 0, 2), (4, 0, 0), (5, 1, 1), (6, 1, 2), (8, 3, 0), (9, 3, 2)]
    assert [(int(e["off"]), int(e["len"])) for e in send] == [(0, 5), (0, 6), (5, 7), (6, 8), (0, 9), (12, 2), (14, 3),
                                                             (14, 4)]
    cs = plan["conn_send"]
    assert [(int(r["first"]), int(r["count"]), int(r["bytes"]), int(r["flags"])) for r in cs] == [
        (0, 4, 26, 0), (4, 2, 11, rm.SHUTDOWN), (6, 0, 0, 0), (6, 2, 7, rm.SHUTDOWN | rm.FAILED)]
    assert plan["summary"] == dict(frames=8, payload_bytes=44, payload_len=0, errors=2, status=0)
    # capacity, gates, malformed indices
    short = rm.plan_model(d.n_decoded, d.conn_out, t["msg_of"], ctl["msg_end"], rep["reply_of"], 5, ext,
                          ctl["ctl_of"], ctl["conn_ctl"], wires, max_sends=7)
    assert short["send"] is None and short["summary"]["status"] == rm.ERR_CAPACITY and short["summary"]["frames"] == 8
    gated = rm.plan_model(d.n_decoded, d.conn_out, t["msg_of"], ctl["msg_end"], rep["reply_of"], 5, ext,
                          ctl["ctl_of"], ctl["conn_ctl"], wires, gate_ok=False)
    assert gated["summary"] == rm.zero_summary()
    bad = rep["reply_of"].copy()
    bad[4] = 3   # the plain list has three entries
    inv = rm.plan_model(d.n_decoded, d.conn_out, t["msg_of"], ctl["msg_end"], bad, 5, ext, ctl["ctl_of"],
                        ctl["conn_ctl"], wires)
    assert inv["summary"] == dict(rm.zero_summary(), errors=1, status=rm.ERR_INVALID) and inv["send"] is None
