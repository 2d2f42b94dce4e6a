"""CPU checks that pin tests/_join_model.py -- the Python restatement of
gevws_join_async / gevws_reply_bodies_async the GPU tests compare the device
with -- on cases whose expected tables are derived by hand."""
import numpy as np

from tests import _join_model as jm
from tests import _messages_model as mm

T, B, C, PING, PONG = 1, 2, 0, 9, 10


def test_two_fragments_join_at_offset_zero():
    d = mm.Decoded([[(0, 0, B, b"ab"), (1, 0, C, b"cde")]])
    w = jm.decoded_join_model(d)
    b = w["bodies"]
    assert b.shape == (1,) and (int(b["off"][0]), int(b["length"][0])) == (0, 5)
    assert int(b["flags"][0]) == jm.WHOLE | jm.JOINED and int(b["opcode"][0]) == B and int(b["conn"][0]) == 0
    assert w["out"].tobytes() == b"abcde" + bytes(11)  # the pad behind the body is zero, not the slots' 0xBF
    assert w["summary"] == dict(frames=1, payload_bytes=16, payload_len=5, errors=0, status=0)
    assert w["written"].all()


def test_a_ping_between_fragments_is_skipped():
    d = mm.Decoded([[(0, 0, T, b"he"), (1, 0, PING, b"PINGPING"), (0, 0, C, b""), (1, 0, PONG, b"x"),
                     (1, 0, C, b"llo")]])
    w = jm.decoded_join_model(d)
    assert w["out"].tobytes() == b"hello" + bytes(11)
    assert int(w["bodies"]["length"][0]) == 5 and w["summary"]["frames"] == 1


def test_base_behind_twenty_inflated_bytes_is_32():
    d = mm.Decoded([[(0, 0, B, b"ab"), (1, 0, C, b"cde")]])
    t = d.model()
    image = np.full(64, 0x11, np.uint8)
    w = jm.join_model(d.frames, d.arena, t["messages"], t["msg_of"], 0, 64, None,
                      dict(payload_bytes=20, status=0), out_image=image)
    assert w["base"] == 32 and int(w["bodies"]["off"][0]) == 32
    assert w["out"].tobytes() == bytes([0x11]) * 32 + b"abcde" + bytes(11) + bytes([0x11]) * 16
    assert w["summary"]["payload_bytes"] == 48
    # a failed inflate gives a zero summary and no records
    z = jm.join_model(d.frames, d.arena, t["messages"], t["msg_of"], 0, 64, None, dict(payload_bytes=20, status=-2))
    assert z["summary"] == jm.zero_summary() and z["bodies"].shape == (0,) and not z["written"].any()


def test_single_frames_stay_in_place_unless_join_all():
    d = mm.Decoded([[(1, 0, B, b"x" * 20), (1, 0, T, b""), (0, 0, B, b"a"), (1, 0, C, b"b")]])
    w = jm.decoded_join_model(d)
    b = w["bodies"]
    assert [int(x) for x in b["flags"]] == [jm.WHOLE, jm.WHOLE, jm.WHOLE | jm.JOINED]
    assert [int(x) for x in b["off"]] == [0, 32, 0]  # the slots of frames 0 and 1 in the arena; d_out offset 0
    assert w["out"].tobytes() == b"ab" + bytes(14)
    assert w["summary"] == dict(frames=3, payload_bytes=16, payload_len=22, errors=0, status=0)
    a = jm.decoded_join_model(d, jm.JOIN_ALL)
    assert [int(x) for x in a["bodies"]["flags"]] == [jm.WHOLE | jm.JOINED] * 3
    assert [int(x) for x in a["bodies"]["off"]] == [0, 32, 32]  # the empty body takes no space
    assert a["out"].tobytes() == b"x" * 20 + bytes(12) + b"ab" + bytes(14)
    assert a["summary"]["payload_bytes"] == 48


def test_what_is_not_delivered():
    conns = [
        [(0, 0, B, b"open")],                                  # no END
        [(1, 0, B, b"ok"), (1, 4, B, b"rsv"), (1, 0, B, b"z")],  # ERR_RSV after one whole message
        [(0, 0, T, b"a"), (1, 0, C, b"\xff")],                 # UTF-8 failure in the second fragment
        (mm.ERR_LEN_MSB, [(1, 0, B, b"never")]),               # status < 0
    ]
    d = mm.Decoded(conns)
    w = jm.decoded_join_model(d, jm.JOIN_ALL)
    b = w["bodies"]
    assert [int(x) for x in b["flags"]] == [0, jm.WHOLE | jm.JOINED, 0]
    assert [int(x) for x in b["status"]] == [0, 0, mm.ERR_UTF8]
    assert [int(x) for x in b["length"]] == [0, 2, 0] and [int(x) for x in b["conn"]] == [0, 1, 2]
    # continued from a carried state: no BEGIN
    st = np.zeros(1, mm.MSG_STATE_DTYPE)
    st["opcode"] = B
    d2 = mm.Decoded([[(1, 0, C, b"tail")]])
    w2 = jm.decoded_join_model(d2, jm.JOIN_ALL, state=st)
    assert int(w2["bodies"]["flags"][0]) == 0 and w2["summary"]["payload_bytes"] == 0


def test_capacity_writes_nothing():
    d = mm.Decoded([[(0, 0, B, b"ab"), (1, 0, C, b"cde")]])
    w = jm.decoded_join_model(d, 0, 15)
    assert w["summary"] == dict(frames=1, payload_bytes=16, payload_len=5, errors=0, status=jm.ERR_CAPACITY)
    assert w["bodies"] is None and np.all(w["out"] == jm.FILL)


def test_reply_lists_by_hand():
    bodies = np.zeros(5, jm.BODY_DTYPE)
    rows = [(0, 5, 0, jm.WHOLE | jm.JOINED), (16, 0, 0, jm.WHOLE | jm.JOINED), (0, 0, 1, 0),
            (16, 7, 1, jm.WHOLE | jm.INFLATED), (32, 3, 2, jm.WHOLE | jm.JOINED)]
    for i, (off, n, c, fl) in enumerate(rows):
        bodies[i]["off"], bodies[i]["length"], bodies[i]["conn"], bodies[i]["flags"] = off, n, c, fl
    w = jm.reply_model(bodies, jm.HANDLER_ECHO_TEXT, np.array([1, 0, 5], np.uint8), np.array([9, 0, 12], np.uint8), 3)
    assert [tuple(int(x) for x in (r["payload_off"], r["length"], r["opcode"], r["window_bits"]))
            for r in w["def_msgs"]] == [(0, 5, 1, 9), (16, 0, 1, 9), (32, 3, 1, 12)]
    assert list(w["def_conn"]) == [0, 0, 2] and list(w["plain_conn"]) == [1]
    p = w["plain"][0]
    assert (int(p["fin"]), int(p["rsv"]), int(p["opcode"]), int(p["masked"]), int(p["length"]), int(p["payload_off"]),
            int(p["payload_len"])) == (1, 0, 1, 0, 7, 16, 7)
    assert list(w["reply_of"]) == [0, 1, -1, 0, 2]
    assert w["def_summary"]["frames"] == 3 and w["plain_summary"]["frames"] == 1
    # no extension table: every reply is plain, binary policy -> opcode 2
    a = jm.reply_model(bodies, jm.HANDLER_ECHO_BINARY, None, None, 3)
    assert a["def_msgs"].shape == (0,) and list(a["plain_conn"]) == [0, 0, 1, 2] and set(a["plain"]["opcode"]) == {2}
    assert jm.reply_model(bodies, jm.HANDLER_NONE, None, None, 3)["plain"].shape == (0,)
    # a body left in its slot, and a connection out of range
    bodies[0]["flags"] = jm.WHOLE
    bad = jm.reply_model(bodies, jm.HANDLER_ECHO_BINARY, None, None, 2)
    assert bad["def_summary"] == dict(frames=0, payload_bytes=0, payload_len=0, errors=2, status=jm.ERR_INVALID)
    assert bad["plain_summary"] == bad["def_summary"] and bad["plain"] is None
