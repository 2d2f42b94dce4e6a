"""Pins tests/_carry_model.py, the plain-Python restatement of
gevws_join_carry_async that the GPU tests compare the device with: hand-derived
cases, and the cut-invariance property -- however a stream of frames is cut
into passes, the delivered messages are those of the uncut batch."""
import zlib

import numpy as np

from tests import _carry_model as cm
from tests import _inflate_gpu_model as gm
from tests import _join_model as jm
from tests import _messages_model as mm

T, B, C, PING = 1, 2, 0, 9
RSV1 = 4


def rec(w, c):
    r = w["carry"][c]
    return tuple(int(r[k]) for k in ("off", "length", "opcode", "flags", "status"))


def summ(s):
    return tuple(s[k] for k in ("frames", "payload_bytes", "payload_len", "errors", "status"))


def body(w, m):
    b = w["bodies"][m]
    return int(b["flags"]), int(b["status"]), int(b["off"]), int(b["length"])


def test_two_passes():
    p1, p2 = cm.chain_model([[[(0, 0, B, b"hello ")]], [[(1, 0, C, b"world")]]], 1 << 20)
    w = p1[2]
    assert body(w, 0) == (0, 0, 0, 0) and summ(w["summary"]) == (0, 0, 0, 0, 0)
    assert rec(w, 0) == (0, 6, B, cm.OPEN, 0) and summ(w["carry_summary"]) == (1, 16, 6, 0, 0)
    assert w["carry_dst"].tobytes() == b"hello " + bytes(10)
    w = p2[2]
    assert body(w, 0) == (jm.WHOLE | jm.JOINED, 0, 0, 11) and summ(w["summary"]) == (1, 16, 11, 0, 0)
    assert w["out"].tobytes() == b"hello world" + bytes(5)
    assert rec(w, 0) == (0, 0, 0, 0, 0) and summ(w["carry_summary"]) == (0, 0, 0, 0, 0) and w["carry_dst"].size == 0
    # a continued body is JOINED without JOIN_ALL too (one frame in this pass)
    assert body(cm.chain_model([[[(0, 0, B, b"hello ")]], [[(1, 0, C, b"world")]]], 1 << 20, flags=0)[1][2], 0) == \
        (jm.WHOLE | jm.JOINED, 0, 0, 11)


def test_three_passes_with_idle_passes_between():
    # (a second connection in front: the carry's offsets are not all 0)
    passes = [[[(0, 0, B, b"0123456789abcdefXY")], [(0, 0, T, b"ab")]],
              [[], []],                                      # no frames at all
              [[], [(1, 0, PING, b"only a ping")]],
              [[], [(0, 0, C, b"cd"), (1, 0, PING, b""), (0, 0, C, b"")]],
              [[(1, 0, C, b"!")], [(1, 0, C, b"e")]]]
    r = [x[2] for x in cm.chain_model(passes, 1 << 20)]
    assert rec(r[0], 0) == (0, 18, B, cm.OPEN, 0) and rec(r[0], 1) == (32, 2, T, cm.OPEN, 0)
    assert r[0]["carry_dst"].tobytes() == b"0123456789abcdefXY" + bytes(14) + b"ab" + bytes(14)
    for k in (1, 2):  # the records move forward unchanged in meaning, the bytes with them
        assert rec(r[k], 0) == (0, 18, B, cm.OPEN, 0) and rec(r[k], 1) == (32, 2, T, cm.OPEN, 0)
        assert r[k]["carry_dst"].tobytes() == r[0]["carry_dst"].tobytes()
        assert summ(r[k]["carry_summary"]) == (2, 48, 20, 0, 0)
    assert summ(r[1]["summary"]) == summ(r[2]["summary"]) == (0, 0, 0, 0, 0)
    assert rec(r[3], 1) == (32, 4, T, cm.OPEN, 0) and r[3]["carry_dst"][32:48].tobytes() == b"abcd" + bytes(12)
    assert cm.delivered(r[4]) == [(0, B, b"0123456789abcdefXY!"), (1, T, b"abcde")]
    assert [int(b["off"]) for b in r[4]["bodies"]] == [0, 32]
    assert not r[4]["carry"].view(np.uint8).any()


def test_lost_over_the_limit():
    passes = [[[(0, 0, B, b"abc")]],
              [[(0, 0, C, b"de")]],                        # 5 > 4: LOST
              [[(1, 0, PING, b"")]],                       # stays LOST
              [[(1, 0, C, b"f"), (1, 0, B, b"next"), (0, 0, B, b"open")]]]
    r = [x[2] for x in cm.chain_model(passes, 4)]
    assert rec(r[0], 0) == (0, 3, B, cm.OPEN, 0)
    assert rec(r[1], 0) == (0, 0, B, cm.LOST, cm.ERR_TOO_BIG) and summ(r[1]["carry_summary"]) == (0, 0, 0, 1, 0)
    assert body(r[1], 0) == (0, 0, 0, 0)
    assert rec(r[2], 0) == (0, 0, B, cm.LOST, cm.ERR_TOO_BIG) and summ(r[2]["carry_summary"]) == (0, 0, 0, 0, 0)
    # its END is undelivered with status 8; the next message is delivered, the one after it carried
    assert body(r[3], 0) == (0, cm.ERR_TOO_BIG, 0, 0) and body(r[3], 1) == (jm.WHOLE | jm.JOINED, 0, 0, 4)
    assert rec(r[3], 0) == (0, 4, B, cm.OPEN, 0) and summ(r[3]["carry_summary"]) == (1, 16, 4, 0, 0)
    # exactly the limit is delivered; one byte more that ends in the pass is body status 8, counted once
    ok = cm.chain_model([[[(0, 0, B, b"abc")]], [[(1, 0, C, b"d")]]], 4)[1][2]
    assert body(ok, 0) == (jm.WHOLE | jm.JOINED, 0, 0, 4) and summ(ok["carry_summary"]) == (0, 0, 0, 0, 0)
    over = cm.chain_model([[[(0, 0, B, b"abc")]], [[(1, 0, C, b"de")]]], 4)[1][2]
    assert body(over, 0) == (0, cm.ERR_TOO_BIG, 0, 0) and summ(over["carry_summary"]) == (0, 0, 0, 1, 0)
    assert rec(over, 0) == (0, 0, 0, 0, 0) and summ(over["summary"]) == (0, 0, 0, 0, 0)


def test_lost_nothing_carried_in():
    """The state says a message is open, the carry holds nothing of it."""
    d = mm.Decoded([[(0, 0, C, b"middle")], [(1, 0, C, b"tail")]])
    st = np.zeros(2, mm.MSG_STATE_DTYPE)
    st["opcode"] = B
    w = cm.carry_model(d.frames, d.arena, d.model(st), 2, 1 << 20, None, None, jm.JOIN_ALL)
    assert rec(w, 0) == (0, 0, B, cm.LOST, 0) and rec(w, 1) == (0, 0, 0, 0, 0)
    assert body(w, 0) == (0, 0, 0, 0) and body(w, 1) == (0, 0, 0, 0)
    assert summ(w["carry_summary"]) == (0, 0, 0, 0, 0)


def test_lost_compressed():
    def model(d, state):
        return gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, state, np.array([1], np.uint8))
    x = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = (x.compress(b"a compressed message") + x.flush(zlib.Z_SYNC_FLUSH))[:-4]
    passes = [[[(0, RSV1, T, z[:5])]], [[(0, 0, C, z[5:9])]], [[(1, 0, C, z[9:]), (0, 0, T, b"plain")]]]
    r = [x[2] for x in cm.chain_model(passes, 1 << 20, model=model)]
    assert rec(r[0], 0) == (0, 0, T, cm.LOST, 0) and rec(r[1], 0) == (0, 0, T, cm.LOST, 0)
    assert body(r[2], 0) == (0, 0, 0, 0)
    assert rec(r[2], 0) == (0, 5, T, cm.OPEN, 0)  # LOST lasted until that message's END and no longer


def test_an_error_drops_the_carry():
    passes = [[[(0, 0, B, b"abc")], [(0, 0, T, b"abc")], [(0, 0, B, b"kept")]],
              [[(1, 0, B, b"interleaved")], [(0, 0, C, b"\xff")], [(0, 0, C, b"!")]],
              [[(1, 0, C, b"x")], [(1, 0, C, b"x")], [(1, 0, C, b"?")]]]
    ch = cm.chain_model(passes, 1 << 20)
    assert [int(x) for x in ch[1][1]["conn_msg"]["error"]] == [mm.ERR_INTERLEAVE, mm.ERR_UTF8, 0]
    r = [x[2] for x in ch]
    assert rec(r[1], 0) == rec(r[1], 1) == (0, 0, 0, 0, 0) and rec(r[1], 2) == (0, 5, B, cm.OPEN, 0)
    assert r[1]["carry_dst"].tobytes() == b"kept!" + bytes(11)
    assert rec(r[2], 0) == rec(r[2], 1) == (0, 0, 0, 0, 0)  # sticky-failed: no messages, and the carry stays zero
    assert cm.delivered(r[2]) == [(2, B, b"kept!?")]


def test_malformed_capacity_and_gates():
    d = mm.Decoded([[(1, 0, C, b"tail")], [(0, 0, B, b"open")]])
    st = np.zeros(2, mm.MSG_STATE_DTYPE)
    st["opcode"][0] = B
    t = d.model(st)
    cin = np.zeros(2, cm.CARRY_DTYPE)
    cin[0] = (16, 5, B, cm.OPEN, 0, [0] * 13)
    src = np.frombuffer(bytes(16) + b"head " + bytes(11), np.uint8)
    w = cm.carry_model(d.frames, d.arena, t, 2, 100, cin, src, jm.JOIN_ALL, carry_src_bytes=21)
    assert cm.delivered(w) == [(0, B, b"head tail")] and rec(w, 1) == (0, 4, B, cm.OPEN, 0)
    inv = dict(jm.zero_summary(), errors=1, status=jm.ERR_INVALID)
    w = cm.carry_model(d.frames, d.arena, t, 2, 100, cin, src, jm.JOIN_ALL, 64, 64, carry_src_bytes=20)
    assert w["summary"] == w["carry_summary"] == inv and w["bodies"] is None and w["carry"] is None
    assert np.all(w["out"] == cm.FILL) and np.all(w["carry_dst"] == cm.FILL)
    cin["off"][0] = 8
    assert cm.carry_model(d.frames, d.arena, t, 2, 100, cin, src, jm.JOIN_ALL, 64, 64)["summary"] == inv
    cin["off"][0] = 16
    assert cm.carry_model(d.frames, d.arena, t, 1, 100, cin[:1], src, jm.JOIN_ALL, 64, 64)["summary"] == inv
    # capacity on one side: nothing written on either, the need in the summary concerned
    w = cm.carry_model(d.frames, d.arena, t, 2, 100, cin, src, jm.JOIN_ALL, 0, 16)
    assert summ(w["summary"]) == (1, 16, 9, 0, jm.ERR_CAPACITY) and summ(w["carry_summary"]) == (1, 16, 4, 0, 0)
    assert w["bodies"] is None and w["carry"] is None and np.all(w["carry_dst"] == cm.FILL)
    w = cm.carry_model(d.frames, d.arena, t, 2, 100, cin, src, jm.JOIN_ALL, 16, 0)
    assert summ(w["summary"]) == (1, 16, 9, 0, 0) and summ(w["carry_summary"]) == (1, 16, 4, 0, jm.ERR_CAPACITY)
    assert w["bodies"] is None and w["carry"] is None and np.all(w["out"] == cm.FILL)
    # gates
    w = cm.carry_model(d.frames, d.arena, t, 2, 100, cin, src, jm.JOIN_ALL, 16, 16, msg_status=jm.ERR_CAPACITY)
    assert summ(w["summary"]) == summ(w["carry_summary"]) == (0, 0, 0, 0, jm.ERR_CAPACITY) and w["carry"] is None
    w = cm.carry_model(d.frames, d.arena, t, 0, 100, None, None, jm.JOIN_ALL, 16, 16)
    assert summ(w["summary"]) == summ(w["carry_summary"]) == (0, 0, 0, 0, 0) and w["carry"] is None


def test_cut_invariance():
    """12 connections, a seeded random stream of frames cut into 1..5 passes at
    frame boundaries: per connection the same (opcode, bytes) sequence as the
    existing join model with JOIN_ALL on the uncut batch."""
    for seed in range(6):
        rng = np.random.default_rng(0xCA7700 + seed)
        conns = cm.random_streams(rng, 12, 60000, text=bool(seed & 1))
        d = mm.Decoded(conns)
        ref = jm.decoded_join_model(d, jm.JOIN_ALL)
        want = cm.sequences(12, [ref])
        assert sum(len(s) for s in want) == sum(1 for frs in conns for f in frs if f[0] and f[2] < 8)
        for npass in range(1, 6):
            passes = cm.split_passes(conns, cm.random_cuts(rng, conns, npass))
            assert len(passes) == npass
            got = cm.sequences(12, [x[2] for x in cm.chain_model(passes, 1 << 20)])
            assert got == want, (seed, npass)
