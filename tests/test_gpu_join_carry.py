"""GPU checks of the join step's carry (gevws_join_carry_async) through the C
ABI, bit-exact against tests/_carry_model.py: d_bodies and d_carry_out field by
field, both summaries, and the WHOLE of d_out and d_carry_dst -- bodies, zeroed
pads, and every other byte still the 0xEE it was prefilled with, 64 guard bytes
behind each capacity included.  cm.chain_device runs a list of passes through
the device message pass and the join, state and carry handed on, every pass
compared with the models; capacities are exactly the needs."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _carry_model as cm
from tests import _inflate_gpu_model as gm
from tests import _join_model as jm
from tests import _messages_model as mm
from tests._helpers import gpu_decode, pack_streams

pytestmark = pytest.mark.gpu

T, B, C, PING, PONG = 1, 2, 0, 9, 10
RSV1 = 4
BIG = 1 << 22


def rnd(rng, n: int) -> bytes:
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def rec(g, c):
    r = g["carry"][c]
    return tuple(int(r[k]) for k in ("off", "length", "opcode", "flags", "status"))


def body(g, m):
    b = g["bodies"][m]
    return int(b["flags"]), int(b["status"]), int(b["off"]), int(b["length"])


# ---------------------------------------------------------------------------- 1. the NULL call
def test_null_call_is_join_async(engine):
    import torch
    rng = np.random.default_rng(0xCA7701)
    conns = []
    for c in range(120):
        conn = []
        for _ in range(int(rng.integers(1, 5))):
            total = int(rng.integers(0, 9001)) if rng.random() < 0.5 else int(rng.integers(0, 200))
            k = int(rng.integers(1, 9))
            cuts = sorted(int(x) for x in rng.integers(0, total + 1, k - 1))
            lens = [b - a for a, b in zip([0, *cuts], [*cuts, total])]
            for i, n in enumerate(lens):
                conn.append((1 if i == k - 1 else 0, 0, B if i == 0 else C, rnd(rng, n)))
                if i < k - 1 and rng.random() < 0.3:
                    conn.append((1, 0, PING if i % 2 else PONG, rnd(rng, i % 126)))
        if c % 37 == 0:
            conn[-1] = (0,) + conn[-1][1:]  # the last message stays open
        conns.append(conn)
    d = mm.Decoded(conns)
    got = cm.run_messages(engine, d)
    t = got["dev"]
    assert t["n_messages"] >= 250
    for flags in (0, jm.JOIN_ALL):
        w = jm.join_model(d.frames, d.arena, got["messages"], got["msg_of"], flags)
        cap = w["out"].size
        a = jm.run_join(engine, t, flags, cap)
        jm.assert_join(a, w, cap, "join_async")
        f = lambda n: torch.full((n,), jm.FILL, dtype=torch.uint8, device=t["frames"].device)  # noqa: E731
        crec, cdst, csum = f(len(conns) * 32), f(4096), f(64)
        # each of the four pointers NULL in turn, the other added arguments set and ignored
        for k in range(4):
            p = [t["conn_msg"], crec, cdst, csum]
            p[k] = None
            bodies, out, summ = f(t["n_messages"] * 32), f(cap + jm.GUARD), f(64)
            engine.join_carry_async(t["frames"], t["n_frames"], t["messages"], t["n_messages"], t["msg_of"],
                                    t["summary"], t["payload"], None, None, flags, bodies, out, cap, summ, p[0],
                                    len(conns), 0, None, None, 0, p[1], p[2], 4096 - 64, p[3])
            torch.cuda.synchronize(engine.device)
            assert np.array_equal(bodies.cpu().numpy(), a["bodies_raw"]), (flags, k)
            assert np.array_equal(out.cpu().numpy(), a["out"]), (flags, k)
            assert summ.cpu().numpy().tobytes() == a["summary"].tobytes(), (flags, k)
        for x in (crec, cdst, csum):
            assert bool((x == jm.FILL).all())


# ---------------------------------------------------------------------------- 2. every shift
CARRIED = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097)
FRAGS = (1, 15, 16, 17, 1040, 5000)


def test_every_shift_at_the_seam(engine):
    """Carried lengths x completing fragment lengths: the prefix / fragment seam
    at every & 15, at a row end and at a tile end -- on the body side (the
    message ends in pass 2) and on the carry side (it stays open in pass 2 and
    ends in pass 3)."""
    rng = np.random.default_rng(0xCA7702)
    pairs = [(a, b) for a in CARRIED for b in FRAGS]
    p1 = [[(0, 0, B, rnd(rng, a))] for a, _ in pairs]
    r = cm.chain_device(engine, [p1, [[(1, 0, C, rnd(rng, b))] for _, b in pairs]], BIG, tag="body side")
    g = r[1][0]
    assert np.all(g["bodies"]["flags"] == jm.WHOLE | jm.JOINED)
    assert [int(x) for x in g["bodies"]["length"]] == [a + b for a, b in pairs]
    assert not g["carry"].view(np.uint8).any()
    r = cm.chain_device(engine, [p1, [[(0, 0, C, rnd(rng, b))] for _, b in pairs],
                                 [[(1, 0, C, rnd(rng, 1))] for _ in pairs]], BIG, flags=0, tag="carry side")
    assert [rec(r[1][0], c)[1:] for c in range(len(pairs))] == [(a + b, B, cm.OPEN, 0) for a, b in pairs]
    assert [int(x) for x in r[2][0]["bodies"]["length"]] == [a + b + 1 for a, b in pairs]


# ---------------------------------------------------------------------------- 3. tiny pieces
def test_tiny_pieces(engine):
    rng = np.random.default_rng(0xCA7703)
    data = rnd(rng, 40)
    frs = [(1 if i == 39 else 0, 0, T if i == 0 else C, bytes([data[i] & 0x7F])) for i in range(40)]

    def part(lo, hi):
        out = []
        for i in range(lo, hi):
            out.append(frs[i])
            if i % 3 == 0:
                out.append((1, 0, PING if i % 2 else PONG, rnd(rng, i)))
        return out
    passes = [[part(0, 1)], [part(1, 7)], [[(1, 0, PING, b"only a ping")]], [part(7, 39)], [part(39, 40)]]
    r = cm.chain_device(engine, passes, BIG)
    assert [rec(g, 0)[1:4] for g, _ in r] == [(1, T, cm.OPEN), (7, T, cm.OPEN), (7, T, cm.OPEN), (39, T, cm.OPEN),
                                              (0, 0, 0)]
    assert cm.delivered(r[4][0]) == [(0, T, bytes(x & 0x7F for x in data))]


# ---------------------------------------------------------------------------- 4. long bodies
def test_long_bodies_on_both_sides_of_the_seam(engine):
    rng = np.random.default_rng(0xCA7704)
    mib = 1 << 20
    a, b = rnd(rng, 3), rnd(rng, mib + 3)
    x, y = rnd(rng, mib), rnd(rng, 5)
    r = cm.chain_device(engine, [[[(0, 0, B, a)], [(0, 0, B, b)]], [[(1, 0, C, x)], [(1, 0, C, y)]]], BIG)
    assert rec(r[0][0], 1) == (16, mib + 3, B, cm.OPEN, 0)  # many workgroups on the carry side too
    assert cm.delivered(r[1][0]) == [(0, B, a + x), (1, B, b + y)]


# ---------------------------------------------------------------------------- 5. cut invariance
def test_cut_invariance_on_the_device(engine):
    """40 connections of text messages, multi-byte characters cut across frames
    and passes, d_state carried through the device message pass: however the
    stream is cut into passes, the delivered (opcode, bytes) per connection are
    those of gevws_join_async with JOIN_ALL on the uncut batch."""
    rng = np.random.default_rng(0xCA7705)
    conns = cm.random_streams(rng, 40, 160 * 1024, text=True)
    d = mm.Decoded(conns)
    got = cm.run_messages(engine, d)
    assert not got["conn_msg"]["error"].any()
    ref = jm.run_join(engine, got["dev"], jm.JOIN_ALL, int(d.arena.size))
    assert int(ref["summary"]["status"]) == 0
    want = cm.sequences(40, [ref])
    assert sum(len(s) for s in want) == int(ref["summary"]["frames"]) > 60
    for npass in (1, 3, 5):
        passes = cm.split_passes(conns, cm.random_cuts(rng, conns, npass))
        r = cm.chain_device(engine, passes, BIG, tag=f"{npass} passes")
        assert cm.sequences(40, [g for g, _ in r]) == want, npass


# ---------------------------------------------------------------------------- 6. idle forward, the scans
def test_idle_forward_and_scans_across_workgroups(engine):
    rng = np.random.default_rng(0xCA7706)
    n = 700
    lens = [int(rng.integers(1, 34)) if c % 3 == 0 else 0 for c in range(n)]
    p1 = [[(0, 0, B, rnd(rng, L))] if L else [] for L in lens]
    idle = [[] for _ in range(n)]
    # pass 3: every carried message ends, every other connection sends one whole message: > 256 bodies
    p3 = [[(1, 0, C, rnd(rng, 1 + c % 40))] if L else [(0, 0, B, rnd(rng, 3)), (1, 0, C, rnd(rng, c % 7))]
          for c, L in enumerate(lens)]
    r = cm.chain_device(engine, [p1, idle, idle, p3], BIG, flags=0)
    for k in (1, 2):  # no frames at all: records and bytes move forward unchanged
        assert r[k][0]["carry"].tobytes() == r[0][0]["carry"].tobytes()
        assert np.array_equal(r[k][0]["carry_dst"], r[0][0]["carry_dst"])
        assert jm.summary_tuple(r[k][0]["summary"]) == (0, 0, 0, 0, 0)
    assert int(r[0][0]["carry_summary"]["frames"]) == len([x for x in lens if x]) == 234
    g = r[3][0]
    assert g["bodies"].shape[0] == n and np.all(g["bodies"]["flags"] == jm.WHOLE | jm.JOINED)
    assert not g["carry"].view(np.uint8).any()


# ---------------------------------------------------------------------------- 7. the limit
def test_limit(engine):
    lim = 100
    passes = [[[(0, 0, B, b"a" * 60)], [(0, 0, B, b"b" * 60)], [(0, 0, B, b"c" * 60)]],
              [[(1, 0, C, b"A" * 40)], [(1, 0, C, b"B" * 41)], [(0, 0, C, b"C" * 41)]],
              [[], [], [(1, 0, PING, b"")]],
              [[], [], [(1, 0, C, b"end"), (1, 0, B, b"next"), (0, 0, B, b"open")]]]
    r = cm.chain_device(engine, passes, lim)
    g = r[1][0]
    assert body(g, 0) == (jm.WHOLE | jm.JOINED, 0, 0, 100)            # exactly the limit
    assert body(g, 1) == (0, cm.ERR_TOO_BIG, 0, 0)                    # one byte more, ends in that pass
    assert rec(g, 2) == (0, 0, B, cm.LOST, cm.ERR_TOO_BIG)            # one byte more, still open
    assert jm.summary_tuple(g["carry_summary"]) == (0, 0, 0, 2, 0) and int(g["summary"]["errors"]) == 0
    assert rec(r[2][0], 2) == (0, 0, B, cm.LOST, cm.ERR_TOO_BIG) and int(r[2][0]["carry_summary"]["errors"]) == 0
    g = r[3][0]
    assert body(g, 0) == (0, cm.ERR_TOO_BIG, 0, 0) and body(g, 1) == (jm.WHOLE | jm.JOINED, 0, 0, 4)
    assert rec(g, 2) == (0, 4, B, cm.OPEN, 0) and int(g["carry_summary"]["errors"]) == 0
    # a message that begins in the batch and is still open over the limit
    r = cm.chain_device(engine, [[[(0, 0, B, b"x" * 101)], [(0, 0, B, b"y" * 100)]]], lim)
    assert rec(r[0][0], 0) == (0, 0, B, cm.LOST, cm.ERR_TOO_BIG) and rec(r[0][0], 1) == (0, 100, B, cm.OPEN, 0)


# ---------------------------------------------------------------------------- 8. a failure drops the carry
def test_failure_drops_the_carry(engine):
    passes = [[[(0, 0, B, b"abc")], [(0, 0, T, b"abc")], [(0, 0, B, b"kept")]],
              [[(1, 0, B, b"interleaved")], [(0, 0, C, b"\xff")], [(0, 0, C, b"!")]],
              [[(1, 0, C, b"x")], [(1, 0, C, b"x")], [(1, 0, C, b"?")]]]
    r = cm.chain_device(engine, passes, BIG)
    assert [rec(r[0][0], c)[1:4] for c in range(3)] == [(3, B, cm.OPEN), (3, T, cm.OPEN), (4, B, cm.OPEN)]
    assert rec(r[1][0], 0) == rec(r[1][0], 1) == (0, 0, 0, 0, 0) and rec(r[1][0], 2) == (0, 5, B, cm.OPEN, 0)
    assert rec(r[2][0], 0) == rec(r[2][0], 1) == (0, 0, 0, 0, 0)
    assert cm.delivered(r[2][0]) == [(2, B, b"kept!?")]


# ---------------------------------------------------------------------------- 9. compressed messages
def test_compressed_messages_are_lost_not_carried(engine):
    import torch
    rng = np.random.default_rng(0xCA7709)

    def z(data):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]
    hello, again = b"Hello, a whole compressed message", b"another whole one " * 9
    openz = z(b"a compressed message that spans two passes")
    ext = np.array([gev_amd.EXT_DEFLATE, 0], np.uint8)
    passes = [
        [[(1, RSV1, T, z(hello)), (0, 0, B, rnd(rng, 33)), (1, 0, C, rnd(rng, 2)), (0, RSV1, T, openz[:7])],
         [(0, 0, B, b"plain, open")]],
        [[(1, 0, C, openz[7:]), (0, RSV1, B, z(again)[:4]), (1, 0, C, z(again)[4:]), (1, 0, B, rnd(rng, 20))],
         [(1, 0, C, b" and closed")]]]
    state, cin, csrc = None, None, None
    for p, conns in enumerate(passes):
        d = mm.Decoded(conns, pad=0xFF)
        got = cm.run_messages(engine, d, state, ext)
        t = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, state, ext)
        mm.assert_tables_equal(got, t, f"pass {p}")
        inf_cap = 1024
        inf = gm.run_inflate(engine, got, 1 << 20, inf_cap)
        isum, irec = inf["summary"], inf["inflated"]
        assert int(isum["status"]) == 0 and int(isum["frames"]) == 1 and int(isum["errors"]) == 0
        base = jm.round16(int(isum["payload_bytes"]))
        dev = got["dev"]["frames"].device
        w = cm.carry_model(d.frames, d.arena, t, 2, BIG, cin, csrc, jm.JOIN_ALL, None, None, irec,
                           dict(payload_bytes=int(isum["payload_bytes"]), status=0))
        oc, cc = int(w["summary"]["payload_bytes"]), w["carry_dst"].size
        before = np.concatenate([inf["out"][:base], np.full(oc - base + jm.GUARD, jm.FILL, np.uint8)])
        w = cm.carry_model(d.frames, d.arena, t, 2, BIG, cin, csrc, jm.JOIN_ALL, oc, cc, irec,
                           dict(payload_bytes=int(isum["payload_bytes"]), status=0), out_image=before)
        g = cm.run_join_carry(engine, got["dev"], 2, BIG, jm.JOIN_ALL, oc, cc, cin, csrc, None,
                              mm._dev(irec, dev, 32), mm._dev(np.array([isum]), dev, 64),
                              out=torch.from_numpy(before.copy()).to(dev))
        cm.assert_join_carry(g, w, oc, cc, f"pass {p}")
        assert np.array_equal(g["out"][:base], inf["out"][:base])  # the inflate's bytes, untouched below base
        fl = [int(x) for x in g["bodies"]["flags"]]
        if p == 0:
            assert fl == [jm.WHOLE | jm.INFLATED, jm.WHOLE | jm.JOINED, 0, 0]
            assert rec(g, 0) == (0, 0, T, cm.LOST, 0) and rec(g, 1) == (0, 11, B, cm.OPEN, 0)
        else:
            assert fl == [0, jm.WHOLE | jm.INFLATED, jm.WHOLE | jm.JOINED, jm.WHOLE | jm.JOINED]
            assert int(g["bodies"]["off"][1]) == 0 and np.all(g["bodies"]["off"][2:] >= base)
            assert not g["carry"].view(np.uint8).any()
            assert cm.delivered(g)[-1] == (1, B, b"plain, open and closed")
        state, cin, csrc = got["state"], w["carry"], w["carry_dst"]


# ---------------------------------------------------------------------------- 10. capacity
def test_capacity_on_either_side_writes_nothing(engine):
    rng = np.random.default_rng(0xCA770A)
    passes = [[[(0, 0, B, rnd(rng, 100))], [(0, 0, B, rnd(rng, 50))], []],
              [[(1, 0, C, rnd(rng, 5000))], [(0, 0, C, rnd(rng, 70))], [(0, 0, T, b"new"), (0, 0, C, b"")]]]
    (d, t, w, cin, csrc) = cm.chain_model(passes, BIG)[1]
    state = cm.chain_model(passes, BIG)[0][1]["state"]
    got = cm.run_messages(engine, d, state)
    mm.assert_tables_equal(got, t)
    oc, cc = w["out"].size, w["carry_dst"].size
    assert (oc, cc) == (5104, 128 + 16)
    for so, sc in ((16, 0), (0, 16), (16, 16)):
        ws = cm.carry_model(d.frames, d.arena, t, 3, BIG, cin, csrc, jm.JOIN_ALL, oc - so, cc - sc)
        assert ws["bodies"] is None and ws["carry"] is None
        assert (ws["summary"]["status"], ws["carry_summary"]["status"]) == \
            (jm.ERR_CAPACITY if so else 0, jm.ERR_CAPACITY if sc else 0)
        assert (ws["summary"]["payload_bytes"], ws["carry_summary"]["payload_bytes"]) == (oc, cc)  # the need
        g = cm.run_join_carry(engine, got["dev"], 3, BIG, jm.JOIN_ALL, oc - so, cc - sc, cin, csrc)
        cm.assert_join_carry(g, ws, oc - so, cc - sc, f"short by {so} / {sc}")
        assert np.all(g["out"] == jm.FILL) and np.all(g["carry_dst"] == jm.FILL)
        assert np.all(g["bodies_raw"] == jm.FILL) and np.all(g["carry_raw"] == jm.FILL)
    g = cm.run_join_carry(engine, got["dev"], 3, BIG, jm.JOIN_ALL, oc, cc, cin, csrc)  # the retry, same inputs
    cm.assert_join_carry(g, w, oc, cc, "the retry")


# ---------------------------------------------------------------------------- 11. gates, malformed input
def poke(summary_dev, **fields):
    """A copy of a device summary with some fields replaced."""
    s = summary_dev.cpu().numpy().copy().view(mm.SUMMARY_DTYPE)
    for k, v in fields.items():
        s[k] = v
    return mm._dev(s, summary_dev.device, 64)


def test_gates_and_malformed_input(engine):
    rng = np.random.default_rng(0xCA770B)
    passes = [[[(0, 0, B, rnd(rng, 21))], [(0, 0, B, rnd(rng, 5))]],
              [[(1, 0, C, rnd(rng, 9))], [(0, 0, C, rnd(rng, 70))]]]
    ch = cm.chain_model(passes, BIG)
    (d, t, w, cin, csrc) = ch[1]
    got = cm.run_messages(engine, d, ch[0][1]["state"])
    oc, cc = w["out"].size, w["carry_dst"].size

    def run(tables=None, n_conns=2, carry_in=cin, src_bytes=None, **model_kw):
        tb = got["dev"] if tables is None else tables
        ws = cm.carry_model(d.frames, d.arena, t, n_conns, BIG, carry_in, csrc, jm.JOIN_ALL, oc, cc,
                            carry_src_bytes=src_bytes, **model_kw)
        g = cm.run_join_carry(engine, tb, n_conns, BIG, jm.JOIN_ALL, oc, cc, carry_in, csrc, src_bytes)
        cm.assert_join_carry(g, ws, oc, cc, str((n_conns, src_bytes, model_kw)))
        return g
    assert csrc.size == 48 and [int(x) for x in cin["off"]] == [0, 32]
    assert jm.summary_tuple(run()["summary"]) == (1, 32, 30, 0, 0)   # the inputs are fine as they are
    run(src_bytes=37)                                                   # ... up to the last carried byte
    # a failed message summary: its status in both summaries, nothing written
    tb = dict(got["dev"], summary=poke(got["dev"]["summary"], status=gev_amd.ERR_CAPACITY))
    g = run(tb, msg_status=gev_amd.ERR_CAPACITY)
    assert jm.summary_tuple(g["summary"]) == jm.summary_tuple(g["carry_summary"]) == (0, 0, 0, 0, gev_amd.ERR_CAPACITY)
    inv = (0, 0, 0, 1, gev_amd.ERR_INVALID)
    bad = cin.copy()
    bad["off"][1] = 8
    g = run(carry_in=bad)                                               # an OPEN record off its boundary
    assert jm.summary_tuple(g["summary"]) == jm.summary_tuple(g["carry_summary"]) == inv
    g = run(src_bytes=36)                                               # off + length = carry_src_bytes + 1
    assert jm.summary_tuple(g["summary"]) == jm.summary_tuple(g["carry_summary"]) == inv
    g = run(n_conns=1, carry_in=cin[:1])                                # a message with conn == n_conns
    assert jm.summary_tuple(g["summary"]) == jm.summary_tuple(g["carry_summary"]) == inv
    for x in ("bodies_raw", "out", "carry_raw", "carry_dst"):
        assert np.all(g[x] == jm.FILL), x
    # n_conns == 0: two zero summaries; max_message_bytes out of range, an unknown flag: the call fails
    g = cm.run_join_carry(engine, got["dev"], 0, BIG, jm.JOIN_ALL, oc, cc)
    assert jm.summary_tuple(g["summary"]) == jm.summary_tuple(g["carry_summary"]) == (0, 0, 0, 0, 0)
    assert np.all(g["carry_raw"] == jm.FILL) and np.all(g["out"] == jm.FILL)
    for lim, flags in ((0, jm.JOIN_ALL), (1 << 32, jm.JOIN_ALL), (BIG, 2)):
        with pytest.raises(RuntimeError):
            cm.run_join_carry(engine, got["dev"], 2, lim, flags, oc, cc, cin, csrc)


# ---------------------------------------------------------------------------- 12. end to end
def test_end_to_end_a_message_over_three_passes(engine):
    import torch
    rng = np.random.default_rng(0xCA770C)
    dev = torch.device("cuda", engine.device)
    text = ("é€" * 20000).encode()
    assert len(text) == 100000
    cuts = (33333, 66666)  # inside a three-byte and inside a two-byte character
    assert (text[cuts[0]] & 0xC0) == 0x80 and (text[cuts[1]] & 0xC0) == 0x80
    parts = [text[:cuts[0]], text[cuts[0]:cuts[1]], text[cuts[1]:]]

    def wire(data, op, fin):
        return wo.encode_frame(data, op, fin, 0, True, rnd(rng, 4))
    streams = [[wire(parts[0][:20000], T, False) + wire(parts[0][20000:], C, False), wire(b"one", T, True)],
               [wire(parts[1], C, False), wire(b"two", T, True)],
               [wire(parts[2][:7], C, False) + wire(b"", PING, True) + wire(parts[2][7:], C, True), b""]]
    state = torch.zeros((2, 8), dtype=torch.uint8, device=dev)
    carry = gev_amd.Carry(engine, 2, 1 << 20)
    kept = 0
    for p, ss in enumerate(streams):
        batch = gpu_decode(engine, *pack_streams(ss))
        msgs = engine.messages(batch, state)
        assert not msgs.conn_msg_host()["error"].any()
        bodies = engine.join(batch, msgs, flags=gev_amd.JOIN_ALL, carry=carry)
        echo = engine.echo_messages(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, None)
        got = echo.plain_wire.cpu().numpy().tobytes()
        if p < 2:  # no reply for the connection whose message is still open
            kept += len(parts[p])
            assert list(echo.plain_conn) == [1] and got == wo.encode_frame((b"one", b"two")[p], 1, True, 0, False)
            r = carry.records_host()
            assert (int(r["flags"][0]), int(r["length"][0]), int(r["opcode"][0])) == (gev_amd.CARRY_OPEN, kept, T)
            assert carry.carried_bytes(0) == text[:kept] and carry.carried_bytes(1) == b""
        else:
            assert list(echo.plain_conn) == [0] and got == wo.encode_frame(text, 1, True, 0, False)
            assert bodies.body_bytes(0) == text
            assert not carry.records_host().view(np.uint8).any() and carry.used == 0
    # the limit through the holder: the body's status, the count, and an empty carry behind it
    state.zero_()
    carry = gev_amd.Carry(engine, 1, 8)
    batch = gpu_decode(engine, *pack_streams([wire(b"12345", B, False)]))
    engine.join(batch, engine.messages(batch, state), flags=gev_amd.JOIN_ALL, carry=carry)
    assert carry.carried_bytes(0) == b"12345" and carry.side == 1
    batch = gpu_decode(engine, *pack_streams([wire(b"6789", C, True)]))
    b2 = engine.join(batch, engine.messages(batch, state), flags=gev_amd.JOIN_ALL, carry=carry)
    assert int(b2.bodies_host()["status"][0]) == gev_amd.MSG_ERR_TOO_BIG and int(b2.carry_summary_host()["errors"]) == 1
    assert carry.side == 0 and carry.used == 0
