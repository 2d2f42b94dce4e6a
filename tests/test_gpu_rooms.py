"""GPU checks of the room broadcast (gevws_reply_rooms_async,
gevws_room_plan_async) through the C ABI, bit-exact against
tests/_rooms_model.py -- both lists, d_plain_of / d_def_of, d_send, d_conn_send,
the summaries, everything else still the 0xEE it was prefilled with -- and of
the whole chain behind a real wire batch (Engine.broadcast)."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm
from tests import _rooms_model as ro
from tests._helpers import gpu_decode

pytestmark = pytest.mark.gpu

T, B, C, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
NONE = ro.ROOM_NONE
SKIP = ro.SKIP_SENDER
D, TK = ro.EXT_DEFLATE, ro.EXT_DEFLATE | ro.EXT_SERVER_TAKEOVER
BLOCK = 256  # kWalkBlock


def both(engine, d, t, ext, wb, rooms, flags=0, max_sends=None, statuses=None, list_rooms=None, plan_conn_out=None,
         tag=""):
    """The room reply step on the control model's bodies and the room plan on
    its tables and synthetic wires: device == model for both calls.  list_rooms:
    the (well formed) tables the plan's d_plain_of / d_def_of come from when
    `rooms` itself is malformed; plan_conn_out: another connection table for the
    plan alone."""
    nc, nm, n = d.conn_out.shape[0], t["messages"].shape[0], d.n_decoded
    st = dict(decoded=0, msg=0, join=0, ctl=0, enc=(0, 0, 0))
    st.update(statuses or {})
    ctl = rm.control_model(d.frames, d.conn_out, n, d.arena, t["msg_of"], t["messages"], t["conn_msg"], t["bodies"])
    want_r = ro.reply_rooms_model(ctl["bodies"], jm.HANDLER_ECHO_BINARY, ext, wb, nc, rooms, flags, st["msg"],
                                  st["join"])
    got_r = ro.run_reply_rooms(engine, ctl["bodies"], st["msg"], st["join"], jm.HANDLER_ECHO_BINARY, ext, wb, nc,
                               rooms, flags)
    ro.assert_reply_rooms(got_r, want_r, (tag, "reply"))
    rep = want_r if list_rooms is None and want_r["plain"] is not None else ro.reply_rooms_model(
        ctl["bodies"], jm.HANDLER_ECHO_BINARY, ext, None, nc, list_rooms or rooms, flags)
    model_w, dev_w = ro.synthetic_wires(rep, ctl)
    for (tab, s), e in zip(dev_w, st["enc"]):
        s["status"] = e
    gate_ok = not (st["decoded"] or st["msg"] or st["join"] or st["ctl"] or any(st["enc"]))
    pco = d.conn_out if plan_conn_out is None else plan_conn_out
    want_p = ro.room_plan_model(n, pco, t["msg_of"], ctl["msg_end"], rep["plain_of"], rep["def_of"], nm, ext,
                                ctl["ctl_of"], ctl["conn_ctl"], model_w, rooms, flags, max_sends, gate_ok)
    cap = max_sends if max_sends is not None else max(int(want_p["summary"]["frames"]), n)
    dsum = d.summary.copy()
    dsum["status"] = st["decoded"]
    got_p = ro.run_room_plan(engine, n, dsum, pco, t["msg_of"], ctl["msg_end"], rep["plain_of"], rep["def_of"],
                             nm, rm.summary_np(frames=nm, status=st["msg"]),
                             rm.summary_np(frames=nm, status=st["join"]), ext, ctl["ctl_of"], ctl["conn_ctl"],
                             rm.summary_np(frames=ctl["ctl"].shape[0], status=st["ctl"]), dev_w, rooms, flags, cap)
    ro.assert_plan(got_p, want_p, (tag, "plan"))
    return dict(reply=got_r, reply_model=want_r, plan=got_p, plan_model=want_p, ctl=ctl, wires=(model_w, dev_w))


def data_batch(rng, n_conns, frag=True):
    """Connections that send one or two data messages, some fragmented, no control frames."""
    conns = []
    for c in range(n_conns):
        frs = []
        for _ in range(int(rng.integers(0, 3))):
            data = bytes(rng.integers(0x20, 0x7F, int(rng.integers(0, 40)), dtype=np.uint8))
            if frag and rng.random() < 0.4 and len(data) > 1:
                cut = int(rng.integers(1, len(data)))
                frs += [(0, 0, B, data[:cut]), (1, 0, C, data[cut:])]
            else:
                frs.append((1, 0, B, data))
        conns.append(frs)
    return conns


# ---------------------------------------------------------------------------- 1. singletons are the echo plan
def test_singletons_are_the_echo_plan(engine):
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x726F6F31)
    d = mm.Decoded(data_batch(rng, BLOCK + 37))
    t = rm.tables_of(d)
    nc, nm, n = d.conn_out.shape[0], t["messages"].shape[0], d.n_decoded
    assert n > BLOCK and nm > 100
    ext = (np.arange(nc) % 3 == 0).astype(np.uint8) * D
    rooms = ro.csr_of(np.arange(nc))
    r = both(engine, d, t, ext, None, rooms, tag="singletons")
    # the echo: gevws_reply_bodies_async's lists, gevws_send_plan_async over them
    ctl = r["ctl"]
    msum, jsum = mm._dev(rm.summary_np(frames=nm), dev, 64), mm._dev(rm.summary_np(frames=nm), dev, 64)
    echo = jm.run_reply(engine, ctl["bodies"], nm, msum, jsum, jm.HANDLER_ECHO_BINARY, ext, None, nc)
    npl, nd = int(echo["plain_summary"]["frames"]), int(echo["def_summary"]["frames"])
    assert npl > 50 and nd > 30
    assert echo["plain"].tobytes() == r["reply"]["plain"].tobytes()
    assert echo["plain_conn"].tobytes() == r["reply"]["plain_conn"].tobytes()
    assert echo["def_conn"].tobytes() == r["reply"]["def_conn"].tobytes()
    reply_of = echo["reply_of"].view(np.int64)[:nm]
    assert np.array_equal(reply_of, np.maximum(r["reply_model"]["plain_of"], r["reply_model"]["def_of"]))
    plan = rm.run_plan(engine, n, d.summary, d.conn_out, t["msg_of"], ctl["msg_end"], reply_of, nm,
                       rm.summary_np(frames=nm), rm.summary_np(frames=nm), ext, ctl["ctl_of"], ctl["conn_ctl"],
                       rm.summary_np(frames=0), r["wires"][1], n)
    assert plan["send"].tobytes() == r["plan"]["send"].tobytes()
    assert plan["conn_send"].tobytes() == r["plan"]["conn_send"].tobytes()
    assert plan["summary"].tobytes() == r["plan"]["summary"].tobytes()
    assert int(plan["summary"]["frames"]) == npl + nd
    # without the sender nobody is left: zero entries, both lists empty
    s = both(engine, d, t, ext, None, rooms, SKIP, tag="singletons, no sender")
    assert jm.summary_tuple(s["plan"]["summary"]) == (0, 0, 0, 0, 0)
    assert int(s["reply"]["plain_summary"]["frames"]) == 0 and int(s["reply"]["def_summary"]["frames"]) == 0
    assert np.all(s["reply_model"]["plain_of"] == -1) and np.all(s["reply_model"]["def_of"] == -1)


# ---------------------------------------------------------------------------- 2. every path once, behind the real chain
def parse(wire: bytes):
    # (the reference reads no header from fewer than 6 buffered bytes: three bare close frames behind the wire
    # let it read a short last frame, and are dropped again)
    got = wo.decode_stream(wire + b"\x88\x00" * 3)
    assert got.status == wo.OK
    frames = [f for f in got.frames if f.stream_pos < len(wire)]
    assert sum(f.header_len + f.header.length for f in frames) == len(wire)
    return frames


def test_every_path_once(engine):
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x726F6F32)

    def fr(payload, op, fin=True):
        return wo.encode_frame(payload, op, fin, 0, True, bytes(rng.integers(0, 256, 4, dtype=np.uint8)))

    words = b"the quick brown fox jumps over the lazy dog; " * 6
    streams = [
        fr(b"hello ", T, False) + fr(b"between", PING) + fr(b"world", C),       # 0 room 0, plain
        fr(b"", T),                                                             # 1 room 0, deflate: an empty message
        fr(words, T),                                                           # 2 room 0, deflate + server takeover
        fr((1000).to_bytes(2, "big") + b"bye", CLOSE) + fr(b"too late", T),     # 3 room 1: a close, a message behind it
        fr(b"ok", T, False) + fr(b"\xff", C),                                   # 4 room 1: fails UTF-8
        fr(b"room one", T),                                                     # 5 room 1
        fr(b"nobody hears this", T) + fr(b"pi", PING),                          # 6 no room
    ]
    nc = len(streams)
    ext_h = np.array([0, D, TK, 0, 0, D, D], np.uint8)
    room_h = np.array([0, 0, 0, 1, 1, 1, NONE], np.uint32)
    published = {0: [(0, b"hello world"), (1, b""), (2, words)], 1: [(5, b"room one")]}   # room -> (sender, bytes)
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ext = mm._dev(ext_h, dev, 1)
    rooms = gev_amd.Rooms.from_conn_room(room_h, dev)
    assert rooms.n_rooms == 2 and rooms.n_members == 6
    for flags in (0, SKIP):
        batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1), aux_slots=nc)
        msgs = engine.messages(batch, conn_ext=ext)
        inf = engine.inflate(batch, msgs, 1 << 16)
        bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)
        res = engine.broadcast(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, rooms, rooms_flags=flags,
                               gather=True)
        cs = res.conn_send_host()
        S, F = gev_amd.CTL_SHUTDOWN, gev_amd.CTL_SHUTDOWN | gev_amd.CTL_FAILED
        assert [int(x) for x in cs["flags"]] == [0, 0, 0, S, F, 0, 0]
        assert [int(x) for x in res.conn_ctl["close_code"]] == [0, 0, 0, 0, 1007, 0, 0]
        assert int(res.summary_host()["errors"]) == 2 and int(cs["count"].sum()) == int(res.summary_host()["frames"])
        # every message is in each list once, whatever the room's size
        assert res.echo.plain_conn.tolist() == [0, 1, 2, 5]
        assert res.echo.def_conn.tolist() == ([0, 2] if flags else [0, 1, 2, 5])
        sends = res.host_sends()
        tails = {0: [(PONG, b"between")], 3: [(CLOSE, (1000).to_bytes(2, "big") + b"bye")],
                 4: [(CLOSE, (1007).to_bytes(2, "big"))], 6: [(PONG, b"pi")]}
        for c in range(nc):
            wire = res.conn_bytes(c)
            assert bytes(sends[c]) == wire and len(wire) == int(cs["bytes"][c]), c
            frames = parse(wire)
            want = [x for s, x in published.get(int(room_h[c]), []) if not (flags and s == c)]
            tail = tails.get(c, [])
            assert len(frames) == len(want) + len(tail) == int(cs["count"][c]), (flags, c, len(frames))
            deflate = ro.takes_deflate(ext_h, c)
            for f, x in zip(frames, want):
                h = f.header
                assert h.fin and not h.masked and h.opcode == T, c
                if deflate:
                    assert h.rsv == 4, c
                    assert zlib.decompressobj(-15).decompress(f.payload + b"\x00\x00\xff\xff") == x, (c, x)
                else:
                    assert h.rsv == 0 and f.payload == x, (c, x)   # the takeover member too: RSV1 clear
            for f, (op, x) in zip(frames[len(want):], tail):       # its own control replies come last
                assert (f.header.opcode, f.header.rsv, f.payload) == (op, 0, x), c
        assert ext_h[2] == TK and not ro.takes_deflate(ext_h, 2) and ro.takes_deflate(ext_h, 1)
        assert int(cs["count"][6]) == 1 and int(cs["count"][5]) == (0 if flags else 1)


# ---------------------------------------------------------------------------- 3. window bits
def test_the_smallest_window_of_the_room(engine):
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x726F6F33)
    # a repeat 1500 bytes back: inside a window of 12 bits, outside one of 10
    blk = bytes(rng.integers(0x20, 0x7F, 1500, dtype=np.uint8))
    texts = [blk + blk[: 1000 + 7 * i] for i in range(4)]
    streams = [wo.encode_frame(x, T, True, 0, True, bytes(rng.integers(0, 256, 4, dtype=np.uint8))) for x in texts]
    ext_h = np.array([D, D, D, 0], np.uint8)
    wb_h = np.array([12, 0, 10, 8], np.uint8)   # the plain member's byte does not count
    room_h = np.zeros(4, np.uint32)
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1), aux_slots=4)
    ext, wb = mm._dev(ext_h, dev, 1), mm._dev(wb_h, dev, 1)
    msgs = engine.messages(batch, conn_ext=ext)
    bodies = engine.join(batch, msgs, engine.inflate(batch, msgs, 1 << 16), flags=gev_amd.JOIN_ALL)
    rooms = gev_amd.Rooms.from_conn_room(room_h, dev)
    got = ro.run_reply_rooms(engine, bodies.bodies_host(), 0, 0, jm.HANDLER_ECHO_TEXT, ext_h, wb_h, 4,
                             ro.csr_of(room_h), 0)
    want = ro.reply_rooms_model(bodies.bodies_host(), jm.HANDLER_ECHO_TEXT, ext_h, wb_h, 4, ro.csr_of(room_h))
    ro.assert_reply_rooms(got, want, "windows")
    assert want["def_msgs"]["window_bits"].tolist() == [10, 10, 10, 10]
    res = engine.broadcast(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, rooms, window_bits=wb)
    assert res.echo.def_conn.tolist() == [0, 1, 2, 3]
    for i, x in enumerate(texts):
        assert res.echo.deflated.payload(i) == gev_amd.deflate_raw(x, 10), i
        assert res.echo.deflated.payload(i) != gev_amd.deflate_raw(x, 12), i
    frames = parse(res.conn_bytes(2))
    assert [zlib.decompressobj(-10).decompress(f.payload + b"\x00\x00\xff\xff") for f in frames] == texts


# ---------------------------------------------------------------------------- 4. block edges
@pytest.mark.parametrize("sizes", [(257,), (1, 255, 1)])
def test_block_edges(engine, sizes):
    nc = BLOCK + 1
    assert sum(sizes) == nc
    d = mm.Decoded([[(1, 0, B, bytes([0x30 + c % 64]))] for c in range(nc)])
    t = rm.tables_of(d)
    room_h = np.repeat(np.arange(len(sizes)), sizes).astype(np.uint32)
    ext = (np.arange(nc) % 2).astype(np.uint8) * D
    rooms = ro.csr_of(room_h)
    r = both(engine, d, t, ext, None, rooms, tag=str(sizes))
    assert int(r["plan"]["summary"]["frames"]) == sum(s * s for s in sizes)
    s = both(engine, d, t, ext, None, rooms, SKIP, tag=f"{sizes}, no sender")
    assert int(s["plan"]["summary"]["frames"]) == sum(s * (s - 1) for s in sizes)
    if sizes == (257,):
        assert int(r["plan"]["summary"]["frames"]) == 66049 and int(s["plan"]["summary"]["frames"]) == 65792


def test_uneven_rooms_with_control_frames(engine):
    """Rooms of random sizes over more than one block of connections, every
    recipient kind, connections that publish twice (their own sub-slice is
    skipped in the middle of the room's), pings and closes between the data."""
    rng = np.random.default_rng(0x726F6F34)
    nc = BLOCK + 61
    conns = data_batch(rng, nc)
    for c in range(nc):
        k = rng.random()
        if k < 0.25:
            conns[c].insert(int(rng.integers(0, len(conns[c]) + 1)), (1, 0, PING, b"pi%d" % c))
        elif k < 0.32:
            conns[c].insert(int(rng.integers(0, len(conns[c]) + 1)), (1, 0, CLOSE, b""))
    d = mm.Decoded(conns)
    t = rm.tables_of(d)
    room_h = rng.integers(0, 9, nc).astype(np.uint32)
    room_h[room_h == 8] = NONE          # one in nine is in no room; room 7 stays empty below
    room_h[room_h == 7] = 3
    ext = rng.choice(np.array([0, D, TK], np.uint8), nc)
    wb = rng.choice(np.array([0, 9, 11, 15], np.uint8), nc)
    rooms = ro.csr_of(room_h, n_rooms=8)
    assert int(rooms[1][8]) - int(rooms[1][7]) == 0 and ro.check_tables(rooms, nc) == 0
    for flags in (0, SKIP):
        r = both(engine, d, t, ext, wb, rooms, flags, tag=f"flags {flags}")
        send = r["plan_model"]["send"]
        assert int(r["plan"]["summary"]["frames"]) > 10 * BLOCK and set(send["wire"].tolist()) == {0, 1, 2}
        assert int(r["plan"]["summary"]["errors"]) > 5
        assert set(r["reply_model"]["def_msgs"]["window_bits"].tolist()) <= {9, 11, 15}
    # a sender with two publications and members on both sides of it
    twice = [c for c in range(nc) if sum(1 for f in conns[c] if f[2] == B) == 2 and room_h[c] != NONE
             and not any(f[2] == CLOSE for f in conns[c])]
    assert any(np.any(room_h[:c] == room_h[c]) and np.any(room_h[c + 1:] == room_h[c]) for c in twice)


# ---------------------------------------------------------------------------- 5. capacity, 6. malformed tables, 7. gates
def small_case():
    good = (1, 0, B, b"good")
    conns = [
        [good, (1, 0, PING, b"pi"), (1, 0, CLOSE, (1000).to_bytes(2, "big")), good],
        [good, (1, 2, B, b"rsv")],
        [(0, 0, T, b"op"), (1, 0, PONG, b""), (1, 0, C, b"en")],
        [good, (1, 0, CLOSE, b"")],
        [good],
    ]
    d = mm.Decoded(conns)
    return d, rm.tables_of(d), np.array([0, D, D, TK, 0], np.uint8), ro.csr_of([0, 0, 1, 1, NONE])


def test_capacity(engine):
    d, t, ext, rooms = small_case()
    r = both(engine, d, t, ext, None, rooms, tag="enough")
    need = int(r["plan"]["summary"]["frames"])
    # room 0: two messages to two members; room 1: two messages to two members; five control replies
    assert need == 4 + 4 + 5
    both(engine, d, t, ext, None, rooms, max_sends=need, tag="exactly the need")
    g = both(engine, d, t, ext, None, rooms, max_sends=need - 1, tag="one entry short")
    assert jm.summary_tuple(g["plan"]["summary"])[::4] == (need, gev_amd.ERR_CAPACITY)
    assert np.all(g["plan"]["send"] == ro.FILL) and np.all(g["plan"]["conn_send"] == ro.FILL)


def test_malformed_tables(engine):
    d, t, ext, rooms = small_case()
    cr, first, members = rooms
    assert (first.tolist(), members.tolist()) == ([0, 2, 4], [0, 1, 2, 3])

    def edit(which, idx, val):
        tabs = [cr.copy(), first.copy(), members.copy()]
        tabs[which][idx] = val
        return tuple(tabs)

    cases = {
        "a member >= n_conns": (edit(2, 1, 5), 1),
        "an out-of-order pair": ((cr, first, np.array([1, 0, 2, 3], np.uint32)), 1),
        "conn_room disagrees with the CSR": (edit(0, 1, 1), 1),
        "a roomed connection missing from the CSR": (edit(0, 4, 0), 1),
        "a room id >= n_rooms": (edit(0, 2, 2), 2),
        "a decreasing first": (edit(1, 1, 5), 3),   # record 1, and slots 2 and 3 now in room 0
    }
    for tag, (bad, count) in cases.items():
        assert ro.check_tables(bad, 5) == count, tag
        g = both(engine, d, t, ext, None, bad, list_rooms=rooms, tag=tag)
        for s in (g["reply"]["def_summary"], g["reply"]["plain_summary"], g["plan"]["summary"]):
            assert jm.summary_tuple(s) == (0, 0, 0, count, gev_amd.ERR_INVALID), tag
    # a window byte of 7 on a deflate-taker: the reply step's (the plan reads no windows)
    wb = np.array([7, 7, 0, 7, 7], np.uint8)   # connection 1 is the only deflate-taking member with a bad byte
    g = both(engine, d, t, ext, wb, rooms, tag="a window byte of 7")
    assert jm.summary_tuple(g["reply"]["def_summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)
    assert int(g["plan"]["summary"]["status"]) == 0
    # a frame that ends a listed message and belongs to no connection
    short = d.conn_out.copy()
    short["nframes"][2] = 2   # connection 2's last fragment
    g = both(engine, d, t, ext, None, rooms, plan_conn_out=short, tag="a frame of no connection")
    assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)


def test_gates(engine):
    d, t, ext, rooms = small_case()
    for k in ("decoded", "msg", "join", "ctl"):
        g = both(engine, d, t, ext, None, rooms, statuses={k: gev_amd.ERR_CAPACITY}, tag=f"failed {k} summary")
        assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 0, 0)
        if k in ("msg", "join"):
            assert jm.summary_tuple(g["reply"]["def_summary"]) == (0, 0, 0, 0, 0)
            assert jm.summary_tuple(g["reply"]["plain_summary"]) == (0, 0, 0, 0, 0)
    for i in range(3):
        enc = [0, 0, 0]
        enc[i] = gev_amd.ERR_CAPACITY
        g = both(engine, d, t, ext, None, rooms, statuses=dict(enc=tuple(enc)), tag=f"failed encode {i}")
        assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 0, 0)
    # malformed tables behind a closed gate are not looked at
    bad = (rooms[0], rooms[1], np.array([9, 9, 9, 9], np.uint32))
    g = both(engine, d, t, ext, None, bad, statuses=dict(join=gev_amd.ERR_CAPACITY), list_rooms=rooms, tag="gate first")
    assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 0, 0)
