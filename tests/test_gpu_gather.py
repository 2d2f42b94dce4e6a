"""GPU checks of the gather (gevws_send_gather_async) through the C ABI,
bit-exact against tests/_gather_model.py -- the whole send buffer with the
bytes behind its used part, d_conn_buf and the summary, everything else still
the 0xEE it was prefilled with -- and of the whole chain behind a real wire
batch (Engine.respond(gather=True)) against Responses.conn_bytes."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _gather_model as gm
from tests import _messages_model as mm
from tests._helpers import gpu_decode

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = (8 * 1024 + 5, 6001, 48 * 1024 + 9)  # the three wires' readable bytes (none a multiple of 16)


def make_wires(seed=0x6761, sizes=SIZES):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, n, dtype=np.uint8) for n in sizes]  # (no zero byte: a pad is told from data)


def at_shift(rng, wire: int, shift: int, length: int, sizes=SIZES):
    """A source offset in `wire` whose low four bits are `shift` (the wires start on 16)."""
    hi = (sizes[wire] - length - shift) // 16
    return int(rng.integers(0, hi + 1)) * 16 + shift


def every_path_lists():
    rng = np.random.default_rng(0x70617468)
    conns = [[], []]                                       # count == 0 at the start
    # every (source offset & 15, destination offset & 15): a prefix of d bytes shifts the destination
    for s in range(16):
        for d in range(16):
            w, ln = int(rng.integers(0, 3)), int(rng.integers(1040, 1101))
            pre = [(int(rng.integers(0, 3)), int(rng.integers(0, 4000)), d)] if d else []
            conns.append(pre + [(w, at_shift(rng, w, s, ln), ln)])
    lengths = [0, 1, 2, 6, 15, 16, 17, 125, 127, 1023, 1024, 1025, 4097]
    for ln in lengths:                                     # each alone in its span ...
        conns.append([(2, at_shift(rng, 2, int(rng.integers(0, 16)), ln), ln)])
    conns.append([])                                       # ... count == 0 in the middle ...
    conns.append([(2, at_shift(rng, 2, int(rng.integers(0, 16)), ln), ln) for ln in lengths])  # ... and back to back
    # long segments: kept from tile to tile, then the step forward to the next long one
    conns.append([(2, 3, 12 * 1024 + 5), (2, 77, 40 * 1024 + 3), (0, 9, 3000)])
    conns.append([(int(rng.integers(0, 3)), int(rng.integers(0, 4000)), int(rng.integers(1030, 1101)))
                  for _ in range(8)])                      # rows of one tile from entry after entry
    conns.append([(2, int(rng.integers(0, 40000)), 6) for _ in range(40)])  # one vector spans three entries
    conns.append([])
    conns.append([(0, SIZES[0] - 100, 100)])               # segments that end on their wire's last byte
    conns.append([(1, SIZES[1] - 1, 1), (2, SIZES[2] - 1500, 1500)])
    conns.append([(0, 5, 700), (1, 6, 30), (2, 7, 1200), (1, 0, 3), (0, 0, 1)])  # all three wires in one span
    conns += [[], [], []]                                  # count == 0 at the end
    return gm.make_lists(conns, flags=[int(rng.integers(0, 4)) for _ in conns])


@pytest.fixture(scope="module")
def every_path():
    wires = make_wires()
    send, cs = every_path_lists()
    want = gm.gather_model(send, cs, wires, list(SIZES), 1 << 30)
    assert want["summary"]["status"] == 0 and send.shape[0] > 512  # (more than two blocks of the table passes)
    return wires, send, cs, want


def test_every_path_once(engine, every_path):
    wires, send, cs, want = every_path
    cap = want["summary"]["payload_bytes"]
    assert cap > 64 * TILE
    got = gm.run_gather(engine, send, cs, wires, list(SIZES), cap)  # (the capacity is exactly the need)
    gm.assert_gather(got, want, "every path")


def test_mapped_host_memory(engine, every_path):
    import torch
    wires, send, cs, want = every_path
    cap = want["summary"]["payload_bytes"]
    arena = gev_amd.PinnedArena(cap + gm.GUARD_BYTES)
    try:
        got = gm.run_gather(engine, send, cs, wires, list(SIZES), cap, pinned=arena)
        gm.assert_gather(got, want, "pinned")
        torch.cuda.synchronize(engine.device)
        assert arena.host[:cap].tobytes() == want["buf"].tobytes()
        assert np.all(arena.host[cap:] == gm.FILL)
    finally:
        arena.close()


def test_tile_runs(engine):
    rng = np.random.default_rng(0x74696C65)
    wires = make_wires(3)
    both = lambda *a, **k: (gm.run_gather(engine, *a, **k), gm.gather_model(*a, **k))  # noqa: E731
    # a little over 4 MiB: 1 030-odd tiles, workgroups with runs of one and of two tiles
    conns, total = [], 0
    while total < 1031 * TILE:
        ents = []
        for _ in range(int(rng.integers(1, 5))):
            w = int(rng.integers(0, 3))
            ln = int(rng.choice([int(rng.integers(0, 200)), int(rng.integers(1024, 5000)), int(rng.integers(5000, 40000))]))
            ln = min(ln, SIZES[w])
            ents.append((w, int(rng.integers(0, SIZES[w] - ln + 1)), ln))
        conns.append(ents)
        total += gm.round16(sum(e[2] for e in ents))
    send, cs = gm.make_lists(conns)
    got, want = both(send, cs, wires, list(SIZES), total + 4096)
    assert 1030 < want["summary"]["payload_bytes"] / TILE < 1045
    gm.assert_gather(got, want, "4 MiB")
    # six tiles a workgroup, so two of its four waves take a second tile four further on: a long segment kept from
    # tile to tile, short entries in between, re-found behind them
    big = [rng.integers(1, 256, 6 * 1024 * 1024 + 11, dtype=np.uint8), wires[1], wires[2]]
    bsz = [big[0].size, SIZES[1], SIZES[2]]
    conns = [[(0, 3, 6 * 1024 * 1024 + 5), (1, 0, 6), (1, 7, 6), (0, 1, 2 * 1024 * 1024 + 1), (2, 77, 40 * 1024 + 3)],
             [(0, 16, 6 * 1024 * 1024 - 64)], [(2, 5, 3)], [(0, 9, 6 * 1024 * 1024 - 9), (0, 0, 4 * 1024 * 1024 + 13)]]
    send, cs = gm.make_lists(conns)
    got, want = both(send, cs, big, bsz, 32 * 1024 * 1024)
    assert want["summary"]["payload_bytes"] > 5 * 1024 * TILE  # 1 024 workgroups: five tiles each and more
    gm.assert_gather(got, want, "24 MiB")
    # a single partial tile; a single 3-byte entry
    send, cs = gm.make_lists([[(0, 1, 700), (2, 2, 33)], [(1, 3, 1500)]])
    got, want = both(send, cs, wires, list(SIZES), 4096)
    assert want["summary"]["payload_bytes"] == 736 + 1504
    gm.assert_gather(got, want, "partial tile")
    send, cs = gm.make_lists([[(1, SIZES[1] - 3, 3)]])
    got, want = both(send, cs, wires, list(SIZES), 16)
    assert want["summary"] == dict(frames=1, payload_bytes=16, payload_len=3, errors=0, status=0)
    gm.assert_gather(got, want, "three bytes")


def test_gates_capacity_and_malformed(engine):
    """Plain failing-status checks: every one is rejected before an address is formed."""
    wires = make_wires(5)
    sizes = list(SIZES)
    base = [[(0, 0, 4), (2, 1, 3)], [], [(1, 2, 9)], [(0, 8, 2000), (0, 16, 8)]]

    def both(edit=None, cap=1 << 16, n_conns=None, **kw):
        send, cs = gm.make_lists(base, n_conns=n_conns)
        if edit:
            edit(send, cs)
        return gm.run_gather(engine, send, cs, wires, sizes, cap, **kw), gm.gather_model(send, cs, wires, sizes, cap, **kw)

    got, want = both()
    assert want["summary"]["status"] == 0
    gm.assert_gather(got, want, "valid")
    # gates: a failed plan, no entries, no connections
    for kw in (dict(plan_status=gm.ERR_CAPACITY), dict(plan_status=gm.ERR_INVALID), dict(plan_frames=0)):
        got, want = both(**kw)
        assert want["buf"] is None and want["summary"]["status"] == 0 and want["summary"]["frames"] == 0
        gm.assert_gather(got, want, ("gate", kw))
    send, cs = gm.make_lists(base)
    for s, c in ((send, cs[:0]), (send[:0], cs)):
        got = gm.run_gather(engine, s, c, wires, sizes, 1 << 16)
        want = gm.gather_model(s, c, wires, sizes, 1 << 16)
        assert want["buf"] is None
        gm.assert_gather(got, want, "empty table")
    # the plan counts fewer entries than the table holds: a valid prefix
    got, want = both(lambda s, c: c.__setitem__(3, (3, 1, 2000, 0, 0)), plan_frames=4)
    assert want["summary"]["status"] == 0 and want["summary"]["frames"] == 4
    gm.assert_gather(got, want, "prefix")
    # capacity: one vector short
    need = gm.gather_model(*gm.make_lists(base), wires, sizes, 1 << 16)["summary"]["payload_bytes"]
    got, want = both(cap=need - 16)
    assert want["summary"]["status"] == gm.ERR_CAPACITY and want["summary"]["payload_bytes"] == need
    gm.assert_gather(got, want, "capacity")
    # each malformed case alone, then two at once
    top = (1 << 64) - 1

    def put(table, i, field, v):
        def edit(send, cs):
            (send if table == "send" else cs)[i][field] = v
        return edit

    def two(send, cs):
        send[1]["wire"] = 7
        cs[2]["bytes"] = 1

    cases = [("wire", put("send", 1, "wire", 3), 2), ("wire top", put("send", 1, "wire", 0xFFFFFFFF), 2),
             ("range", put("send", 2, "off", SIZES[1] - 8), 2), ("range wraps", put("send", 2, "off", top - 3), 2),
             ("len wraps", put("send", 2, "len", top), 2), ("conn", put("send", 0, "conn", 4), 2),
             ("conn top", put("send", 0, "conn", 0xFFFFFFFF), 2), ("other conn", put("send", 0, "conn", 2), 2),
             ("count beyond", put("conn_send", 3, "count", 3), 1), ("count wraps", put("conn_send", 3, "count", top), 1),
             ("first beyond", put("conn_send", 3, "first", 6), 3), ("first wraps", put("conn_send", 3, "first", top), 3),
             ("overlap", put("conn_send", 2, "first", 1), 2), ("precedes", put("conn_send", 1, "first", 1), 1),
             ("bytes", put("conn_send", 2, "bytes", 8), 1), ("bytes of none", put("conn_send", 1, "bytes", 16), 1),
             ("two", two, 3)]
    for tag, edit, errors in cases:
        got, want = both(edit)
        assert want["buf"] is None and want["summary"] == dict(frames=0, payload_bytes=0, payload_len=0, errors=errors,
                                                               status=gm.ERR_INVALID), (tag, want["summary"])
        gm.assert_gather(got, want, tag)


def comp(data: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]


def test_respond_gather_end_to_end(engine):
    import torch
    rng = np.random.default_rng(0x67326533)
    dev = torch.device("cuda", engine.device)

    def key():
        return bytes(rng.integers(0, 256, 4, dtype=np.uint8))

    def frames_of(data: bytes, op: int, cuts, rsv=0, pings=True):
        edges = [0, *cuts, len(data)]
        s = b""
        for i in range(len(edges) - 1):
            last = i == len(edges) - 2
            s += wo.encode_frame(data[edges[i]:edges[i + 1]], op if i == 0 else 0, last, rsv if i == 0 else 0, True,
                                 key())
            if pings and not last:
                s += wo.encode_frame(b"ping %d" % i, 9, True, 0, True, key())
        return s

    blob = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    words = b"the quick brown fox jumps over the lazy dog; " * 40
    close = wo.encode_frame((1000).to_bytes(2, "big") + b"bye", 8, True, 0, True, key())
    streams = [
        frames_of(blob, 2, (100, 1500)) + frames_of(b"short", 2, (), pings=False),          # plain, pings between fragments
        frames_of(comp(words), 1, (3, 20), rsv=4),                                          # deflate
        b"",                                                                                # idle
        frames_of(b"before", 1, (), pings=False) + close + frames_of(b"behind the close", 1, (), pings=False),
        frames_of(b"fine", 1, (2,)) + frames_of(b"bad \xff\xfe utf-8", 1, (), pings=False) + frames_of(b"late", 1, ()),
        frames_of(comp(b"inflates " * 9), 1, (), rsv=4) + wo.encode_frame(b"pong me", 9, True, 0, True, key()),
    ]
    D = gev_amd.EXT_DEFLATE
    ext_h = np.array([0, D, 0, 0, 0, D], np.uint8)
    nc = len(streams)
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    conns = np.stack([offs, lens], 1)
    ext = mm._dev(ext_h, dev, 1)

    def chain():
        batch = gpu_decode(engine, b"".join(streams), conns, aux_slots=nc)
        msgs = engine.messages(batch, conn_ext=ext)
        inf = engine.inflate(batch, msgs, 1 << 20)
        return batch, msgs, engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)

    res = engine.respond(*chain(), gev_amd.HANDLER_ECHO_TEXT, ext, gather=True)
    old = engine.respond(*chain(), gev_amd.HANDLER_ECHO_TEXT, ext)
    # without the gather every field and byte is as before, and the gather changes none of them
    assert old.send_buf is None and old.conn_buf is None and old.gather_summary is None
    assert old.send_host().tobytes() == res.send_host().tobytes()
    assert old.conn_send_host().tobytes() == res.conn_send_host().tobytes()
    for a, b in ((old.echo.plain_wire, res.echo.plain_wire), (old.echo.def_wire, res.echo.def_wire),
                 (old.ctl_wire, res.ctl_wire)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        old.host_sends()
    cs, cb, gs = res.conn_send_host(), res.conn_buf, res.gather_summary
    S, F = gev_amd.CTL_SHUTDOWN, gev_amd.CTL_SHUTDOWN | gev_amd.CTL_FAILED
    assert [int(x) for x in cs["flags"]] == [0, 0, 0, S, F, 0] == [int(x) for x in cb["flags"]]
    assert int(cs["count"][2]) == 0 and int(cb["bytes"][2]) == 0 and int(cs["bytes"][0]) > 3000
    buf = res.send_buf.cpu().numpy()
    assert int(gs["status"]) == 0 and int(gs["errors"]) == 0 and int(gs["frames"]) == int(res.summary_host()["frames"])
    assert buf.size == int(gs["payload_bytes"]) and int(gs["payload_len"]) == int(cs["bytes"].sum())
    sends = res.host_sends()
    assert len(sends) == nc
    end = 0
    for c in range(nc):
        off, nb = int(cb["off"][c]), int(cb["bytes"][c])
        want = old.conn_bytes(c)  # the three-wire join on the host
        assert off == end and off % 16 == 0 and nb == int(cs["bytes"][c]) == len(want), c
        assert buf[off: off + nb].tobytes() == want, c
        assert bytes(sends[c]) == want, c
        end = off + gm.round16(nb)
        assert not buf[off + nb: end].any(), c
        assert not cb["reserved"][c].any()
    assert end == buf.size
    # what leaves is what a host that walks the frames would send: spot checks of the kinds
    first = wo.decode_stream(bytes(sends[0]) + b"\x88\x00" * 3).frames
    assert [f.header.opcode for f in first[:4]] == [10, 10, 1, 1] and first[2].payload == blob
    assert bytes(sends[4])[-4:] == b"\x88\x02" + (1007).to_bytes(2, "big")
