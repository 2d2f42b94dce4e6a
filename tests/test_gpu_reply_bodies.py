"""GPU checks of the reply step (gevws_reply_bodies_async) through the C ABI,
bit-exact against tests/_join_model.py -- both lists, their connection tables,
d_reply_of and the two summaries, everything else still the 0xEE it was
prefilled with -- and of the whole chain decode -> messages -> inflate -> join
-> reply -> deflate -> encode behind a real wire batch (Engine.echo_messages)."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _join_model as jm
from tests import _messages_model as mm
from tests._helpers import gpu_decode

pytestmark = pytest.mark.gpu

COUNT_BLOCK = 256  # k_reply_count / k_reply_emit: bodies a workgroup (kWalkBlock)


def summary_dev(engine, **fields):
    import torch
    s = np.zeros(1, mm.SUMMARY_DTYPE)
    for k, v in fields.items():
        s[k] = v
    return mm._dev(s, torch.device("cuda", engine.device), 64)


def make_bodies(rows):
    """rows of (off, length, conn, flags) -> BODY_DTYPE records."""
    b = np.zeros(len(rows), jm.BODY_DTYPE)
    for i, (off, n, c, fl) in enumerate(rows):
        b[i]["off"], b[i]["length"], b[i]["conn"], b[i]["flags"], b[i]["opcode"] = off, n, c, fl, 1 + i % 2
    return b


def both(engine, bodies, policy, ext, wbits, n_conns, msg=None, join=None, tag=""):
    n = bodies.shape[0]
    msg = dict(frames=n) if msg is None else msg
    join = dict(frames=n) if join is None else join
    got = jm.run_reply(engine, bodies, n, summary_dev(engine, **msg), summary_dev(engine, **join), policy, ext, wbits,
                       n_conns)
    want = jm.reply_model(bodies, policy, ext, wbits, n_conns, msg.get("status", 0), join.get("status", 0))
    jm.assert_reply(got, want, tag)
    return got, want


J, I, W = jm.WHOLE | jm.JOINED, jm.WHOLE | jm.INFLATED, jm.WHOLE
ROWS = [(0, 5, 0, J), (16, 0, 0, J), (0, 0, 1, 0), (16, 7, 1, I), (32, 300, 2, J), (336, 0, 3, I), (336, 1, 3, J),
        (0, 0, 4, 0), (352, 70000, 5, J)]
EXT = np.array([1, 0, 5, 1, 1, 0], np.uint8)
WBITS = np.array([9, 15, 12, 0, 8, 11], np.uint8)


def test_policies_and_mixed_connections(engine):
    bodies = make_bodies(ROWS)
    g, w = both(engine, bodies, gev_amd.HANDLER_ECHO_TEXT, EXT, WBITS, 6, tag="text")
    assert (int(g["def_summary"]["frames"]), int(g["plain_summary"]["frames"])) == (5, 2)
    assert list(w["reply_of"]) == [0, 1, -1, 0, 2, 3, 4, -1, 1]
    assert list(w["def_msgs"]["window_bits"]) == [9, 9, 12, 0, 0] and set(w["def_msgs"]["opcode"]) == {1}
    assert list(w["def_conn"]) == [0, 0, 2, 3, 3] and list(w["plain_conn"]) == [1, 5]
    both(engine, bodies, gev_amd.HANDLER_ECHO_BINARY, EXT, WBITS, 6, tag="binary")
    both(engine, bodies, gev_amd.HANDLER_ECHO_BINARY, EXT, None, 6, tag="no window bits")
    g, _ = both(engine, bodies, gev_amd.HANDLER_NONE, EXT, WBITS, 6, tag="none")
    assert (int(g["def_summary"]["frames"]), int(g["plain_summary"]["frames"])) == (0, 0)
    # d_conn_ext == NULL: all replies are plain, the empty messages too
    g, w = both(engine, bodies, gev_amd.HANDLER_ECHO_BINARY, None, WBITS, 6, tag="no extension table")
    assert int(g["plain_summary"]["frames"]) == 7 and list(w["plain"]["payload_len"]) == [5, 0, 7, 300, 0, 1, 70000]


def test_invalid_records_and_policy(engine):
    import torch
    bodies = make_bodies(ROWS)
    left = bodies.copy()
    left[4]["flags"] = W  # a body left in its frame's slot (a join without JOIN_ALL)
    g, _ = both(engine, left, gev_amd.HANDLER_ECHO_BINARY, EXT, WBITS, 6, tag="left in place")
    assert jm.summary_tuple(g["def_summary"]) == jm.summary_tuple(g["plain_summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)
    g, _ = both(engine, bodies, gev_amd.HANDLER_ECHO_TEXT, EXT[:5], WBITS[:5], 5, tag="conn >= n_conns")
    assert int(g["def_summary"]["errors"]) == 1
    left[8]["conn"] = 77
    g, _ = both(engine, left, gev_amd.HANDLER_ECHO_TEXT, EXT, WBITS, 6, tag="both")
    assert int(g["plain_summary"]["errors"]) == 2
    both(engine, left, gev_amd.HANDLER_NONE, EXT, WBITS, 6, tag="NONE looks at no record")
    # gates: a failed join or message summary gives zero summaries and writes nothing else
    both(engine, bodies, gev_amd.HANDLER_ECHO_TEXT, EXT, WBITS, 6, join=dict(frames=9, status=gev_amd.ERR_CAPACITY))
    both(engine, bodies, gev_amd.HANDLER_ECHO_TEXT, EXT, WBITS, 6, msg=dict(frames=9, status=gev_amd.ERR_CAPACITY))
    # the message summary's count gates the records
    g, w = both(engine, bodies[:4], gev_amd.HANDLER_ECHO_TEXT, EXT, WBITS, 6)
    got = jm.run_reply(engine, bodies, 9, summary_dev(engine, frames=4), summary_dev(engine, frames=4),
                       gev_amd.HANDLER_ECHO_TEXT, EXT, WBITS, 6)
    jm.assert_reply(got, w, "gated count")
    # an unknown policy fails the call
    dev = torch.device("cuda", engine.device)
    t = torch.zeros(4096, dtype=torch.uint8, device=dev)
    for policy in (3, -1, 99):
        st = gev_amd.lib.gevws_reply_bodies_async(engine._ctx, None, t.data_ptr(), 4, t.data_ptr(), t.data_ptr(),
                                                  policy, None, None, 6, t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                                  t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr())
        assert st == gev_amd.ERR_INVALID, policy


def test_compaction_across_blocks(engine):
    rng = np.random.default_rng(0x72706C)
    n = 3 * COUNT_BLOCK + 41
    rows, off = [], 0
    for m in range(n):
        k = int(rng.integers(0, 4))
        length = int(rng.integers(0, 40))
        rows.append((off, length, m // 3, [0, J, I, J][k]))
        off += jm.round16(length)
    ext = (np.arange(n // 3 + 1) % 3 != 0).astype(np.uint8)
    wb = (8 + np.arange(n // 3 + 1) % 8).astype(np.uint8)
    g, w = both(engine, make_bodies(rows), gev_amd.HANDLER_ECHO_BINARY, ext, wb, n // 3 + 1)
    assert int(g["def_summary"]["frames"]) > COUNT_BLOCK and int(g["plain_summary"]["frames"]) > 100
    assert np.all(np.diff(w["def_conn"].astype(np.int64)) >= 0)  # one run per connection, as takeover requires


def test_summaries_gate_the_deflate_and_the_encode(engine):
    """The two summaries as gevws_deflate_async's d_prev and
    gevws_encode_replies_async's d_dispatched: the lists' counts, read on the
    device."""
    import torch
    dev = torch.device("cuda", engine.device)
    data = [b"first body, " * 9, b"", b"second " * 40, b"plain one", b"x" * 33]
    arena, rows, off = bytearray(), [], 0
    for i, x in enumerate(data):
        rows.append((off, len(x), i, J))
        arena += x + bytes(jm.round16(len(x)) - len(x))
        off += jm.round16(len(x))
    d_arena = mm._dev(np.frombuffer(bytes(arena) + bytes(gev_amd.IN_PAD), np.uint8), dev)
    ext = np.array([1, 1, 1, 0, 0], np.uint8)
    got = jm.run_reply(engine, make_bodies(rows), 5, summary_dev(engine, frames=5), summary_dev(engine, frames=5),
                       gev_amd.HANDLER_ECHO_TEXT, ext, None, 5)
    t = got["dev"]
    cap = 4096
    frames = torch.zeros((5, 32), dtype=torch.uint8, device=dev)
    out = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    dsum = torch.zeros(64, dtype=torch.uint8, device=dev)
    engine.deflate_async(t["def_msgs"], 5, t["def_summary"], d_arena, len(arena), 0, frames, out, cap, dsum)
    wire = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    woff = torch.zeros(5, dtype=torch.int64, device=dev)
    esum = torch.zeros(64, dtype=torch.uint8, device=dev)
    engine.encode_replies_async(t["plain"], 5, t["plain_summary"], d_arena, wire, cap, woff, esum)
    torch.cuda.synchronize(engine.device)
    ds = dsum.cpu().numpy().view(mm.SUMMARY_DTYPE)[0]
    assert (int(ds["status"]), int(ds["frames"])) == (0, 3)
    fr = frames[:3].cpu().numpy().reshape(-1).view(gev_amd.OUT_FRAME_DTYPE)
    outh = out.cpu().numpy()
    for k in range(3):
        p = outh[int(fr["payload_off"][k]):][: int(fr["payload_len"][k])].tobytes()
        assert p == gev_amd.deflate_raw(data[k]) and int(fr["rsv"][k]) == 4 and int(fr["opcode"][k]) == 1
    es = esum.cpu().numpy().view(mm.SUMMARY_DTYPE)[0]
    assert (int(es["status"]), int(es["frames"])) == (0, 2)
    want = b"".join(wo.encode_frame(x, 1, True, 0, False) for x in data[3:])
    assert wire[: int(es["payload_bytes"])].cpu().numpy().tobytes() == want


# ---------------------------------------------------------------------------- end to end
def test_echo_messages_end_to_end(engine):
    import torch
    rng = np.random.default_rng(0x65326532)
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

    def comp(co, data):
        return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]

    kib = bytes(rng.integers(0, 256, 1024, dtype=np.uint8))
    words = (b"the quick brown fox jumps over the lazy dog; " * 40)
    tk_msgs = [words[:700], b"", words[100:1500]]
    received = [
        [kib, b"short"],                       # plain connection: 1 KiB in 7 fragments, pings in between
        [words],                               # deflate, no takeover: one compressed message in 3 fragments
        tk_msgs,                               # deflate with server takeover: compressed messages in
        [b"", bytes(range(256)) * 3],          # deflate connection sending plain messages, one empty
    ]
    streams = [
        frames_of(kib, 2, (100, 101, 300, 555, 800, 1023)) + frames_of(b"short", 2, (), pings=False),
        frames_of(comp(zlib.compressobj(6, zlib.DEFLATED, -15), words), 1, (3, 20), rsv=4),
        b"".join(frames_of(comp(zlib.compressobj(6, zlib.DEFLATED, -15), x), 1, (1,) if x else (), rsv=4)
                 for x in tk_msgs),
        frames_of(b"", 2, (), pings=False) + frames_of(received[3][1], 2, (255, 256, 700)),
    ]
    ext_h = np.array([0, gev_amd.EXT_DEFLATE, gev_amd.EXT_DEFLATE | gev_amd.EXT_SERVER_TAKEOVER, gev_amd.EXT_DEFLATE],
                     np.uint8)
    wb_h = np.array([0, 0, 12, 10], np.uint8)
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1))
    ext, wb = mm._dev(ext_h, dev, 1), mm._dev(wb_h, dev, 1)
    msgs = engine.messages(batch, conn_ext=ext)
    assert not msgs.conn_msg_host()["error"].any()
    inf = engine.inflate(batch, msgs, 1 << 20)
    bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)
    rec, mh = bodies.bodies_host(), msgs.messages_host()
    flat = [(c, x) for c, xs in enumerate(received) for x in xs]
    assert [int(c) for c in mh["conn"]] == [c for c, _ in flat]
    assert [bodies.body_bytes(m) for m in range(len(flat))] == [x for _, x in flat]
    assert np.all(rec["flags"] & gev_amd.BODY_WHOLE)
    ctxs = torch.zeros((4, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    echo = engine.echo_messages(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, wb, ctxs)
    # the wire buffers parsed on the host: every reply equals the message received, in per-connection order
    plain = wo.decode_stream(echo.plain_wire.cpu().numpy().tobytes())
    assert plain.status == wo.OK and plain.consumed == echo.plain_wire.numel()
    assert list(echo.plain_conn) == [0, 0] and [f.payload for f in plain.frames] == received[0]
    assert all(f.header.fin and f.header.rsv == 0 and f.header.opcode == 1 and not f.header.masked
               for f in plain.frames)
    wire = echo.def_wire.cpu().numpy().tobytes()
    dfl = wo.decode_stream(wire)
    assert dfl.status == wo.OK and dfl.consumed == len(wire) and len(dfl.frames) == len(flat) - 2
    assert list(echo.def_conn) == [c for c, _ in flat if c]
    assert list(echo.reply_of) == [0, 1, *range(len(flat) - 2)]
    pos = 0
    for k, f in enumerate(dfl.frames):  # the offset table points at each reply's header
        assert int(echo.def_off[k]) == pos
        pos += f.header_len + len(f.payload)
    inflaters = {}
    for c, f, (_, want) in zip(echo.def_conn, dfl.frames, [x for x in flat if x[0]]):
        assert f.header.fin and f.header.rsv == 4 and f.header.opcode == 1
        takeover = bool(int(ext_h[c]) & gev_amd.EXT_SERVER_TAKEOVER)
        z = inflaters.setdefault(int(c), zlib.decompressobj(-15)) if takeover else zlib.decompressobj(-15)
        assert z.decompress(f.payload + b"\x00\x00\xff\xff") == want, (int(c), len(want))
    # byte for byte what Engine.deflate gives for the same messages with a host-built list
    sel = [m for m in range(len(flat)) if flat[m][0]]
    host = np.zeros(len(sel), gev_amd.DEFLATE_MSG_DTYPE)
    for k, m in enumerate(sel):
        host[k]["payload_off"], host[k]["length"] = rec["off"][m], rec["length"][m]
        host[k]["opcode"], host[k]["window_bits"] = 1, wb_h[flat[m][0]]
    ctxs2 = torch.zeros((4, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    ref = engine.deflate(host, bodies.out, int(bodies.summary_host()["payload_bytes"]),
                         msg_conn=np.array([flat[m][0] for m in sel], np.uint32), conn_ext=ext, contexts=ctxs2)
    assert [ref.payload(k) for k in range(len(sel))] == [f.payload for f in dfl.frames]
    assert torch.equal(ctxs, ctxs2)
