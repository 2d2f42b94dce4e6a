"""GPU checks of the control step and the send plan (gevws_control_async,
gevws_send_plan_async) through the C ABI, bit-exact against
tests/_respond_model.py -- every table, the summaries, d_bodies and the aux
region, everything else still the 0xEE it was prefilled with -- and of the whole
chain behind a real wire batch (Engine.respond)."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm
from tests._helpers import gpu_decode
from tests._session import host_walk

pytestmark = pytest.mark.gpu

T, B, C, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
NO = rm.NO_FRAME
BLOCK = 256  # frames / connections / messages a workgroup (kWalkBlock)


def comp(data: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]


def control_both(engine, d, t, flags=0, n_decoded=None, tag="", **kw):
    got = rm.run_control(engine, d, t, flags, **kw)
    model_kw = {k: v for k, v in kw.items() if k in ("msg_status", "join_status")}
    want = rm.control_model(d.frames, d.conn_out, d.n_decoded if n_decoded is None else n_decoded, d.arena, t["msg_of"],
                            t["messages"], t["conn_msg"], t["bodies"], flags, got["aux_off"], got["aux_cap"],
                            **model_kw)
    rm.assert_control(got, want, d, t, tag)
    return got, want


def wires_of(rep: dict, ctl: dict, n_def=None):
    """Offset tables and encode summaries as the three encodes would leave them
    (a 2-byte header and the payload, frames back to back); the deflated wire's
    payloads are taken as long as the plain bytes."""
    n_def = rep["def_msgs"].shape[0] if n_def is None else n_def
    sizes = [[2 + int(x) for x in rep["plain"]["payload_len"]], [2 + int(x) for x in rep["def_msgs"]["length"][:n_def]],
             [2 + int(x) for x in ctl["ctl"]["payload_len"]]]
    tabs = [np.concatenate([[0], np.cumsum(s)[:-1]]).astype(np.uint64) if s else np.zeros(0, np.uint64) for s in sizes]
    model = [(tab, len(s), int(sum(s))) for tab, s in zip(tabs, sizes)]
    dev = [(tab, rm.summary_np(frames=len(s), payload_bytes=int(sum(s)))) for tab, s in zip(tabs, sizes)]
    return model, dev


def plan_both(engine, d, t, ctl, ext, max_sends=None, reply_of=None, statuses=None, tag=""):
    """The plan on the control model's tables, the reply model's d_reply_of and
    synthetic wires: device == model."""
    n, nm, nc = d.n_decoded, t["messages"].shape[0], d.conn_out.shape[0]
    rep = jm.reply_model(ctl["bodies"], jm.HANDLER_ECHO_BINARY, ext, None, nc)
    ro = rep["reply_of"] if reply_of is None else reply_of
    model_w, dev_w = wires_of(rep, ctl)
    st = dict(decoded=0, msg=0, join=0, ctl=0, enc=(0, 0, 0))
    st.update(statuses or {})
    for (tab, s), e in zip(dev_w, st["enc"]):
        s["status"] = e
    gate_ok = not (st["decoded"] or st["msg"] or st["join"] or st["ctl"] or any(st["enc"]))
    cap = n if max_sends is None else max_sends
    want = rm.plan_model(n, d.conn_out, t["msg_of"], ctl["msg_end"], ro, nm, ext, ctl["ctl_of"], ctl["conn_ctl"],
                         model_w, cap, gate_ok)
    dsum = d.summary.copy()
    dsum["status"] = st["decoded"]
    got = rm.run_plan(engine, n, dsum, d.conn_out, t["msg_of"], ctl["msg_end"], ro, nm,
                      rm.summary_np(frames=nm, status=st["msg"]), rm.summary_np(frames=nm, status=st["join"]), ext,
                      ctl["ctl_of"], ctl["conn_ctl"],
                      rm.summary_np(frames=ctl["ctl"].shape[0], status=st["ctl"]), dev_w, cap)
    rm.assert_plan(got, want, tag)
    return got, want


# ---------------------------------------------------------------------------- 1. every path once, behind the real chain
def test_every_path_once(engine):
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x63746C31)

    def fr(payload, op, fin=True, rsv=0):
        return wo.encode_frame(payload, op, fin, rsv, True, bytes(rng.integers(0, 256, 4, dtype=np.uint8)))

    good = fr(b"good", B)
    code = lambda c, reason=b"": c.to_bytes(2, "big") + reason  # noqa: E731
    streams = [
        fr(b"ab", B, False) + fr(b"between", PING) + fr(b"cd", C) + fr(b"behind the FIN", PING),   # 0
        fr(b"a pong", PONG),                                                                        # 1
        fr(b"", CLOSE),                                                                             # 2
        fr(code(1000, b"bye"), CLOSE),                                                              # 3
        fr(code(999), CLOSE),                                                                       # 4
        fr(code(1005), CLOSE),                                                                      # 5
        fr(code(1000, b"\xc3\x28"), CLOSE),                                                         # 6
        fr(code(1001, b"r" * 123), CLOSE),                                                          # 7
        fr(b"he", T, False) + fr(code(1000), CLOSE) + fr(b"llo", C),                                # 8
        good + fr(b"", CLOSE) + good,                                                               # 9
        good + fr(b"rsv", B, rsv=2) + good,                                                         # 10 error 1
        good + fr(b"", 5) + fr(b"", PING),                                                          # 11 error 2
        good + fr(b"", PING, False),                                                                # 12 error 3
        good + fr(b"", C),                                                                          # 13 error 4
        good + fr(b"a", T, False) + fr(b"b", T),                                                    # 14 error 5
        good + fr(b"ok", T, False) + fr(b"\xff", C) + good,                                         # 15 text UTF-8
        fr(b"\x07\x00", B, rsv=4) + fr(b"pi", PING) + fr(comp(b"hello hello hello"), B, rsv=4),     # 16 broken stream
        fr(comp(b"x" * 200), T, rsv=4) + good,                                                      # 17 over the limit
        fr(b"comes in failed", PING) + good,                                                        # 18
        b"",                                                                                        # 19
        fr(b"before", PING) + b"\x82\xff\x80" + bytes(11),                                          # 20 LEN_MSB
    ]
    nc = len(streams)
    ext_h = np.zeros(nc, np.uint8)
    ext_h[16] = ext_h[17] = gev_amd.EXT_DEFLATE
    st_h = np.zeros(nc, mm.MSG_STATE_DTYPE)
    st_h[18]["failed"] = mm.ERR_OPCODE
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1))
    ext = mm._dev(ext_h, dev, 1)
    msgs = engine.messages(batch, state=mm._dev(st_h, dev, 8), conn_ext=ext)
    inf = engine.inflate(batch, msgs, 64)
    bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)
    d = mm.Decoded.from_arrays(batch.frames_host(), batch.conn_out_host(), batch.payload_host())
    t = dict(messages=msgs.messages_host(), msg_of=msgs.msg_of_host(), conn_msg=msgs.conn_msg_host(),
             bodies=bodies.bodies_host())
    assert int(d.conn_out["status"][20]) == gev_amd.ERR_LEN_MSB and int(d.conn_out["nframes"][20]) == 1
    assert [int(x) for x in t["conn_msg"]["error"][10:16]] == [1, 2, 3, 4, 5, 6]
    first = [int(x) for x in d.conn_out["first_frame"]]
    S, F = rm.SHUTDOWN, rm.SHUTDOWN | rm.FAILED
    cuts = [(NO, 0, 0), (NO, 0, 0), (first[2], 0, S), (first[3], 0, S), (first[4], 0, S), (first[5], 0, S),
            (first[6], 0, S), (first[7], 0, S), (first[8] + 1, 0, S), (first[9] + 1, 0, S), (first[10] + 1, 1002, F),
            (first[11] + 1, 1002, F), (first[12] + 1, 1002, F), (first[13] + 1, 1002, F), (first[14] + 2, 1002, F),
            (first[15] + 2, 1007, F), (first[16], 1007, F), (first[17], 1009, F), (NO, 0, 0), (NO, 0, 0), (NO, 0, 0)]
    for flags in (0, gev_amd.CONTROL_NO_PING_FOR_PONG):
        got, want = control_both(engine, d, t, flags, tag=f"flags {flags}")
        assert [(int(r["cut_frame"]), int(r["close_code"]), int(r["flags"])) for r in want["conn_ctl"]] == cuts
        assert int(got["summary"]["errors"]) == 16 and int(got["summary"]["status"]) == 0
        assert [op for _, op, _ in rm.conn_replies(want, 1)] == ([] if flags else [9])
        assert [op for _, op, _ in rm.conn_replies(want, 0)] == [10, 10]
        assert rm.conn_replies(want, 16) == [(first[16], 8, (1007).to_bytes(2, "big"))]   # no pong behind the cut
        assert rm.conn_replies(want, 7)[0][2] == code(1001, b"r" * 123)
        assert not rm.conn_replies(want, 18) and not rm.conn_replies(want, 20)
        # the messages behind a cut are not delivered any more
        wb = want["bodies"]
        for c, n_closed in ((8, 1), (9, 1), (10, 0), (15, 0), (16, 1), (17, 1)):
            mine = wb[wb["conn"] == c]
            assert int(np.count_nonzero(mine["status"] == rm.ERR_CLOSED)) == n_closed, c
        plan_both(engine, d, t, want, ext_h, tag=f"plan, flags {flags}")


# ---------------------------------------------------------------------------- 2. across block boundaries
def random_batch(rng, n_conns, n_frames):
    counts = rng.integers(1, 4, n_conns)
    counts[rng.integers(0, n_conns, 8)] = 0
    while counts.sum() < n_frames:
        counts[rng.integers(0, n_conns)] += 1
    while counts.sum() > n_frames:
        c = rng.integers(0, n_conns)
        counts[c] -= counts[c] > 0
    for edge in range(BLOCK, n_frames, BLOCK):   # a connection's frames straddle every block boundary
        ends = np.flatnonzero(np.cumsum(counts) == edge)
        if ends.size:
            nxt = ends[0] + 1 + int(np.flatnonzero(counts[ends[0] + 1:])[0])
            counts[ends[0]] -= 1
            counts[nxt] += 1
    conns = []
    for c in range(n_conns):
        frs, open_msg = [], False
        for _ in range(int(counts[c])):
            k = rng.random()
            data = bytes(rng.integers(0x20, 0x7F, int(rng.integers(0, 20)), dtype=np.uint8))
            if k < 0.30:
                frs.append((1, 0, [PING, PONG][int(rng.integers(0, 2))], data))
            elif k < 0.34:
                frs.append((1, 0, CLOSE, b"" if rng.random() < 0.5 else (1000).to_bytes(2, "big") + data))
            elif k < 0.38:
                frs.append((1, 1, B, data))           # ERR_RSV
            elif open_msg:
                fin = int(rng.random() < 0.6)
                frs.append((fin, 0, C, data))
                open_msg = not fin
            else:
                fin = int(rng.random() < 0.6)
                frs.append((fin, 0, B, data))
                open_msg = not fin
        conns.append(frs)
    return conns


def test_compaction_across_blocks(engine):
    rng = np.random.default_rng(0x63746C32)
    n = 3 * BLOCK + 41
    conns = random_batch(rng, BLOCK + 44, n)
    # a cut in the first and in the last block, whatever the draw
    conns[0] = [(1, 0, CLOSE, b"")] + conns[0][1:]
    last = max(c for c in range(len(conns)) if conns[c])
    conns[last] = conns[last][:-1] + [(1, 0, CLOSE, (1001).to_bytes(2, "big"))]
    d = mm.Decoded(conns)
    assert d.n_decoded == n and d.conn_out.shape[0] > BLOCK
    t0 = rm.tables_of(d)
    whole = np.flatnonzero(t0["bodies"]["flags"] & jm.WHOLE)
    failed = {int(m): int(rng.choice([6, 7, 8])) for m in rng.choice(whole, 12, replace=False)}
    t = rm.tables_of(d, inflated_status=failed)
    conn_of = np.repeat(np.arange(d.conn_out.shape[0]), d.conn_out["nframes"])
    for edge in (BLOCK, 2 * BLOCK, 3 * BLOCK):   # a connection's frames straddle each block boundary
        assert conn_of[edge - 1] == conn_of[edge], edge
    ext = (np.arange(d.conn_out.shape[0]) % 3 == 0).astype(np.uint8)
    for flags in (0, 1):
        got, want = control_both(engine, d, t, flags, tag=f"flags {flags}")
        cut = want["conn_ctl"]["cut_frame"]
        has = cut != NO
        assert int(cut[has].min()) < BLOCK and int(cut[has].max()) >= 3 * BLOCK
        assert int(got["summary"]["frames"]) > 100 and int(got["summary"]["payload_bytes"]) > 20
        assert np.count_nonzero(want["conn_ctl"]["flags"] == rm.SHUTDOWN) > 5
        assert np.count_nonzero(want["conn_ctl"]["flags"] == rm.SHUTDOWN | rm.FAILED) > 10
        assert np.count_nonzero(want["bodies"]["status"] == rm.ERR_CLOSED) > 5
        g, w = plan_both(engine, d, t, want, ext, tag=f"plan, flags {flags}")
        assert int(g["summary"]["frames"]) > BLOCK and len(set(w["send"]["wire"])) == 3
        assert np.all(np.diff(w["send"]["conn"].astype(np.int64)) >= 0)


# ---------------------------------------------------------------------------- 3. gates and capacity
def test_gates_capacity_and_malformed_tables(engine):
    good = (1, 0, B, b"good")
    conns = [
        [good, (1, 0, PING, b"pi"), (1, 0, CLOSE, (1000).to_bytes(2, "big")), good],
        [good, (1, 2, B, b"rsv")],
        [(0, 0, T, b"op"), (1, 0, PONG, b""), (1, 0, C, b"en")],
        [good, (1, 0, CLOSE, b"")],
    ]
    d = mm.Decoded(conns)
    t = rm.tables_of(d)
    ext = np.array([0, 0, 1, 0], np.uint8)
    _, ctl = control_both(engine, d, t, aux_slots=2, tag="exactly enough slots")
    assert ctl["summary"] == dict(frames=5, payload_bytes=2, payload_len=0, errors=3, status=0)
    g, w = control_both(engine, d, t, aux_slots=1, tag="one slot short")
    assert w["summary"]["status"] == gev_amd.ERR_CAPACITY and int(g["summary"]["payload_bytes"]) == 2
    # gates: a zero summary, nothing else read or written
    for kw in (dict(msg_status=gev_amd.ERR_CAPACITY), dict(join_status=gev_amd.ERR_CAPACITY)):
        g, _ = control_both(engine, d, t, tag=str(kw), **kw)
        assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 0, 0)
    g, _ = control_both(engine, d, t, n_decoded=0, decoded_status=gev_amd.ERR_CAPACITY, tag="failed decode")
    assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 0, 0)
    # malformed tables: INVALID with the count, caught before anything is indexed by them
    bad = dict(t, msg_of=t["msg_of"].copy())
    bad["msg_of"][0] = 1 << 40
    g, _ = control_both(engine, d, bad, tag="msg_of past the table")
    assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)
    bad["msg_of"][6] = -2
    g, _ = control_both(engine, d, bad, tag="two connections")
    assert int(g["summary"]["errors"]) == 2
    bad = dict(t, conn_msg=t["conn_msg"].copy())
    bad["conn_msg"]["error_frame"][1] = 1 << 40
    g, _ = control_both(engine, d, bad, tag="error_frame past the batch")
    assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)
    bad["conn_msg"]["error_frame"][1] = 3   # connection 0's frame
    control_both(engine, d, bad, tag="error_frame of another connection")
    # the plan: exactly enough entries, one short, the gates, a reply outside its list
    g, w = plan_both(engine, d, t, ctl, ext, tag="plan")
    n_send = int(g["summary"]["frames"])
    assert n_send == 9 and [(int(e["frame"]), int(e["wire"])) for e in w["send"]] == [
        (0, 0), (1, 2), (2, 2), (4, 0), (5, 2), (7, 2), (8, 1), (9, 0), (10, 2)]   # frame 3's message is behind the close
    assert [(int(r["first"]), int(r["count"])) for r in w["conn_send"]] == [(0, 3), (3, 2), (5, 2), (7, 2)]
    plan_both(engine, d, t, ctl, ext, max_sends=n_send, tag="exactly enough entries")
    g, w = plan_both(engine, d, t, ctl, ext, max_sends=n_send - 1, tag="one entry short")
    assert jm.summary_tuple(g["summary"])[::4] == (n_send, gev_amd.ERR_CAPACITY)
    for k in ("decoded", "msg", "join", "ctl"):
        g, _ = plan_both(engine, d, t, ctl, ext, statuses={k: gev_amd.ERR_CAPACITY}, tag=f"failed {k} summary")
        assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 0, 0)
    for i in range(3):
        enc = [0, 0, 0]
        enc[i] = gev_amd.ERR_CAPACITY
        g, _ = plan_both(engine, d, t, ctl, ext, statuses=dict(enc=tuple(enc)), tag=f"failed encode {i}")
        assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 0, 0)
    rep = jm.reply_model(ctl["bodies"], jm.HANDLER_ECHO_BINARY, ext, None, 4)
    for m, r in ((0, 1 << 40), (int(np.flatnonzero(rep["reply_of"] >= 0)[-1]), 7)):
        ro = rep["reply_of"].copy()
        ro[m] = r
        g, _ = plan_both(engine, d, t, ctl, ext, reply_of=ro, tag=f"reply_of[{m}] = {r}")
        assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)
    bad_ctl = dict(ctl, ctl_of=ctl["ctl_of"].copy())
    bad_ctl["ctl_of"][1] = 5   # d_ctl has five entries
    g, _ = plan_both(engine, d, t, bad_ctl, ext, tag="ctl_of past the list")
    assert jm.summary_tuple(g["summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)


# ---------------------------------------------------------------------------- 4. end to end
def test_respond_end_to_end(engine):
    import torch
    rng = np.random.default_rng(0x65326533)
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

    kib = bytes(rng.integers(0, 256, 1024, dtype=np.uint8))
    words = (b"the quick brown fox jumps over the lazy dog; " * 40)
    tk_msgs = [words[:700], b"", words[100:1500]]
    close = wo.encode_frame((1000).to_bytes(2, "big") + b"bye", 8, True, 0, True, key())
    streams = [
        frames_of(kib, 2, (100, 101, 300, 555, 800, 1023)) + frames_of(b"short", 2, (), pings=False),
        frames_of(comp(words), 1, (3, 20), rsv=4),
        frames_of(comp(tk_msgs[0]), 1, (1,), rsv=4) + frames_of(comp(tk_msgs[1]), 1, (), rsv=4) + close
        + frames_of(comp(tk_msgs[2]), 1, (1,), rsv=4),
        frames_of(b"", 2, (), pings=False) + frames_of(bytes(range(256)) * 3, 2, (255, 256, 700)),
        frames_of(b"fine", 1, (2,)) + wo.encode_frame(b"rsv", 2, True, 4, True, key()) + frames_of(b"late", 1, ()),
        frames_of(comp(b"inflates " * 9), 1, (), rsv=4) + wo.encode_frame(b"\x07\x00", 1, True, 4, True, key())
        + wo.encode_frame(b"behind", 9, True, 0, True, key()) + frames_of(comp(b"good again"), 1, (), rsv=4),
    ]
    D, TK = gev_amd.EXT_DEFLATE, gev_amd.EXT_DEFLATE | gev_amd.EXT_SERVER_TAKEOVER
    ext_h = np.array([0, D, TK, D, 0, D], np.uint8)
    wb_h = np.array([0, 0, 12, 10, 0, 0], np.uint8)
    nc = len(streams)
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    conns = np.stack([offs, lens], 1)
    ext, wb = mm._dev(ext_h, dev, 1), mm._dev(wb_h, dev, 1)

    def chain(aux_slots):
        batch = gpu_decode(engine, b"".join(streams), conns, aux_slots=aux_slots)
        msgs = engine.messages(batch, conn_ext=ext)
        inf = engine.inflate(batch, msgs, 1 << 20)
        return batch, msgs, engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)

    batch, msgs, bodies = chain(nc - 1)
    with pytest.raises(ValueError):   # fewer aux slots than connections
        engine.respond(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, wb)
    batch, msgs, bodies = chain(nc)
    assert [int(x) for x in msgs.conn_msg_host()["error"]] == [0, 0, 0, 0, 1, 0]
    ctxs = torch.zeros((nc, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    res = engine.respond(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, wb, ctxs)
    cs = res.conn_send_host()
    S, F = gev_amd.CTL_SHUTDOWN, gev_amd.CTL_SHUTDOWN | gev_amd.CTL_FAILED
    assert [int(x) for x in cs["flags"]] == [0, 0, S, 0, F, F]
    assert [int(x) for x in res.conn_ctl["close_code"]] == [0, 0, 0, 0, 1002, 1007]
    assert int(res.summary_host()["errors"]) == 3 and int(cs["count"].sum()) == int(res.summary_host()["frames"])
    echoed = {}
    for c in range(nc):
        want = host_walk(streams[c], bool(ext_h[c]), 1 << 20)
        wire = res.conn_bytes(c)
        # (the reference reads no header from fewer than 6 buffered bytes, read.go:20-23: three bare close
        # frames behind the wire let it read a short last reply, and are dropped again)
        got = wo.decode_stream(wire + b"\x88\x00" * 3)
        frames = [f for f in got.frames if f.stream_pos < len(wire)]
        assert got.status == wo.OK and len(wire) == int(cs["bytes"][c]), c
        assert sum(f.header_len + f.header.length for f in frames) == len(wire), c
        assert len(frames) == len(want) == int(cs["count"][c]), (c, len(frames), len(want))
        z = zlib.decompressobj(-15)
        for f, (kind, x) in zip(frames, want):
            h = f.header
            assert h.fin and not h.masked, c
            if kind == "ctl":
                assert wire[f.stream_pos: f.stream_pos + f.header_len + h.length] == x, c
            elif kind == "fail":
                assert (h.opcode, h.rsv, f.payload) == (8, 0, x.to_bytes(2, "big")), c
            elif ext_h[c]:
                assert (h.opcode, h.rsv) == (1, 4), c
                zz = z if ext_h[c] & gev_amd.EXT_SERVER_TAKEOVER else zlib.decompressobj(-15)
                assert zz.decompress(f.payload + b"\x00\x00\xff\xff") == x, (c, len(x))
                echoed.setdefault(c, []).append(x)
            else:
                assert (h.opcode, h.rsv, f.payload) == (1, 0, x), c
    # the walk itself: pongs between the fragments, nothing behind the close or the failures
    assert [k for k, _ in host_walk(streams[0], False, 1 << 20)] == ["ctl"] * 6 + ["echo", "echo"]
    assert [k for k, _ in host_walk(streams[2], True, 1 << 20)] == ["ctl", "echo", "echo", "ctl"]
    assert [k for k, _ in host_walk(streams[4], False, 1 << 20)] == ["ctl", "echo", "fail"]
    assert [k for k, _ in host_walk(streams[5], True, 1 << 20)] == ["echo", "fail"]
    # the takeover connection's window saw only the messages before the cut
    host_ctx = bytearray(gev_amd.DEF_CTX_BYTES)
    assert echoed[2] == tk_msgs[:2]
    for x in tk_msgs[:2]:
        gev_amd.deflate_raw_ctx(x, host_ctx, window_bits=12)
    assert ctxs[2].cpu().numpy().tobytes() == bytes(host_ctx)
    assert not ctxs[[0, 1, 3, 4, 5]].any()
    # the stripped bodies, and Engine.echo_messages on the same (rewritten) bodies gives the same two wires
    st = bodies.bodies_host()["status"]
    assert [int(x) for x in st] == [0, 0, 0, 0, 0, gev_amd.MSG_ERR_CLOSED, 0, 0, 0, 0, gev_amd.MSG_ERR_DEFLATE,
                                    gev_amd.MSG_ERR_CLOSED]
    ctxs2 = torch.zeros((nc, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    echo = engine.echo_messages(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, wb, ctxs2)
    assert torch.equal(echo.def_wire, res.echo.def_wire) and torch.equal(echo.plain_wire, res.echo.plain_wire)
    assert torch.equal(ctxs, ctxs2)
