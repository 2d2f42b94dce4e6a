"""The join step's and the reply step's contracts (gevws_join_async,
gevws_reply_bodies_async; include/gevws.h) restated in plain Python over the
tables of tests/_messages_model.py, and the helpers that run both device steps
behind a message pass on a hand-built decoded batch.

The model is pinned on the CPU by hand-derived cases (tests/test_join_model.py);
the GPU tests compare the device's records, the whole of d_out and the
summaries with it, byte for byte."""
from __future__ import annotations

import numpy as np

from tests import _messages_model as mm

JOIN_ALL = 1
WHOLE, JOINED, INFLATED = 1, 2, 4
COMPRESSED = 4
INF_DONE = 1
EXT_DEFLATE = 1
HANDLER_NONE, HANDLER_ECHO_BINARY, HANDLER_ECHO_TEXT = 0, 1, 2
ERR_CAPACITY, ERR_INVALID = -2, -3
FILL = 0xEE

BODY_DTYPE = np.dtype([("off", "<u8"), ("length", "<u8"), ("conn", "<u4"), ("opcode", "u1"), ("flags", "u1"),
                       ("status", "u1"), ("reserved", "u1", (9,))])
DEFLATE_MSG_DTYPE = np.dtype([("payload_off", "<u8"), ("length", "<u8"), ("opcode", "u1"), ("window_bits", "u1"),
                              ("reserved", "u1", (6,))])
OUT_FRAME_DTYPE = np.dtype([("fin", "u1"), ("rsv", "u1"), ("opcode", "u1"), ("masked", "u1"), ("mask", "u1", (4,)),
                            ("length", "<i8"), ("payload_off", "<u8"), ("payload_len", "<u8")])


def round16(x: int) -> int:
    return (x + 15) // 16 * 16


def zero_summary():
    return dict(frames=0, payload_bytes=0, payload_len=0, errors=0, status=0)


def join_model(frames, arena, messages, msg_of, flags=0, out_cap=None, inflated=None, inflate_summary=None,
               msg_status=0, out_image=None):
    """What gevws_join_async must produce: dict(bodies, out, summary, base,
    written).  messages / msg_of: the message pass's tables (its summary's
    status in msg_status); inflated / inflate_summary: the inflate step's
    records and its summary as a dict(payload_bytes, status), or None.  `out` is
    the whole of d_out (out_cap bytes) starting from out_image, or from FILL;
    `written` marks the bytes the call must have written.  out_cap None: exactly
    the need."""
    n = messages.shape[0] if msg_status == 0 else 0
    if inflate_summary is not None and inflate_summary["status"] != 0:
        n = 0
    bodies = np.zeros(n, BODY_DTYPE)
    base = round16(int(inflate_summary["payload_bytes"])) if n and inflate_summary is not None else 0
    cur, delivered, total = base, 0, 0
    copies = []
    by_msg = {}
    for f in np.flatnonzero(msg_of >= 0):
        by_msg.setdefault(int(msg_of[f]), []).append(int(f))
    for m in range(n):
        r = messages[m]
        b = bodies[m]
        b["conn"], b["opcode"], b["status"] = r["conn"], r["opcode"], r["status"]
        mflags = int(r["flags"])
        whole = mflags & mm.BEGIN and mflags & mm.END and int(r["status"]) == mm.OK
        if mflags & COMPRESSED:
            if inflated is None:
                continue
            b["status"] = inflated["status"][m]
            if whole and int(inflated["flags"][m]) & INF_DONE and int(inflated["status"][m]) == mm.OK:
                b["flags"], b["off"], b["length"] = WHOLE | INFLATED, inflated["out_off"][m], inflated["length"][m]
                delivered, total = delivered + 1, total + int(inflated["length"][m])
            continue
        if not whole:
            continue
        delivered, total = delivered + 1, total + int(r["length"])
        b["length"] = r["length"]
        if int(r["nframes"]) >= 2 or flags & JOIN_ALL:
            fs = by_msg.get(m, [])  # (its data frames in order; all of them lie from first_frame on)
            assert not fs or fs[0] == int(r["first_frame"])
            data = b"".join(arena[int(frames["payload_off"][f]):][: int(frames["length"][f])].tobytes() for f in fs)
            assert len(data) == int(r["length"]) and len(fs) == int(r["nframes"])
            b["flags"], b["off"] = WHOLE | JOINED, cur
            copies.append((cur, data))
            cur += round16(len(data))
        else:
            b["flags"], b["off"] = WHOLE, frames["payload_off"][int(r["first_frame"])]
    if n == 0:
        summary = zero_summary()
    else:
        summary = dict(frames=delivered, payload_bytes=cur, payload_len=total, errors=0, status=0)
    if out_cap is None:
        out_cap = cur
    out = np.full(out_cap, FILL, np.uint8) if out_image is None else out_image[:out_cap].copy()
    written = np.zeros(out_cap, bool)
    if cur > out_cap:
        summary = dict(frames=summary["frames"], payload_bytes=cur, payload_len=summary["payload_len"], errors=0,
                       status=ERR_CAPACITY)
        return dict(bodies=None, out=out, summary=summary, base=base, written=written)
    for off, data in copies:
        pad = round16(len(data))
        out[off: off + len(data)] = np.frombuffer(data, np.uint8)
        out[off + len(data): off + pad] = 0
        written[off: off + pad] = True
    return dict(bodies=bodies, out=out, summary=summary, base=base, written=written)


def reply_model(bodies, policy, conn_ext, window_bits, n_conns, msg_status=0, join_status=0):
    """What gevws_reply_bodies_async must produce: dict(def_msgs, def_conn,
    plain, plain_conn, reply_of, def_summary, plain_summary); the lists are None
    where nothing may be written."""
    n = bodies.shape[0] if msg_status == 0 and join_status == 0 else 0
    dmsgs, dconn, plain, pconn = [], [], [], []
    reply_of = np.full(n, -1, np.int64)
    bad = 0
    op = 1 if policy == HANDLER_ECHO_TEXT else 2
    for m in range(n if policy != HANDLER_NONE else 0):
        b = bodies[m]
        fl, c = int(b["flags"]), int(b["conn"])
        if not fl & WHOLE:
            continue
        if not fl & (JOINED | INFLATED) or c >= n_conns:
            bad += 1
            continue
        if conn_ext is not None and int(conn_ext[c]) & EXT_DEFLATE:
            reply_of[m] = len(dmsgs)
            dmsgs.append((int(b["off"]), int(b["length"]), op, int(window_bits[c]) if window_bits is not None else 0))
            dconn.append(c)
        else:
            reply_of[m] = len(plain)
            plain.append((int(b["off"]), int(b["length"])))
            pconn.append(c)
    if bad:
        s = dict(zero_summary(), errors=bad, status=ERR_INVALID)
        return dict(def_msgs=None, def_conn=None, plain=None, plain_conn=None, reply_of=None, def_summary=s,
                    plain_summary=dict(s))
    dm = np.zeros(len(dmsgs), DEFLATE_MSG_DTYPE)
    for k, (off, length, o, wb) in enumerate(dmsgs):
        dm[k]["payload_off"], dm[k]["length"], dm[k]["opcode"], dm[k]["window_bits"] = off, length, o, wb
    pl = np.zeros(len(plain), OUT_FRAME_DTYPE)
    for k, (off, length) in enumerate(plain):
        pl[k]["fin"], pl[k]["opcode"], pl[k]["length"] = 1, op, length
        pl[k]["payload_off"], pl[k]["payload_len"] = off, length
    return dict(def_msgs=dm, def_conn=np.array(dconn, np.uint32), plain=pl, plain_conn=np.array(pconn, np.uint32),
                reply_of=reply_of, def_summary=dict(zero_summary(), frames=len(dmsgs)),
                plain_summary=dict(zero_summary(), frames=len(plain)))


def decoded_join_model(d: mm.Decoded, flags=0, out_cap=None, state=None):
    """join_model behind the plain message pass's model of a hand-built batch."""
    t = d.model(state)
    return join_model(d.frames, d.arena, t["messages"], t["msg_of"], flags, out_cap)


# ---------------------------------------------------------------------------- device runs
GUARD = 64  # bytes behind out_cap that no call may touch


def summary_tuple(s):
    return tuple(int(s[k]) for k in ("frames", "payload_bytes", "payload_len", "errors", "status"))


def run_join(engine, dev_tables: dict, flags: int, out_cap: int, inflated=None, inflate_summary=None, out=None):
    """gevws_join_async behind a message pass's device tensors (the "dev" entry
    of tests/_inflate_gpu_model.run_messages_ext): host copies of d_bodies, the
    whole of d_out (prefilled FILL unless `out`, the inflate's buffer, is given;
    GUARD bytes behind out_cap) and the summary, plus the device tensors."""
    import torch
    t = dev_tables
    dev = t["frames"].device
    nm = t["n_messages"]
    bodies = torch.full((max(nm, 1) * 32,), FILL, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.full((out_cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    engine.join_async(t["frames"], t["n_frames"], t["messages"], nm, t["msg_of"], t["summary"], t["payload"],
                      inflated, inflate_summary, flags, bodies, out, out_cap, summ)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0], bodies_raw=bodies.cpu().numpy(),
                bodies=bodies[: nm * 32].cpu().numpy().view(BODY_DTYPE), out=out.cpu().numpy(),
                dev=dict(bodies=bodies, out=out, summary=summ, n_messages=nm))


def assert_join(got: dict, want: dict, out_cap: int, tag="") -> None:
    """The device's records, the whole of d_out and the summary == the model's."""
    s = got["summary"]
    assert summary_tuple(s) == tuple(want["summary"][k] for k in ("frames", "payload_bytes", "payload_len", "errors",
                                                                  "status")), (tag, summary_tuple(s), want["summary"])
    assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), tag
    out = got["out"]
    assert np.all(out[out_cap:] == FILL), (tag, "written past out_cap")
    bad = np.flatnonzero(out[:out_cap] != want["out"])
    assert bad.size == 0, (tag, "d_out differs at", bad[:8], out[bad[:8]], want["out"][bad[:8]])
    if want["bodies"] is None:
        assert np.all(got["bodies_raw"] == FILL), (tag, "d_bodies written by a call that did not fit")
        return
    gb, wb = got["bodies"], want["bodies"]
    assert gb.shape == wb.shape, tag
    for k in BODY_DTYPE.names if gb.shape[0] else ():
        bad =np.flatnonzero((gb[k] != wb[k]).reshape(gb.shape[0], -1).any(axis=1))
        assert bad.size == 0, (tag, k, bad[:8], gb[k][bad[:8]], wb[k][bad[:8]])
    assert np.all(got["bodies_raw"][gb.shape[0] * 32:] == FILL), tag


def run_reply(engine, bodies_np, n_messages, msg_summary_dev, join_summary_dev, policy, conn_ext, window_bits,
              n_conns):
    """gevws_reply_bodies_async on host records (BODY_DTYPE): host copies of
    everything it may write, each prefilled with FILL."""
    import torch
    dev = msg_summary_dev.device
    cap = max(n_messages, 1)
    bodies = mm._dev(bodies_np, dev, 32)
    ext = None if conn_ext is None else mm._dev(np.asarray(conn_ext, np.uint8), dev, 1)
    wb = None if window_bits is None else mm._dev(np.asarray(window_bits, np.uint8), dev, 1)
    f = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    dm, dc, ds, pl, pc, ps, ro = f(cap * 24), f(cap * 4), f(64), f(cap * 32), f(cap * 4), f(64), f(cap * 8)
    engine.reply_bodies_async(bodies, n_messages, msg_summary_dev, join_summary_dev, policy, ext, wb, n_conns, dm, dc,
                              ds, pl, pc, ps, ro)
    torch.cuda.synchronize(engine.device)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(def_msgs=h(dm), def_conn=h(dc), def_summary=h(ds).view(mm.SUMMARY_DTYPE)[0], plain=h(pl),
                plain_conn=h(pc), plain_summary=h(ps).view(mm.SUMMARY_DTYPE)[0], reply_of=h(ro),
                dev=dict(def_msgs=dm, def_conn=dc, def_summary=ds, plain=pl, plain_conn=pc, plain_summary=ps))


def assert_reply(got: dict, want: dict, tag="") -> None:
    for k in ("def_summary", "plain_summary"):
        s = got[k]
        assert summary_tuple(s) == tuple(want[k][x] for x in ("frames", "payload_bytes", "payload_len", "errors",
                                                              "status")), (tag, k, summary_tuple(s), want[k])
        assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), (tag, k)
    if want["def_msgs"] is None:
        for k in ("def_msgs", "def_conn", "plain", "plain_conn", "reply_of"):
            assert np.all(got[k] == FILL), (tag, k, "written by a call that failed")
        return
    for k, dt in (("def_msgs", DEFLATE_MSG_DTYPE), ("def_conn", np.dtype("<u4")), ("plain", OUT_FRAME_DTYPE),
                  ("plain_conn", np.dtype("<u4")), ("reply_of", np.dtype("<i8"))):
        w = np.ascontiguousarray(want[k]).view(np.uint8).reshape(-1)
        assert got[k][: w.size].tobytes() == w.tobytes(), (tag, k, got[k][: w.size].view(dt), want[k])
        assert np.all(got[k][w.size:] == FILL), (tag, k, "written past the list")
