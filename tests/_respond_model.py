"""The control step's and the send plan's contracts (gevws_control_async,
gevws_send_plan_async; include/gevws.h) restated in plain Python over the tables
of tests/_messages_model.py and tests/_join_model.py, and the helpers that run
both device steps on hand-built tables.

The model is pinned on the CPU (tests/test_respond_model.py) against
oracle.ws_oracle.on_message / handle_close for every control reply and by
hand-derived cases; the GPU tests compare every output of the device with it,
byte for byte."""
from __future__ import annotations

import numpy as np

from tests import _join_model as jm
from tests import _messages_model as mm

NO_PING_FOR_PONG = 1
SHUTDOWN, FAILED = 1, 2
ERR_CLOSED = 9
ERR_DEFLATE, ERR_TOO_BIG = 7, 8
AUX_SLOT = 128
NO_FRAME = mm.NO_FRAME
ERR_CAPACITY, ERR_INVALID = -2, -3
FILL = jm.FILL
WIRE_PLAIN, WIRE_DEFLATED, WIRE_CONTROL = 0, 1, 2

CONN_CTL_DTYPE = np.dtype([("cut_frame", "<u8"), ("close_code", "<u4"), ("flags", "<u4"), ("reserved", "<u8", (2,))])
SEND_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8"), ("frame", "<u8"), ("conn", "<u4"), ("wire", "<u4")])
CONN_SEND_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("bytes", "<u8"), ("flags", "<u4"),
                            ("reserved", "<u4")])

# util.CheckCloseFrameData's texts (util/util.go:65-85)
_DEFINED = {1000, 1001, 1002, 1003, 1007, 1008, 1009, 1010, 1011, 1005, 1006, 1015}


def _utf8_ok(b: bytes) -> bool:
    return mm.text_message_verdict([b])[0]


def close_reply_body(payload: bytes) -> bytes:
    """util.HandleClose's reply body for a close frame with this payload (b"" : a bare header)."""
    if not payload:
        return b""
    code, reason = (int.from_bytes(payload[:2], "big"), payload[2:]) if len(payload) >= 2 else (0, b"")
    err = None
    if code <= 999:
        err = b"status code is not in use"
    elif code in (1005, 1006, 1015):
        err = b"status code is only application level"
    elif code == 1004:
        err = b"status code has no meaning yet"
    elif 1000 <= code <= 2999 and code not in _DEFINED:
        err = b"status code is not defined in spec"
    elif not _utf8_ok(reason):
        err = b"invalid utf8 sequence in close reason"
    if err is not None:
        code, reason = 1002, err
    return code.to_bytes(2, "big") + reason[:123]


def close_code_of(status: int) -> int:
    if status in (mm.ERR_UTF8, ERR_DEFLATE):
        return 1007
    return 1009 if status == ERR_TOO_BIG else 1002


def zero_summary():
    return dict(frames=0, payload_bytes=0, payload_len=0, errors=0, status=0)


def control_model(frames, conn_out, n_decoded, arena, msg_of, messages, conn_msg, bodies, flags=0, aux_off=0,
                  aux_cap=None, msg_status=0, join_status=0):
    """What gevws_control_async must produce: dict(ctl, ctl_conn, ctl_of,
    msg_end, conn_ctl, bodies, aux, replies, summary).  `aux` maps a slot to the
    bytes written there, `replies` lists (frame, conn, opcode, payload bytes) of
    every control reply; the tables are None where nothing may be written.
    aux_cap None: as many slots as needed."""
    n = n_decoded if msg_status == 0 and join_status == 0 else 0
    nm = messages.shape[0] if msg_status == 0 else 0
    if n == 0 or conn_out.shape[0] == 0:
        return dict(ctl=None, ctl_conn=None, ctl_of=None, msg_end=None, conn_ctl=None, bodies=None, aux={}, replies=[],
                    summary=zero_summary())
    n_conns = conn_out.shape[0]
    cls = {}                       # frame -> (kind, conn): 1 payload reply, 2 close with body, 3 bare close, 4 failure
    cuts = [(NO_FRAME, 0, 0)] * n_conns
    last_of = {}                   # message -> (its last data frame in the batch, the connection that saw it)
    bad = 0
    for c in range(n_conns):
        first, nfr, status = int(conn_out["first_frame"][c]), int(conn_out["nframes"][c]), int(conn_out["status"][c])
        end = min(first + nfr, n) if first < n else first
        err, errf = int(conn_msg["error"][c]), int(conn_msg["error_frame"][c])
        if status != 0 or end <= first or (err != 0 and errf == NO_FRAME):
            continue
        cut_b = NO_FRAME
        if 1 <= err <= 6:
            if not first <= errf < end:
                bad += 1
                continue
            cut_b = errf
        stop = cut_b + 1 if cut_b != NO_FRAME else end
        mo = [int(msg_of[f]) for f in range(first, stop)]
        if any(m < -1 or m >= nm for m in mo):
            bad += 1
            continue
        cut_a = cut_c = NO_FRAME
        fail_status = 0
        mine = {}
        order = []
        for f, m in zip(range(first, stop), mo):
            if m >= 0:
                if m not in mine:
                    order.append(m)
                mine[m] = f
            op, L = int(frames["opcode"][f]), int(frames["length"][f])
            if op == 8:
                cls[f] = (3 if L == 0 else 2, c)
                if cut_a == NO_FRAME:
                    cut_a = f
            elif op == 9 or (op == 10 and not flags & NO_PING_FOR_PONG):
                cls[f] = (1, c)
        for m in order:
            last_of[m] = (mine[m], c)
            if cut_c == NO_FRAME and int(bodies["status"][m]) != 0:
                cut_c, fail_status = mine[m], int(bodies["status"][m])
        cut = min(cut_a, cut_b, cut_c)
        if cut == NO_FRAME:
            continue
        fl, code = SHUTDOWN, 0
        if cut == cut_b:
            fl, code = SHUTDOWN | FAILED, close_code_of(err)
        elif cut == cut_c:
            fl, code = SHUTDOWN | FAILED, close_code_of(fail_status)
        if fl & FAILED:
            cls[cut] = (4, c)
        for f in range(cut + 1, stop):
            cls.pop(f, None)
        cuts[c] = (cut, code, fl)
    if bad:
        return dict(ctl=None, ctl_conn=None, ctl_of=None, msg_end=None, conn_ctl=None, bodies=None, aux={}, replies=[],
                    summary=dict(zero_summary(), errors=bad, status=ERR_INVALID))
    nrep = len(cls)
    nslots = sum(1 for k, _ in cls.values() if k in (2, 4))
    shut = sum(1 for _, _, fl in cuts if fl)
    summary = dict(frames=nrep, payload_bytes=nslots, payload_len=0, errors=shut, status=0)
    if aux_cap is not None and nslots > aux_cap // AUX_SLOT:
        summary["status"] = ERR_CAPACITY
        return dict(ctl=None, ctl_conn=None, ctl_of=None, msg_end=None, conn_ctl=None, bodies=None, aux={}, replies=[],
                    summary=summary)
    ctl = np.zeros(nrep, jm.OUT_FRAME_DTYPE)
    ctl_conn = np.zeros(nrep, np.uint32)
    ctl_of = np.full(n, -1, np.int64)
    aux, replies, slot = {}, [], 0
    for r, f in enumerate(sorted(cls)):
        kind, c = cls[f]
        ctl_of[f], ctl_conn[r] = r, c
        o = ctl[r]
        o["fin"] = 1
        off, L = int(frames["payload_off"][f]), int(frames["length"][f])
        payload = arena[off: off + L].tobytes()
        if kind == 1:
            o["opcode"] = 10 if int(frames["opcode"][f]) == 9 else 9
            o["length"], o["payload_off"], o["payload_len"] = L, off, L
            replies.append((f, c, int(o["opcode"]), payload))
            continue
        o["opcode"] = 8
        body = b""
        if kind == 2:
            body = close_reply_body(payload)
        elif kind == 4:
            body = cuts[c][1].to_bytes(2, "big")
        if kind != 3:
            aux[slot] = body
            o["length"], o["payload_off"], o["payload_len"] = len(body), aux_off + slot * AUX_SLOT, len(body)
            slot += 1
        replies.append((f, c, 8, body))
    msg_end = np.full(nm, NO_FRAME, np.uint64)
    out_bodies = bodies[:nm].copy()
    for m, (f, c) in last_of.items():
        if int(messages["flags"][m]) & mm.END:
            msg_end[m] = f
        cut = cuts[c][0]
        if cut != NO_FRAME and f > cut:
            b = out_bodies[m]
            b["off"], b["length"], b["flags"], b["status"] = 0, 0, 0, ERR_CLOSED
    conn_ctl = np.zeros(n_conns, CONN_CTL_DTYPE)
    for c, (cut, code, fl) in enumerate(cuts):
        conn_ctl[c]["cut_frame"], conn_ctl[c]["close_code"], conn_ctl[c]["flags"] = cut, code, fl
    return dict(ctl=ctl, ctl_conn=ctl_conn, ctl_of=ctl_of, msg_end=msg_end, conn_ctl=conn_ctl, bodies=out_bodies, aux=aux,
                replies=replies, summary=summary)


def plan_model(n_decoded, conn_out, msg_of, msg_end, reply_of, n_messages, conn_ext, ctl_of, conn_ctl, wires,
               max_sends=None, gate_ok=True):
    """What gevws_send_plan_async must produce: dict(send, conn_send, summary).
    wires: three (offset table, count, wire total), plain / deflated / control;
    gate_ok False: one of the input summaries failed.  max_sends None: enough."""
    n_conns = conn_out.shape[0]
    if not gate_ok or n_decoded == 0 or n_conns == 0:
        return dict(send=None, conn_send=None, summary=zero_summary())
    n = n_decoded
    fconn = np.full(n, -1, np.int64)
    for c in range(n_conns):
        lo = min(int(conn_out["first_frame"][c]), n)
        hi = min(lo + int(conn_out["nframes"][c]), n)
        fconn[lo:hi] = c
    entries, bad = [], 0
    pre_n, pre_b = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    nbytes = 0
    for f in range(n):
        pre_n[f], pre_b[f] = len(entries), nbytes
        c = int(fconn[f])
        k = int(ctl_of[f])
        if k >= 0:
            wire, idx = WIRE_CONTROL, k
        else:
            m = int(msg_of[f])
            if m < 0:
                continue
            if m >= n_messages:
                bad += 1
                continue
            if int(msg_end[m]) != f or int(reply_of[m]) < 0:
                continue
            if c < 0:
                bad += 1
                continue
            wire = WIRE_DEFLATED if conn_ext is not None and int(conn_ext[c]) & 1 else WIRE_PLAIN
            idx = int(reply_of[m])
        tab, cnt, total = wires[wire]
        if c < 0 or idx >= cnt:
            bad += 1
            continue
        off = int(tab[idx])
        nxt = int(tab[idx + 1]) if idx + 1 < cnt else total
        if nxt < off:
            bad += 1
            continue
        entries.append((off, nxt - off, f, c, wire))
        nbytes += nxt - off
    pre_n[n], pre_b[n] = len(entries), nbytes
    if bad:
        return dict(send=None, conn_send=None, summary=dict(zero_summary(), errors=bad, status=ERR_INVALID))
    shut = int(np.count_nonzero(conn_ctl["flags"][:n_conns] & SHUTDOWN))
    summary = dict(frames=len(entries), payload_bytes=nbytes, payload_len=0, errors=shut, status=0)
    if max_sends is not None and len(entries) > max_sends:
        summary["status"] = ERR_CAPACITY
        return dict(send=None, conn_send=None, summary=summary)
    send = np.zeros(len(entries), SEND_DTYPE)
    for k, e in enumerate(entries):
        send[k] = e
    conn_send = np.zeros(n_conns, CONN_SEND_DTYPE)
    for c in range(n_conns):
        lo = min(int(conn_out["first_frame"][c]), n)
        hi = min(lo + int(conn_out["nframes"][c]), n)
        conn_send[c] = (pre_n[lo], pre_n[hi] - pre_n[lo], pre_b[hi] - pre_b[lo], conn_ctl["flags"][c], 0)
    return dict(send=send, conn_send=conn_send, summary=summary)


def conn_replies(ctlm: dict, c: int):
    """The model's control replies of connection c as (frame, opcode, payload)."""
    return [(f, op, p) for f, cc, op, p in ctlm["replies"] if cc == c]


# ---------------------------------------------------------------------------- hand-built chains
def tables_of(d: mm.Decoded, state=None, inflated_status=None, flags=jm.JOIN_ALL):
    """The message pass's and the join's model tables of a hand-built batch:
    dict(messages, msg_of, conn_msg, bodies).  inflated_status: {message: status}
    stands for an inflate step that failed those messages (their bodies become
    undelivered with that status)."""
    t = d.model(state)
    j = jm.join_model(d.frames, d.arena, t["messages"], t["msg_of"], flags)
    bodies = j["bodies"].copy()
    for m, st in (inflated_status or {}).items():
        bodies[m]["off"], bodies[m]["length"], bodies[m]["flags"], bodies[m]["status"] = 0, 0, 0, st
    return dict(messages=t["messages"], msg_of=t["msg_of"], conn_msg=t["conn_msg"], bodies=bodies)


def summary_np(**fields):
    s = np.zeros(1, mm.SUMMARY_DTYPE)
    for k, v in fields.items():
        s[k] = v
    return s


def run_control(engine, d: mm.Decoded, t: dict, flags=0, aux_slots=None, msg_status=0, join_status=0,
                decoded_status=0):
    """gevws_control_async on hand-built tables: host copies of everything it
    may write, each prefilled with FILL (the payload arena's aux region too)."""
    import torch
    dev = torch.device("cuda", engine.device)
    nf, nc, nm = d.frames.shape[0], d.conn_out.shape[0], t["messages"].shape[0]
    pay_bytes = (d.arena.size + 15) // 16 * 16
    need = aux_slots if aux_slots is not None else nc
    aux_off, aux_cap = pay_bytes, need * AUX_SLOT
    pay = torch.full((pay_bytes + aux_cap + AUX_SLOT + 16,), FILL, dtype=torch.uint8, device=dev)
    if d.arena.size:
        pay[: d.arena.size] = torch.from_numpy(d.arena.copy()).to(dev)
    dsum = d.summary.copy()
    dsum["status"] = decoded_status
    fr, co, sm = mm._dev(d.frames, dev, 32), mm._dev(d.conn_out, dev, 32), mm._dev(dsum, dev, 64)
    mo, ms, cm = mm._dev(t["msg_of"], dev, 8), mm._dev(t["messages"], dev, 32), mm._dev(t["conn_msg"], dev, 32)
    bodies = mm._dev(t["bodies"], dev, 32)
    msum = mm._dev(summary_np(frames=nm, status=msg_status), dev, 64)
    jsum = mm._dev(summary_np(frames=nm, status=join_status), dev, 64)
    f = lambda nbytes: torch.full((max(nbytes, 8),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    ctl, cc, cof, mend, cctl, summ = f(nf * 32), f(nf * 4), f(nf * 8), f(nm * 8), f(nc * 32), f(64)
    engine.control_async(fr, nf, co, nc, sm, pay, aux_off, aux_cap, mo, ms, nm, cm, msum, bodies, jsum, flags, ctl, cc,
                         cof, mend, cctl, summ)
    torch.cuda.synchronize(engine.device)
    h = lambda x: x.cpu().numpy()  # noqa: E731
    return dict(ctl=h(ctl), ctl_conn=h(cc), ctl_of=h(cof), msg_end=h(mend), conn_ctl=h(cctl),
                summary=h(summ).view(mm.SUMMARY_DTYPE)[0], bodies=h(bodies)[: nm * 32], payload=h(pay),
                aux_off=aux_off, aux_cap=aux_cap,
                dev=dict(frames=fr, conn_out=co, decoded=sm, payload=pay, msg_of=mo, messages=ms, conn_msg=cm,
                         bodies=bodies, msg_summary=msum, join_summary=jsum, ctl=ctl, ctl_conn=cc, ctl_of=cof,
                         msg_end=mend, conn_ctl=cctl, summary=summ, n_frames=nf, n_conns=nc, n_messages=nm))


def _same(got: np.ndarray, want, tag):
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got[: w.size].tobytes() == w.tobytes(), (tag, "differs from the model")
    assert np.all(got[w.size:] == FILL), (tag, "written past the table")


def assert_control(got: dict, want: dict, d: mm.Decoded, t: dict, tag="") -> None:
    """Every output of the device == the model's, untouched bytes included."""
    s = got["summary"]
    assert jm.summary_tuple(s) == tuple(want["summary"][k] for k in ("frames", "payload_bytes", "payload_len", "errors",
                                                                     "status")), (tag, jm.summary_tuple(s), want["summary"])
    assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), tag
    pay = got["payload"]
    image = np.full(pay.size, FILL, np.uint8)
    image[: d.arena.size] = d.arena
    for slot, body in want["aux"].items():
        o = got["aux_off"] + slot * AUX_SLOT
        image[o: o + len(body)] = np.frombuffer(body, np.uint8)
    bad = np.flatnonzero(pay != image)
    assert bad.size == 0, (tag, "payload arena / aux region differs at", bad[:8])
    if want["ctl"] is None:
        for k in ("ctl", "ctl_conn", "ctl_of", "msg_end", "conn_ctl"):
            assert np.all(got[k] == FILL), (tag, k, "written by a call that wrote nothing")
        assert got["bodies"].tobytes() == np.ascontiguousarray(t["bodies"]).tobytes(), (tag, "d_bodies changed")
        return
    for k in ("ctl", "ctl_conn", "ctl_of", "msg_end", "conn_ctl"):
        _same(got[k], want[k], (tag, k))
    assert got["bodies"].tobytes() == want["bodies"].tobytes(), (tag, "d_bodies differs",
                                                                 got["bodies"].view(jm.BODY_DTYPE), want["bodies"])


def run_plan(engine, n_frames, decoded, conn_out, msg_of, msg_end, reply_of, n_messages, msg_summary, join_summary,
             conn_ext, ctl_of, conn_ctl, ctl_summary, wires, max_sends):
    """gevws_send_plan_async on host tables (numpy; the summaries SUMMARY_DTYPE
    records, wires three (offset table, encode summary)): host copies of what it
    may write, prefilled with FILL."""
    import torch
    dev = torch.device("cuda", engine.device)
    nc = conn_out.shape[0]
    D = lambda a, mn=8: mm._dev(a, dev, mn)  # noqa: E731
    f = lambda nbytes: torch.full((max(nbytes, 8),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    send, cs, summ = f(max_sends * 32), f(nc * 32), f(64)
    ext = None if conn_ext is None else D(np.asarray(conn_ext, np.uint8), 1)
    w = [(D(np.asarray(tab, np.uint64)), D(s, 64)) for tab, s in wires]
    engine.send_plan_async(n_frames, D(decoded, 64), D(conn_out, 32), nc, D(np.asarray(msg_of, np.int64)),
                           D(np.asarray(msg_end, np.uint64)), D(np.asarray(reply_of, np.int64)), n_messages,
                           D(msg_summary, 64), D(join_summary, 64), ext, D(np.asarray(ctl_of, np.int64)),
                           D(conn_ctl, 32), D(ctl_summary, 64), w[0][0], w[0][1], w[1][0], w[1][1], w[2][0], w[2][1],
                           send, max_sends, cs, summ)
    torch.cuda.synchronize(engine.device)
    return dict(send=send.cpu().numpy(), conn_send=cs.cpu().numpy(),
                summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0])


def assert_plan(got: dict, want: dict, tag="") -> None:
    s = got["summary"]
    assert jm.summary_tuple(s) == tuple(want["summary"][k] for k in ("frames", "payload_bytes", "payload_len", "errors",
                                                                     "status")), (tag, jm.summary_tuple(s), want["summary"])
    assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), tag
    if want["send"] is None:
        assert np.all(got["send"] == FILL) and np.all(got["conn_send"] == FILL), (tag, "written by a call that failed")
        return
    _same(got["send"], want["send"], (tag, "send"))
    _same(got["conn_send"], want["conn_send"], (tag, "conn_send"))
