#!/usr/bin/env python3
"""Measure the room broadcast on a fan-out shape: a device-resident pass of
4 096 connections in rooms of 64, each sending one 1 KiB text message.  Every
message is framed once and named 64 times: 262 144 plan entries, about 270 MB
gathered from a 4 MB wire.

One checked pass through Engine.broadcast(gather=True) comes first: sampled
connections' spans are compared with the frames their room's members must be
sent.  Then the room reply step, the room plan and the gather over that plan are
each timed by HIP events around `reps` calls, and the gather is timed beside
itself over an echo plan of the same entry count and bytes (every entry its own
slice of a 270 MB wire: what a pure echo of as many bytes reads), alternating in
one process and clock state.  Medians of `rounds`; one JSON line.

    python tools/bench_rooms.py [--rounds 7] [--warmup 2] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CONNS, ROOM, MSG = 4096, 64, 1024
REPLY_LAUNCHES, PLAN_LAUNCHES, GATHER_LAUNCHES = 5, 12, 7


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import gev_amd
    from oracle import ws_oracle as wo
    eng = gev_amd.Engine(0)
    dev = torch.device("cuda", 0)
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    host = lambda t: t.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    # ---- the pass: one masked 1 KiB text frame a connection
    rng = np.random.default_rng(0x726F6F6D)
    texts = rng.integers(0x20, 0x7F, (N_CONNS, MSG), dtype=np.uint8)
    keys = rng.integers(0, 256, (N_CONNS, 4), dtype=np.uint8)
    hdr = np.frombuffer(wo.write_header(True, 0, 1, MSG, True, b"\0\0\0\0", None), np.uint8).copy()
    hl = hdr.size
    wire_in = np.zeros((N_CONNS, hl + MSG), np.uint8)
    wire_in[:, :hl] = hdr
    wire_in[:, hl - 4: hl] = keys
    wire_in[:, hl:] = texts ^ np.tile(keys, (1, MSG // 4))
    arena = z(wire_in.size + gev_amd.IN_PAD)
    arena[: wire_in.size] = torch.from_numpy(wire_in.reshape(-1)).to(dev)
    conns = np.stack([np.arange(N_CONNS) * (hl + MSG), np.full(N_CONNS, hl + MSG)], 1).astype(np.int64)
    pay_cap = N_CONNS * MSG + 64
    out = eng.alloc_batch(N_CONNS, N_CONNS, pay_cap, aux_slots=N_CONNS)
    eng.decode_async(arena, wire_in.size, torch.from_numpy(conns).to(dev), N_CONNS, out, N_CONNS, pay_cap)
    torch.cuda.synchronize()
    assert int(out.summary_host()["status"]) == 0 and int(out.summary_host()["frames"]) == N_CONNS
    msgs = eng.messages(out)
    bodies = eng.join(out, msgs, flags=gev_amd.JOIN_ALL)
    rooms = gev_amd.Rooms.from_conn_room(np.arange(N_CONNS, dtype=np.uint32) // ROOM, dev)
    nf, nm = msgs.n_frames, bodies.n_messages
    assert nf == nm == N_CONNS and rooms.n_rooms == N_CONNS // ROOM

    # ---- the checked pass
    res = eng.broadcast(out, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, None, rooms, gather=True)
    n_entries, plan_bytes = int(res.summary_host()["frames"]), int(res.summary_host()["payload_bytes"])
    frame = lambda c: wo.write_header(True, 0, 1, MSG, False, b"\0\0\0\0", None) + texts[c].tobytes()  # noqa: E731
    assert n_entries == N_CONNS * ROOM and plan_bytes == n_entries * len(frame(0))
    sends = res.host_sends()
    for c in (0, 63, 64, 2049, N_CONNS - 1):
        g = c // ROOM
        assert bytes(sends[c]) == b"".join(frame(s) for s in range(g * ROOM, (g + 1) * ROOM)), c
    want_buf, want_conn_buf = res.send_buf, res.conn_buf
    nbytes = int(want_buf.numel())
    wires = (res.echo.plain_wire, None, None)
    wb = [int(res.echo.plain_wire.numel()), 0, 0]

    # ---- the steps on buffers of their own
    ctl, ctl_conn, ctl_sum = z(nf, 32), z(nf, dt=torch.int32), z(64)
    ctl_of, msg_end, conn_ctl = z(nf, dt=torch.int64), z(nm, dt=torch.int64), z(N_CONNS, 32)
    aux_cap = gev_amd._abi.AUX_SLOT * out.aux_slots
    aux_off = (out.payload.numel() - 16 - aux_cap) // 16 * 16
    eng.control_async(out.frames, nf, out.conn_out, N_CONNS, out.summary, out.payload, aux_off, aux_cap, msgs.msg_of,
                      msgs.messages, nm, msgs.conn_msg, msgs.summary, bodies.bodies, bodies.summary, 0, ctl, ctl_conn,
                      ctl_of, msg_end, conn_ctl, ctl_sum)
    def_msgs, def_conn, def_sum = z(nm, 24), z(nm, dt=torch.int32), z(64)
    plain, plain_conn, plain_sum = z(nm, 32), z(nm, dt=torch.int32), z(64)
    plain_of, def_of = z(nm, dt=torch.int64), z(nm, dt=torch.int64)

    def reply():
        eng.reply_rooms_async(bodies.bodies, nm, msgs.summary, bodies.summary, gev_amd.HANDLER_ECHO_TEXT, None, None,
                              N_CONNS, rooms, 0, def_msgs, def_conn, def_sum, plain, plain_conn, plain_sum, plain_of,
                              def_of)

    reply()
    wcap = int(res.echo.plain_wire.numel()) + 16
    plain_wire, plain_off, plain_enc = z(wcap + gev_amd._abi.OUT_PAD), z(nm, dt=torch.int64), z(64)
    eng.encode_replies_async(plain, nm, plain_sum, bodies.out, plain_wire, wcap, plain_off, plain_enc)
    none_off, def_enc, ctl_enc = z(1, dt=torch.int64), z(64), z(64)   # the other two wires are empty
    send, conn_send, plan_sum = z(n_entries, 32), z(N_CONNS, 32), z(64)

    def plan():
        eng.room_plan_async(nf, out.summary, out.conn_out, N_CONNS, msgs.msg_of, msg_end, plain_of, def_of, nm,
                            msgs.summary, bodies.summary, None, ctl_of, conn_ctl, ctl_sum, plain_off, plain_enc,
                            none_off, def_enc, none_off, ctl_enc, rooms, 0, send, n_entries, conn_send, plan_sum)

    buf, conn_buf, gsum = z(nbytes), z(N_CONNS, 32), z(64)
    room_wires = (plain_wire[: wb[0]], None, None)

    def gather():
        eng.send_gather_async(send, n_entries, conn_send, N_CONNS, plan_sum, room_wires, wb, buf, nbytes, conn_buf,
                              gsum)

    # ---- an echo plan of as many entries and bytes: every entry its own slice of one wire
    flen = plan_bytes // n_entries
    e_send = torch.zeros((n_entries, 4), dtype=torch.int64, device=dev)
    k = torch.arange(n_entries, dtype=torch.int64, device=dev)
    e_send[:, 0], e_send[:, 1], e_send[:, 2] = k * flen, flen, k
    e_send[:, 3] = k // ROOM   # conn in the low word, wire 0 in the high
    e_cs = torch.zeros((N_CONNS, 4), dtype=torch.int64, device=dev)
    c = torch.arange(N_CONNS, dtype=torch.int64, device=dev)
    e_cs[:, 0], e_cs[:, 1], e_cs[:, 2] = c * ROOM, ROOM, ROOM * flen
    e_plan = np.zeros(1, gev_amd.SUMMARY_DTYPE)
    e_plan["frames"], e_plan["payload_bytes"] = n_entries, plan_bytes
    e_plan = torch.from_numpy(e_plan.view(np.uint8).copy()).to(dev)
    e_wire = torch.randint(0, 256, (plan_bytes + 32,), dtype=torch.uint8, device=dev)
    e_buf, e_conn_buf, e_gsum = z(nbytes), z(N_CONNS, 32), z(64)
    e_wb = [plan_bytes, 0, 0]

    def gather_echo():
        eng.send_gather_async(e_send.view(torch.uint8), n_entries, e_cs.view(torch.uint8), N_CONNS, e_plan,
                              (e_wire[:plan_bytes], None, None), e_wb, e_buf, nbytes, e_conn_buf, e_gsum)

    for _ in range(args.warmup):
        reply(), plan(), gather(), gather_echo()
    torch.cuda.synchronize()
    ps, gs, es = host(plan_sum), host(gsum), host(e_gsum)
    assert int(host(plain_sum)["frames"]) == nm and int(host(def_sum)["frames"]) == 0
    assert int(ps["status"]) == 0 and int(ps["frames"]) == n_entries and int(ps["payload_bytes"]) == plan_bytes
    assert torch.equal(send, res.send[:n_entries]) and torch.equal(conn_send, res.conn_send)
    assert int(gs["status"]) == 0 and int(gs["payload_bytes"]) == nbytes and torch.equal(buf, want_buf)
    assert conn_buf.cpu().numpy().reshape(-1).view(gev_amd.CONN_BUF_DTYPE).tobytes() == want_conn_buf.tobytes()
    assert int(es["status"]) == 0 and int(es["payload_bytes"]) == nbytes and int(es["payload_len"]) == plan_bytes
    assert nbytes == plan_bytes and torch.equal(e_buf, e_wire[:plan_bytes])   # (every span is a multiple of 16)
    tr, tp, tg, te = [], [], [], []
    for _ in range(args.rounds):
        tr.append(timed(reply))
        tp.append(timed(plan))
        tg.append(timed(gather))
        te.append(timed(gather_echo))
    r, p, g, e = median(tr), median(tp), median(tg), median(te)
    spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]  # noqa: E731
    line = json.dumps(dict(
        path="room broadcast: gevws_reply_rooms_async, gevws_room_plan_async, gevws_send_gather_async over the room "
             "plan and over an echo plan of as many bytes",
        shape="%d connections in rooms of %d, one %d-byte text message each" % (N_CONNS, ROOM, MSG),
        connections=N_CONNS, rooms=rooms.n_rooms, messages=nm, entries=n_entries, wire_bytes=wb[0],
        plan_bytes=plan_bytes, buffer_bytes=nbytes, reply_ms=round(r, 4), reply_launches=REPLY_LAUNCHES,
        plan_ms=round(p, 4), plan_launches=PLAN_LAUNCHES, plan_ns_per_entry=round(p * 1e6 / n_entries, 3),
        plan_table_gb_s=round(64 * n_entries / p / 1e6, 1), gather_ms=round(g, 4), gather_launches=GATHER_LAUNCHES,
        gather_gb_s=round((plan_bytes + nbytes) / g / 1e6, 1), gather_write_gb_s=round(nbytes / g / 1e6, 1),
        echo_gather_ms=round(e, 4), echo_gather_gb_s=round((plan_bytes + nbytes) / e / 1e6, 1),
        room_over_echo=round(g / e, 3), reply_ms_spread=spread(tr), plan_ms_spread=spread(tp),
        gather_ms_spread=spread(tg), echo_gather_ms_spread=spread(te), rounds=args.rounds, reps=args.reps,
        warmup=args.warmup))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
