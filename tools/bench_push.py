#!/usr/bin/env python3
"""Measure the push pass on two fan-out shapes over 16 384 connections, half of
them deflate-takers: one ALL push ("all"), and one push a room over 1 024 rooms
of 16 members ("rooms"), each at 64 B and 4 KiB bodies.  Either way the plan
has 16 384 entries.

One checked pass through Engine.push(gather=True) comes first: sampled
connections' spans are parsed and compared with the bodies they must be sent.
Then every step of the chain -- push_lists, deflate, the two encodes, push_plan,
gather -- is timed by HIP events around `reps` calls on buffers of its own, and
in the same run the unchanged gevws_room_plan_async over a client-originated pass
with the same rooms and the same number of output entries (one member of each
room sends one message of the same size), as the yardstick for the plan.
Medians of `rounds`; one JSON line a shape and body size.

    python tools/bench_push.py [--rounds 7] [--warmup 2] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CONNS, ROOM = 16384, 16
LISTS_LAUNCHES, PLAN_LAUNCHES, ROOM_PLAN_LAUNCHES = 5, 9, 12


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
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    rng = np.random.default_rng(0x70757368)
    ext_h = (np.arange(N_CONNS) % 2).astype(np.uint8) * gev_amd.EXT_DEFLATE
    ext = up(ext_h)

    def room_plan_yardstick(conn_room, senders, size):
        """gevws_room_plan_async behind a real pass: `senders` each send one
        masked text frame of `size` bytes, the other connections nothing."""
        text = rng.integers(0x20, 0x7F, size, dtype=np.uint8).tobytes()
        frame = np.frombuffer(wo.encode_frame(text, 1, True, 0, True, b"\x01\x02\x03\x04"), np.uint8)
        ns, fl = len(senders), frame.size
        arena = z(ns * fl + gev_amd.IN_PAD)
        arena[: ns * fl] = up(np.tile(frame, ns))
        conns = np.zeros((N_CONNS, 2), np.int64)
        conns[senders, 1] = fl   # (the others are idle: no bytes)
        conns[:, 0] = np.cumsum(conns[:, 1]) - conns[:, 1]
        pay_cap = ns * ((size + 15) // 16 * 16) + 64
        out = eng.alloc_batch(N_CONNS, ns, pay_cap, aux_slots=N_CONNS)
        eng.decode_async(arena, ns * fl, up(conns), N_CONNS, out, ns, pay_cap)
        torch.cuda.synchronize()
        assert int(out.summary_host()["status"]) == 0 and int(out.summary_host()["frames"]) == ns
        msgs = eng.messages(out)
        bodies = eng.join(out, msgs, flags=gev_amd.JOIN_ALL)
        rooms = gev_amd.Rooms.from_conn_room(conn_room, dev)
        res = eng.broadcast(out, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, rooms)
        n_entries = int(res.summary_host()["frames"])
        nf, nm = msgs.n_frames, bodies.n_messages
        # the plan again on its own tables
        ctl, ctl_conn, ctl_sum = z(nf, 32), z(nf, dt=torch.int32), z(64)
        ctl_of, msg_end, conn_ctl = z(nf, dt=torch.int64), z(nm, dt=torch.int64), z(N_CONNS, 32)
        aux_cap = gev_amd._abi.AUX_SLOT * out.aux_slots
        aux_off = (out.payload.numel() - 16 - aux_cap) // 16 * 16
        eng.control_async(out.frames, nf, out.conn_out, N_CONNS, out.summary, out.payload, aux_off, aux_cap,
                          msgs.msg_of, msgs.messages, nm, msgs.conn_msg, msgs.summary, bodies.bodies, bodies.summary, 0,
                          ctl, ctl_conn, ctl_of, msg_end, conn_ctl, ctl_sum)
        plain_of, def_of = up(res.plain_of), up(res.def_of)
        tabs = []
        for off_h, wire in ((res.echo.plain_off, res.echo.plain_wire), (res.echo.def_off, res.echo.def_wire)):
            s = np.zeros(1, gev_amd.SUMMARY_DTYPE)
            s["frames"], s["payload_bytes"] = off_h.size, int(wire.numel())
            tabs.append((up(np.concatenate([off_h.astype(np.int64), np.zeros(1, np.int64)])), up(s.view(np.uint8))))
        none_off, ctl_enc = z(1, dt=torch.int64), z(64)
        send, conn_send, plan_sum = z(max(n_entries, 1), 32), z(N_CONNS, 32), z(64)

        def plan():
            eng.room_plan_async(nf, out.summary, out.conn_out, N_CONNS, msgs.msg_of, msg_end, plain_of, def_of, nm,
                                msgs.summary, bodies.summary, ext, ctl_of, conn_ctl, ctl_sum, tabs[0][0], tabs[0][1],
                                tabs[1][0], tabs[1][1], none_off, ctl_enc, rooms, 0, send, n_entries, conn_send,
                                plan_sum)

        plan()
        torch.cuda.synchronize()
        assert int(host(plan_sum)["status"]) == 0 and int(host(plan_sum)["frames"]) == n_entries
        assert torch.equal(send[:n_entries], res.send[:n_entries])
        return plan, n_entries

    def measure(shape, size):
        body = rng.integers(0x20, 0x7F, size, dtype=np.uint8).tobytes()
        if shape == "all":
            conn_room = np.zeros(N_CONNS, np.uint32)
            items = [(gev_amd.PUSH_ALL, 0, 1, body)]
            senders = np.array([0])
        else:
            conn_room = (np.arange(N_CONNS) // ROOM).astype(np.uint32)
            items = [(gev_amd.PUSH_ROOM, g, 1, body) for g in range(N_CONNS // ROOM)]
            senders = np.arange(0, N_CONNS, ROOM)
        recs_h, arena_h, _ = gev_amd.push_records(items)
        rooms = gev_amd.Rooms.from_conn_room(conn_room, dev)
        n, src_bytes = recs_h.size, arena_h.size - gev_amd.IN_PAD
        recs, src = up(recs_h.view(np.uint8).reshape(-1, 32)), up(arena_h)

        # ---- the checked pass
        res = eng.push(recs, src, ext, rooms, gather=True)
        ps = res.summary_host()
        n_entries, plan_bytes = int(ps["frames"]), int(ps["payload_bytes"])
        assert n_entries == N_CONNS
        sends = res.host_sends()
        for c in (0, 1, ROOM, N_CONNS // 2 + 1, N_CONNS - 1):
            got = wo.decode_stream(bytes(sends[c]) + b"\x88\x00" * 3)
            f = got.frames[0]
            assert got.status == wo.OK and f.header.opcode == 1 and f.header.fin, c
            data = zlib.decompressobj(-15).decompress(f.payload + b"\x00\x00\xff\xff") if f.header.rsv else f.payload
            assert data == body and bool(f.header.rsv) == bool(ext_h[c]), c
        nbytes = int(res.send_buf.numel())
        nd, npl = int(res.echo.def_off.size), int(res.echo.plain_off.size)
        assert nd == npl == n

        # ---- the steps on buffers of their own
        def_msgs, def_sum, plain, plain_sum = z(n, 24), z(64), z(n, 32), z(64)
        plain_of, def_of = z(n, dt=torch.int64), z(n, dt=torch.int64)

        def lists():
            eng.push_lists_async(recs, n, None, src_bytes, ext, None, None, N_CONNS, rooms, 0, def_msgs, def_sum, plain,
                                 plain_sum, plain_of, def_of)

        lists()
        dcap = n * ((gev_amd.deflate_bound(size) + 15) // 16 * 16) + 16
        d_frames, d_out, d_sum = z(n, 32), z(dcap + gev_amd._abi.OUT_PAD), z(64)

        def deflate():
            eng.deflate_async(def_msgs, n, def_sum, src, src_bytes, 0, d_frames, d_out, dcap, d_sum)

        deflate()
        pcap, wcap = n * (size + 14) + 16, n * (gev_amd.deflate_bound(size) + 14) + 16
        p_wire, p_off, p_enc = z(pcap + gev_amd._abi.OUT_PAD), z(n, dt=torch.int64), z(64)
        d_wire, d_off, d_enc = z(wcap + gev_amd._abi.OUT_PAD), z(n, dt=torch.int64), z(64)

        def encode_plain():
            eng.encode_replies_async(plain, n, plain_sum, src, p_wire, pcap, p_off, p_enc)

        def encode_deflated():
            eng.encode_replies_async(d_frames, n, d_sum, d_out, d_wire, wcap, d_off, d_enc)

        encode_plain(), encode_deflated()
        send, conn_send, plan_sum = z(n_entries, 32), z(N_CONNS, 32), z(64)

        def plan():
            eng.push_plan_async(recs, n, None, src_bytes, plain_sum, def_sum, plain_of, def_of, p_off, p_enc, d_off,
                                d_enc, ext, None, N_CONNS, rooms, 0, send, n_entries, conn_send, plan_sum)

        plan()
        torch.cuda.synchronize()
        wb = [int(host(p_enc)["payload_bytes"]), int(host(d_enc)["payload_bytes"]), 0]
        wires = (p_wire[: wb[0]], d_wire[: wb[1]], None)
        buf, conn_buf, gsum = z(nbytes), z(N_CONNS, 32), z(64)

        def gather():
            eng.send_gather_async(send, n_entries, conn_send, N_CONNS, plan_sum, wires, wb, buf, nbytes, conn_buf, gsum)

        yard_err, room_plan, yard_entries = None, None, 0
        try:
            room_plan, yard_entries = room_plan_yardstick(conn_room, senders, size)
        except Exception as e:  # the push figures stand without their yardstick
            yard_err = repr(e)
        steps = dict(lists=lists, deflate=deflate, encode_plain=encode_plain, encode_deflated=encode_deflated,
                     plan=plan, gather=gather)
        if room_plan is not None:
            steps["room_plan"] = room_plan
        for _ in range(args.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        assert int(host(plan_sum)["status"]) == 0 and int(host(plan_sum)["frames"]) == n_entries
        assert torch.equal(send, res.send[:n_entries]) and torch.equal(conn_send, res.conn_send)
        assert int(host(gsum)["status"]) == 0 and torch.equal(buf, res.send_buf)
        times = {k: [] for k in steps}
        for _ in range(args.rounds):
            for k, fn in steps.items():   # alternating: one process, one clock state
                times[k].append(timed(fn))
        med = {k: median(v) for k, v in times.items()}
        line = dict(
            path="push pass: gevws_push_lists_async, gevws_deflate_async, gevws_encode_replies_async x2, "
                 "gevws_push_plan_async, gevws_send_gather_async; gevws_room_plan_async at the same entry count",
            shape="%s: %d connections, %d pushes of %d bytes, half the connections take deflate"
                  % (shape, N_CONNS, n, size),
            connections=N_CONNS, pushes=n, body_bytes=size, entries=n_entries, plan_bytes=plan_bytes,
            buffer_bytes=nbytes, lists_launches=LISTS_LAUNCHES, plan_launches=PLAN_LAUNCHES,
            room_plan_launches=ROOM_PLAN_LAUNCHES, room_plan_entries=yard_entries, room_plan_error=yard_err,
            rounds=args.rounds, reps=args.reps, warmup=args.warmup)
        for k, v in med.items():
            line[k + "_ms"] = round(v, 4)
            line[k + "_ms_spread"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        line["plan_ns_per_entry"] = round(med["plan"] * 1e6 / n_entries, 3)
        if room_plan is not None and yard_entries:
            line["room_plan_ns_per_entry"] = round(med["room_plan"] * 1e6 / yard_entries, 3)
            line["plan_over_room_plan"] = round(med["plan"] / med["room_plan"], 3)
        return line

    for shape in ("all", "rooms"):
        for size in (64, 4096):
            text = json.dumps(measure(shape, size))
            print(text, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
