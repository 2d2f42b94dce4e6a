#!/usr/bin/env python3
"""Measure the control step and the send plan (gevws_control_async,
gevws_send_plan_async) on the C5 shape of gev_amd/workloads.py -- 1 MiB binary
messages in fragments of up to 64 KiB with ping / pong frames in between --
beside the reply chain they stand in: reply -> encode of the plain list ->
encode of the control replies.  Behind a decode, the message pass and a join
with GEVWS_JOIN_ALL; the three alternate in one process and clock state, each
timed by HIP events around `reps` rounds of launches; one JSON line, medians.

    python tools/bench_respond.py [--rounds 7] [--warmup 2] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import gev_amd
    from gev_amd import workloads
    lay = workloads.config_c5()
    b0 = lay.desc["b0"]
    lay.desc["b0"] = np.where((b0 & 0x0F) == 1, (b0 & 0xF0) | 2, b0)  # text -> binary: the payload is not UTF-8
    eng = gev_amd.Engine(0)
    dev = torch.device("cuda", 0)
    n_conns = lay.conns.shape[0]
    arena = torch.zeros(lay.arena_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(lay.desc.view(np.uint8).reshape(-1).copy()).to(dev)
    out = eng.alloc_batch(n_conns, lay.n_frames, lay.payload_padded, aux_slots=n_conns)
    eng.synth(arena, desc, lay.n_frames, lay.seed)
    eng.decode_async(arena, lay.arena_bytes, torch.from_numpy(lay.conns.copy()).to(dev), n_conns, out, lay.n_frames,
                     lay.payload_padded)
    torch.cuda.synchronize()
    assert int(out.summary_host()["status"]) == 0 and int(out.summary_host()["frames"]) == lay.n_frames
    msgs = eng.messages(out)
    bodies = eng.join(out, msgs, flags=gev_amd.JOIN_ALL)
    nf, nm = msgs.n_frames, bodies.n_messages
    # one checked pass through the public call, then the raw calls on buffers of its sizes
    res = eng.respond(out, msgs, bodies, gev_amd.HANDLER_ECHO_BINARY, None)
    n_ctl, n_send = int(res.ctl_summary["frames"]), int(res.summary_host()["frames"])
    assert n_send == n_ctl + int(np.count_nonzero(res.echo.reply_of >= 0)) and int(res.summary_host()["errors"]) == 0
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    aux_cap = 128 * n_conns
    aux_off = (out.payload.numel() - 16 - aux_cap) // 16 * 16
    ctl, ctl_conn, ctl_sum = z(nf, 32), z(nf, dt=torch.int32), z(64)
    ctl_of, msg_end, conn_ctl = z(nf, dt=torch.int64), z(nm, dt=torch.int64), z(n_conns, 32)
    def_msgs, def_conn, def_sum = z(nm, 24), z(nm, dt=torch.int32), z(64)
    plain, plain_conn, plain_sum = z(nm, 32), z(nm, dt=torch.int32), z(64)
    reply_of = z(nm, dt=torch.int64)
    pcap = int(res.echo.plain_wire.numel()) + 16
    ccap = int(res.ctl_wire.numel()) + 16
    pwire, cwire = z(pcap + 16), z(ccap + 16)
    poff, coff, doff = z(nm, dt=torch.int64), z(nf, dt=torch.int64), z(1, dt=torch.int64)
    penc, cenc, denc = z(64), z(64), z(64)
    send, conn_send, plan_sum = z(nf, 32), z(n_conns, 32), z(64)

    def control():
        eng.control_async(out.frames, nf, out.conn_out, n_conns, out.summary, out.payload, aux_off, aux_cap,
                          msgs.msg_of, msgs.messages, nm, msgs.conn_msg, msgs.summary, bodies.bodies, bodies.summary, 0,
                          ctl, ctl_conn, ctl_of, msg_end, conn_ctl, ctl_sum)

    def chain():
        eng.reply_bodies_async(bodies.bodies, nm, msgs.summary, bodies.summary, gev_amd.HANDLER_ECHO_BINARY, None, None,
                               n_conns, def_msgs, def_conn, def_sum, plain, plain_conn, plain_sum, reply_of)
        eng.encode_replies_async(plain, nm, plain_sum, bodies.out, pwire, pcap, poff, penc)
        eng.encode_replies_async(ctl, nf, ctl_sum, out.payload, cwire, ccap, coff, cenc)

    def plan():
        eng.send_plan_async(nf, out.summary, out.conn_out, n_conns, msgs.msg_of, msg_end, reply_of, nm, msgs.summary,
                            bodies.summary, None, ctl_of, conn_ctl, ctl_sum, poff, penc, doff, denc, coff, cenc, send,
                            nf, conn_send, plan_sum)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    for _ in range(args.warmup):
        control(), chain(), plan()
    torch.cuda.synchronize()
    ps = plan_sum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
    assert int(ps["status"]) == 0 and int(ps["frames"]) == n_send
    assert torch.equal(send[:n_send], res.send[:n_send])
    tc, tr, tp = [], [], []
    for _ in range(args.rounds):
        tc.append(timed(control))
        tr.append(timed(chain))
        tp.append(timed(plan))
    c, r, p = median(tc), median(tr), median(tp)
    line = json.dumps({
        "path": "control step and send plan (gevws_control_async, gevws_send_plan_async) beside reply + two encodes",
        "shape": lay.name, "connections": n_conns, "frames": nf, "messages": nm, "control_replies": n_ctl,
        "plan_entries": n_send, "control_ms": round(c, 4), "plan_ms": round(p, 4),
        "reply_and_encodes_ms": round(r, 4), "added_over_chain": round((c + p) / r, 3),
        "control_ns_per_frame": round(c * 1e6 / nf, 1), "plan_ns_per_frame": round(p * 1e6 / nf, 1),
        "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
