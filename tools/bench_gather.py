#!/usr/bin/env python3
"""Measure the gather (gevws_send_gather_async) beside a plain streaming copy
of as many bytes (gevws_copy_async), on two shapes:

  c5      the respond shape of tools/bench_respond.py: config_c5's 256 replies
          of 1 MiB and its control replies, through the whole chain.  One
          checked pass through Engine.respond(gather=True) comes first: every
          span is compared with Responses.conn_bytes.
  small   control replies only: 256 Ki pongs of 2-127 bytes over 4 096
          connections, a hand-built send list over one wire, checked against
          the concatenation on the host.  Every output vector is assembled by
          its lane from up to eight entries.

The gather and the copy alternate in one process and clock state, each timed by
HIP events around `reps` calls; medians of `rounds`; one JSON line a shape.

    python tools/bench_gather.py [--rounds 7] [--warmup 2] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES = 7  # kernels a call, behind one memset


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
    eng = gev_amd.Engine(0)
    dev = torch.device("cuda", 0)
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def measure(shape, send, max_sends, conn_send, n_conns, plan_sum, wires, want_buf, want_conn_buf, extra):
        """The raw call on buffers of the checked pass's sizes, beside the copy of as many bytes."""
        nbytes = int(want_buf.numel())
        buf, conn_buf, gsum = z(nbytes), z(n_conns, 32), z(64)
        src = torch.randint(0, 256, (nbytes + 16,), dtype=torch.uint8, device=dev)
        dst = z(nbytes)
        wb = [int(w.numel()) if w is not None else 0 for w in wires]

        def gather():
            eng.send_gather_async(send, max_sends, conn_send, n_conns, plan_sum, wires, wb, buf, nbytes, conn_buf, gsum)

        def copy():
            eng.copy_(dst, src, nbytes)

        for _ in range(args.warmup):
            gather(), copy()
        torch.cuda.synchronize()
        gs = gsum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        assert int(gs["status"]) == 0 and int(gs["payload_bytes"]) == nbytes
        assert torch.equal(buf, want_buf) and torch.equal(conn_buf[:n_conns].cpu(), want_conn_buf)
        assert torch.equal(dst, src[:nbytes])
        tg, tc = [], []
        for _ in range(args.rounds):
            tg.append(timed(gather))
            tc.append(timed(copy))
        g, c = median(tg), median(tc)
        entries, length = int(gs["frames"]), int(gs["payload_len"])
        line = json.dumps(dict(
            path="gather (gevws_send_gather_async) beside gevws_copy_async over as many bytes", shape=shape,
            connections=n_conns, entries=entries, buffer_bytes=nbytes, payload_len=length,
            mean_entry_bytes=round(length / max(entries, 1), 1), launches=LAUNCHES, gather_ms=round(g, 4),
            copy_ms=round(c, 4), gather_over_copy=round(g / c, 3),
            gather_gb_s=round((length + nbytes) / g / 1e6, 1), copy_gb_s=round(2 * nbytes / c / 1e6, 1),
            gather_ns_per_entry=round(g * 1e6 / max(entries, 1), 2), gather_ms_spread=[round(min(tg), 4), round(max(tg), 4)],
            copy_ms_spread=[round(min(tc), 4), round(max(tc), 4)], rounds=args.rounds, reps=args.reps,
            warmup=args.warmup, **extra))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    # ---- the C5 respond shape
    lay = workloads.config_c5()
    b0 = lay.desc["b0"]
    lay.desc["b0"] = np.where((b0 & 0x0F) == 1, (b0 & 0xF0) | 2, b0)  # text -> binary: the payload is not UTF-8
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
    res = eng.respond(out, msgs, bodies, gev_amd.HANDLER_ECHO_BINARY, None, gather=True)
    sends = res.host_sends()
    for c in range(n_conns):  # the checked pass: every span is the host's three-wire join
        assert bytes(sends[c]) == res.conn_bytes(c), c
    n_ctl = int(res.ctl_summary["frames"])
    wires = (res.echo.plain_wire, res.echo.def_wire, res.ctl_wire)
    conn_buf = torch.from_numpy(res.conn_buf.view(np.uint8).reshape(-1, 32).copy())
    measure(lay.name, res.send, msgs.n_frames, res.conn_send, n_conns, res.summary, wires, res.send_buf, conn_buf,
            dict(control_replies=n_ctl, replies=int(res.summary_host()["frames"]) - n_ctl))
    del res, sends, bodies, msgs, out, arena

    # ---- control replies only
    rng = np.random.default_rng(0x736D616C)
    n_conns, per = 4096, 64
    n = n_conns * per
    lens = rng.integers(2, 128, n).astype(np.uint64)   # a pong: a 2-byte header and up to 125 bytes
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    order = rng.permutation(n)                          # the control wire is in reply order, not in send order
    wire_h = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    send_h = np.zeros(n, gev_amd.SEND_DTYPE)
    send_h["off"], send_h["len"] = offs[order], lens[order]
    send_h["frame"], send_h["conn"], send_h["wire"] = np.arange(n), np.arange(n) // per, gev_amd.WIRE_CONTROL
    cs_h = np.zeros(n_conns, gev_amd.CONN_SEND_DTYPE)
    cs_h["first"], cs_h["count"] = np.arange(n_conns) * per, per
    cs_h["bytes"] = send_h["len"].reshape(n_conns, per).sum(1)
    spans = (cs_h["bytes"] + 15) // 16 * 16
    span_off = np.concatenate([[0], np.cumsum(spans)[:-1]]).astype(np.uint64)
    want = np.zeros(int(spans.sum()), np.uint8)
    for c in range(n_conns):  # the concatenation on the host
        p = int(span_off[c])
        for e in send_h[c * per: (c + 1) * per]:
            ln = int(e["len"])
            want[p: p + ln] = wire_h[int(e["off"]): int(e["off"]) + ln]
            p += ln
    want_cb = np.zeros(n_conns, gev_amd.CONN_BUF_DTYPE)
    want_cb["off"], want_cb["bytes"] = span_off, cs_h["bytes"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    wire = z(wire_h.size + 32)
    wire[: wire_h.size] = up(wire_h)
    plan = np.zeros(1, gev_amd.SUMMARY_DTYPE)
    plan["frames"] = n
    measure("small: %d pongs of 2-127 bytes over %d connections" % (n, n_conns), up(send_h).reshape(-1, 32), n,
            up(cs_h).reshape(-1, 32), n_conns, up(plan), (None, None, wire[: wire_h.size]), up(want),
            torch.from_numpy(want_cb.view(np.uint8).reshape(-1, 32).copy()), dict(control_replies=n, replies=0))
    eng.close()


if __name__ == "__main__":
    main()
