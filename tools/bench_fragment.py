#!/usr/bin/env python3
"""Measure outbound fragmentation (gevws_fragment_async,
gevws_fragment_offsets_async) on the send half of Engine.respond, on a C5-like
shape: config_c5's 1 MiB messages as binary, every `--deflate-every`-th
connection with permessage-deflate, so that there is one plain wire and one
deflated wire.  The limit is None (the chain without the new steps: the
baseline), 64 KiB, 4 KiB and 1 KiB.

For each limit, one JSON line:
  respond_wall_ms   Engine.respond(gather=True) as a caller sees it, host
                    synchronisations included (median of `--wall-reps` calls
                    behind a warm-up call); the first call of each limit is
                    checked: every reply of sampled connections is reassembled
                    from its frames and compared with the None pass's.
  fragment_ms       gevws_fragment_async over both record lists
  encode_ms         gevws_encode_replies_async over both lists (None: over the
                    records; else over the fragments -- more, smaller frames
                    make the encode's boundary path busier, and that is the
                    encode's)
  offsets_ms        gevws_fragment_offsets_async for both
each timed by HIP events around `--reps` calls on buffers of their own, medians
of `--rounds` rounds behind `--warmup` warm-up rounds.

    python tools/bench_fragment.py [--rounds 7] [--warmup 2] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = (None, 64 * 1024, 4 * 1024, 1024)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--deflate-every", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import gev_amd
    from gev_amd import workloads
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

    def rounds_of(fn):
        for _ in range(args.warmup):
            timed(fn)
        ts = [timed(fn) for _ in range(args.rounds)]
        return median(ts), [round(min(ts), 4), round(max(ts), 4)]

    lay = workloads.config_c5()
    b0 = lay.desc["b0"]
    lay.desc["b0"] = np.where((b0 & 0x0F) == 1, (b0 & 0xF0) | 2, b0)  # text -> binary: the payload is not UTF-8
    n_conns = lay.conns.shape[0]
    ext_h = np.where(np.arange(n_conns) % args.deflate_every == 0, gev_amd.EXT_DEFLATE, 0).astype(np.uint8)
    ext = torch.from_numpy(ext_h).to(dev)
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

    def respond(F):
        return eng.respond(out, msgs, bodies, gev_amd.HANDLER_ECHO_BINARY, ext, gather=True, max_fragment_bytes=F)

    def replies(wire: bytes):
        """A connection's data replies reassembled from its frames (control frames left out)."""
        got = wo.decode_stream(wire + b"\x88\x00" * 3)
        assert got.status == wo.OK
        msgs_, cur = [], None
        for f in got.frames:
            if f.stream_pos >= len(wire) or f.header.opcode & 8:
                continue
            cur = [f.payload] if f.header.opcode else cur + [f.payload]
            if f.header.fin:
                msgs_.append(cur)
                cur = None
        return msgs_

    base = respond(None)
    sample = sorted({0, 1, args.deflate_every, n_conns - 1} & set(range(n_conns)))
    base_sends = base.host_sends()   # one device-to-host copy of the send buffer
    base_replies = {c: replies(bytes(base_sends[c])) for c in sample}
    del base_sends
    # the two record lists as the chain builds them (the bodies are the control step's now)
    nm = bodies.n_messages
    def_msgs, def_conn, def_sum = z(nm, 24), z(nm, dt=torch.int32), z(64)
    plain, plain_conn, plain_sum = z(nm, 32), z(nm, dt=torch.int32), z(64)
    reply_of = torch.full((nm,), -1, dtype=torch.int64, device=dev)
    eng.reply_bodies_async(bodies.bodies, nm, msgs.summary, bodies.summary, gev_amd.HANDLER_ECHO_BINARY, ext, None,
                           n_conns, def_msgs, def_conn, def_sum, plain, plain_conn, plain_sum, reply_of)
    torch.cuda.synchronize()
    dfl = base.echo.deflated
    lists = []
    for recs, gate, payload in ((plain, plain_sum, bodies.out), (dfl.frames, dfl.summary, dfl.out)):
        k = int(host(gate)["frames"])
        total = int(recs[:k].cpu().numpy().reshape(-1).view(gev_amd.OUT_FRAME_DTYPE)["payload_len"].sum())
        lists.append((recs, gate, payload, k, total))

    for F in LIMITS:
        res = base if F is None else respond(F)
        frames_sent, sends = 0, res.host_sends()
        for c in sample:   # the checked pass: the same messages, no frame above the limit
            got = replies(bytes(sends[c]))
            assert [b"".join(m) for m in got] == [b"".join(m) for m in base_replies[c]], (F, c)
            assert F is None or all(len(p) <= F for m in got for p in m), (F, c)
            frames_sent += sum(len(m) for m in got)
        wall = []
        for _ in range(args.wall_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            respond(F)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        del res, sends
        # the steps on buffers of their own
        bufs = []
        for recs, gate, payload, k, total in lists:
            kf = k if F is None else k + total // F
            wcap = total + 14 * kf + 16
            bufs.append(dict(frags=z(max(kf, 1), 32), first=z(nm + 1, dt=torch.int64), fsum=z(64),
                             wire=torch.empty(wcap + 16, dtype=torch.uint8, device=dev), wcap=wcap, kf=max(kf, 1),
                             frag_off=z(max(kf, 1), dt=torch.int64), esum=z(64), off=z(nm, dt=torch.int64), rsum=z(64)))

        def fragment():
            for (recs, gate, payload, k, total), b in zip(lists, bufs):
                eng.fragment_async(recs, nm, gate, F, b["frags"], b["kf"], b["first"], b["fsum"])

        def encode():
            for (recs, gate, payload, k, total), b in zip(lists, bufs):
                if F is None:
                    eng.encode_replies_async(recs, nm, gate, payload, b["wire"], b["wcap"], b["off"], b["esum"])
                else:
                    eng.encode_replies_async(b["frags"], b["kf"], b["fsum"], payload, b["wire"], b["wcap"],
                                             b["frag_off"], b["esum"])

        def offsets():
            for (recs, gate, payload, k, total), b in zip(lists, bufs):
                eng.fragment_offsets_async(b["first"], nm, gate, b["fsum"], b["frag_off"], b["esum"], b["off"],
                                           b["rsum"])

        line = dict(path="send half of Engine.respond with a frame size limit", shape=lay.name + ", binary",
                    connections=n_conns, deflate_connections=int((ext_h != 0).sum()), max_fragment_bytes=F,
                    replies=[x[3] for x in lists], payload_bytes=[x[4] for x in lists],
                    respond_wall_ms=round(median(wall), 3), respond_wall_spread=[round(min(wall), 3), round(max(wall), 3)],
                    sampled_frames=frames_sent)
        if F is not None:
            line["fragment_ms"], line["fragment_ms_spread"] = rounds_of(fragment)
        line["encode_ms"], line["encode_ms_spread"] = rounds_of(encode)
        if F is not None:
            line["offsets_ms"], line["offsets_ms_spread"] = rounds_of(offsets)
            fs = [host(b["fsum"]) for b in bufs]
            assert all(int(s["status"]) == 0 for s in fs) and all(int(host(b["rsum"])["status"]) == 0 for b in bufs)
            line["fragments"] = [int(s["frames"]) for s in fs]
            line["split_records"] = [int(s["payload_bytes"]) for s in fs]
            line["new_steps_ms"] = round(line["fragment_ms"] + line["offsets_ms"], 4)
            line["fragment_ns_per_fragment"] = round(line["fragment_ms"] * 1e6 / max(sum(line["fragments"]), 1), 3)
        assert all(int(host(b["esum"])["status"]) == 0 for b in bufs)
        line["wire_bytes"] = [int(host(b["esum"])["payload_bytes"]) for b in bufs]
        for k_ in ("fragment_ms", "encode_ms", "offsets_ms"):
            if k_ in line:
                line[k_] = round(line[k_], 4)
        line.update(rounds=args.rounds, reps=args.reps, warmup=args.warmup, wall_reps=args.wall_reps)
        s = json.dumps(line)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")
        del bufs
    eng.close()


if __name__ == "__main__":
    main()
