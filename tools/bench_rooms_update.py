#!/usr/bin/env python3
"""Measure the membership update on the device (gevws_rooms_update_async)
against the host path it replaces: Rooms.from_conn_room on the updated array --
a stable numpy argsort and three uploads.

Shapes: 16 384 connections in 1 024 rooms, 1 M connections in 256 rooms (a
one-pass sort) and 1 M connections in 1 M rooms (a three-pass sort); each with
1 % of the connections changed and as a pure build.  Per shape, alternating in
one process and clock state:

  device_ms        the call alone, HIP events around `reps` calls, the change
                   records already in device memory
  device_wall_ms   host clock: the change records uploaded, the call, a
                   synchronise (what a server that keeps its tables resident pays)
  update_wall_ms   host clock: Rooms.update / Rooms.build as they stand, with
                   their allocations and the summary read back
  host_wall_ms     host clock: the changes applied to the host array,
                   Rooms.from_conn_room, a synchronise

The device's tables are compared with the host's once per shape before anything
is timed.  Medians of `rounds`; one JSON line per shape.

    python tools/bench_rooms_update.py [--rounds 7] [--warmup 2] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16384, 1024), (1 << 20, 256), (1 << 20, 1 << 20)]
CHANGED = 0.01


def median(xs):
    return sorted(xs)[len(xs) // 2]


def passes_of(n_rooms: int) -> int:
    return 0 if n_rooms == 0 else max(1, ((n_rooms - 1).bit_length() + 7) // 8)


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
    eng = gev_amd.Engine(0)
    dev = torch.device("cuda", 0)
    host = lambda t: t.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = []
    for n_conns, n_rooms in SHAPES:
        rng = np.random.default_rng(0x72756200 + n_rooms % 251)
        cr = rng.integers(0, n_rooms, n_conns).astype(np.uint32)
        cr[rng.random(n_conns) < 0.1] = gev_amd.ROOM_NONE
        rooms = gev_amd.Rooms.from_conn_room(cr, dev, n_rooms)
        for kind in ("update", "build"):
            k = int(n_conns * CHANGED) if kind == "update" else 0
            ch = np.zeros(k, gev_amd.ROOM_CHANGE_DTYPE)
            ch["conn"] = rng.choice(n_conns, k, replace=False)
            ch["room"] = rng.integers(0, n_rooms, k)
            ch["room"][rng.random(k) < 0.1] = gev_amd.ROOM_NONE
            ch_bytes = ch.view(np.uint8)
            d_ch = torch.from_numpy(ch_bytes.copy()).to(dev) if k else None
            out = torch.empty(n_conns, dtype=torch.int32, device=dev)
            first = torch.empty(n_rooms + 1, dtype=torch.int32, device=dev)
            members = torch.empty(n_conns, dtype=torch.int32, device=dev)
            summ = torch.zeros(64, dtype=torch.uint8, device=dev)

            def call(changes=d_ch):
                eng.rooms_update_async(rooms.conn_room, n_conns, n_rooms, changes, k, None, None, None, 0, out, first,
                                       members, summ)

            def device_wall():
                call(torch.from_numpy(ch_bytes).to(dev) if k else None)

            def update_wall():
                return rooms.update(eng, ch) if k else gev_amd.Rooms.build(eng, rooms.conn_room, n_rooms)

            def host_path():
                new = cr.copy()
                new[ch["conn"]] = ch["room"]
                return gev_amd.Rooms.from_conn_room(new, dev, n_rooms)

            # ---- checked once: the device's tables are the host's
            call()
            torch.cuda.synchronize()
            s = host(summ)
            want = host_path()
            assert int(s["status"]) == 0 and int(s["frames"]) == want.n_members and int(s["payload_bytes"]) == k
            assert torch.equal(out, want.conn_room) and torch.equal(first, want.room_first)
            assert torch.equal(members[: want.n_members], want.room_members)
            got = update_wall()
            assert torch.equal(got.room_members, want.room_members) and torch.equal(got.conn_room, want.conn_room)
            for _ in range(args.warmup):
                call(), device_wall(), update_wall(), host_path()
            torch.cuda.synchronize()
            td, tw, tu, th = [], [], [], []
            for _ in range(args.rounds):
                td.append(timed(call))
                tw.append(wall(device_wall))
                tu.append(wall(update_wall))
                th.append(wall(host_path))
            d, w, u, h = median(td), median(tw), median(tu), median(th)
            spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]  # noqa: E731
            p = passes_of(n_rooms)
            line = json.dumps(dict(
                path="membership update: gevws_rooms_update_async against Rooms.from_conn_room on the updated array",
                shape="%d connections, %d rooms, %s" % (n_conns, n_rooms,
                                                        "%d changes" % k if k else "a pure build"),
                connections=n_conns, rooms=n_rooms, changes=k, members=int(s["frames"]), moved=int(s["payload_len"]),
                sort_passes=p, launches=7 + (1 if k else 0) + 5 * p, device_ms=round(d, 4),
                device_wall_ms=round(w, 4), update_wall_ms=round(u, 4), host_wall_ms=round(h, 4),
                host_over_device_wall=round(h / w, 2), host_over_update_wall=round(h / u, 2),
                device_ns_per_conn=round(d * 1e6 / n_conns, 3), device_ms_spread=spread(td),
                device_wall_ms_spread=spread(tw), update_wall_ms_spread=spread(tu), host_wall_ms_spread=spread(th),
                rounds=args.rounds, reps=args.reps, warmup=args.warmup))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
