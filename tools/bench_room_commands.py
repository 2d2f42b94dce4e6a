#!/usr/bin/env python3
"""Measure the room-command step (gevws_room_commands_async) alone, beside the
room reply step (gevws_reply_rooms_async) on the same bodies in the same
process: the parent has no such step, so the reply step's count / emit pair --
the same 32-byte record a body -- is the yardstick.

Shapes: the rooms shape of DESIGN 5.11 (4 096 connections in rooms of 64, one
1 KiB text body each) and, for a per-body figure clear of the launch floor,
1 048 576 bodies of 64 bytes from 16 384 connections in rooms of 64.  Per shape
three command shares: 0 %, 1 % and 100 % of the bodies are "/join N" or "/leave"
(a tenth of the joins out of range: rejected).  The bodies are what the join
leaves (JOINED, on 16-byte boundaries of d_out), built directly.

Every call is timed by its own pair of stream events: the command step strips
its bodies in place, so d_bodies is restored (a device copy, outside the events)
before every call of either step.  One checked call per share comes first: the
counts of the summary against the bodies built.  Medians of `rounds` sums over
`reps` calls; one JSON line per shape and share.

    python tools/bench_room_commands.py [--rounds 7] [--warmup 2] [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOM = 64
SHAPES = [(4096, 1, 1024), (16384, 64, 64)]   # (connections, bodies a connection, bytes a body)
SHARES = (0.0, 0.01, 1.0)
COMMAND_LAUNCHES, REPLY_LAUNCHES = 4, 5    # kernels a call (each behind its memsets)


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
    eng = gev_amd.Engine(0)
    dev = torch.device("cuda", 0)
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    host = lambda t: t.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731

    def timed(fn, prep):
        """The sum of `reps` calls, each between its own events, prep() before each outside them."""
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for e0, e1 in evs:
            prep()
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in evs) / args.reps

    lines = []
    for n_conns, per_conn, MSG in SHAPES:
        n = n_conns * per_conn
        n_rooms = n_conns // ROOM
        rooms = gev_amd.Rooms.from_conn_room(np.arange(n_conns, dtype=np.uint32) // ROOM, dev)
        rng = np.random.default_rng(0x636D6400 + per_conn)
        out_bytes = n * MSG
        base_out = rng.integers(0x61, 0x7B, out_bytes, dtype=np.uint8)     # letters: no body is a command by chance
        for share in SHARES:
            is_cmd = rng.random(n) < share if 0 < share < 1 else np.full(n, share >= 1)
            rejected = is_cmd & (rng.random(n) < 0.1)
            leave = is_cmd & ~rejected & (rng.random(n) < 0.2)
            out = base_out.reshape(n, MSG).copy()
            bodies = np.zeros(n, gev_amd.BODY_DTYPE)
            bodies["off"] = np.arange(n, dtype=np.uint64) * MSG
            bodies["length"] = MSG
            bodies["conn"] = np.arange(n) // per_conn
            bodies["opcode"], bodies["flags"] = 1, gev_amd.BODY_WHOLE | gev_amd.BODY_JOINED
            for m in np.flatnonzero(is_cmd).tolist():
                text = b"/leave" if leave[m] else b"/join %d" % (n_rooms + m % 7 if rejected[m] else m % n_rooms)
                out[m, : len(text)] = np.frombuffer(text, np.uint8)
                bodies["length"][m] = len(text)
            d_out, d_saved = up(out), up(bodies)
            d_bodies = d_saved.clone()
            msg_sum, join_sum = z(64), z(64)
            msg_sum.view(torch.int64)[0] = n
            changes, change_of, cmd_sum = z(n, 8), z(n, dt=torch.int64), z(64)
            def_msgs, def_conn, def_sum = z(n, 24), z(n, dt=torch.int32), z(64)
            plain, plain_conn, plain_sum = z(n, 32), z(n, dt=torch.int32), z(64)
            plain_of, def_of = z(n, dt=torch.int64), z(n, dt=torch.int64)

            def restore():
                d_bodies.copy_(d_saved)

            def commands():
                eng.room_commands_async(d_bodies, n, msg_sum, join_sum, None, d_out, out_bytes, n_conns, n_rooms, 0,
                                        changes, n, change_of, cmd_sum)

            def reply():
                eng.reply_rooms_async(d_bodies, n, msg_sum, join_sum, gev_amd.HANDLER_ECHO_TEXT, None, None, n_conns,
                                      rooms, 0, def_msgs, def_conn, def_sum, plain, plain_conn, plain_sum, plain_of,
                                      def_of)

            # ---- checked once: the step's counts are the bodies'; the reply step behind it skips the stripped ones
            restore(), commands(), reply()
            torch.cuda.synchronize()
            cs, ps = host(cmd_sum), host(plain_sum)
            n_cmd, n_rej = int(is_cmd.sum()), int(rejected.sum())
            assert int(cs["status"]) == 0 and int(cs["payload_len"]) == n_cmd and int(cs["payload_bytes"]) == n_rej
            assert int(cs["frames"]) == n_cmd - n_rej and int(ps["status"]) == 0 and int(ps["frames"]) == n - n_cmd
            got = changes[: n_cmd - n_rej].cpu().numpy().reshape(-1).view(gev_amd.ROOM_CHANGE_DTYPE)
            want_m = np.flatnonzero(is_cmd & ~rejected)
            assert np.array_equal(got["conn"], want_m // per_conn)
            assert np.array_equal(got["room"], np.where(leave[want_m], gev_amd.ROOM_NONE, want_m % n_rooms))
            for _ in range(args.warmup):
                restore(), commands(), restore(), reply()
            torch.cuda.synchronize()
            tc, tr = [], []
            for _ in range(args.rounds):
                tc.append(timed(commands, restore))
                tr.append(timed(reply, restore))
            c, r = median(tc), median(tr)
            spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]  # noqa: E731
            read_bytes = 32 * n + 16 * n_cmd + n            # count: the records and the candidates' vectors; emit: classes
            line = json.dumps(dict(
                path="room commands: gevws_room_commands_async beside gevws_reply_rooms_async on the same bodies",
                shape="%d bodies of %d bytes, %d connections in rooms of %d, %g %% commands" % (n, MSG, n_conns, ROOM,
                                                                                           share * 100),
                bodies=n, connections=n_conns, rooms=n_rooms, command_share=share, commands=n_cmd, rejected=n_rej,
                changes=n_cmd - n_rej, commands_ms=round(c, 4), reply_rooms_ms=round(r, 4),
                commands_over_reply=round(c / r, 3), commands_ns_per_body=round(c * 1e6 / n, 3),
                reply_ns_per_body=round(r * 1e6 / n, 3), commands_launches=COMMAND_LAUNCHES,
                reply_launches=REPLY_LAUNCHES, commands_read_bytes=read_bytes,
                commands_ms_spread=spread(tc), reply_rooms_ms_spread=spread(tr), rounds=args.rounds, reps=args.reps,
                warmup=args.warmup))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
