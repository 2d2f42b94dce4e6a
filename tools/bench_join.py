#!/usr/bin/env python3
"""Measure the join step (gevws_join_async with GEVWS_JOIN_ALL: every whole
message's fragments gathered into one contiguous body) behind a decode and the
message pass, beside gevws_copy_async moving the same number of bytes (L read
+ L written) in the same process and clock state, and the reply step
(gevws_reply_bodies_async) as time per message.

Two shapes:
  c5     the C5 layout of gev_amd/workloads.py -- 1 MiB messages in fragments
         of up to 64 KiB with ping / pong frames in between -- as binary
         messages (the synthetic payload is not UTF-8, and a text message that
         fails the check is not delivered);
  small  16 fragments of 64..512 bytes a message, 16 messages a connection.
Join, copy and reply alternate in one process, each timed by HIP events around
`reps` launches; one JSON line per shape, medians over the rounds.

    python tools/bench_join.py [--rounds 7] [--warmup 2] [--shapes c5,small] [--out FILE]

--carry measures gevws_join_carry_async instead: the C5-like shape (64
connections, one 1 MiB binary message each, fragments up to 64 KiB) with every
message cut over 2, 4 and 16 passes.  Per pass: the bytes the call moves on
both sides (lengths read + 16-rounded lengths written), its time, and the ratio
to gevws_copy_async moving as many bytes; one JSON line per cut.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def layout_c5():
    import numpy as np
    from gev_amd import workloads
    lay = workloads.config_c5()
    b0 = lay.desc["b0"]
    lay.desc["b0"] = np.where((b0 & 0x0F) == 1, (b0 & 0xF0) | 2, b0)  # text -> binary
    return lay


def layout_small(n_conns: int = 4096, msgs_per_conn: int = 16, frags: int = 16, seed: int = 0x6A6F696E):
    import numpy as np
    from gev_amd import workloads
    rng = np.random.default_rng(seed)
    b0 = np.tile(np.array([0x02] + [0x00] * (frags - 2) + [0x80], np.uint8), msgs_per_conn)
    lengths, b0s, ms = [], [], []
    for _ in range(n_conns):
        lengths.append(rng.integers(64, 513, msgs_per_conn * frags).astype(np.int64))
        b0s.append(b0)
        ms.append(np.ones(b0.shape[0], np.uint8))
    return workloads.assemble("small fragments: 16 x 64..512 B a message", lengths, b0s, ms, seed)


SHAPES = {"c5": layout_c5, "small": layout_small}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def layouts_cut(passes: int, n_conns: int = 64, message_bytes: int = 1 << 20, max_fragment: int = 65536,
                control_prob: float = 0.25, seed: int = 0x63617272):
    """The C5-like shape with every connection's one binary message cut over
    `passes` passes of message_bytes / passes bytes each: a layout per pass."""
    import numpy as np
    from gev_amd import workloads
    rng = np.random.default_rng(seed + passes)
    per = message_bytes // passes
    lays = []
    for p in range(passes):
        lengths, b0s, ms = [], [], []
        for _ in range(n_conns):
            L, B = [], []
            left = per if p < passes - 1 else message_bytes - per * (passes - 1)
            while left > 0:
                f = int(min(left, rng.integers(1, max_fragment + 1)))
                left -= f
                L.append(f)
                B.append((0x80 if left == 0 and p == passes - 1 else 0) | (0x2 if p == 0 and len(L) == 1 else 0))
                if left > 0 and rng.random() < control_prob:
                    L.append(int(rng.integers(0, 126)))
                    B.append(0x80 | (0x9 if rng.random() < 0.5 else 0xA))
            lengths.append(np.array(L, np.int64))
            b0s.append(np.array(B, np.uint8))
            ms.append(np.ones(len(L), np.uint8))
        lays.append(workloads.assemble(f"C5-like, pass {p + 1} of {passes}", lengths, b0s, ms, seed + 97 * p))
    return lays


def bench_carry(eng, args):
    """gevws_join_carry_async pass by pass for messages cut over 2, 4 and 16
    passes: per pass the bytes the call moves (read + written, both sides), its
    time, and the ratio to gevws_copy_async moving as many bytes."""
    import numpy as np
    import torch

    import gev_amd
    dev = torch.device("cuda", 0)
    n_conns, message_bytes = 64, 1 << 20

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    for k in (2, 4, 16):
        state = torch.zeros((n_conns, 8), dtype=torch.uint8, device=dev)
        carry = gev_amd.Carry(eng, n_conns, 2 * message_bytes)
        want0 = b""
        rows = []
        for p, lay in enumerate(layouts_cut(k, n_conns, message_bytes)):
            arena = torch.zeros(lay.arena_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
            desc = torch.from_numpy(lay.desc.view(np.uint8).reshape(-1).copy()).to(dev)
            out = eng.alloc_batch(n_conns, lay.n_frames, lay.payload_padded)
            eng.synth(arena, desc, lay.n_frames, lay.seed)
            eng.decode_async(arena, lay.arena_bytes, torch.from_numpy(lay.conns.copy()).to(dev), n_conns, out,
                             lay.n_frames, lay.payload_padded)
            torch.cuda.synchronize()
            assert int(out.summary_host()["status"]) == 0 and int(out.summary_host()["frames"]) == lay.n_frames
            msgs = eng.messages(out, state)
            n = int(msgs.summary_host()["frames"])
            assert n == n_conns and not msgs.conn_msg_host()["error"].any()
            fr, co = out.frames_host(), out.conn_out_host()
            for f in range(int(co["first_frame"][0]), int(co["first_frame"][0]) + int(co["nframes"][0])):
                if not int(fr["opcode"][f]) & 8:  # connection 0's bytes, for the check behind the last pass
                    o = int(fr["payload_off"][f])
                    want0 += out.payload[o: o + int(fr["length"][f])].cpu().numpy().tobytes()
            src_side, src_used = carry.side, carry.used
            res = eng.join(out, msgs, flags=gev_amd.JOIN_ALL, carry=carry)  # sizes the arenas, checks, swaps
            s, cs = res.summary_host(), res.carry_summary_host()
            last = p == k - 1
            assert int(s["frames"]) == (n_conns if last else 0) and int(cs["frames"]) == (0 if last else n_conns)
            assert int(cs["errors"]) == 0
            if last:
                assert res.body_bytes(0) == want0 and len(want0) == message_bytes
            else:
                assert carry.carried_bytes(0) == want0
            moved = sum(int(x["payload_len"]) + int(x["payload_bytes"]) for x in (s, cs))
            copy_bytes = moved // 2 // 16 * 16
            csrc = torch.empty(copy_bytes + 16, dtype=torch.uint8, device=dev)
            cdst = torch.empty(copy_bytes + 16, dtype=torch.uint8, device=dev)
            dst_side = 1 - src_side

            def join():
                eng.join_carry_async(out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary,
                                     out.payload, None, None, gev_amd.JOIN_ALL, res.bodies, res.out, res.out_cap,
                                     res.summary, msgs.conn_msg, n_conns, carry.max_message_bytes,
                                     carry.records[src_side], carry.arenas[src_side], src_used,
                                     carry.records[dst_side], carry.arenas[dst_side], carry.cap(dst_side),
                                     res.carry_summary)

            def copy():
                eng.copy_(cdst, csrc, copy_bytes)

            for _ in range(args.warmup):
                join(), copy()
            torch.cuda.synchronize()
            tj, tc = [], []
            for _ in range(args.rounds):
                tj.append(timed(join))
                tc.append(timed(copy))
            j, c = median(tj), median(tc)
            rows.append({"pass": p + 1, "frames": lay.n_frames, "carried_in_bytes": src_used,
                         "bytes_moved": moved, "join_ms": round(j, 4), "GBps": round(moved / j / 1e6, 1),
                         "copy_ms": round(c, 4), "join_over_copy": round(j / c, 3)})
            del arena, out, msgs, res, csrc, cdst
            torch.cuda.empty_cache()
        line = json.dumps({
            "path": "join step with the carry (gevws_join_carry_async, JOIN_ALL), pass by pass",
            "shape": f"C5-like: {n_conns} connections, one 1 MiB message each, fragments up to 64 KiB",
            "passes": k, "message_bytes_moved_total": sum(r["bytes_moved"] for r in rows),
            "moved_over_message_bytes": round(sum(r["bytes_moved"] for r in rows) / (n_conns * message_bytes), 2),
            "rows": rows, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--shapes", default="c5,small")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--carry", action="store_true",
                    help="instead of the shapes: the join with its carry, 1 MiB messages cut over 2, 4 and 16 passes")
    args = ap.parse_args()
    import numpy as np
    import torch

    import gev_amd

    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)
    if args.carry:
        bench_carry(eng, args)
        eng.close()
        return
    for shape in args.shapes.split(","):
        lay = SHAPES[shape]()
        n_frames, n_conns = lay.n_frames, lay.n_conns
        arena = torch.zeros(lay.arena_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        desc = torch.from_numpy(lay.desc.view(np.uint8).reshape(-1).copy()).to(dev)
        conns = torch.from_numpy(lay.conns.copy()).to(dev)
        eng.synth(arena, desc, n_frames, lay.seed)
        out = eng.alloc_batch(n_conns, n_frames, lay.payload_padded)
        eng.decode_async(arena, lay.arena_bytes, conns, n_conns, out, n_frames, lay.payload_padded)
        torch.cuda.synchronize()
        ds = out.summary_host()
        assert int(ds["status"]) == 0 and int(ds["frames"]) == n_frames
        msgs = eng.messages(out)
        n = int(msgs.summary_host()["frames"])
        assert not msgs.conn_msg_host()["error"].any()
        first = eng.join(out, msgs, flags=gev_amd.JOIN_ALL)  # sizes the arena, and checks the result
        js = first.summary_host()
        body_bytes, taken = int(js["payload_len"]), int(js["payload_bytes"])
        assert int(js["frames"]) == n
        fr = out.frames_host()
        data = fr["length"][(fr["opcode"] & 8) == 0]
        assert body_bytes == int(data.sum())
        # spot-check a few bodies against the frames they were gathered from
        mh, mo, pay = msgs.messages_host(), msgs.msg_of_host(), out.payload
        for m in sorted({0, n // 2, n - 1}):
            fs = np.flatnonzero(mo == m)
            want = b"".join(pay[int(fr["payload_off"][f]): int(fr["payload_off"][f]) + int(fr["length"][f])]
                            .cpu().numpy().tobytes() for f in fs)
            assert first.body_bytes(m) == want and len(want) == int(mh["length"][m])
        bodies, dout, jsum = first.bodies, first.out, first.summary
        cap = first.out_cap
        copy_bytes = body_bytes // 16 * 16
        src = out.payload
        dst = torch.empty(copy_bytes + 16, dtype=torch.uint8, device=dev)
        cap_m = max(n, 1)
        dm = torch.zeros((cap_m, 24), dtype=torch.uint8, device=dev)
        pl = torch.zeros((cap_m, 32), dtype=torch.uint8, device=dev)
        dc, pc = (torch.zeros(cap_m, dtype=torch.int32, device=dev) for _ in range(2))
        dsum, psum = (torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(2))
        ro = torch.zeros(cap_m, dtype=torch.int64, device=dev)
        ext = torch.from_numpy((np.arange(n_conns) % 2).astype(np.uint8)).to(dev)  # every other connection deflate

        def join():
            eng.join_async(out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary, out.payload, None,
                           None, gev_amd.JOIN_ALL, bodies, dout, cap, jsum)

        def copy():
            eng.copy_(dst, src, copy_bytes)

        def reply():
            eng.reply_bodies_async(bodies, n, msgs.summary, jsum, gev_amd.HANDLER_ECHO_BINARY, ext, None, n_conns, dm,
                                   dc, dsum, pl, pc, psum, ro)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps

        for _ in range(args.warmup):
            join(), copy(), reply()
        torch.cuda.synchronize()
        t_join, t_copy, t_reply = [], [], []
        for _ in range(args.rounds):  # the three alternate
            t_join.append(timed(join))
            t_copy.append(timed(copy))
            t_reply.append(timed(reply))
        rs = dsum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        ps = psum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        assert int(rs["status"]) == 0 and int(rs["frames"]) + int(ps["frames"]) == n
        j, c, r = median(t_join), median(t_copy), median(t_reply)
        line = json.dumps({
            "path": "join step (JOIN_ALL) behind a decode and the message pass", "shape": shape, "layout": lay.name,
            "conns": n_conns, "frames": n_frames, "messages": n, "body_bytes": body_bytes, "out_bytes": taken,
            "join_ms": round(j, 4), "join_rounds_ms": [round(t, 4) for t in t_join],
            "join_read_plus_write_GBps": round((body_bytes + taken) / j / 1e6, 1),
            "copy_ms": round(c, 4), "copy_rounds_ms": [round(t, 4) for t in t_copy],
            "copy_read_plus_write_GBps": round(2 * copy_bytes / c / 1e6, 1),
            "join_over_copy": round(j / c, 3),
            "reply_ms": round(r, 4), "reply_ns_per_message": round(r * 1e6 / max(n, 1), 2),
            "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del arena, out, msgs, first, bodies, dout, dst, dm, pl
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
