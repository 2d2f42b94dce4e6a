#!/usr/bin/env python3
"""Measure the message step (gevws_messages_async: fragment assembly, frame
checks, UTF-8 check of text messages) behind a decode, beside that decode's
own unmask: the unmask moves every payload byte twice (read + write), the
UTF-8 pass reads it once.

Two shapes -- 16 384 text frames of 64 KiB, and 2 M text frames of 440 bytes
(the C4 frame size) -- times three payloads: pure ASCII, dense 3-byte text,
mixed 1- to 4-byte text.  Every frame is a masked single-frame text message;
the frames of a shape share one payload template (the rate does not depend on
the bytes differing from frame to frame, the kernels keep no state between
frames).  Decode and message step alternate in one process; the decode's phases
come from gevws_ctx_timing, the message step from HIP events around its
launches.  One JSON line per (shape, payload), medians over the rounds.

    python tools/bench_messages.py [--rounds 7] [--warmup 2] [--shapes big,small]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (frames, payload bytes a frame, connections)
    "big": (16384, 65536, 256),
    "small": (2 * 1024 * 1024, 440, 4096),
}


def template(kind: str, nbytes: int, rng) -> bytes:
    if kind == "ascii":
        return bytes(rng.integers(0x20, 0x7F, nbytes).astype("u1"))
    if kind == "dense3":
        cps = rng.integers(0x3040, 0x9FFF, nbytes // 3)  # kana and CJK: three bytes each
    else:
        cps = rng.choice([*rng.integers(0x20, 0x7F, 8), *rng.integers(0xA0, 0x800, 3), *rng.integers(0x800, 0xD800, 3),
                          *rng.integers(0x10000, 0x110000, 2)], nbytes)
    b = "".join(map(chr, cps)).encode() + b"...."
    cut = min(nbytes, len(b) - 4)
    while cut and (b[cut] & 0xC0) == 0x80:  # no character cut by the end
        cut -= 1
    return b[:cut] + b"." * (nbytes - cut)


def wire_frame(payload: bytes, key: bytes):
    import numpy as np
    L = len(payload)
    assert L % 4 == 0 and len(key) == 4
    hdr = bytes([0x81]) + (bytes([0x80 | 126]) + L.to_bytes(2, "big") if L <= 0xFFFF
                           else bytes([0x80 | 127]) + L.to_bytes(8, "big")) + key
    body = np.frombuffer(payload, "<u4") ^ np.frombuffer(key, "<u4")[0]
    return np.concatenate([np.frombuffer(hdr, np.uint8), body.view(np.uint8)])


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3, help="message steps per timed window")
    ap.add_argument("--shapes", default="big,small")
    ap.add_argument("--kinds", default="ascii,dense3,mixed")
    args = ap.parse_args()
    import numpy as np
    import torch

    import gev_amd

    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)
    rng = np.random.default_rng(0x6D7367)
    for shape in args.shapes.split(","):
        n, L, n_conns = SHAPES[shape]
        for kind in args.kinds.split(","):
            text = template(kind, L, rng)
            text.decode("utf-8")  # the template is valid
            one = wire_frame(text, bytes(rng.integers(1, 256, 4).astype("u1")))
            arena = torch.zeros(one.size * n + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
            arena[: one.size * n] = torch.from_numpy(one.copy()).to(dev).repeat(n)
            per = n // n_conns
            offs = np.arange(n_conns, dtype=np.int64) * per * one.size
            conns = torch.from_numpy(np.stack([offs, np.full(n_conns, per * one.size, np.int64)], 1)).to(dev)
            padded = (L + 15) // 16 * 16
            out = eng.alloc_batch(n_conns, n, padded * n)
            msgs = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            msg_of = torch.empty(n, dtype=torch.int64, device=dev)
            conn_msg = torch.empty((n_conns, 32), dtype=torch.uint8, device=dev)
            summ = torch.zeros(64, dtype=torch.uint8, device=dev)

            def decode():
                eng.decode_async(arena, one.size * n, conns, n_conns, out, n, padded * n)

            def messages():
                eng.messages_async(out.frames, n, out.conn_out, n_conns, out.summary, out.payload, None, msgs, n,
                                   msg_of, conn_msg, summ)

            for _ in range(args.warmup):
                decode()
                messages()
            torch.cuda.synchronize()
            s = summ.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
            ds = out.summary_host()
            assert int(ds["status"]) == 0 and int(ds["frames"]) == n and int(ds["payload_len"]) == n * L
            assert (int(s["status"]), int(s["frames"]), int(s["errors"]), int(s["payload_len"])) == (0, n, 0, n * L)
            t_msg, t_dec, t_unmask = [], [], []
            eng.set_timing(True)
            for _ in range(args.rounds):  # decode and message step alternate
                decode()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    messages()
                e1.record()
                torch.cuda.synchronize()
                ms, calls = eng.timing()
                assert calls == 1
                t_msg.append(e0.elapsed_time(e1) / args.reps)
                t_dec.append(sum(ms))
                t_unmask.append(ms[3])
            eng.set_timing(False)
            m, u = median(t_msg), median(t_unmask)
            print(json.dumps({
                "path": "message step (assembly + frame checks + UTF-8) behind a decode", "shape": shape,
                "payload": kind, "frames": n, "frame_bytes": L, "conns": n_conns, "text_bytes": n * L,
                "messages_ms": round(m, 4), "messages_rounds_ms": [round(t, 4) for t in t_msg],
                "messages_text_GBps": round(n * L / m / 1e6, 1),
                "decode_ms": round(median(t_dec), 4), "unmask_ms": round(u, 4),
                "unmask_rounds_ms": [round(t, 4) for t in t_unmask],
                "unmask_read_plus_write_GBps": round(2 * n * L / u / 1e6, 1),
                "messages_over_unmask": round(m / u, 3), "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}), flush=True)
            del arena, out, msgs, msg_of, conn_msg
            torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
