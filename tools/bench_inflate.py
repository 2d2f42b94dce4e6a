#!/usr/bin/env python3
"""Measure the inflate step (gevws_inflate_async: one wave per compressed
message) behind a decode and the message pass, beside two baselines for the
same batch: that decode's own unmask (gevws_ctx_timing), and zlib inflating
the same messages on this machine's CPUs, on one core and on 16 processes.

Two shapes -- 16 384 connections with one 4 KiB text message each, and 1 024
with one of 256 KiB -- times two payloads: compressible text (zlib level 6)
and level-0 stored blocks, which is the copy bound.  Every message is one
masked text frame with RSV1; a shape's messages cycle through eight distinct
texts.  Decode, message pass and inflate step alternate in one process; the
inflate step is timed by HIP events around its launches.  One JSON line per
(shape, payload), medians over the rounds.

    python tools/bench_inflate.py [--rounds 7] [--warmup 2] [--shapes many,large]

--takeover measures client context takeover instead (gevws_inflate_ctx_async):
16 384 connections x 8 text messages of about 512 B, compressed by one
persistent compressor per connection, against the same messages compressed
independently -- the compressed bytes of both, the inflate step's time for
both (alternating in one process), and zlib with a persistent decompressobj
per connection.  Two JSON lines with "mode": "takeover".

    python tools/bench_inflate.py --takeover [--commit ID]

--carry measures compressed messages that span two passes
(gevws_inflate_carry_async, gevws_join_carry_ext_async) on the same shapes,
with or without --takeover: every connection's stream is cut in two inside its
middle message (the only one, without --takeover), at the middle of that
message's payload.  Pass 1 holds the messages before it and its first half as
an open fragment, pass 2 its second half with the FIN and the messages behind
it.  One JSON line per case with "mode": "carry": the END pass's inflate beside
the plain call over the same messages whole in one batch (alternating), the
open pass's inflate and join, and the bytes the join moved into the carry.

    python tools/bench_inflate.py --carry [--takeover] [--commit ID]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # name: (connections = messages, inflated bytes a message)
    "many": (16384, 4096),
    "large": (1024, 256 * 1024),
}
LEVELS = {"text": 6, "stored": 0}
DISTINCT = 8
TAIL = b"\x00\x00\xff\xff"
WORDS = ("the quick brown fox jumps over the lazy dog while websocket frames carry compressed json payloads "
         "status ok error null true false id name value timestamp price volume bid ask größe naïve €").split()


def text(nbytes: int, rng) -> bytes:
    """nbytes of word soup with numbers in it: compresses about 3:1."""
    parts = []
    size = 0
    while size < nbytes + 8:
        w = WORDS[int(rng.integers(0, len(WORDS)))] if rng.random() < 0.8 else str(int(rng.integers(0, 10 ** 6)))
        parts.append(w)
        size += len(w.encode()) + 1
    b = " ".join(parts).encode()
    cut = nbytes
    while cut and (b[cut] & 0xC0) == 0x80:
        cut -= 1
    return b[:cut] + b"." * (nbytes - cut)


def deflate(data: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    s = c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)
    assert s.endswith(TAIL)
    return s[:-4]


def wire_frame(payload: bytes, key: bytes, b0: int = 0xC1):
    import numpy as np
    L = len(payload)
    hdr = bytes([b0]) + (bytes([0x80 | L]) if L <= 125 else bytes([0x80 | 126]) + L.to_bytes(2, "big") if L <= 0xFFFF
                           else bytes([0x80 | 127]) + L.to_bytes(8, "big")) + key  # FIN | RSV1 | text, masked
    body = np.frombuffer(payload, np.uint8) ^ np.resize(np.frombuffer(key, np.uint8), L)
    return np.concatenate([np.frombuffer(hdr, np.uint8), body])


def inflate_all(job):
    """zlib over `count` messages cycling through `payloads`: (seconds, bytes out)."""
    payloads, count = job
    t0 = time.perf_counter()
    total = 0
    for i in range(count):
        total += len(zlib.decompressobj(-15).decompress(payloads[i % len(payloads)] + TAIL))
    return time.perf_counter() - t0, total


def cpu_baselines(payloads, n: int, rounds: int):
    """Medians of the wall time zlib takes for the n messages: one core, and 16 processes sharing them."""
    import multiprocessing as mp
    one = sorted(inflate_all((payloads, n))[0] for _ in range(rounds))[rounds // 2]
    jobs = [(payloads, n // 16 + (1 if k < n % 16 else 0)) for k in range(16)]
    with mp.get_context("spawn").Pool(16) as pool:  # fresh interpreters: no GPU state in them
        pool.map(inflate_all, jobs)  # warm-up: the workers are up
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(inflate_all, jobs)
            walls.append(time.perf_counter() - t0)
    return one, sorted(walls)[rounds // 2]


def median(xs):
    return sorted(xs)[len(xs) // 2]


TAKEOVER_CONNS, TAKEOVER_MSGS, TAKEOVER_BYTES, TAKEOVER_SCRIPTS = 16384, 8, 512, 64


def inflate_chains(job):
    """zlib over `count` connections cycling through `scripts` (a connection's
    payloads in order): one persistent decompressobj a connection when `keep`,
    a fresh one a message otherwise; (seconds, bytes out)."""
    scripts, count, keep = job
    t0 = time.perf_counter()
    total = 0
    for i in range(count):
        d = zlib.decompressobj(-15)
        for p in scripts[i % len(scripts)]:
            if not keep:
                d = zlib.decompressobj(-15)
            total += len(d.decompress(p + TAIL))
    return time.perf_counter() - t0, total


def cpu_chain_baselines(scripts, n: int, keep: bool, rounds: int):
    import multiprocessing as mp
    one = sorted(inflate_chains((scripts, n, keep))[0] for _ in range(rounds))[rounds // 2]
    jobs = [(scripts, n // 16 + (1 if k < n % 16 else 0), keep) for k in range(16)]
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(inflate_chains, jobs)
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(inflate_chains, jobs)
            walls.append(time.perf_counter() - t0)
    return one, sorted(walls)[rounds // 2]


def takeover_main(args):
    """--takeover: 16 384 connections x 8 text messages of about 512 B, each
    connection's messages compressed by one persistent compressor (client
    context takeover) against the same messages compressed independently; the
    inflate step of both, alternating in one process."""
    import numpy as np
    rng = np.random.default_rng(0x74616B)
    n, per = TAKEOVER_CONNS, TAKEOVER_MSGS
    texts = [[text(TAKEOVER_BYTES - 32 + int(rng.integers(0, 64)), rng) for _ in range(per)]
             for _ in range(TAKEOVER_SCRIPTS)]
    kept, alone = [], []
    for script in texts:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        kept.append([(c.compress(t) + c.flush(zlib.Z_SYNC_FLUSH))[:-4] for t in script])
        alone.append([deflate(t, 6) for t in script])
    cpu = {}
    if not args.no_cpu:
        cpu = {"takeover": cpu_chain_baselines(kept, n, True, args.rounds),
               "independent": cpu_chain_baselines(alone, n, False, args.rounds)}

    import torch

    import gev_amd

    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)
    nm = n * per
    inflated_bytes = sum(len(t) for i in range(n) for t in texts[i % TAKEOVER_SCRIPTS])
    limit = max(len(t) for s in texts for t in s)
    ctx = torch.zeros((n, gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev)
    runs = {}
    for mode, scripts, ext_byte in (("takeover", kept, 3), ("independent", alone, 1)):
        streams = [np.concatenate([wire_frame(p, bytes(rng.integers(1, 256, 4).astype("u1"))) for p in s])
                   for s in scripts]
        lens = np.array([streams[i % TAKEOVER_SCRIPTS].size for i in range(n)], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        in_bytes = int(lens.sum())
        arena = torch.zeros(in_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        arena[:in_bytes] = torch.from_numpy(np.concatenate([streams[i % TAKEOVER_SCRIPTS] for i in range(n)])).to(dev)
        comp_bytes = sum(len(p) for i in range(n) for p in scripts[i % TAKEOVER_SCRIPTS])
        payload_cap = sum((len(p) + 15) // 16 * 16 for i in range(n) for p in scripts[i % TAKEOVER_SCRIPTS])
        runs[mode] = dict(
            arena=arena, in_bytes=in_bytes, conns=torch.from_numpy(np.stack([offs, lens], 1)).to(dev),
            comp_bytes=comp_bytes, payload_cap=payload_cap, out=eng.alloc_batch(n, nm, payload_cap),
            ext=torch.full((n,), ext_byte, dtype=torch.uint8, device=dev), t_inf=[], t_msg=[])
    msgs = torch.empty((nm, 32), dtype=torch.uint8, device=dev)
    msg_of = torch.empty(nm, dtype=torch.int64, device=dev)
    conn_msg = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    msum = torch.zeros(64, dtype=torch.uint8, device=dev)
    inflated = torch.empty((nm, 32), dtype=torch.uint8, device=dev)
    out_cap = nm * ((limit + 15) // 16 * 16)
    d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    isum = torch.zeros(64, dtype=torch.uint8, device=dev)

    def one_round(r, timed):
        ctx.zero_()  # fresh connections (outside the timed span)
        eng.decode_async(r["arena"], r["in_bytes"], r["conns"], n, r["out"], nm, r["payload_cap"])
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        eng.messages_ext_async(r["out"].frames, nm, r["out"].conn_out, n, r["out"].summary, r["out"].payload, None,
                               msgs, nm, msg_of, conn_msg, msum, r["ext"])
        e[1].record()
        if r is runs["takeover"]:
            eng.inflate_ctx_async(r["out"].frames, nm, msgs, nm, msg_of, msum, r["out"].payload, limit, None,
                                  inflated, d_out, out_cap, isum, r["ext"], ctx, n)
        else:  # today's call
            eng.inflate_async(r["out"].frames, nm, msgs, nm, msg_of, msum, r["out"].payload, limit, None, inflated,
                              d_out, out_cap, isum)
        e[2].record()
        torch.cuda.synchronize()
        if timed:
            r["t_msg"].append(e[0].elapsed_time(e[1]))
            r["t_inf"].append(e[1].elapsed_time(e[2]))

    for mode, r in runs.items():  # warm-up, and the bytes are the texts
        for _ in range(args.warmup):
            one_round(r, False)
        s = isum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        assert (int(s["status"]), int(s["frames"]), int(s["errors"]), int(s["payload_len"])) == \
            (0, nm, 0, inflated_bytes), (mode, s)
        rec = inflated.cpu().numpy().reshape(-1).view(gev_amd.INFLATED_DTYPE)
        for i in (0, 1, per - 1, per, nm - 1):
            o, want = int(rec["out_off"][i]), texts[(i // per) % TAKEOVER_SCRIPTS][i % per]
            assert d_out[o:o + len(want)].cpu().numpy().tobytes() == want, (mode, i)
    for _ in range(args.rounds):  # the two alternate
        for r in runs.values():
            one_round(r, True)
    for mode, r in runs.items():
        m = median(r["t_inf"])
        line = {"path": "inflate step, client context takeover (one wave per connection's chain) against the same "
                        "messages compressed independently (one wave per message)",
                "mode": "takeover", "variant": mode, "commit": args.commit, "connections": n,
                "messages_per_connection": per, "messages": nm, "inflated_bytes": inflated_bytes,
                "compressed_bytes": r["comp_bytes"],
                "compressed_vs_independent": round(r["comp_bytes"] / runs["independent"]["comp_bytes"], 4),
                "inflate_ms": round(m, 4), "inflate_rounds_ms": [round(t, 4) for t in r["t_inf"]],
                "inflate_out_GBps": round(inflated_bytes / m / 1e6, 2), "messages_ms": round(median(r["t_msg"]), 4),
                "context_bytes": n * gev_amd.INF_CTX_BYTES if mode == "takeover" else 0,
                "rounds": args.rounds, "warmup": args.warmup}
        if mode in cpu:
            one, many = cpu[mode]
            line.update({"zlib_1core_ms": round(one * 1e3, 2), "zlib_16proc_ms": round(many * 1e3, 2),
                         "zlib_1core_out_GBps": round(inflated_bytes / one / 1e9, 3),
                         "zlib_16proc_out_GBps": round(inflated_bytes / many / 1e9, 3)})
        print(json.dumps(line), flush=True)
    eng.close()


def carry_main(args):
    """--carry: see the module docstring."""
    import numpy as np
    import torch

    import gev_amd

    rng = np.random.default_rng(0x636172)
    cases = []  # (name, connections, ext byte, per-connection scripts of (text, payload))
    if args.takeover:
        scripts = []
        for _ in range(TAKEOVER_SCRIPTS):
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            ts = [text(TAKEOVER_BYTES - 32 + int(rng.integers(0, 64)), rng) for _ in range(TAKEOVER_MSGS)]
            scripts.append([(t, (c.compress(t) + c.flush(zlib.Z_SYNC_FLUSH))[:-4]) for t in ts])
        cases.append(("takeover", TAKEOVER_CONNS, 3, scripts))
    else:
        for shape in args.shapes.split(","):
            n, size = SHAPES[shape]
            texts = [text(size, rng) for _ in range(DISTINCT)]
            for kind in args.kinds.split(","):
                cases.append((f"{shape}/{kind}", n, 1, [[(t, deflate(t, LEVELS[kind]))] for t in texts]))
    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)

    def key():
        return bytes(rng.integers(1, 256, 4).astype("u1"))

    for name, n, ext_byte, scripts in cases:
        per, ns = len(scripts[0]), len(scripts)
        mid = per // 2
        nm = n * per
        limit = max(len(t) for sc in scripts for t, _ in sc)
        inflated_bytes = sum(len(t) for i in range(n) for t, _ in scripts[i % ns])

        def batch(streams, max_frames):
            lens = np.array([streams[i % ns].size for i in range(n)], np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
            in_bytes = int(lens.sum())
            arena = torch.zeros(in_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
            arena[:in_bytes] = torch.from_numpy(np.concatenate([streams[i % ns] for i in range(n)])).to(dev)
            cap = in_bytes + 16 * max_frames
            return dict(arena=arena, in_bytes=in_bytes, conns=torch.from_numpy(np.stack([offs, lens], 1)).to(dev),
                        cap=cap, out=eng.alloc_batch(n, max_frames, cap), frames=max_frames)

        whole = batch([np.concatenate([wire_frame(p, key()) for _, p in sc]) for sc in scripts], nm)
        first, second = [], []
        for sc in scripts:
            p = sc[mid][1]
            h = len(p) // 2
            first.append(np.concatenate([wire_frame(q, key()) for _, q in sc[:mid]] + [wire_frame(p[:h], key(), 0x41)]))
            second.append(np.concatenate([wire_frame(p[h:], key(), 0x80)] + [wire_frame(q, key()) for _, q in sc[mid + 1:]]))
        p1, p2 = batch(first, n * (mid + 1)), batch(second, n * (per - mid))
        carried = sum(len(scripts[i % ns][mid][1]) // 2 for i in range(n))
        carry_cap = sum((len(scripts[i % ns][mid][1]) // 2 + 15) // 16 * 16 for i in range(n))
        ext = torch.full((n,), ext_byte, dtype=torch.uint8, device=dev)
        ctx = torch.zeros((n, gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev) if args.takeover else None
        state = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
        msgs = torch.empty((nm, 32), dtype=torch.uint8, device=dev)
        msg_of = torch.empty(nm, dtype=torch.int64, device=dev)
        conn_msg = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        msum, isum, jsum, csum = (torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(4))
        inflated = torch.empty((nm, 32), dtype=torch.uint8, device=dev)
        bodies = torch.empty((nm, 32), dtype=torch.uint8, device=dev)
        out_cap = nm * ((limit + 15) // 16 * 16)
        d_out = torch.empty(out_cap + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        crec = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        czero = torch.zeros((n, 32), dtype=torch.uint8, device=dev)  # the carry in front of the first pass
        cdst = torch.zeros(carry_cap + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        t = {k: [] for k in ("whole", "open_inflate", "open_join", "end_inflate")}

        def front(b):
            eng.decode_async(b["arena"], b["in_bytes"], b["conns"], n, b["out"], b["frames"], b["cap"])
            eng.messages_ext_async(b["out"].frames, b["frames"], b["out"].conn_out, n, b["out"].summary,
                                   b["out"].payload, state, msgs, b["frames"], msg_of, conn_msg, msum, ext)

        def inflate(b, carry):
            o = b["out"]
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            if carry is None:  # the call before the carry
                eng.inflate_ctx_async(o.frames, b["frames"], msgs, b["frames"], msg_of, msum, o.payload, limit, state,
                                      inflated, d_out, out_cap, isum, ext if ctx is not None else None, ctx, n)
            else:
                eng.inflate_carry_async(o.frames, b["frames"], msgs, b["frames"], msg_of, msum, o.payload, limit,
                                        state, inflated, d_out, out_cap, isum, ext if ctx is not None else None, ctx,
                                        n, carry[0], carry[1], carry[2])
            e[1].record()
            return e

        def check(want_frames, want_len):
            s = isum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
            assert (int(s["status"]), int(s["frames"]), int(s["errors"]), int(s["payload_len"])) == \
                (0, want_frames, 0, want_len), (name, s)

        def one_round(timed):
            state.zero_()
            if ctx is not None:
                ctx.zero_()
            front(whole)
            ew = inflate(whole, None)
            torch.cuda.synchronize()
            if not timed:
                check(nm, inflated_bytes)
            state.zero_()
            if ctx is not None:
                ctx.zero_()
            front(p1)
            e1 = inflate(p1, (czero, cdst, 0))
            ej = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ej[0].record()
            eng.join_carry_ext_async(p1["out"].frames, p1["frames"], msgs, p1["frames"], msg_of, msum,
                                     p1["out"].payload, inflated, isum, gev_amd.JOIN_ALL, bodies, d_out, out_cap, jsum,
                                     conn_msg, n, 0xFFFFFFFF, None, None, 0, crec, cdst, carry_cap, csum,
                                     gev_amd.CARRY_KEEP_COMPRESSED)
            ej[1].record()
            torch.cuda.synchronize()
            if not timed:
                c = csum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
                assert (int(c["status"]), int(c["frames"]), int(c["payload_len"]), int(c["payload_bytes"])) == \
                    (0, n, carried, carry_cap), (name, c)
            front(p2)
            e2 = inflate(p2, (crec, cdst, carry_cap))
            torch.cuda.synchronize()
            if not timed:
                check(n * (per - mid), sum(len(x) for i in range(n) for x, _ in scripts[i % ns][mid:]))
                rec = inflated.cpu().numpy().reshape(-1).view(gev_amd.INFLATED_DTYPE)
                for i in (0, 1, n - 1):  # the carried message's bytes are its text
                    want = scripts[i % ns][mid][0]
                    o = int(rec["out_off"][i * (per - mid)])
                    assert d_out[o:o + len(want)].cpu().numpy().tobytes() == want, (name, i)
            else:
                t["whole"].append(ew[0].elapsed_time(ew[1]))
                t["open_inflate"].append(e1[0].elapsed_time(e1[1]))
                t["open_join"].append(ej[0].elapsed_time(ej[1]))
                t["end_inflate"].append(e2[0].elapsed_time(e2[1]))

        for _ in range(args.warmup):
            one_round(False)
        for _ in range(args.rounds):
            one_round(True)
        line = {"path": "compressed messages cut in two passes inside the middle message: the END pass's "
                        "gevws_inflate_carry_async beside the call without a carry over the same messages whole in "
                        "one batch; the open pass's inflate and gevws_join_carry_ext_async",
                "mode": "carry", "case": name, "takeover": bool(args.takeover), "commit": args.commit,
                "connections": n, "messages_per_connection": per, "messages_in_end_pass": n * (per - mid),
                "inflated_bytes": inflated_bytes, "carried_bytes": carried, "carry_arena_bytes": carry_cap,
                "whole_inflate_ms": round(median(t["whole"]), 4),
                "end_inflate_carry_ms": round(median(t["end_inflate"]), 4),
                "open_inflate_carry_ms": round(median(t["open_inflate"]), 4),
                "open_join_carry_ms": round(median(t["open_join"]), 4),
                "open_join_read_plus_write_bytes": carried + carry_cap,
                "rounds_ms": {k: [round(x, 4) for x in v] for k, v in t.items()},
                "rounds": args.rounds, "warmup": args.warmup}
        print(json.dumps(line), flush=True)
        del whole, p1, p2, msgs, msg_of, inflated, bodies, d_out, cdst
        torch.cuda.empty_cache()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="many,large")
    ap.add_argument("--kinds", default="text,stored")
    ap.add_argument("--no-cpu", action="store_true", help="skip the zlib baselines")
    ap.add_argument("--takeover", action="store_true",
                    help="client context takeover against independently compressed messages (16 384 x 8 x ~512 B)")
    ap.add_argument("--carry", action="store_true",
                    help="compressed messages that span two passes; with --takeover on the takeover shape")
    ap.add_argument("--commit", default="", help="recorded in the --takeover and --carry lines")
    args = ap.parse_args()
    if args.carry:
        return carry_main(args)
    if args.takeover:
        return takeover_main(args)
    import numpy as np

    rng = np.random.default_rng(0x696E66)
    cases = []
    for shape in args.shapes.split(","):
        n, size = SHAPES[shape]
        texts = [text(size, rng) for _ in range(DISTINCT)]
        for kind in args.kinds.split(","):
            payloads = [deflate(t, LEVELS[kind]) for t in texts]
            cpu = (None, None) if args.no_cpu else cpu_baselines(payloads, n, args.rounds)
            cases.append((shape, kind, n, size, texts, payloads, cpu))

    import torch

    import gev_amd

    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)
    for shape, kind, n, size, texts, payloads, (cpu_one, cpu_16) in cases:
        frames = [wire_frame(p, bytes(rng.integers(1, 256, 4).astype("u1"))) for p in payloads]
        lens = np.array([frames[i % DISTINCT].size for i in range(n)], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        in_bytes = int(lens.sum())
        host = np.concatenate([frames[i % DISTINCT] for i in range(n)])
        arena = torch.zeros(in_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        arena[:in_bytes] = torch.from_numpy(host).to(dev)
        del host
        conns = torch.from_numpy(np.stack([offs, lens], 1)).to(dev)
        comp_bytes = sum(len(payloads[i % DISTINCT]) for i in range(n))
        payload_cap = sum((len(payloads[i % DISTINCT]) + 15) // 16 * 16 for i in range(n))
        out = eng.alloc_batch(n, n, payload_cap)
        msgs = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        msg_of = torch.empty(n, dtype=torch.int64, device=dev)
        conn_msg = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        msum = torch.zeros(64, dtype=torch.uint8, device=dev)
        ext = torch.ones(n, dtype=torch.uint8, device=dev)
        inflated = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        out_cap = n * ((size + 15) // 16 * 16)
        d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
        isum = torch.zeros(64, dtype=torch.uint8, device=dev)

        def decode():
            eng.decode_async(arena, in_bytes, conns, n, out, n, payload_cap)

        def messages():
            eng.messages_ext_async(out.frames, n, out.conn_out, n, out.summary, out.payload, None, msgs, n, msg_of,
                                   conn_msg, msum, ext)

        def inflate():
            eng.inflate_async(out.frames, n, msgs, n, msg_of, msum, out.payload, size, None, inflated, d_out, out_cap,
                              isum)

        for _ in range(args.warmup):
            decode(), messages(), inflate()
        torch.cuda.synchronize()
        s = isum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        assert (int(s["status"]), int(s["frames"]), int(s["errors"]), int(s["payload_len"])) == (0, n, 0, n * size), s
        rec = inflated.cpu().numpy().reshape(-1).view(gev_amd.INFLATED_DTYPE)
        for i in (0, 1, DISTINCT - 1, n - 1):  # the bytes are the texts
            o = int(rec["out_off"][i])
            assert d_out[o:o + size].cpu().numpy().tobytes() == texts[i % DISTINCT], i
        t_inf, t_msg, t_unmask, t_dec = [], [], [], []
        eng.set_timing(True)
        for _ in range(args.rounds):  # the three steps alternate
            decode()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            messages()
            e[1].record()
            inflate()
            e[2].record()
            torch.cuda.synchronize()
            ms, calls = eng.timing()
            assert calls == 1
            t_msg.append(e[0].elapsed_time(e[1]))
            t_inf.append(e[1].elapsed_time(e[2]))
            t_dec.append(sum(ms))
            t_unmask.append(ms[3])
        eng.set_timing(False)
        m, u = median(t_inf), median(t_unmask)
        line = {
            "path": "inflate step (permessage-deflate, one wave per message) behind a decode and the message pass",
            "shape": shape, "payload": kind, "zlib_level": LEVELS[kind], "messages": n, "message_bytes": size,
            "compressed_bytes": comp_bytes, "inflated_bytes": n * size,
            "inflate_ms": round(m, 4), "inflate_rounds_ms": [round(t, 4) for t in t_inf],
            "inflate_out_GBps": round(n * size / m / 1e6, 2),
            "messages_ms": round(median(t_msg), 4), "decode_ms": round(median(t_dec), 4),
            "unmask_ms": round(u, 4), "unmask_rounds_ms": [round(t, 4) for t in t_unmask],
            "unmask_read_plus_write_GBps": round(2 * comp_bytes / u / 1e6, 1),
            "rounds": args.rounds, "warmup": args.warmup}
        if cpu_one is not None:
            line.update({"zlib_1core_ms": round(cpu_one * 1e3, 2),
                         "zlib_1core_out_GBps": round(n * size / cpu_one / 1e9, 3),
                         "zlib_16proc_ms": round(cpu_16 * 1e3, 2),
                         "zlib_16proc_out_GBps": round(n * size / cpu_16 / 1e9, 3)})
        print(json.dumps(line), flush=True)
        del arena, out, msgs, msg_of, conn_msg, inflated, d_out
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
