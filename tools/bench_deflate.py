#!/usr/bin/env python3
"""Measure the deflate step (gevws_deflate_async: one wave per outbound
message, fixed-Huffman and stored blocks) beside baselines for the same batch:
zlib level 1 with Z_FIXED (the same block types) and zlib level 1 with its
default strategy (dynamic codes), each on one core and on 16 processes of this
machine, and the unmask of a decode of a batch of the same sizes
(gevws_ctx_timing), which is what moving the bytes once costs.

Two shapes -- 16 384 messages of 4 KiB and 1 024 of 256 KiB -- times two
payloads: the word soup of tools/bench_inflate.py and random bytes (stored
blocks: the copy bound of this step).  A shape's messages cycle through eight
distinct payloads.  The decode and the deflate step alternate in one process;
the deflate step is timed by HIP events around its launches.  One JSON line
per (shape, payload), medians over the rounds.

--dynamic adds a leg with GEVWS_DEFLATE_DYNAMIC (dynamic-Huffman blocks where
they are smaller): the same shapes and payloads, the fixed-mode step and the
dynamic-mode step alternating in the same rounds, and a second line per case
with "mode": "dynamic" that carries the fixed-mode step of the same process
beside it and the sizes against both zlib yardsticks.

--takeover measures server context takeover instead (gevws_deflate_ctx_async):
the plain texts of tools/bench_inflate.py's takeover shape -- 16 384
connections x 8 messages of about 512 B, 64 distinct scripts -- compressed by
the takeover call (every connection keeps its window; the slots are zeroed
outside the timed span) and by the independent call on the same messages,
alternating in one process.  The yardstick is zlib level 1 with one persistent
compressobj a connection and Z_SYNC_FLUSH per message.  Two JSON lines with
"mode": "takeover".

Every line carries the SHA-256 of the payload bytes the step wrote; --root DIR
imports gev_amd from another checkout, so two builds can be compared (times and
digests) by the same tool in one session.

    python tools/bench_deflate.py [--rounds 7] [--warmup 2] [--shapes many,large] [--dynamic] [--commit ID]
                                  [--out FILE] [--root DIR]
    python tools/bench_deflate.py --takeover [--commit ID] [--out FILE]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_inflate import DISTINCT, SHAPES, TAIL, median, text  # noqa: E402
from bench_inflate import TAKEOVER_BYTES, TAKEOVER_CONNS, TAKEOVER_MSGS, TAKEOVER_SCRIPTS  # noqa: E402

ZLIB = {"zlib1_fixed": zlib.Z_FIXED, "zlib1_default": zlib.Z_DEFAULT_STRATEGY}


def zdeflate(data: bytes, strategy: int) -> bytes:
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
    return (c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH))[:-4]


def deflate_all(job):
    """zlib level 1 over `count` messages cycling through `plains`: (seconds, bytes out)."""
    plains, count, strategy = job
    t0 = time.perf_counter()
    total = 0
    for i in range(count):
        total += len(zdeflate(plains[i % len(plains)], strategy))
    return time.perf_counter() - t0, total


def cpu_baselines(plains, n: int, rounds: int, strategy: int):
    """Medians of the wall time zlib takes for the n messages: one core, and 16 processes sharing them."""
    import multiprocessing as mp
    one = median([deflate_all((plains, n, strategy))[0] for _ in range(rounds)])
    jobs = [(plains, n // 16 + (1 if k < n % 16 else 0), strategy) for k in range(16)]
    with mp.get_context("spawn").Pool(16) as pool:  # fresh interpreters: no GPU state in them
        pool.map(deflate_all, jobs)  # warm-up: the workers are up
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(deflate_all, jobs)
            walls.append(time.perf_counter() - t0)
    return one, median(walls)


def masked_frame(payload: bytes, key: bytes):
    import numpy as np
    L = len(payload)
    hdr = bytes([0x82]) + (bytes([0x80 | L]) if L <= 125 else bytes([0x80 | 126]) + L.to_bytes(2, "big") if L <= 0xFFFF
                           else bytes([0x80 | 127]) + L.to_bytes(8, "big")) + key  # FIN | binary, masked
    body = np.frombuffer(payload, np.uint8) ^ np.resize(np.frombuffer(key, np.uint8), L)
    return np.concatenate([np.frombuffer(hdr, np.uint8), body])


def emit(line, out):
    text_line = json.dumps(line)
    print(text_line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text_line + "\n")


def takeover_texts():
    """The plain texts of tools/bench_inflate.py --takeover: TAKEOVER_SCRIPTS scripts of TAKEOVER_MSGS messages."""
    import numpy as np
    rng = np.random.default_rng(0x74616B)
    return [[text(TAKEOVER_BYTES - 32 + int(rng.integers(0, 64)), rng) for _ in range(TAKEOVER_MSGS)]
            for _ in range(TAKEOVER_SCRIPTS)]


def zlib_chains(job):
    """zlib level 1 over `count` connections cycling through `scripts`: one persistent compressobj a
    connection, Z_SYNC_FLUSH per message; (seconds, wire bytes)."""
    scripts, count = job
    t0 = time.perf_counter()
    total = 0
    for i in range(count):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        for t in scripts[i % len(scripts)]:
            total += len(c.compress(t) + c.flush(zlib.Z_SYNC_FLUSH)) - 4
    return time.perf_counter() - t0, total


def zlib_chain_baselines(scripts, n: int, rounds: int):
    import multiprocessing as mp
    one = median([zlib_chains((scripts, n))[0] for _ in range(rounds)])
    jobs = [(scripts, n // 16 + (1 if k < n % 16 else 0)) for k in range(16)]
    with mp.get_context("spawn").Pool(16) as pool:  # fresh interpreters: no GPU state in them
        pool.map(zlib_chains, jobs)
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(zlib_chains, jobs)
            walls.append(time.perf_counter() - t0)
    return one, median(walls)


def takeover_main(args):
    import numpy as np
    texts = takeover_texts()
    n, per, ns = TAKEOVER_CONNS, TAKEOVER_MSGS, TAKEOVER_SCRIPTS
    assert n % ns == 0
    zlib_bytes = zlib_chains((texts, ns))[1] * (n // ns)
    cpu = None
    if not args.no_cpu:
        cpu = zlib_chain_baselines(texts, n, args.rounds)
        print(f"[bench_deflate] takeover zlib1 persistent: 1 core {cpu[0] * 1e3:.0f} ms, 16 processes "
              f"{cpu[1] * 1e3:.0f} ms", file=sys.stderr, flush=True)

    import torch

    import gev_amd

    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)
    r16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    # the step's input: a group of the 64 scripts' messages, each on a 16-byte boundary, n / 64 times
    group = b"".join(t + bytes(r16(len(t)) - len(t)) for s in texts for t in s)
    lens = np.array([len(t) for s in texts for t in s], np.uint64)
    offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.uint64)
    reps = n // ns
    src_bytes = len(group) * reps
    src = torch.empty(src_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
    src[:src_bytes].view(reps, len(group))[:] = torch.from_numpy(np.frombuffer(group, np.uint8).copy()).to(dev)
    nm = n * per
    rec = np.zeros(nm, gev_amd.DEFLATE_MSG_DTYPE)
    rec["payload_off"] = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(len(group)) + offs[None, :]).reshape(-1)
    rec["length"], rec["opcode"] = np.tile(lens, reps), 1
    plain_bytes = int(rec["length"].sum())
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1, 24).copy()).to(dev)
    d_conn = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), per)).to(dev)
    d_ext = torch.full((n,), gev_amd.EXT_DEFLATE | gev_amd.EXT_SERVER_TAKEOVER, dtype=torch.uint8, device=dev)
    d_ctx = torch.zeros((n, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
    out_cap = int(sum(r16(gev_amd.deflate_bound(int(x))) for x in lens)) * reps
    d_out = torch.empty(out_cap + gev_amd._abi.OUT_PAD, dtype=torch.uint8, device=dev)
    d_frames = torch.empty((nm, 32), dtype=torch.uint8, device=dev)
    dsum = torch.zeros(64, dtype=torch.uint8, device=dev)

    def step(takeover: bool):
        if takeover:
            eng.deflate_ctx_async(d_rec, nm, None, src, src_bytes, 0, d_frames, d_out, out_cap, dsum, d_conn, d_ext,
                                  d_ctx, n)
        else:
            eng.deflate_async(d_rec, nm, None, src, src_bytes, 0, d_frames, d_out, out_cap, dsum)

    def checked(takeover: bool):
        """(wire bytes, digest) after a run whose payloads a persistent / a fresh inflater reads back."""
        d_ctx.zero_()
        step(takeover)
        torch.cuda.synchronize()
        s = dsum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        assert (int(s["status"]), int(s["frames"]), int(s["errors"])) == (0, nm, 0), s
        fr = d_frames.cpu().numpy().reshape(-1).view(gev_amd.OUT_FRAME_DTYPE)
        for c in (0, 1, ns - 1, ns, n - 1):
            d = zlib.decompressobj(-15)
            slot = bytearray(gev_amd.DEF_CTX_BYTES)
            for k in range(per):
                i = c * per + k
                o, ln = int(fr["payload_off"][i]), int(fr["payload_len"][i])
                p = d_out[o:o + ln].cpu().numpy().tobytes()
                if not takeover:
                    d = zlib.decompressobj(-15)
                assert d.decompress(p + TAIL) == texts[c % ns][k], (c, k)
                want = gev_amd.deflate_raw_ctx(texts[c % ns][k], slot) if takeover else \
                    gev_amd.deflate_raw(texts[c % ns][k])
                assert p == want, (c, k)
            if takeover:
                assert d_ctx[c].cpu().numpy().tobytes() == bytes(slot), c
        digest = hashlib.sha256(d_out[:int(s["payload_bytes"])].cpu().numpy().tobytes()).hexdigest()
        return int(s["payload_len"]), digest

    variants = [("takeover", True), ("independent", False)]
    for _ in range(args.warmup):
        for _, tk in variants:
            step(tk)
    wire = {name: checked(tk) for name, tk in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):  # the two calls alternate; the slots are zeroed outside the timed span
        for name, tk in variants:
            d_ctx.zero_()
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            step(tk)
            e[1].record()
            torch.cuda.synchronize()
            times[name].append(e[0].elapsed_time(e[1]))
    for name, _ in variants:
        m = median(times[name])
        line = {"path": "deflate step, server context takeover (one wave per connection's chain) against the same "
                        "messages compressed independently (one wave per message)",
                "mode": "takeover", "variant": name, "commit": args.commit, "connections": n,
                "messages_per_connection": per, "messages": nm, "scripts": ns, "plain_bytes": plain_bytes,
                "wire_bytes": wire[name][0], "ratio": round(wire[name][0] / plain_bytes, 4),
                "wire_vs_independent": round(wire[name][0] / wire["independent"][0], 4),
                "payload_sha256": wire[name][1],
                "context_bytes": n * gev_amd.DEF_CTX_BYTES if name == "takeover" else 0,
                "deflate_ms": round(m, 4), "deflate_rounds_ms": [round(t, 4) for t in times[name]],
                "deflate_in_GBps": round(plain_bytes / m / 1e6, 3),
                "messages_per_s": round(nm / m * 1e3), "time_vs_independent": round(m / median(times["independent"]), 4),
                "zlib1_persistent_bytes": zlib_bytes, "wire_vs_zlib1_persistent": round(wire[name][0] / zlib_bytes, 4),
                "rounds": args.rounds, "warmup": args.warmup}
        if cpu:
            line.update({"zlib1_persistent_1core_ms": round(cpu[0] * 1e3, 2),
                         "zlib1_persistent_16proc_ms": round(cpu[1] * 1e3, 2),
                         "zlib1_persistent_16proc_in_GBps": round(plain_bytes / cpu[1] / 1e9, 3)})
        emit(line, args.out)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="many,large")
    ap.add_argument("--kinds", default="text,random")
    ap.add_argument("--no-cpu", action="store_true", help="skip the zlib baselines")
    ap.add_argument("--dynamic", action="store_true", help="also time the step with GEVWS_DEFLATE_DYNAMIC")
    ap.add_argument("--commit", default=None, help="recorded in every line")
    ap.add_argument("--out", default=None, help="append the lines to this file too")
    ap.add_argument("--takeover", action="store_true",
                    help="server context takeover against the independent call (16 384 x 8 x ~512 B)")
    ap.add_argument("--root", default=None, help="import gev_amd from this checkout (another build, same tool)")
    args = ap.parse_args()
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    if args.takeover:
        return takeover_main(args)
    import numpy as np

    rng = np.random.default_rng(0x646566)
    cases = []
    for shape in args.shapes.split(","):
        n, size = SHAPES[shape]
        for kind in args.kinds.split(","):
            plains = [text(size, rng) if kind == "text" else rng.integers(0, 256, size, dtype=np.uint8).tobytes()
                      for _ in range(DISTINCT)]
            cpu = {}
            for name, strategy in ZLIB.items():
                cpu[name] = {"bytes": sum(len(zdeflate(plains[i % DISTINCT], strategy)) for i in range(DISTINCT))
                             * (n // DISTINCT)}
                if not args.no_cpu:
                    cpu[name]["one"], cpu[name]["p16"] = cpu_baselines(plains, n, args.rounds, strategy)
                    print(f"[bench_deflate] {shape} {kind} {name}: 1 core {cpu[name]['one'] * 1e3:.0f} ms, "
                          f"16 processes {cpu[name]['p16'] * 1e3:.0f} ms", file=sys.stderr, flush=True)
            cases.append((shape, kind, n, size, plains, cpu))

    import torch

    import gev_amd

    dev = torch.device("cuda", 0)
    eng = gev_amd.Engine(0)
    for shape, kind, n, size, plains, cpu in cases:
        assert size % 16 == 0 and n % DISTINCT == 0
        # the step's input: the messages back to back, each on a 16-byte boundary
        src_bytes = n * size
        src = torch.empty(src_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        block = torch.from_numpy(np.frombuffer(b"".join(plains), np.uint8).copy()).to(dev)
        src[:src_bytes].view(n // DISTINCT, DISTINCT * size)[:] = block
        rec = np.zeros(n, gev_amd.DEFLATE_MSG_DTYPE)
        rec["payload_off"], rec["length"], rec["opcode"] = np.arange(n, dtype=np.uint64) * size, size, 2
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1, 24).copy()).to(dev)
        out_cap = n * ((gev_amd.deflate_bound(size) + 15) // 16 * 16)
        d_out = torch.empty(out_cap + gev_amd._abi.OUT_PAD, dtype=torch.uint8, device=dev)
        d_frames = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        dsum = torch.zeros(64, dtype=torch.uint8, device=dev)
        # a decode of masked frames of the same sizes: its unmask is the yardstick for moving the bytes
        frames = [masked_frame(p, bytes(rng.integers(1, 256, 4).astype("u1"))) for p in plains]
        lens = np.array([frames[i % DISTINCT].size for i in range(n)], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        in_bytes = int(lens.sum())
        arena = torch.zeros(in_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
        arena[:in_bytes] = torch.from_numpy(np.concatenate([frames[i % DISTINCT] for i in range(n)])).to(dev)
        conns = torch.from_numpy(np.stack([offs, lens], 1)).to(dev)
        out = eng.alloc_batch(n, n, n * size)

        def decode():
            eng.decode_async(arena, in_bytes, conns, n, out, n, n * size)

        def deflate(flags=0):
            eng.deflate_async(d_rec, n, None, src, src_bytes, flags, d_frames, d_out, out_cap, dsum)

        def checked(flags):
            """The step's compressed bytes after a run whose payloads inflate to the messages."""
            deflate(flags)
            torch.cuda.synchronize()
            s = dsum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
            assert (int(s["status"]), int(s["frames"]), int(s["errors"])) == (0, n, 0), s
            fr = d_frames.cpu().numpy().reshape(-1).view(gev_amd.OUT_FRAME_DTYPE)
            for i in (0, 1, DISTINCT - 1, n - 1):
                o, c = int(fr["payload_off"][i]), int(fr["payload_len"][i])
                p = d_out[o:o + c].cpu().numpy().tobytes()
                assert zlib.decompressobj(-15).decompress(p + TAIL) == plains[i % DISTINCT], i
            digest = hashlib.sha256(d_out[:int(s["payload_bytes"])].cpu().numpy().tobytes()).hexdigest()
            return int(s["payload_len"]), digest

        modes = [("fixed", 0)] + ([("dynamic", gev_amd.DEFLATE_DYNAMIC)] if args.dynamic else [])
        for _ in range(args.warmup):
            decode()
            for _, flags in modes:
                deflate(flags)
        comp = {name: checked(flags) for name, flags in modes}
        t_def, t_unmask = {name: [] for name, _ in modes}, []
        eng.set_timing(True)
        for _ in range(args.rounds):  # the decode and the step's modes alternate
            decode()
            for name, flags in modes:
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                deflate(flags)
                e[1].record()
                torch.cuda.synchronize()
                t_def[name].append(e[0].elapsed_time(e[1]))
            ms, calls = eng.timing()
            assert calls == 1
            t_unmask.append(ms[3])
        eng.set_timing(False)
        u = median(t_unmask)
        for name, _ in modes:
            m, comp_bytes = median(t_def[name]), comp[name][0]
            line = {
                "path": "deflate step (permessage-deflate outbound, one wave per message, compressed twice: size, emit)",
                "mode": name, "commit": args.commit,
                "shape": shape, "payload": kind, "messages": n, "message_bytes": size, "plain_bytes": n * size,
                "compressed_bytes": comp_bytes, "ratio": round(comp_bytes / (n * size), 4),
                "payload_sha256": comp[name][1],
                "deflate_ms": round(m, 4), "deflate_rounds_ms": [round(t, 4) for t in t_def[name]],
                "deflate_in_GBps": round(n * size / m / 1e6, 2), "deflate_out_GBps": round(comp_bytes / m / 1e6, 2),
                "unmask_ms": round(u, 4), "unmask_rounds_ms": [round(t, 4) for t in t_unmask],
                "unmask_read_plus_write_GBps": round(2 * n * size / u / 1e6, 1),
                "rounds": args.rounds, "warmup": args.warmup}
            if name != "fixed":  # the fixed-mode step of the same process beside it
                f = median(t_def["fixed"])
                line.update({"fixed_deflate_ms": round(f, 4), "fixed_compressed_bytes": comp["fixed"][0],
                             "time_vs_fixed": round(m / f, 4), "size_vs_fixed": round(comp_bytes / comp["fixed"][0], 4)})
            for zname, c in cpu.items():
                line[f"{zname}_bytes"] = c["bytes"]
                line[f"size_vs_{zname}"] = round(comp_bytes / c["bytes"], 4)
                if "one" in c:
                    line.update({f"{zname}_1core_ms": round(c["one"] * 1e3, 2),
                                 f"{zname}_1core_in_GBps": round(n * size / c["one"] / 1e9, 3),
                                 f"{zname}_16proc_ms": round(c["p16"] * 1e3, 2),
                                 f"{zname}_16proc_in_GBps": round(n * size / c["p16"] / 1e9, 3)})
            emit(line, args.out)
        del src, d_out, d_frames, arena, out
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
