"""GPU checks of the deflate step (gevws_deflate_async): outbound messages
compressed on the device.  Every comparison is exact: a payload is the bytes
gevws_deflate_raw (the host twin, pinned on the CPU in tests/test_deflate_host.py)
gives for the same message, zlib inflates it to the input, and the records,
the layout of d_out and the summary are as include/gevws.h states them.  The
source arenas have 0xFF in every pad byte, so a byte read past `length` that
counted would change the payload; d_out and the records are filled with 0xEE
first, so a byte written that should not be shows."""
import functools
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _inflate_corpus as ic

pytestmark = pytest.mark.gpu

T, B = 1, 2
TAIL = b"\x00\x00\xff\xff"
FILL = 0xEE
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 70000,
         300000]


@functools.lru_cache(maxsize=None)
def host(data: bytes, wb: int = 0) -> bytes:
    return gev_amd.deflate_raw(data, wb)


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


def build(msgs):
    """(arena with 0xFF pads and IN_PAD bytes of 0xFF behind, src_bytes, records) for [(bytes, opcode, wb)]."""
    rec = np.zeros(len(msgs), gev_amd.DEFLATE_MSG_DTYPE)
    parts, off = [], 0
    for i, (data, op, wb) in enumerate(msgs):
        rec[i]["payload_off"], rec[i]["length"], rec[i]["opcode"], rec[i]["window_bits"] = off, len(data), op, wb
        parts.append(data + b"\xff" * (r16(len(data)) - len(data)))
        off += r16(len(data))
    arena = np.frombuffer(b"".join(parts) + b"\xff" * gev_amd.IN_PAD, np.uint8).copy()
    return arena, off, rec


def run(engine, arena, src_bytes, rec, out_cap, flags=0, prev=None, max_msgs=None):
    """One gevws_deflate_async call on fresh 0xEE-filled outputs; everything back on the host."""
    import torch
    dev = torch.device("cuda", engine.device)
    n = rec.shape[0] if max_msgs is None else max_msgs
    d_src = torch.from_numpy(arena).to(dev)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 24).copy()).to(dev) \
        if rec.shape[0] else torch.zeros((1, 24), dtype=torch.uint8, device=dev)
    frames = torch.full((max(rec.shape[0], 1), 32), FILL, dtype=torch.uint8, device=dev)
    out = torch.full((out_cap + gev_amd._abi.OUT_PAD,), FILL, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    d_prev = None
    if prev is not None:
        s = np.zeros(1, gev_amd.SUMMARY_DTYPE)
        s["frames"], s["status"] = prev
        d_prev = torch.from_numpy(s.view(np.uint8).copy()).to(dev)
    engine.deflate_async(d_rec, n, d_prev, d_src, src_bytes, flags, frames, out, out_cap, summ)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0],
                frames=frames.cpu().numpy().reshape(-1).view(gev_amd.OUT_FRAME_DTYPE), out=out.cpu().numpy(),
                dev=dict(frames=frames, out=out, summary=summ))


def check(got, msgs, want_payloads, plain=None):
    """Records, layout, pads, sentinel and summary of a call that fitted."""
    n = len(msgs)
    s, fr, out = got["summary"], got["frames"], got["out"]
    assert int(s["status"]) == gev_amd.OK and int(s["errors"]) == 0 and int(s["frames"]) == n
    off = 0
    for i, ((data, op, wb), want) in enumerate(zip(msgs, want_payloads)):
        f = fr[i]
        c = len(want)
        is_plain = bool(plain[i]) if plain is not None else False
        assert (int(f["fin"]), int(f["rsv"]), int(f["opcode"]), int(f["masked"])) == (1, 0 if is_plain else 4, op, 0), i
        assert not f["mask"].any() and int(f["length"]) == c and int(f["payload_len"]) == c, (i, len(data), wb)
        assert int(f["payload_off"]) == off and off % 16 == 0, i
        assert out[off:off + c].tobytes() == want, (i, len(data), wb)
        assert not out[off + c:off + r16(c)].any(), i
        off += r16(c)
    assert int(s["payload_bytes"]) == off and int(s["payload_len"]) == sum(len(w) for w in want_payloads)
    assert np.all(out[off:] == FILL)
    assert np.all(fr[n:].view(np.uint8) == FILL)


def untouched(got):
    return np.all(got["out"] == FILL) and np.all(got["frames"].view(np.uint8) == FILL)


@pytest.fixture(scope="module")
def corpus():
    """[(bytes, opcode, window_bits)] over SIZES: all four kinds up to 4 097, two (rotating) above."""
    rng = np.random.default_rng(0x6465666C)
    msgs, k = [], 0
    for n in SIZES:
        kinds = range(4) if n <= 4097 else ((k % 4), (k + 1) % 4)
        for kind in kinds:
            msgs.append((ic.sample(rng, n, kind), T if kind in (2, 3) else B, 0))
        k += 1
    return msgs


def test_sizes_and_kinds(engine, corpus):
    arena, src_bytes, rec = build(corpus)
    want = [host(d, wb) for d, _, wb in corpus]
    for (d, _, _), w in zip(corpus, want):
        assert zlib.decompressobj(-15).decompress(w + TAIL) == d
        assert len(w) <= gev_amd.deflate_bound(len(d))
    need = sum(r16(len(w)) for w in want)
    got = run(engine, arena, src_bytes, rec, need + 4096)
    check(got, corpus, want)
    assert sorted(set(int(x) for x in rec["length"])) == sorted(SIZES)


def test_window_bits_in_one_batch(engine):
    text = ic.sample(np.random.default_rng(70), 70000, 0)
    period = np.random.default_rng(71).integers(0, 256, 3000, dtype=np.uint8).tobytes() * 8
    msgs = [(text, T, 9), (text, T, 12), (text, T, 15), (period, B, 8), (period, B, 11), (period, B, 12),
            (period, B, 0)]
    arena, src_bytes, rec = build(msgs)
    want = [host(d, wb) for d, _, wb in msgs]
    for (d, _, wb), w in zip(msgs, want):
        if wb != 8:  # (zlib's raw inflate may not open with 8; the host test says which)
            assert zlib.decompressobj(-(wb or 15)).decompress(w + TAIL) == d
    assert len(want[4]) > len(period) > 4 * len(want[5])  # a 3 000-byte period: out of reach of 2^11, inside 2^12
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want))
    check(got, msgs, want)


def test_alone_and_as_entry_37_of_64(engine):
    rng = np.random.default_rng(0x3337)
    sizes = [int(x) for x in rng.choice([0, 1, 5, 64, 100, 300, 1000, 4096, 5000, 9000, 20000], 64)]
    msgs = [(ic.sample(rng, n, int(rng.integers(0, 4))), B, int(rng.choice([0, 9, 10, 15]))) for n in sizes]
    mine = (ic.sample(rng, 13001, 0), T, 10)
    msgs[37] = mine
    arena, src_bytes, rec = build(msgs)
    want = [host(d, wb) for d, _, wb in msgs]
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want))
    check(got, msgs, want)
    a1, n1, r1 = build([mine])
    a1[n1 - (r16(13001) - 13001):n1] = 0x00  # another pad behind it, too
    alone = run(engine, a1, n1, r1, r16(len(want[37])))
    check(alone, [mine], [want[37]])
    f = got["frames"][37]
    assert alone["out"][:len(want[37])].tobytes() == \
        got["out"][int(f["payload_off"]):int(f["payload_off"]) + int(f["payload_len"])].tobytes()


def test_plain_if_not_smaller(engine):
    rng = np.random.default_rng(0x706C)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    msgs = [(rnd(1000), B, 0), (b"", T, 0), (ic.sample(rng, 1000, 0), T, 0), (rnd(5000), B, 0), (b"abc", T, 0),
            (ic.sample(rng, 70000, 2), T, 12), (rnd(17), B, 9)]
    comp = [host(d, wb) for d, _, wb in msgs]
    plain = [len(c) >= len(d) for (d, _, _), c in zip(msgs, comp)]
    assert plain == [True, True, False, True, True, False, True]
    want = [d if p else c for (d, _, _), c, p in zip(msgs, comp, plain)]
    arena, src_bytes, rec = build(msgs)
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want),
              flags=gev_amd.DEFLATE_PLAIN_IF_NOT_SMALLER)
    check(got, msgs, want, plain)
    # without the flag everything is compressed
    got = run(engine, arena, src_bytes, rec, sum(r16(len(c)) for c in comp))
    check(got, msgs, comp)


def test_capacity_then_retry(engine):
    rng = np.random.default_rng(0x636170)
    msgs = [(ic.sample(rng, n, k), B, 0) for n, k in ((100, 0), (0, 0), (5000, 1), (777, 2), (16, 1))]
    want = [host(d) for d, _, _ in msgs]
    need = sum(r16(len(w)) for w in want)
    arena, src_bytes, rec = build(msgs)
    short = run(engine, arena, src_bytes, rec, need - 1)
    s = short["summary"]
    assert int(s["status"]) == gev_amd.ERR_CAPACITY and int(s["payload_bytes"]) == need and int(s["errors"]) == 0
    assert untouched(short)
    full = run(engine, arena, src_bytes, rec, need)
    check(full, msgs, want)
    # Engine.deflate retries by itself
    import torch
    res = engine.deflate(rec, torch.from_numpy(arena).to(torch.device("cuda", engine.device)), src_bytes, out_cap=16)
    assert [res.payload(i) for i in range(len(msgs))] == want
    assert res.frames_host().tobytes() == full["frames"].tobytes()


def test_malformed_records(engine):
    rng = np.random.default_rng(0x626164)
    msgs = [(ic.sample(rng, n, 0), B, 0) for n in (100, 200, 300, 400, 500, 600)]
    arena, src_bytes, rec = build(msgs)
    bad = {
        "opcode 0": ("opcode", 0), "opcode 9": ("opcode", 9), "window_bits 7": ("window_bits", 7),
        "window_bits 16": ("window_bits", 16), "unaligned": ("payload_off", int(rec[2]["payload_off"]) + 8),
        "past the end": ("payload_off", r16(src_bytes)), "too long": ("length", src_bytes),
        "above 2^32 - 1": ("length", 2 ** 32), "wraps": ("length", 2 ** 64 - 16),
    }
    for name, (field, value) in bad.items():
        r = rec.copy()
        r[2][field] = value
        got = run(engine, arena, src_bytes, r, 4096)
        s = got["summary"]
        assert int(s["status"]) == gev_amd.ERR_INVALID and int(s["errors"]) == 1, name
        assert int(s["frames"]) == 0 and int(s["payload_bytes"]) == 0 and int(s["payload_len"]) == 0, name
        assert untouched(got), name
    r = rec.copy()
    for i, (field, value) in enumerate(list(bad.values())[:5]):
        r[i][field] = value if field != "payload_off" else int(r[i]["payload_off"]) + 4
    got = run(engine, arena, src_bytes, r, 4096)
    assert int(got["summary"]["status"]) == gev_amd.ERR_INVALID and int(got["summary"]["errors"]) == 5
    assert untouched(got)
    # the last byte of the arena is still in range
    r = rec.copy()
    r[5]["length"] = src_bytes - int(r[5]["payload_off"])
    assert int(run(engine, arena, src_bytes, r, 8192)["summary"]["status"]) == gev_amd.OK


def test_count_follows_the_previous_step(engine):
    rng = np.random.default_rng(0x70726576)
    msgs = [(ic.sample(rng, n, 0), T, 0) for n in (50, 1500, 7, 300, 20)]
    want = [host(d) for d, _, _ in msgs]
    arena, src_bytes, rec = build(msgs)
    got = run(engine, arena, src_bytes, rec, 4096, prev=(3, gev_amd.OK))
    check(got, msgs[:3], want[:3])
    got = run(engine, arena, src_bytes, rec, 4096, prev=(9, gev_amd.OK))  # no more than max_msgs
    check(got, msgs, want)
    for prev, max_msgs in (((5, gev_amd.ERR_CAPACITY), 5), ((0, gev_amd.OK), 5), (None, 0)):
        got = run(engine, arena, src_bytes, rec, 4096, prev=prev, max_msgs=max_msgs)
        assert not got["summary"].tobytes().strip(b"\0"), (prev, max_msgs)
        assert untouched(got)


def test_closed_loop_on_the_device(engine):
    """deflate -> encode (unmasked, as a server sends) -> decode -> message pass
    with every connection EXT_DEFLATE -> inflate: the original messages."""
    import torch
    rng = np.random.default_rng(0x6C6F6F70)
    dev = torch.device("cuda", engine.device)
    utf8 = lambda b: b.decode("utf-8", "ignore").encode()  # noqa: E731
    groups = [  # one connection each; a frame needs six bytes at hand to be decoded, so each ends with a big one
        [(utf8(ic.sample(rng, 1000, 0)), T), (b"", T), (ic.sample(rng, 300, 1), B), (b"a", T),
         (utf8(ic.sample(rng, 70000, 0)), T)],
        [(ic.sample(rng, 5000, 1), B), (ic.sample(rng, 4096, 3), T), (ic.sample(rng, 33000, 2), T)],
        [(ic.sample(rng, 70000, 1), B)],
    ]
    flat = [(d, op, int(rng.choice([0, 10, 15]))) for g in groups for d, op in g]
    arena, src_bytes, rec = build(flat)
    want = [host(d, wb) for d, _, wb in flat]
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want))
    check(got, flat, want)
    n = len(flat)
    # the records and d_out go to the encoder as they stand
    wire_cap = sum(len(w) + 10 for w in want)
    wire = torch.full((wire_cap + gev_amd._abi.OUT_PAD,), FILL, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(n, dtype=torch.int64, device=dev)
    esum = torch.zeros(64, dtype=torch.uint8, device=dev)
    engine.encode_async(got["dev"]["frames"], n, got["dev"]["out"], wire, wire_cap, out_off, esum)
    torch.cuda.synchronize(engine.device)
    es = esum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
    assert int(es["status"]) == gev_amd.OK
    total = int(es["payload_bytes"])
    wire_host = wire[:total].cpu().numpy().tobytes()
    offs = [int(x) for x in out_off.cpu().numpy()] + [total]
    # the oracle's frame parser on the wire bytes: FIN, RSV1, unmasked, the lengths
    res = wo.decode_stream(wire_host + b"\0" * 8)
    assert len(res.frames) >= n
    for i, (fr, (d, op, _), w) in enumerate(zip(res.frames, flat, want)):
        h = fr.header
        assert (h.fin, h.rsv, h.opcode, h.masked, h.length) == (True, 4, op, False, len(w)), i
        assert fr.stream_pos == offs[i] and fr.payload == w, i
    # back in: one connection per group
    table, k = [], 0
    for g in groups:
        table.append((offs[k], offs[k + len(g)] - offs[k]))
        k += len(g)
    from tests._helpers import gpu_decode
    out = gpu_decode(engine, np.frombuffer(wire_host, np.uint8).copy(), np.array(table, np.int64))
    assert int(out.summary_host()["frames"]) == n
    conn_ext = torch.full((len(groups),), gev_amd.EXT_DEFLATE, dtype=torch.uint8, device=dev)
    state = torch.zeros((len(groups), 8), dtype=torch.uint8, device=dev)
    msgs = engine.messages(out, state=state, conn_ext=conn_ext)
    m = msgs.messages_host()
    assert m.shape[0] == n and np.all(m["flags"] & gev_amd.MSG_COMPRESSED != 0)
    assert [int(x) for x in m["opcode"]] == [op for _, op, _ in flat]
    inf = engine.inflate(out, msgs, 1 << 20, state=state)
    s = inf.summary_host()
    assert int(s["frames"]) == n and int(s["errors"]) == 0
    for i, (d, _, _) in enumerate(flat):
        assert inf.message_bytes(i) == d, i
    assert not state.cpu().numpy().any()
