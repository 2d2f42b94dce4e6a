"""GPU checks of client context takeover (gevws_inflate_ctx_async): the inflate
step with a 32 KiB window per connection, carried between messages and
between passes in caller-owned slots.  Through the C ABI on hand-built decoded
batches; every comparison is exact.

The oracle for message k of a chain is "the window as stored blocks, then the
payload" under the no-takeover rules (tests/_inflate_takeover.py: zlib's bytes,
the Python model's verdicts); the slots are compared byte for byte with the
model's image and with what gevws_inflate_raw_ctx leaves on the host.  Chains
come from one persistent zlib compressor, Z_SYNC_FLUSH per message, and every
chain of two or more messages is asserted to hold one that an empty window
rejects or decodes differently.  Slots of connections without the takeover bit
are filled with 0x5A and must come back untouched."""
import zlib

import numpy as np
import pytest

import gev_amd
from tests import _inflate_corpus as ic
from tests import _inflate_gpu_model as gm
from tests import _inflate_model as im
from tests import _inflate_takeover as tk
from tests import _messages_model as mm
from tests import _takeover_far as far

pytestmark = pytest.mark.gpu

T, B, C, PING = 1, 2, 0, 9
RSV1 = 4
BIG = 1 << 24
PLAIN, DEFLATE, TAKE = 0, 1, 3
ping = (1, 0, PING, b"hb")


def frames_of(payload: bytes, op: int = B, cuts=(), between=None, rsv=RSV1):
    edges = [0, *cuts, len(payload)]
    out = []
    for i in range(len(edges) - 1):
        last = i == len(edges) - 2
        out.append((1 if last else 0, rsv if i == 0 else 0, op if i == 0 else C, payload[edges[i]:edges[i + 1]]))
        if between is not None and not last:
            out.append(between)
    return out


def ascii_text(rng, n: int) -> bytes:
    return bytes(rng.integers(0x20, 0x7F, n, dtype=np.uint8))


class Conn:
    """One connection's messages: (frames, compressed payload or None, data)."""

    def __init__(self, ext):
        self.ext, self.msgs = ext, []

    def add(self, frames, payload=None, data=b""):
        self.msgs.append((frames, payload, data))

    def frames(self, lo=0, hi=None):
        return [f for fr, _, _ in self.msgs[lo:hi] for f in fr]


def assert_chain_needs_its_window(conn: Conn):
    comp = [(p, d) for _, p, d in conn.msgs if p is not None]
    if conn.ext == TAKE and len(comp) >= 2:
        assert any(tk.empty_window_differs(p, d) for p, d in comp[1:])


def device_slots(engine, slots, ext):
    """The model's slots on the device; those of connections without the
    takeover bit filled with 0x5A (never read, never written)."""
    import torch
    ctx = tk.slots_to_device(slots, torch.device("cuda", engine.device))
    for c, e in enumerate(ext):
        if not e & tk.EXT_TAKEOVER:
            ctx[c] = 0x5A
    return ctx


def run_pass(engine, conns, ext, ctx, slots, limit=BIG, out_cap=None, state=None, tag=""):
    """Message pass + gevws_inflate_ctx_async on hand-built connections, both
    compared with the model; `slots` (the model's) is updated, `ctx` (the
    device's) must then hold the same bytes.  Returns (device, model)."""
    d = mm.Decoded(conns, pad=0xFF)
    ext = np.asarray(ext, np.uint8)
    got = gm.run_messages_ext(engine, d, ext, state)
    want = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, state, ext)
    mm.assert_tables_equal(got, want, tag)
    winf = tk.model_inflate_ctx(d, want, limit, want["state"], ext, slots)
    cap = winf["payload_bytes"] if out_cap is None else out_cap
    ginf = tk.run_inflate_ctx(engine, got, limit, cap, ext, ctx)
    gm.assert_inflated(ginf, winf, cap, tag)
    assert_slots(ctx, slots, ext, tag)
    ginf["tables"] = got
    return ginf, winf


def assert_slots(ctx, slots, ext, tag=""):
    dev = tk.slots_from_device(ctx)
    for c, e in enumerate(ext):
        if e & tk.EXT_TAKEOVER:
            assert dev[c] == slots[c].image(), (tag, "slot", c)
        else:
            assert dev[c] == b"\x5A" * tk.CTX_BYTES, (tag, "slot of a connection without takeover touched", c)


def host_slot(conn: Conn, limit=1 << 17) -> bytes:
    """The slot gevws_inflate_raw_ctx leaves after the connection's compressed messages."""
    ctx = bytearray(tk.CTX_BYTES)
    for _, p, _ in conn.msgs:
        if p is not None:
            gev_amd.inflate_raw_ctx(p, limit, ctx)
    return bytes(ctx)


def message_bytes(ginf, winf):
    """The inflated bytes per connection, in order, from the device's own records."""
    per = {}
    inf, out, msgs = ginf["inflated"], ginf["out"], ginf["tables"]["messages"]
    for m in range(inf.shape[0]):
        if int(inf["flags"][m]) == gm.INF_DONE:
            o, n = int(inf["out_off"][m]), int(inf["length"][m])
            per.setdefault(int(msgs["conn"][m]), []).append((int(inf["status"][m]), out[o:o + n].tobytes()))
    return per


# ---------------------------------------------------------------------------- the mixed batch of tests 1, 2 and 5
def mixed_batch(seed=0x6D6978, n_conns=150):
    rng = np.random.default_rng(seed)
    combos = [(lv, sg) for lv in (1, 6, 9) for sg in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED)]
    conns = []
    for c in range(n_conns):
        ext = (TAKE, DEFLATE, PLAIN)[c % 3] if c >= 12 else TAKE
        conn = Conn(ext)
        n_msgs = c + 1 if c < 12 else int(rng.integers(1, 13))             # 1 .. 12 messages
        level, strategy = combos[c % len(combos)]
        comp = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        prev, ncomp = b"", 0
        for j in range(n_msgs):
            kind = int(rng.integers(0, 8))
            # connections alternate: ASCII content as text or binary messages, or any bytes as binary ones
            text = kind % 2 == 0 and c % 2 == 0
            n = int(rng.choice([0, 1, 15, 16, 17, 300, 300, 1000, 3000])) if c % 10 else int(rng.choice([300, 9000]))
            if (kind == 7 and j) or ext == PLAIN:                          # an uncompressed message in between
                data = ascii_text(rng, min(n, 200))
                cuts = [len(data) // 2] if j % 2 else []
                conn.add(frames_of(data, T, cuts, ping if j % 4 == 1 else None, rsv=0))
                continue
            if ncomp < 2:                                                  # the first two share bytes for certain
                n = max(n, 300)
            fresh = ascii_text(rng, n) if c % 2 == 0 else ic.sample(rng, n, int(rng.integers(0, 4)))
            data = (prev[: n // 2] + fresh)[:n] if ncomp else fresh        # half of it seen before
            if ncomp and n >= 16:
                data = prev[-40:] + data[40:]
            ncomp += 1
            if ext == TAKE:
                s = comp.compress(data) + comp.flush(zlib.Z_SYNC_FLUSH)
                payload = s[:-4]
            else:
                payload = ic.deflate(data, level, strategy)
            k = int(rng.integers(0, 4))
            cuts = sorted(int(x) for x in rng.integers(0, len(payload) + 1, k)) if j % 3 == 0 else []
            conn.add(frames_of(payload, T if text else B, cuts, ping if cuts and j % 2 else None), payload, data)
            prev = data if len(data) >= 16 else prev
        assert_chain_needs_its_window(conn)
        conns.append(conn)
    # an empty message on a takeover connection, text and binary, between two that share their bytes
    conn = Conn(TAKE)
    payloads = tk.chain([b"shared bytes " * 20, b"", b"shared bytes " * 20, b""])
    assert payloads[1] == b"\x00"
    for p, data, op in zip(payloads, [b"shared bytes " * 20, b"", b"shared bytes " * 20, b""], (T, T, B, B)):
        conn.add(frames_of(p, op), p, data)
    assert_chain_needs_its_window(conn)
    conns.append(conn)
    return conns


def expected_data(conn: Conn):
    return [d for _, p, d in conn.msgs if p is not None]


# ---------------------------------------------------------------------------- 1. one batch
def test_one_batch_with_takeover_deflate_and_plain_connections(engine):
    conns = mixed_batch()
    ext = [c.ext for c in conns]
    assert {TAKE, DEFLATE, PLAIN} <= set(ext) and sum(len(f[3]) for c in conns for f in c.frames()) < 2 << 20
    slots = [tk.Slot() for _ in conns]
    ctx = device_slots(engine, slots, ext)
    state = np.zeros(len(conns), mm.MSG_STATE_DTYPE)
    ginf, winf = run_pass(engine, [c.frames() for c in conns], ext, ctx, slots, state=state)
    assert winf["errors"] == 0 and winf["frames"] > 300
    per = message_bytes(ginf, winf)
    dev = tk.slots_from_device(ctx)
    for c, conn in enumerate(conns):
        if conn.ext != PLAIN:
            assert [b for _, b in per.get(c, [])] == expected_data(conn), c
        if conn.ext == TAKE:
            assert dev[c] == host_slot(conn), c                            # the host's slot, byte for byte
    assert not ginf["state"].view(np.uint8).any()


# ---------------------------------------------------------------------------- 2. three passes
def test_three_passes_with_the_slots_carried(engine):
    conns = mixed_batch(0x337061, 90)
    ext = [c.ext for c in conns]
    rng = np.random.default_rng(3)
    one_slots = [tk.Slot() for _ in conns]
    one_ctx = device_slots(engine, one_slots, ext)
    ginf, winf = run_pass(engine, [c.frames() for c in conns], ext, one_ctx, one_slots, tag="one batch")
    whole = message_bytes(ginf, winf)
    slots = [tk.Slot() for _ in conns]
    ctx = device_slots(engine, slots, ext)
    cuts = [sorted(int(x) for x in rng.integers(0, len(c.msgs) + 1, 2)) for c in conns]
    parts = {}
    for p in range(3):
        frames = [c.frames(([0] + k)[p], (k + [None])[p]) for c, k in zip(conns, cuts)]
        g, w = run_pass(engine, frames, ext, ctx, slots, tag=f"pass {p}")
        for c, got in message_bytes(g, w).items():
            parts.setdefault(c, []).extend(got)
    assert parts == whole
    assert tk.slots_from_device(ctx) == tk.slots_from_device(one_ctx)


# ---------------------------------------------------------------------------- 3. window edges
def edge_conns():
    rng = np.random.default_rng(0x656467)
    conns = []
    datas = tk.wrap_chain(rng)
    for level in (1, 9):
        conn = Conn(TAKE)
        for p, d in zip(tk.chain(datas, level), datas):
            conn.add(frames_of(p, B, [len(p) // 3] if len(p) > 3000 else []), p, d)
        assert tk.empty_window_differs(conn.msgs[-1][1], datas[-1])
        conns.append(conn)
    for n in (32768, 32767, 40000):                                        # distance 32 768 behind n bytes
        payloads, ds, status = tk.history_and_match(rng, n)
        conn = Conn(TAKE)
        for p, d in zip(payloads, ds):
            conn.add(frames_of(p, B), p, d)
        assert tk.zlib_inflate_dict(ds[0][-tk.WIN:], payloads[1]) == (status != im.OK, ds[1])
        conn.status = status
        conns.append(conn)
    return conns


def check_edges(per, conns):
    for c, conn in enumerate(conns):
        want = [(im.OK, d) for d in expected_data(conn)]
        if getattr(conn, "status", im.OK) != im.OK:
            want[-1] = (im.ERR_DEFLATE, b"")
        assert per[c] == want, c


def test_window_edges_in_one_batch_and_across_a_pass_boundary(engine):
    conns = edge_conns()
    ext = [TAKE] * len(conns)
    slots = [tk.Slot() for _ in conns]
    ctx = device_slots(engine, slots, ext)
    ginf, winf = run_pass(engine, [c.frames() for c in conns], ext, ctx, slots, tag="one batch")
    check_edges(message_bytes(ginf, winf), conns)
    assert [int(s.broken) for s in slots] == [0, 0, 0, im.ERR_DEFLATE, 0]
    assert slots[0].total == 119917 and slots[2].total == 32771
    one = tk.slots_from_device(ctx)
    assert [one[c] for c in range(len(conns))] == [host_slot(c) for c in conns]
    # the last message of every chain in a pass of its own
    slots = [tk.Slot() for _ in conns]
    ctx = device_slots(engine, slots, ext)
    g1, w1 = run_pass(engine, [c.frames(0, -1) for c in conns], ext, ctx, slots, tag="first pass")
    g2, w2 = run_pass(engine, [c.frames(-1) for c in conns], ext, ctx, slots, tag="second pass")
    per = message_bytes(g1, w1)
    for c, got in message_bytes(g2, w2).items():
        per[c] = per[c] + got
    check_edges(per, conns)
    assert tk.slots_from_device(ctx) == one


# ---------------------------------------------------------------------------- 4. failures in mid-chain
def test_a_failure_in_mid_chain_loses_the_context(engine):
    rng = np.random.default_rng(0x6661696C)
    texts = [ascii_text(rng, 300) for _ in range(3)]
    datas = [texts[0], texts[1], texts[0] + texts[1], texts[2] + texts[0], texts[1]]
    bad = b"\x06garbage"
    assert im.inflate(bad)[0] == im.ERR_DEFLATE
    LIMIT = 500
    conns = []
    p = tk.chain(datas)
    conn = Conn(TAKE)                                                      # 0: DEFLATE in the middle
    for j, op in ((0, T), (1, B)):
        conn.add(frames_of(p[j], op), p[j], datas[j])
    conn.add(frames_of(bad, B), bad, b"")
    conn.add([(1, 0, T, b"a plain message")])
    for j in (2, 3):
        conn.add(frames_of(p[j], B), p[j], b"")
    conns.append(conn)
    conn = Conn(TAKE)                                                      # 1: a neighbour that is fine
    for j in range(5):
        conn.add(frames_of(p[j], T), p[j], datas[j])
    assert tk.empty_window_differs(p[2], datas[2]) and len(datas[2]) > LIMIT
    conns.append(conn)
    conn = Conn(TAKE)                                                      # 2: TOO_BIG in the middle
    q = tk.chain([texts[0][:200], texts[0] * 2, texts[1][:100], texts[2][:50]])
    assert tk.empty_window_differs(q[1], texts[0] * 2)
    for j in range(4):
        conn.add(frames_of(q[j], B), q[j], b"")
    conns.append(conn)
    conn = Conn(DEFLATE)                                                   # 3: without takeover the later ones inflate
    for part in (ic.deflate(texts[0]), bad, ic.deflate(texts[1])):
        conn.add(frames_of(part, B), part, b"")
    conns.append(conn)
    latin = [b"caf\xe9 " * 30, b"caf\xe9 " * 30 + b"ok", b"plain ascii"]   # 4: a UTF-8 failure keeps the chain
    u = tk.chain(latin)
    assert tk.empty_window_differs(u[1], latin[1])
    conn = Conn(TAKE)
    for part, d, op in zip(u, latin, (T, B, T)):
        conn.add(frames_of(part, op), part, d)
    conns.append(conn)
    ext = [c.ext for c in conns]
    slots = [tk.Slot() for _ in conns]
    ctx = device_slots(engine, slots, ext)
    state = np.zeros(len(conns), mm.MSG_STATE_DTYPE)
    # conn 1's third message is 600 bytes: it would be TOO_BIG under LIMIT, so conn 1 runs in the BIG pass below
    frames = [c.frames() for c in conns]
    frames[1] = []
    ginf, winf = run_pass(engine, frames, ext, ctx, slots, limit=LIMIT, state=state, tag="failures")
    per = message_bytes(ginf, winf)
    D, TB = im.ERR_DEFLATE, im.ERR_TOO_BIG
    assert per[0] == [(0, datas[0]), (0, datas[1]), (D, b""), (D, b""), (D, b"")]
    assert per[2] == [(0, texts[0][:200]), (TB, b""), (TB, b""), (TB, b"")]
    assert per[3] == [(0, texts[0]), (D, b""), (0, texts[1])]
    assert per[4] == [(mm.ERR_UTF8, latin[0]), (0, latin[1]), (0, latin[2])]
    assert [int(x) for x in ginf["state"]["failed"]] == [D, 0, TB, D, mm.ERR_UTF8]
    assert int(ginf["summary"]["errors"]) == 3 + 3 + 1 + 1
    assert [s.broken for s in slots] == [D, 0, TB, 0, 0] and [s.total for s in slots[:3]] == [600, 0, 200]
    # the next pass: the sticky status, nothing decoded; the neighbour's chain goes on from its window
    nxt = [frames_of(ic.deflate(b"valid on its own"), B), conns[1].frames(), frames_of(ic.deflate(b"so is this"), T),
           [], frames_of(tk.chain(latin + [latin[1]])[3], B)]
    ginf, winf = run_pass(engine, nxt, ext, ctx, slots, tag="after the failures")
    per = message_bytes(ginf, winf)
    assert per[0] == [(D, b"")] and per[2] == [(TB, b"")]
    assert per[1] == [(0, d) for d in datas] and per[4] == [(0, latin[1])]
    assert [int(x) for x in ginf["state"]["failed"]] == [D, 0, TB, 0, 0]


# ---------------------------------------------------------------------------- 5. capacity
def test_capacity_leaves_the_slots_untouched_then_the_retry_fits(engine):
    conns = mixed_batch(0x636170, 40)
    ext = [c.ext for c in conns]
    slots = [tk.Slot() for _ in conns]
    ctx = device_slots(engine, slots, ext)
    half = [c.frames(0, len(c.msgs) // 2) for c in conns]
    run_pass(engine, half, ext, ctx, slots, tag="first half")              # slots with something in them
    rest = [c.frames(len(c.msgs) // 2) for c in conns]
    d = mm.Decoded(rest, pad=0xFF)
    e = np.asarray(ext, np.uint8)
    got = gm.run_messages_ext(engine, d, e)
    want = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, None, e)
    after = [s.copy() for s in slots]
    winf = tk.model_inflate_ctx(d, want, BIG, want["state"], e, after)
    need = winf["payload_bytes"]
    before = ctx.clone()
    state_before = got["dev"]["state"].cpu().numpy().copy()
    short = tk.run_inflate_ctx(engine, got, BIG, need - 1, e, ctx)
    s = short["summary"]
    assert int(s["status"]) == gev_amd.ERR_CAPACITY and int(s["payload_bytes"]) == need
    assert np.all(short["out"] == 0xEE) and np.all(short["inflated"].view(np.uint8) == 0xEE)
    assert bool((ctx == before).all()) and np.array_equal(got["dev"]["state"].cpu().numpy(), state_before)
    gm.assert_inflated(tk.run_inflate_ctx(engine, got, BIG, need, e, ctx), winf, need)
    assert_slots(ctx, after, ext)
    assert any(a.total != b.total for a, b in zip(after, slots))


# ---------------------------------------------------------------------------- 6. PENDING
def test_messages_that_are_not_whole_stop_the_chain(engine):
    rng = np.random.default_rng(0x70656E)
    texts = [ascii_text(rng, 200) for _ in range(2)]
    datas = [texts[0], texts[1] + texts[0], texts[0] + texts[1], texts[1]]
    p = tk.chain(datas)
    assert all(tk.empty_window_differs(p[j], datas[j]) for j in (1, 2, 3))
    ext = [TAKE, TAKE, DEFLATE]
    slots = [tk.Slot() for _ in ext]
    ctx = device_slots(engine, slots, ext)
    whole = [frames_of(x, B) for x in p]
    # conn 0: its last message has no END.  conn 1: its first has no BEGIN (open in the carried state), and
    # everything behind it waits.  conn 2, without takeover: only the message that is not whole waits.
    state = np.zeros(3, mm.MSG_STATE_DTYPE)
    state["opcode"][1], state["reserved"][1][0] = 2, 1
    state["opcode"][2], state["reserved"][2][0] = 2, 1
    first = [whole[0] + whole[1] + [(0, RSV1, B, p[2][:5])],
             [(1, 0, C, p[0][3:])] + whole[1] + whole[2],
             [(1, 0, C, b"rest")] + frames_of(ic.deflate(texts[0]), B)]
    ginf, winf = run_pass(engine, first, ext, ctx, slots, state=state, tag="first pass")
    P, Dn = gm.INF_PENDING, gm.INF_DONE
    assert [int(x) for x in ginf["inflated"]["flags"]] == [Dn, Dn, P, P, P, P, P, Dn]
    assert slots[0].total == 600 and slots[0].window() == datas[0] + datas[1]
    assert tk.slots_from_device(ctx)[1] == bytes(tk.CTX_BYTES)             # untouched
    # the next pass shows the waiting messages whole
    second = [whole[2] + whole[3], whole[0] + whole[1] + whole[2], []]
    ginf, winf = run_pass(engine, second, ext, ctx, slots, tag="second pass")
    per = message_bytes(ginf, winf)
    assert per[0] == [(0, datas[2]), (0, datas[3])] and per[1] == [(0, d) for d in datas[:3]]
    assert slots[0].total == 1200 and slots[1].total == 1000


# ---------------------------------------------------------------------------- 6b. more than 8 192 messages
def test_a_batch_past_the_grid_threshold(engine):
    """Above 8 192 messages the kernels' workgroup-to-message mapping rounds its
    range length to a multiple of 16 (the grid is larger than the batch).  Known
    texts, so the expectation is the data itself; 16 distinct scripts."""
    rng = np.random.default_rng(0x67726964)
    scripts = []
    for _ in range(16):
        base = ascii_text(rng, 60)
        datas = [base[: 20 + 5 * j] + ascii_text(rng, 3) for j in range(8)]
        payloads = tk.chain(datas)
        assert tk.empty_window_differs(payloads[1], datas[1])
        conn = Conn(TAKE)
        for p, d in zip(payloads, datas):
            conn.add(frames_of(p, T), p, d)
        scripts.append(conn)
    n = 1100
    assert n * 8 > 8192
    d = mm.Decoded([scripts[c % 16].frames() for c in range(n)], pad=0xFF)
    ext = np.full(n, TAKE, np.uint8)
    got = gm.run_messages_ext(engine, d, ext)
    assert got["dev"]["n_messages"] == n * 8
    import torch
    ctx = torch.zeros((n, tk.CTX_BYTES), dtype=torch.uint8, device=got["dev"]["frames"].device)
    want_bytes = sum(len(x) for s in scripts for x in expected_data(s)) * (n // 16) + \
        sum(len(x) for s in scripts[: n % 16] for x in expected_data(s))
    cap = n * 8 * 64
    res = tk.run_inflate_ctx(engine, got, BIG, cap, ext, ctx)
    s, inf = res["summary"], res["inflated"]
    assert (int(s["status"]), int(s["frames"]), int(s["errors"]), int(s["payload_len"])) == (0, n * 8, 0, want_bytes)
    assert np.all(inf["flags"] == gm.INF_DONE) and np.all(inf["status"] == 0)
    for m in range(n * 8):
        want = scripts[(m // 8) % 16].msgs[m % 8][2]
        o = int(inf["out_off"][m])
        assert res["out"][o:o + int(inf["length"][m])].tobytes() == want, m
    host = [host_slot(c) for c in scripts]
    dev = tk.slots_from_device(ctx)
    assert all(dev[c] == host[c % 16] for c in range(n))


# ---------------------------------------------------------------------------- 7. equivalence with the plain call
def test_null_contexts_and_no_takeover_bit_are_the_plain_call(engine):
    rng = np.random.default_rng(0x65717569)
    streams = [p for p, _ in ic.valid_streams(rng)] + ic.malformed_streams(rng, 300)
    conns = []
    for i in range(0, len(streams), 3):
        conn = []
        for j, p in enumerate(streams[i:i + 3]):
            conn += frames_of(p, T if (i + j) % 2 else B, [len(p) // 2] if j == 1 else [])
        conns.append(conn + ([(0, RSV1, B, b"\x00")] if i % 2 else []))     # some end in a PENDING message
    d = mm.Decoded(conns, pad=0xFF)
    n = len(conns)
    ones = np.ones(n, np.uint8)
    got = gm.run_messages_ext(engine, d, ones)
    three = gm.run_messages_ext(engine, d, np.full(n, 3, np.uint8))        # the message step masks the byte
    for k in ("messages", "msg_of", "conn_msg", "state"):
        assert three[k].tobytes() == got[k].tobytes(), k
    assert three["summary"].tobytes() == got["summary"].tobytes()
    for limit in (BIG, 40):
        state0 = got["dev"]["state"].clone()
        plain = gm.run_inflate(engine, got, limit, 1 << 20)
        used = int(plain["summary"]["payload_bytes"])
        assert int(plain["summary"]["errors"]) > 50 and int(plain["summary"]["frames"]) > 50
        state1 = got["dev"]["state"].clone()
        ctx = tk.slots_to_device([tk.Slot() for _ in conns], got["dev"]["frames"].device)
        ctx[:] = 0x5A
        for ext, slots in ((None, None), (ones, None), (None, ctx), (ones, ctx), (np.zeros(n, np.uint8), ctx)):
            got["dev"]["state"].copy_(state0)
            again = tk.run_inflate_ctx(engine, got, limit, 1 << 20, ext, slots)
            assert again["inflated"].tobytes() == plain["inflated"].tobytes()
            assert again["summary"].tobytes() == plain["summary"].tobytes()
            assert again["out"][:used].tobytes() == plain["out"][:used].tobytes() and np.all(again["out"][used:] == 0xEE)
            assert bool((got["dev"]["state"] == state1).all())
        assert bool((ctx == 0x5A).all())


# ---------------------------------------------------------------------------- 8. a malformed conn index
def test_a_conn_index_past_n_conns_is_invalid_and_writes_nothing(engine):
    import torch
    rng = np.random.default_rng(0x696478)
    datas = [ascii_text(rng, 100), ascii_text(rng, 100)]
    conns = [[f for p in tk.chain(datas + datas) for f in frames_of(p, B)] for _ in range(6)]
    d = mm.Decoded(conns, pad=0xFF)
    ext = np.full(6, TAKE, np.uint8)
    got = gm.run_messages_ext(engine, d, ext)
    nm = got["dev"]["n_messages"]
    assert nm == 24
    msgs = got["dev"]["messages"][: nm * 32].cpu().numpy().view(mm.MESSAGE_DTYPE).copy()
    msgs["conn"][5], msgs["conn"][13], msgs["conn"][23] = 6, 0xFFFFFFFF, 7
    got["dev"]["messages"][: nm * 32] = torch.from_numpy(msgs.view(np.uint8)).to(got["dev"]["messages"].device)
    slots = [tk.Slot() for _ in conns]
    for s in slots:
        s.append(datas[0])
    ctx = tk.slots_to_device(slots, got["dev"]["frames"].device)
    before, state_before = ctx.clone(), got["dev"]["state"].clone()
    res = tk.run_inflate_ctx(engine, got, BIG, 1 << 16, ext, ctx, n_conns=6)
    s = res["summary"]
    assert int(s["status"]) == gev_amd.ERR_INVALID and int(s["errors"]) == 3
    assert (int(s["frames"]), int(s["payload_bytes"]), int(s["payload_len"])) == (0, 0, 0)
    assert np.all(res["out"] == 0xEE) and np.all(res["inflated"].view(np.uint8) == 0xEE)
    assert bool((ctx == before).all()) and bool((got["dev"]["state"] == state_before).all())


# ---------------------------------------------------------------------------- 9. old connections: relocated slots
def old_slots(rng):
    """(the `odd` slot at 70 001 bytes, the `edge` slot at 131 055, their histories): tests/_takeover_far.py."""
    hist = far.history_messages(rng)
    odd, edge = tk.Slot(), tk.Slot()
    odd.append(b"".join(hist[:3]))
    edge.append(b"".join(hist))
    return odd, edge, b"".join(hist[:3]), b"".join(hist)


def relocated_batch():
    """(plan, conns, slots, number of far cases, number of edge cases) of the test below."""
    rng = far.rng_of(0x666172)
    odd, edge, h_odd, h_edge = old_slots(rng)
    cases = far.far_cases(odd.total, far.U_INF)
    edges = far.edge_cases(edge.total, far.U_INF)
    first = far.message(rng, h_odd, "text")
    chain_odd = [first, far.message(rng, h_odd + first, "tiled", 5000), first[-300:]]
    short = h_edge[-4000:-3983]
    chain_edge = [short, b"", far.message(rng, h_edge + short, "runs")]
    plan = [(odd, h_odd, s, chain_odd, 6) for _, s in [("unrelocated", 0)] + cases]
    plan += [(edge, h_edge, s, chain_edge, 9) for _, s in [("unrelocated", 0)] + edges]
    plan.append((tk.Slot(), b"", 0, chain_odd[:2], 6))                        # a fresh connection
    below32 = dict(cases)["below 2^32"]
    for kind in ("random", "period"):                                         # the other kinds cross 2^32 too
        plan.append((odd, h_odd, below32, [far.message(rng, h_odd, kind), first[:300]], 1))
    assert len(plan) == 15
    conns, slots = [], []
    for slot, history, shift, chain, level in plan:
        conn = Conn(TAKE)
        for p, m in zip(far.peer_chain(history, chain, level), chain):
            conn.add(frames_of(p, B, [len(p) // 3] if len(p) > 3000 else []), p, m)
        if history:                                                           # ... and the farthest distance there is
            whole = history + b"".join(chain)
            conn.add(frames_of(tk.match_at(32768), B), tk.match_at(32768), whole[-32768:][:3])
            assert tk.empty_window_differs(conn.msgs[0][1], chain[0])
        conns.append(conn)
        slots.append(slot.relocated(shift))
    return plan, conns, slots, len(cases), len(edges)


def test_relocated_slots_in_one_batch(engine):
    """Fifteen connections, each with the slot of a connection that has been open for a long time -- `total`
    raised across 2^31, 2^32, 2^48 and 2^62 --, one unrelocated and one fresh, three or four messages each so
    the chain runs in registers across the boundary.  The payloads are zlib's, made with the history as its
    dictionary, so the expected bytes are the messages; records, bytes and slots are the model's (run_pass)
    and the host twin's on the same relocated slots, and every relocated connection ends as the unrelocated
    one, `total` apart."""
    plan, conns, slots, n_far, n_edge = relocated_batch()
    before = [s.image() for s in slots]
    ext = [TAKE] * len(conns)
    ctx = device_slots(engine, slots, ext)
    ginf, winf = run_pass(engine, [c.frames() for c in conns], ext, ctx, slots, limit=1 << 17, tag="relocated")
    assert winf["errors"] == 0
    per = message_bytes(ginf, winf)
    dev = tk.slots_from_device(ctx)
    for c, conn in enumerate(conns):
        assert per[c] == [(im.OK, d) for d in expected_data(conn)], c         # zlib's reference: the messages
        host = bytearray(before[c])                                           # the host twin on the same slot
        for _, p, d in conn.msgs:
            assert gev_amd.inflate_raw_ctx(p, 1 << 17, host) == (im.OK, d), c
        assert dev[c] == bytes(host), c

    def translated(c, base):
        a, b = tk.Slot(dev[c]), tk.Slot(dev[base])
        assert (a.total, a.broken, a.ring) == (b.total + plan[c][2], 0, b.ring), c
    for c in range(1, 1 + n_far):
        translated(c, 0)
    for c in range(2 + n_far, 2 + n_far + n_edge):
        translated(c, 1 + n_far)
