"""GPU checks of server context takeover (gevws_deflate_ctx_async): a takeover
connection's messages compressed with the connection's earlier messages as
history, the window and the hash table carried in its slot of d_def_ctx.
Every comparison is exact: payloads and slots are the bytes
gevws_deflate_raw_ctx (the host twin, pinned on the CPU in
tests/test_deflate_takeover_host.py) gives for the same chain; zlib inflates
a chain with one inflater.  The source arenas have 0xFF in every pad byte;
d_out and the records are filled with 0xEE first."""
import zlib

import numpy as np
import pytest

import gev_amd
from tests import _inflate_corpus as ic
from tests import _takeover_far as far

pytestmark = pytest.mark.gpu

T, B = 1, 2
TAIL = b"\x00\x00\xff\xff"
FILL = 0xEE
DYN, PLAIN = gev_amd.DEFLATE_DYNAMIC, gev_amd.DEFLATE_PLAIN_IF_NOT_SMALLER
EXT_D, EXT_S = gev_amd.EXT_DEFLATE, gev_amd.EXT_DEFLATE | gev_amd.EXT_SERVER_TAKEOVER
CTX = gev_amd.DEF_CTX_BYTES


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


def build(msgs, pad=0xFF):
    """(arena, src_bytes, records, msg_conn) for [(conn, bytes, opcode, wb)]."""
    rec = np.zeros(len(msgs), gev_amd.DEFLATE_MSG_DTYPE)
    parts, off = [], 0
    for i, (_, data, op, wb) in enumerate(msgs):
        rec[i]["payload_off"], rec[i]["length"], rec[i]["opcode"], rec[i]["window_bits"] = off, len(data), op, wb
        parts.append(data + bytes([pad]) * (r16(len(data)) - len(data)))
        off += r16(len(data))
    arena = np.frombuffer(b"".join(parts) + bytes([pad]) * gev_amd.IN_PAD, np.uint8).copy()
    return arena, off, rec, np.array([c for c, _, _, _ in msgs], np.uint32)


def model(msgs, ext, slots, flags=0):
    """The host's answer: (payloads, plain flags); `slots` (bytearrays) are advanced."""
    want, plain = [], []
    for c, data, _, wb in msgs:
        if ext[c] & gev_amd.EXT_SERVER_TAKEOVER:
            want.append(gev_amd.deflate_raw_ctx(data, slots[c], wb, flags & DYN))
            plain.append(False)
        else:
            comp = gev_amd.deflate_raw(data, wb, flags & DYN)
            p = bool(flags & PLAIN) and len(comp) >= len(data)
            want.append(data if p else comp)
            plain.append(p)
    return want, plain


def fresh(n):
    return [bytearray(CTX) for _ in range(n)]


def slots_np(slots):
    return np.frombuffer(b"".join(bytes(s) for s in slots), np.uint8).reshape(len(slots), CTX).copy()


def run(engine, arena, src_bytes, rec, conn, ext, ctx, out_cap, flags=0, prev=None, max_msgs=None, null=()):
    """One gevws_deflate_ctx_async call on fresh 0xEE-filled outputs; ctx: uint8 [n_conns, CTX] before the call."""
    import torch
    dev = torch.device("cuda", engine.device)
    n = rec.shape[0] if max_msgs is None else max_msgs
    d_src = torch.from_numpy(arena).to(dev)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 24).copy()).to(dev)
    d_conn = torch.from_numpy(conn.view(np.int32).copy()).to(dev)
    d_ext = torch.from_numpy(np.asarray(ext, np.uint8).copy()).to(dev)
    d_ctx = torch.from_numpy(ctx.copy()).to(dev)
    frames = torch.full((max(rec.shape[0], 1), 32), FILL, dtype=torch.uint8, device=dev)
    out = torch.full((out_cap + gev_amd._abi.OUT_PAD,), FILL, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    d_prev = None
    if prev is not None:
        s = np.zeros(1, gev_amd.SUMMARY_DTYPE)
        s["frames"], s["status"] = prev
        d_prev = torch.from_numpy(s.view(np.uint8).copy()).to(dev)
    engine.deflate_ctx_async(d_rec, n, d_prev, d_src, src_bytes, flags, frames, out, out_cap, summ,
                             None if "conn" in null else d_conn, None if "ext" in null else d_ext,
                             None if "ctx" in null else d_ctx, len(ext))
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0],
                frames=frames.cpu().numpy().reshape(-1).view(gev_amd.OUT_FRAME_DTYPE), out=out.cpu().numpy(),
                ctx=d_ctx.cpu().numpy(), dev=dict(frames=frames, out=out, summary=summ))


def check(got, msgs, want, plain):
    """Records, layout, pads, sentinel and summary of a call that fitted."""
    n = len(msgs)
    s, fr, out = got["summary"], got["frames"], got["out"]
    assert int(s["status"]) == gev_amd.OK and int(s["errors"]) == 0 and int(s["frames"]) == n
    off = 0
    for i, ((c, data, op, wb), w) in enumerate(zip(msgs, want)):
        f = fr[i]
        assert (int(f["fin"]), int(f["rsv"]), int(f["opcode"]), int(f["masked"])) == (1, 0 if plain[i] else 4, op, 0), i
        assert not f["mask"].any() and int(f["length"]) == len(w) and int(f["payload_len"]) == len(w), (i, c, len(data))
        assert int(f["payload_off"]) == off, i
        assert out[off:off + len(w)].tobytes() == w, (i, c, len(data), wb)
        assert not out[off + len(w):off + r16(len(w))].any(), i
        off += r16(len(w))
    assert int(s["payload_bytes"]) == off and int(s["payload_len"]) == sum(len(w) for w in want)
    assert np.all(out[off:] == FILL) and np.all(fr[n:].view(np.uint8) == FILL)


def untouched(got, ctx_before):
    return np.all(got["out"] == FILL) and np.all(got["frames"].view(np.uint8) == FILL) and \
        np.array_equal(got["ctx"], ctx_before)


def one_call(engine, msgs, ext, slots, flags=0, pad=0xFF):
    """The call against the model, payloads and slots; `slots` are advanced.  The slots after the call."""
    before = slots_np(slots)
    want, plain = model(msgs, ext, slots, flags)
    arena, src_bytes, rec, conn = build(msgs, pad)
    got = run(engine, arena, src_bytes, rec, conn, ext, before, sum(r16(len(w)) for w in want), flags)
    check(got, msgs, want, plain)
    after = slots_np(slots)
    bad = [c for c in range(len(ext)) if not np.array_equal(got["ctx"][c], after[c])]
    assert not bad, bad[:8]
    return want


def scripts(rng, n_conns, per, sizes, kinds=(0, 1, 2, 3)):
    out = []
    for c in range(n_conns):
        for _ in range(per if isinstance(per, int) else int(rng.integers(per[0], per[1] + 1))):
            n = int(rng.choice(sizes))
            kind = int(rng.choice(kinds))
            out.append((c, ic.sample(rng, n, kind), T if kind in (2, 3) else B, 0))
    return out


@pytest.mark.parametrize("flags", [0, DYN, PLAIN, DYN | PLAIN])
def test_mixed_batch(engine, flags):
    rng = np.random.default_rng(0x6D6978)
    n_conns = 150
    ext = [EXT_S if c % 3 != 2 else EXT_D for c in range(n_conns)]
    ext[5] |= gev_amd.EXT_CLIENT_TAKEOVER
    msgs = scripts(rng, n_conns, (1, 6), [0, 0, 1, 2, 3, 5, 17, 100, 300, 511, 512, 600])
    # multi-run messages that start at odd ring offsets, behind an odd history
    big = []
    for c, first in ((0, 7), (1, 4091), (3, 13), (4, 1)):
        big += [(c, ic.sample(rng, first, 0), T, 0), (c, ic.sample(rng, 9001, c % 4), B, 0), (c, b"", T, 0),
                (c, ic.sample(rng, 4097, 0), T, 0), (c, ic.sample(rng, 2, 1), B, 0)]
    msgs = sorted(msgs + big, key=lambda m: m[0])  # (stable: one run a connection)
    slots = fresh(n_conns)
    want = one_call(engine, msgs, ext, slots, flags)
    # zlib reads every takeover chain with one inflater
    infl = {}
    for (c, data, _, wb), w in zip(msgs, want):
        if ext[c] & gev_amd.EXT_SERVER_TAKEOVER:
            d = infl.setdefault(c, zlib.decompressobj(-15))
            assert d.decompress(w + TAIL) == data, c
    # a second call continues every chain
    msgs2 = scripts(rng, n_conns, (0, 3), [0, 1, 3, 300, 512, 5000])
    want2 = one_call(engine, msgs2, ext, slots, flags, pad=0x00)
    for (c, data, _, wb), w in zip(msgs2, want2):
        if ext[c] & gev_amd.EXT_SERVER_TAKEOVER:
            assert infl.setdefault(c, zlib.decompressobj(-15)).decompress(w + TAIL) == data, c


@pytest.mark.parametrize("flags", [0, DYN])
def test_passes(engine, flags):
    rng = np.random.default_rng(0x70617373)
    n_conns = 12
    ext = [EXT_S] * n_conns
    msgs = scripts(rng, n_conns, 8, [0, 1, 3, 17, 300, 512, 4097], kinds=(0, 0, 1, 2, 3))
    ref_slots = fresh(n_conns)
    ref = one_call(engine, msgs, ext, ref_slots, flags)
    for cuts in ((1, 7), (4, 4), (1,) * 8):
        slots = fresh(n_conns)
        got, k0 = {}, 0
        for cut in cuts:
            part = [(i, m) for i, m in enumerate(msgs) if k0 <= i % 8 < k0 + cut]
            # (0x00 behind every message where the one pass had 0xFF: the slots do not see the pad)
            for (i, _), w in zip(part, one_call(engine, [m for _, m in part], ext, slots, flags, pad=0x00)):
                got[i] = w
            k0 += cut
        assert [got[i] for i in range(len(msgs))] == ref, cuts
        assert slots == ref_slots, cuts


def test_window_edges(engine):
    rng = np.random.default_rng(0x65646765)
    x = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    lens = []
    for extra in (0, 1):  # the second X at distance 30 720, and one byte out of reach
        a = x + bytes(30720 - 64 - 16 + extra)
        b = bytes(16) + x + b"tail"
        msgs = [(0, a, B, 0), (0, b, B, 0)]
        want = one_call(engine, msgs, [EXT_S], fresh(1))
        d = zlib.decompressobj(-15)
        assert [d.decompress(w + TAIL) for w in want] == [a, b]
        lens.append(len(want[1]))
    assert lens[0] + 40 < lens[1], lens  # a 64-byte match against 64 literals
    # a stream past 65 536 bytes: the ring wraps twice, the 16-bit positions once
    text = ic.sample(rng, 9000, 0)
    msgs = [(0, text[i:] + text[:i], T, 0) for i in range(0, 80, 10)]
    slots = fresh(1)
    want = one_call(engine, msgs, [EXT_S], slots)
    assert int.from_bytes(slots[0][:8], "little") == 72000
    assert all(len(w) < len(want[0]) for w in want[1:])  # history helps
    # window_bits 8 with history: zlib's 256-byte window follows, so every distance is <= 256
    msgs = [(0, ic.sample(rng, n, 0), T, 8) for n in (300, 100, 511, 30, 700)]
    want = one_call(engine, msgs, [EXT_S], fresh(1))
    d = zlib.decompressobj(-8)
    assert [d.decompress(w + TAIL) for w in want] == [m[1] for m in msgs]


def test_capacity_then_retry(engine):
    rng = np.random.default_rng(0x636170)
    ext = [EXT_S, EXT_D, EXT_S]
    slots = fresh(3)
    one_call(engine, scripts(rng, 3, 2, [300, 512]), ext, slots)  # a history to keep
    before = slots_np(slots)
    msgs = scripts(rng, 3, 3, [0, 100, 777, 5000])
    want, plain = model(msgs, ext, slots)
    need = sum(r16(len(w)) for w in want)
    arena, src_bytes, rec, conn = build(msgs)
    short = run(engine, arena, src_bytes, rec, conn, ext, before, need - 1)
    s = short["summary"]
    assert int(s["status"]) == gev_amd.ERR_CAPACITY and int(s["payload_bytes"]) == need and int(s["errors"]) == 0
    assert untouched(short, before)
    full = run(engine, arena, src_bytes, rec, conn, ext, short["ctx"], need)
    check(full, msgs, want, plain)
    assert np.array_equal(full["ctx"], slots_np(slots))
    # Engine.deflate retries by itself and leaves the contexts where the call that fitted put them
    import torch
    dev = torch.device("cuda", engine.device)
    d_ctx = torch.from_numpy(before.copy()).to(dev)
    res = engine.deflate(rec, torch.from_numpy(arena).to(dev), src_bytes, out_cap=16, msg_conn=conn,
                         conn_ext=torch.tensor(ext, dtype=torch.uint8, device=dev), contexts=d_ctx)
    assert [res.payload(i) for i in range(len(msgs))] == want
    assert np.array_equal(d_ctx.cpu().numpy(), slots_np(slots))


def test_invalid_calls(engine):
    rng = np.random.default_rng(0x696E76)
    ext = [EXT_S, EXT_S, EXT_D, EXT_S]
    slots = fresh(4)
    one_call(engine, scripts(rng, 4, 2, [300]), ext, slots)
    before = slots_np(slots)
    msgs = scripts(rng, 4, 4, [0, 100, 300])
    arena, src_bytes, rec, conn = build(msgs)

    def invalid(rec, conn, errors, name):
        got = run(engine, arena, src_bytes, rec, conn, ext, before, 1 << 16)
        s = got["summary"]
        assert int(s["status"]) == gev_amd.ERR_INVALID and int(s["errors"]) == errors, (name, s)
        assert int(s["frames"]) == 0 and int(s["payload_bytes"]) == 0 and int(s["payload_len"]) == 0, name
        assert untouched(got, before), name

    assert [int(x) for x in conn] == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    c = conn.copy()
    c[7] = 4  # (a run's last message: the run before it stays one run)
    invalid(rec, c, 1, "conn index = n_conns")
    c[11] = 0xFFFFFFFF
    invalid(rec, c, 2, "conn indices >= n_conns")
    r = rec.copy()
    r[1]["opcode"] = 9  # in mid-chain of connection 0
    invalid(r, conn, 1, "malformed in mid-chain")
    r[10]["window_bits"] = 7  # ... and one of the connection without takeover
    invalid(r, conn, 2, "malformed twice")
    c = conn.copy()
    c[12:16] = 1  # connection 3's messages go to connection 1, behind connection 2's: a second run
    invalid(rec, c, 1, "a takeover connection in two separate runs")
    c = conn.copy()
    c[[8, 0]] = c[[0, 8]]  # a connection without takeover may stand anywhere ... but 0 is now in two runs
    invalid(rec, c, 1, "split by a plain connection's message")
    # the same records, in order, are fine
    got = run(engine, arena, src_bytes, rec, conn, ext, before, 1 << 16)
    assert int(got["summary"]["status"]) == gev_amd.OK


def test_null_pointers_and_no_takeover_bit(engine):
    import torch
    rng = np.random.default_rng(0x6E756C6C)
    n_conns = 5
    msgs = scripts(rng, n_conns, 3, [0, 3, 300, 4097, 9000])
    arena, src_bytes, rec, conn = build(msgs)
    ctx = rng.integers(0, 256, (n_conns, CTX), dtype=np.uint8)  # (never looked at)
    dev = torch.device("cuda", engine.device)
    for flags in (0, DYN | PLAIN):
        want, plain = model(msgs, [EXT_D] * n_conns, None, flags)
        frames = torch.full((len(msgs), 32), FILL, dtype=torch.uint8, device=dev)
        out = torch.full(((1 << 17) + gev_amd._abi.OUT_PAD,), FILL, dtype=torch.uint8, device=dev)
        summ = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
        engine.deflate_async(torch.from_numpy(rec.view(np.uint8).reshape(-1, 24).copy()).to(dev), len(msgs), None,
                             torch.from_numpy(arena).to(dev), src_bytes, flags, frames, out, 1 << 17, summ)
        torch.cuda.synchronize(engine.device)
        for null, ext in (("conn",), [EXT_S] * n_conns), (("ext",), [EXT_S] * n_conns), \
                (("ctx",), [EXT_S] * n_conns), ((), [EXT_D, gev_amd.EXT_CLIENT_TAKEOVER | EXT_D, 0, EXT_D, 3]):
            got = run(engine, arena, src_bytes, rec, conn, ext, ctx, 1 << 17, flags, null=null)
            check(got, msgs, want, plain)
            assert got["summary"].tobytes() == summ.cpu().numpy().tobytes(), null
            assert got["frames"].tobytes() == frames.cpu().numpy().tobytes(), null
            assert got["out"].tobytes() == out.cpu().numpy().tobytes(), null
            assert np.array_equal(got["ctx"], ctx), null


def test_gated_count(engine):
    rng = np.random.default_rng(0x67617465)
    ext = [EXT_S, EXT_S]
    msgs = scripts(rng, 2, 4, [100, 300, 512])
    arena, src_bytes, rec, conn = build(msgs)
    slots = fresh(2)
    want, plain = model(msgs[:6], ext, slots)  # connection 1's chain ends in its middle
    got = run(engine, arena, src_bytes, rec, conn, ext, slots_np(fresh(2)), 1 << 14, prev=(6, gev_amd.OK))
    s = got["summary"]
    assert int(s["frames"]) == 6
    off = 0
    for i, w in enumerate(want):
        assert got["out"][off:off + len(w)].tobytes() == w, i
        off += r16(len(w))
    assert np.all(got["out"][off:] == FILL) and np.all(got["frames"][6:].view(np.uint8) == FILL)
    assert np.array_equal(got["ctx"], slots_np(slots))
    assert int.from_bytes(slots[1][:8], "little") == sum(len(m[1]) for m in msgs[4:6])
    before = slots_np(slots)
    got = run(engine, arena, src_bytes, rec, conn, ext, before, 1 << 14, prev=(8, gev_amd.ERR_CAPACITY))
    assert not got["summary"].tobytes().strip(b"\0") and untouched(got, before)


def test_past_the_grid_threshold(engine):
    """More than 8 192 messages: the grid is 1 024 x 16 workgroups, messages 16 apart."""
    rng = np.random.default_rng(0x67726964)
    n_conns = 1100
    ext = [EXT_S if c % 5 else EXT_D for c in range(n_conns)]
    base = [ic.sample(rng, 40, 0) for _ in range(16)]
    msgs = [(c, base[(c + k) % 16][: 8 + (c + 3 * k) % 32], T, 0) for c in range(n_conns) for k in range(8)]
    assert len(msgs) > 8192
    one_call(engine, msgs, ext, fresh(n_conns))


# ---------------------------------------------------------------------------- old connections: relocated slots
def old_slots(rng):
    """(the `odd` slot at 70 001 bytes, the `edge` slot at 131 055, their histories), made by the host twin."""
    hist = far.history_messages(rng)
    ctx = bytearray(CTX)
    for k, m in enumerate(hist):
        gev_amd.deflate_raw_ctx(m, ctx, 0, 0)
        if k == 2:
            odd = bytes(ctx)
    return odd, bytes(ctx), b"".join(hist[:3]), b"".join(hist)


@pytest.mark.parametrize("flags", [0, DYN])
def test_relocated_slots_in_one_batch(engine, flags):
    """Thirteen connections, each with the slot of a connection that has been open for a long time -- `total`
    raised across 2^31, 2^32, 2^48 and 2^62 (tests/_takeover_far.py) --, one unrelocated and one fresh, two or
    three messages each so the chain runs in registers across the boundary.  Payloads, records and slots are
    the host twin's on the same slots (one_call), the device's bytes inflate with zlib and the history as its
    dictionary, and every relocated connection ends as the unrelocated one, `total` apart."""
    rng = far.rng_of(0x666172)
    odd, edge, h_odd, h_edge = old_slots(rng)
    cases = far.far_cases(far.DefSlot(odd).total, far.U_DEF)
    edges = far.edge_cases(far.DefSlot(edge).total, far.U_DEF)
    first = far.message(rng, h_odd, "text")
    chain_odd = [first, far.message(rng, h_odd + first, "tiled", 5000), first[-300:]]
    short = h_edge[-4000:-3983]
    chain_edge = [short, b"", far.message(rng, h_edge + short, "runs")]
    conns = [(odd, h_odd, s, chain_odd) for _, s in [("unrelocated", 0)] + cases]
    conns += [(edge, h_edge, s, chain_edge) for _, s in [("unrelocated", 0)] + edges]
    conns.append((bytes(CTX), b"", 0, chain_odd[:2]))                        # a fresh connection
    # the other kinds of message cross 2^32 too, on further connections
    below32 = dict(cases)["below 2^32"]
    for kind in ("random", "period"):
        conns.append((odd, h_odd, below32, [far.message(rng, h_odd, kind), far.message(rng, h_odd, "text", 300)]))
    assert len(conns) == 15
    slots = [far.DefSlot(s).relocated(shift) for s, _, shift, _ in conns]
    msgs = [(c, m, B, 0) for c, (_, _, _, chain) in enumerate(conns) for m in chain]
    want = one_call(engine, msgs, [EXT_S] * len(conns), slots, flags)       # the device == the host twin
    at = 0
    for c, (_, history, _, chain) in enumerate(conns):
        stream = history
        for m in chain:
            d = zlib.decompressobj(-15, zdict=stream[-32768:]) if stream else zlib.decompressobj(-15)
            assert d.decompress(want[at] + TAIL) == m, (c, len(m))
            stream, at = stream + m, at + 1
    for c in range(1, 1 + len(cases)):                                       # translation: connection 0 is unrelocated
        far.assert_def_translated(slots[c], slots[0], conns[c][2], c)
    e0 = 1 + len(cases)
    for c in range(e0 + 1, e0 + 1 + len(edges)):
        far.assert_def_translated(slots[c], slots[e0], conns[c][2], c)
    per = len(chain_odd)
    assert all(want[c * per:(c + 1) * per] == want[:per] for c in range(1, 1 + len(cases)))


def test_closed_loop_at_a_far_position(engine):
    """deflate on relocated slots -> encode -> decode -> message pass -> inflate on the matching relocated
    inflate slots: the original messages, across 2^31 and across 2^32."""
    import torch
    from tests import _inflate_takeover as tk
    from tests._helpers import gpu_decode
    rng = far.rng_of(0x6C6F6F70)
    dev = torch.device("cuda", engine.device)
    odd, _, h_odd, _ = old_slots(rng)
    cases = dict(far.far_cases(far.DefSlot(odd).total, far.U_DEF))
    shifts = [cases["below 2^31"], cases["below 2^32"], cases["on 2^32"], cases["near 2^62"]]
    n_conns = len(shifts)
    ext = [EXT_S | gev_amd.EXT_CLIENT_TAKEOVER] * n_conns
    d_ext = torch.tensor(ext, dtype=torch.uint8, device=dev)
    slots = [far.DefSlot(odd).relocated(s) for s in shifts]
    inf = tk.Slot()
    inf.append(h_odd)
    assert bytes(inf.ring) == far.DefSlot(odd).ring                          # the two windows hold the same stream
    inf_slots = [inf.relocated(s) for s in shifts]
    def_ctx = torch.from_numpy(slots_np(slots)).to(dev)
    inf_ctx = tk.slots_to_device(inf_slots, dev)
    state = torch.zeros((n_conns, 8), dtype=torch.uint8, device=dev)
    first = far.message(rng, h_odd, "text")
    chain = [first, far.message(rng, h_odd + first, "period", 5000), first[-300:]]
    msgs = [(c, m, B, 0) for c in range(n_conns) for m in chain]
    per, n = len(chain), len(msgs)
    arena, src_bytes, rec, conn = build(msgs)
    want, _ = model(msgs, ext, slots)
    res = engine.deflate(rec, torch.from_numpy(arena).to(dev), src_bytes, msg_conn=conn, conn_ext=d_ext,
                         contexts=def_ctx)
    assert [res.payload(i) for i in range(n)] == want
    wire_cap = sum(len(w) + 10 for w in want)
    wire = torch.zeros(wire_cap + gev_amd._abi.OUT_PAD, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(n, dtype=torch.int64, device=dev)
    esum = torch.zeros(64, dtype=torch.uint8, device=dev)
    engine.encode_async(res.frames, n, res.out, wire, wire_cap, out_off, esum)
    torch.cuda.synchronize(engine.device)
    es = esum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
    assert int(es["status"]) == gev_amd.OK
    total = int(es["payload_bytes"])
    offs = [int(x) for x in out_off.cpu().numpy()] + [total]
    table = [(offs[c * per], offs[(c + 1) * per] - offs[c * per]) for c in range(n_conns)]
    out = gpu_decode(engine, wire[:total].cpu().numpy(), np.array(table, np.int64))
    assert int(out.summary_host()["frames"]) == n
    m = engine.messages(out, state=state, conn_ext=d_ext)
    assert m.messages_host().shape[0] == n
    got = engine.inflate(out, m, 1 << 17, state=state, conn_ext=d_ext, contexts=inf_ctx)
    s = got.summary_host()
    assert int(s["frames"]) == n and int(s["errors"]) == 0
    for i, (_, data, _, _) in enumerate(msgs):
        assert got.message_bytes(i) == data, i
    assert np.array_equal(def_ctx.cpu().numpy(), slots_np(slots))
    after = inf_ctx.cpu().numpy()
    assert np.array_equal(def_ctx.cpu().numpy()[:, 64:64 + 32768], after[:, 64:])
    sent = sum(len(x) for x in chain)
    for c, s in enumerate(shifts):
        assert int.from_bytes(after[c, :8].tobytes(), "little") == 70001 + s + sent and not after[c, 8:64].any()


def test_round_trip_on_the_device(engine):
    """deflate with contexts -> encode -> decode -> message pass -> inflate with
    client-takeover slots: the plain messages, over two passes."""
    import torch
    from tests._helpers import gpu_decode
    rng = np.random.default_rng(0x72747270)
    dev = torch.device("cuda", engine.device)
    n_conns, per = 16, 2
    utf8 = lambda b: b.decode("utf-8", "ignore").encode()  # noqa: E731
    ext = [EXT_S | gev_amd.EXT_CLIENT_TAKEOVER] * n_conns
    d_ext = torch.tensor(ext, dtype=torch.uint8, device=dev)
    def_ctx = torch.zeros((n_conns, CTX), dtype=torch.uint8, device=dev)
    inf_ctx = torch.zeros((n_conns, gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev)
    state = torch.zeros((n_conns, 8), dtype=torch.uint8, device=dev)
    words = [utf8(ic.sample(rng, 400, 0)) for _ in range(4)]
    slots = fresh(n_conns)
    for p in range(2):
        msgs = []
        for c in range(n_conns):
            for k in range(per):  # similar texts: the later ones lean on the earlier ones
                msgs.append((c, utf8(words[(c + k + p) % 4][: 300 + 7 * c]) + b" #%d.%d.%d" % (c, p, k), T, 0))
        arena, src_bytes, rec, conn = build(msgs)
        want, _ = model(msgs, ext, slots)
        res = engine.deflate(rec, torch.from_numpy(arena).to(dev), src_bytes, msg_conn=conn, conn_ext=d_ext,
                             contexts=def_ctx)
        n = len(msgs)
        assert [res.payload(i) for i in range(n)] == want
        wire_cap = sum(len(w) + 10 for w in want)
        wire = torch.zeros(wire_cap + gev_amd._abi.OUT_PAD, dtype=torch.uint8, device=dev)
        out_off = torch.zeros(n, dtype=torch.int64, device=dev)
        esum = torch.zeros(64, dtype=torch.uint8, device=dev)
        engine.encode_async(res.frames, n, res.out, wire, wire_cap, out_off, esum)
        torch.cuda.synchronize(engine.device)
        es = esum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
        assert int(es["status"]) == gev_amd.OK
        total = int(es["payload_bytes"])
        offs = [int(x) for x in out_off.cpu().numpy()] + [total]
        table = [(offs[c * per], offs[(c + 1) * per] - offs[c * per]) for c in range(n_conns)]
        out = gpu_decode(engine, wire[:total].cpu().numpy(), np.array(table, np.int64))
        assert int(out.summary_host()["frames"]) == n
        m = engine.messages(out, state=state, conn_ext=d_ext)
        assert m.messages_host().shape[0] == n
        inf = engine.inflate(out, m, 1 << 16, state=state, conn_ext=d_ext, contexts=inf_ctx)
        s = inf.summary_host()
        assert int(s["frames"]) == n and int(s["errors"]) == 0
        for i, (_, data, _, _) in enumerate(msgs):
            assert inf.message_bytes(i) == data, (p, i)
    assert np.array_equal(def_ctx.cpu().numpy(), slots_np(slots))
    # the two windows hold the same stream
    assert np.array_equal(def_ctx.cpu().numpy()[:, 64:64 + 32768], inf_ctx.cpu().numpy()[:, 64:])
