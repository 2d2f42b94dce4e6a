"""GPU checks of compressed messages that span passes
(gevws_inflate_carry_async, gevws_join_carry_ext_async) through the C ABI,
bit-exact against tests/_inflate_carry_model.py: icm.chain_device runs a list
of passes through the device message pass, the inflate with the carry and the
join with GEVWS_CARRY_KEEP_COMPRESSED, state, slots and carry handed on, and
compares every output of every pass with the models over FILL-patterned
buffers, as gm.assert_inflated and cm.assert_join_carry do.  Malformed streams
are verdicts of a bounded decoder and malformed records are rejected before
they are indexed: nothing here provokes a fault."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _carry_model as cm
from tests import _inflate_carry_model as icm
from tests import _inflate_gpu_model as gm
from tests import _inflate_takeover as it
from tests import _join_model as jm
from tests import _messages_model as mm
from tests._helpers import gpu_decode, pack_streams

pytestmark = pytest.mark.gpu

T, B, C, PING = 1, 2, 0, 9
RSV1 = icm.RSV1
BIG = 1 << 22
DEFL, TAKE = it.EXT_DEFLATE, it.EXT_DEFLATE | it.EXT_TAKEOVER
OPENZ = icm.OPEN | icm.COMPRESSED


def rnd(rng, n: int) -> bytes:
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def rec(g, c):
    r = g["carry"][c]
    return tuple(int(r[k]) for k in ("length", "opcode", "flags", "status"))


def two_passes(wires, cuts, op=B):
    """Each wire cut in two at its cut: pass 1 opens it, pass 2 holds the rest and the FIN."""
    return [[[(0, RSV1, op, w[:k])] for w, k in zip(wires, cuts)], [[(1, 0, C, w[k:])] for w, k in zip(wires, cuts)]]


def delivered_all(res, datas, op=B):
    seq = icm.sequences(len(datas), [g for _, g, _ in res])
    assert seq == [[(op, d)] for d in datas]


# ---------------------------------------------------------------------------- 1. prefix lengths
PREFIX = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)


def test_prefix_lengths(engine):
    """The carried length at the ragged last vector and on both sides of the
    1 KiB refill; 0 is a message opened by an empty fragment."""
    rng = np.random.default_rng(0x1CA001)
    datas = [rnd(rng, 1500) + b"refill boundary " * 200 + rnd(rng, 1200) for _ in PREFIX]
    wires = [icm.z(d) for d in datas]
    assert all(len(w) > 2600 for w in wires)
    ext = np.full(len(PREFIX), DEFL, np.uint8)
    res = icm.chain_device(engine, two_passes(wires, PREFIX), ext, BIG, BIG, tag="prefix")
    assert [rec(res[0][1], c) for c in range(len(PREFIX))] == [(k, B, OPENZ, 0) for k in PREFIX]
    assert np.all(res[1][1]["bodies"]["flags"] == jm.WHOLE | jm.INFLATED)
    delivered_all(res, datas)
    # the same cuts on takeover connections, a message in front so that the chain has a window
    slots = [it.Slot() for _ in PREFIX]
    first = rnd(rng, 700)
    chains = [it.chain([first, d]) for d in datas]
    passes = [[[(1, RSV1, B, ch[0]), (0, RSV1, B, ch[1][:k])] for ch, k in zip(chains, PREFIX)],
              [[(1, 0, C, ch[1][k:])] for ch, k in zip(chains, PREFIX)]]
    res, ctx = icm.chain_device(engine, passes, np.full(len(PREFIX), TAKE, np.uint8), BIG, BIG, slots=slots,
                                tag="prefix, takeover")
    assert it.slots_from_device(ctx) == [s.image() for s in slots]
    assert icm.sequences(len(PREFIX), [g for _, g, _ in res]) == [[(B, first), (B, d)] for d in datas]


# ---------------------------------------------------------------------------- 2. a cut inside every structure
def test_cut_inside_every_structure(engine):
    rng = np.random.default_rng(0x1CA002)
    fixed = icm.z(b"hello hello hello, fixed codes", 6, zlib.Z_FIXED)
    text = b"".join(rng.choice([b"dynamic ", b"header ", b"cut ", b"here "]) for _ in range(400))
    dyn = icm.z(text, 9)
    raw = rnd(rng, 3000)
    st = icm.z(raw, 0)
    assert (fixed[0] >> 1) & 3 == 1 and (dyn[0] >> 1) & 3 == 2 and (st[0] >> 1) & 3 == 0
    assert st[1:3] == (3000).to_bytes(2, "little")
    cases = [
        (fixed, 3, b"hello hello hello, fixed codes"),   # inside a fixed-Huffman code
        (dyn, 6, text),                                  # inside the dynamic block's header (the code lengths)
        (st, 3, raw),                                    # between LEN and NLEN
        (st, 5 + 500, raw),                              # inside stored data: skip() crosses prefix -> frame
        (st, 5 + 1500, raw),                             # ... with more than a refill on either side
        (dyn, len(dyn) - 1, text),                       # only the last byte is left for the second pass
        (fixed, len(fixed) - 1, b"hello hello hello, fixed codes"),
    ]
    ext = np.full(len(cases), DEFL, np.uint8)
    res = icm.chain_device(engine, two_passes([w for w, _, _ in cases], [k for _, k, _ in cases]), ext, BIG, BIG)
    delivered_all(res, [d for _, _, d in cases])


# ---------------------------------------------------------------------------- 3. three passes and an idle one
def test_three_passes_and_an_idle_pass(engine):
    rng = np.random.default_rng(0x1CA003)
    data = " ".join(str(rng.choice(["compressed", "text", "spans", "passes", "€", "idle", "ping"]))
                    for _ in range(900)).encode()
    wire = icm.z(data)
    assert len(wire) > 300
    a, b = 40, len(wire) - 21
    passes = [[[(0, RSV1, T, wire[:a])], [(1, 0, B, b"beside it")]],
              [[(0, 0, C, wire[a:100]), (1, 0, PING, b"mid"), (0, 0, C, wire[100:b])], []],
              [[], []],
              [[(1, 0, PING, b"only a ping")], [(0, 0, B, b"plain, ")]],
              [[(1, 0, C, wire[b:])], [(1, 0, C, b"carried too")]]]
    ext = np.array([DEFL, 0], np.uint8)
    res = icm.chain_device(engine, passes, ext, BIG, BIG)
    for p, n in ((0, a), (1, b), (2, b), (3, b)):
        assert rec(res[p][1], 0) == (n, T, OPENZ, 0), p
        assert res[p][1]["carry_dst"][:n].tobytes() == wire[:n]
    assert [int(x) for x in res[1][0]["inflated"]["flags"]] == [gm.INF_PENDING]
    assert rec(res[3][1], 1) == (7, B, icm.OPEN, 0)
    assert not res[4][1]["carry"].view(np.uint8).any()
    assert icm.sequences(2, [g for _, g, _ in res]) == [[(T, data)], [(B, b"beside it"), (B, b"plain, carried too")]]


# ---------------------------------------------------------------------------- 4. takeover
def test_takeover_chain_goes_on_behind_a_carried_message(engine):
    rng = np.random.default_rng(0x1CA004)
    one, two = rnd(rng, 900) + b"window " * 50, rnd(rng, 2500)
    three = two[300:1800] + b"tail" + two[:200]   # its matches reach back into the second message
    ch = it.chain([one, two, three])
    assert it.empty_window_differs(ch[2], three)
    plain_z = icm.z(b"no takeover here " * 30)
    k = len(ch[1]) // 2
    conns = [[(1, RSV1, B, ch[0]), (0, RSV1, B, ch[1][:k]), (1, 0, C, ch[1][k:]), (1, RSV1, B, ch[2])],
             [(0, RSV1, T, plain_z[:9]), (1, 0, C, plain_z[9:])],
             [(0, 0, B, b"plain and "), (1, 0, C, b"uncompressed")]]
    ext = np.array([TAKE, DEFL, 0], np.uint8)
    want = [[(B, one), (B, two), (B, three)], [(T, b"no takeover here " * 30)], [(B, b"plain and uncompressed")]]
    cut = [cm.split_passes(conns, [[2], [1], [1]]), [conns]]
    images = []
    for passes in cut:
        slots = [it.Slot() for _ in conns]
        res, ctx = icm.chain_device(engine, passes, ext, BIG, BIG, slots=slots, tag=f"{len(passes)} passes")
        assert icm.sequences(3, [g for _, g, _ in res]) == want
        images.append(it.slots_from_device(ctx))
        assert images[-1] == [s.image() for s in slots]
    assert images[0] == images[1], "the slot is a function of the stream, not of the cut"
    host = bytearray(it.CTX_BYTES)
    for payload, data in zip(ch, (one, two, three)):
        assert gev_amd.inflate_raw_ctx(payload, 1 << 16, host) == (0, data)
    assert bytes(host) == images[0][0] and not any(images[0][1]) and not any(images[0][2])


# ---------------------------------------------------------------------------- 5. cut invariance on the device
def test_cut_invariance_on_the_device(engine):
    rng = np.random.default_rng(0x1CA005)
    n_conns = 300
    conns, ext, want = icm.random_streams(rng, n_conns)
    passes = cm.split_passes(conns, icm.byte_cuts(rng, conns, 3))
    slots = [it.Slot() for _ in range(n_conns)]
    res, ctx = icm.chain_device(engine, passes, ext, BIG, BIG, slots=slots)
    assert icm.sequences(n_conns, [g for _, g, _ in res]) == want
    assert sum(int(np.count_nonzero(g["carry"]["flags"] == OPENZ)) for _, g, _ in res) >= 20
    assert it.slots_from_device(ctx) == [s.image() for s in slots]


# ---------------------------------------------------------------------------- 6. verdicts
def stored_wire(data: bytes) -> bytes:
    w = icm.z(data, 0)
    assert w[:5] == b"\x00" + len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little")
    return w


def test_verdicts_at_the_end_pass(engine):
    rng = np.random.default_rng(0x1CA006)
    data = rnd(rng, 100)
    w = stored_wire(data)
    bad = w[:4] + bytes([w[4] ^ 0x10]) + w[5:]   # NLEN no longer ~LEN: malformed by the bytes of the END pass
    not_utf8 = b"\xff\xfe not utf-8 \xc0" * 5
    utf = stored_wire(not_utf8)
    ext = np.array([DEFL, TAKE, DEFL], np.uint8)
    slots = [it.Slot() for _ in range(3)]
    passes = [[[(0, RSV1, B, bad[:3])], [(0, RSV1, B, bad[:3])], [(0, RSV1, T, utf[:30])]],
              [[(1, 0, C, bad[3:])], [(1, 0, C, bad[3:]), (1, RSV1, B, w)], [(1, 0, C, utf[30:])]]]
    res, ctx = icm.chain_device(engine, passes, ext, BIG, BIG, slots=slots, tag="deflate / utf8")
    inf, g, _ = res[1]
    assert [(int(r["flags"]), int(r["status"]), int(r["length"])) for r in inf["inflated"]] == \
        [(1, gm.ERR_DEFLATE, 0), (1, gm.ERR_DEFLATE, 0), (1, gm.ERR_DEFLATE, 0), (1, mm.ERR_UTF8, len(not_utf8))]
    assert [int(x) for x in inf["state"]["failed"]] == [gm.ERR_DEFLATE, gm.ERR_DEFLATE, mm.ERR_UTF8]
    off = int(inf["inflated"]["out_off"][3])
    assert inf["out"][off: off + len(not_utf8)].tobytes() == not_utf8   # failed UTF-8: the bytes are kept
    assert not np.any(g["bodies"]["flags"]) and [int(x) for x in g["bodies"]["status"]] == \
        [gm.ERR_DEFLATE] * 3 + [mm.ERR_UTF8]
    img = it.slots_from_device(ctx)
    assert img == [s.image() for s in slots] and img[1][8] == gm.ERR_DEFLATE and slots[1].broken == gm.ERR_DEFLATE
    # inflated output over max_message_bytes (the inflate's limit)
    res = icm.chain_device(engine, two_passes([w, w], [50, 5]), np.array([DEFL, DEFL], np.uint8), 99, BIG,
                           tag="too big out")
    assert [(int(r["flags"]), int(r["status"])) for r in res[1][0]["inflated"]] == [(1, gm.ERR_TOO_BIG)] * 2
    # compressed bytes over the carry's limit: LOST / TOO_BIG, then DONE with TOO_BIG at the END
    slots = [it.Slot() for _ in range(2)]
    passes = [[[(0, RSV1, B, w[:40])], [(0, RSV1, B, w[:70])]],
              [[(0, 0, C, w[40:80])], [(1, 0, PING, b"")]],
              [[(1, 0, C, w[80:])], [(1, 0, C, w[70:]), (1, RSV1, B, icm.z(b"after the loss"))]]]
    res, ctx = icm.chain_device(engine, passes, np.array([DEFL, TAKE], np.uint8), BIG, 64, slots=slots,
                                tag="too big carried")
    assert rec(res[0][1], 0) == (40, B, OPENZ, 0) and rec(res[0][1], 1) == (0, B, icm.LOST, gm.ERR_TOO_BIG)
    assert rec(res[1][1], 0) == (0, B, icm.LOST, gm.ERR_TOO_BIG) == rec(res[1][1], 1)
    assert [int(res[p][1]["carry_summary"]["errors"]) for p in range(3)] == [1, 1, 0]
    assert [(int(r["flags"]), int(r["status"]), int(r["length"])) for r in res[2][0]["inflated"]] == \
        [(1, gm.ERR_TOO_BIG, 0)] * 3
    assert int(res[2][0]["summary"]["errors"]) == 3 and it.slots_from_device(ctx)[1][8] == gm.ERR_TOO_BIG
    assert not res[2][1]["carry"].view(np.uint8).any()


# ---------------------------------------------------------------------------- 7. mismatches and PENDING
def open_state(ops, compressed):
    st = np.zeros(len(ops), mm.MSG_STATE_DTYPE)
    for c, (op, z) in enumerate(zip(ops, compressed)):
        st[c]["opcode"] = op
        st[c]["reserved"][0] = 1 if z else 0
    return st


def test_mismatches_stay_pending_and_undelivered(engine):
    w = icm.z(b"never delivered " * 8)
    cin = np.zeros(4, cm.CARRY_DTYPE)
    csrc = np.frombuffer(b"0123456789abcdef" + w[:16], np.uint8).copy()
    cin[1] = (0, 16, B, icm.OPEN, 0, [0] * 13)          # an OPEN plain record under a compressed message
    cin[2] = (0, 0, B, icm.LOST, 0, [0] * 13)           # LOST with status 0
    cin[3] = (16, 16, B, OPENZ, 0, [0] * 13)            # an OPEN | COMPRESSED record under a plain message
    ext = np.full(4, DEFL, np.uint8)
    passes = [[[(1, 0, C, w[16:])], [(1, 0, C, w[16:])], [(1, 0, C, w[16:])], [(1, 0, C, b"plain end")]]]
    start = (open_state([B] * 4, [1, 1, 1, 0]), cin, csrc)
    (inf, g, e), = icm.chain_device(engine, passes, ext, BIG, BIG, start=start)
    assert [int(x) for x in e["tables"]["messages"]["flags"]] == [gm.COMPRESSED | mm.END] * 3 + [mm.END]
    assert [int(x) for x in inf["inflated"]["flags"]] == [gm.INF_PENDING] * 3 + [0]
    assert not np.any(g["bodies"]["flags"]) and not np.any(g["bodies"]["status"])
    assert int(g["summary"]["frames"]) == 0 and not g["carry"].view(np.uint8).any()
    # the same records under messages that stay open: every one ends LOST with status 0
    passes = [[[(0, 0, C, w[16:20])], [(0, 0, C, w[16:20])], [(0, 0, C, w[16:20])], [(0, 0, C, b"plain")]]]
    (inf, g, e), = icm.chain_device(engine, passes, ext, BIG, BIG, start=start)
    assert [rec(g, c) for c in range(4)] == [(0, B, icm.LOST, 0)] * 4
    assert [int(x) for x in inf["inflated"]["flags"]] == [gm.INF_PENDING] * 3 + [0]


# ---------------------------------------------------------------------------- 8. capacity and retry
def test_capacity_writes_nothing_and_the_retry_fits(engine):
    import torch
    rng = np.random.default_rng(0x1CA008)
    dev = torch.device("cuda", engine.device)
    one, two = rnd(rng, 500), b"carried over a cut " * 40
    ch = it.chain([one, two])
    k = len(ch[1]) // 2
    ext = np.array([TAKE, DEFL], np.uint8)
    other = icm.z(rnd(rng, 200))
    assert len(other) > 200
    p1 = [[(1, RSV1, B, ch[0]), (0, RSV1, T, ch[1][:k])], [(0, RSV1, B, other[:33])]]
    p2 = [[(1, 0, C, ch[1][k:])], [(0, 0, C, other[33:50])]]
    slots = [it.Slot(), it.Slot()]
    res, ctx = icm.chain_device(engine, [p1], ext, BIG, BIG, slots=slots)
    e1 = res[0][2]
    start = (res[0][0]["state"], e1["join"]["carry"], e1["join"]["carry_dst"])
    before = it.slots_from_device(ctx)
    e = icm.chain_model([p2], ext, BIG, BIG, slots=[s.copy() for s in slots], start=start)[0]
    got = cm.run_messages(engine, e["d"], start[0], ext)
    mm.assert_tables_equal(got, e["tables"])
    need = e["inf"]["payload_bytes"]
    assert need == jm.round16(len(two))
    state0 = got["state"].copy()
    inf = icm.run_inflate_carry(engine, got, BIG, need - 16, ext, ctx, 2, start[1], start[2])
    s = inf["summary"]
    assert (int(s["status"]), int(s["payload_bytes"])) == (jm.ERR_CAPACITY, need)
    assert np.all(inf["inflated_raw"] == icm.FILL) and np.all(inf["out"] == icm.FILL)
    assert it.slots_from_device(ctx) == before and inf["state"].tobytes() == state0.tobytes()
    inf = icm.run_inflate_carry(engine, got, BIG, need, ext, ctx, 2, start[1], start[2])
    gm.assert_inflated(inf, e["inf"], need, "retry")
    assert inf["out"][: len(two)].tobytes() == two
    # the join: carry_cap short of connection 1's open compressed message -> none of the four outputs
    w = e["join"]
    oc, cc = w["out"].size, w["carry_dst"].size
    assert cc == 64 and rec(dict(carry=w["carry"]), 1) == (50, B, OPENZ, 0)
    isum = dict(payload_bytes=need, status=0)
    img = np.concatenate([inf["out"][: jm.round16(need)], np.full(oc - jm.round16(need), icm.FILL, np.uint8)])
    short = icm.carry_model_ext(e["d"].frames, e["d"].arena, e["tables"], 2, BIG, start[1], start[2], jm.JOIN_ALL, oc,
                                cc - 16, e["inf"]["inflated"], isum, out_image=img,
                                carry_flags=icm.KEEP_COMPRESSED)
    assert short["carry"] is None and short["carry_summary"]["status"] == jm.ERR_CAPACITY
    pre = torch.from_numpy(np.concatenate([img, np.full(jm.GUARD, icm.FILL, np.uint8)])).to(dev)
    g = icm.run_join_carry_ext(engine, got["dev"], 2, BIG, jm.JOIN_ALL, oc, cc - 16, start[1], start[2], None,
                               inf["dev"]["inflated"], inf["dev"]["summary"], pre)
    cm.assert_join_carry(g, short, oc, cc - 16, "short carry_cap")
    assert np.all(g["bodies_raw"] == icm.FILL)


# ---------------------------------------------------------------------------- 9. malformed input
def test_malformed_input_is_rejected_before_it_is_indexed(engine):
    w = icm.z(b"malformed records " * 10)
    ext = np.array([DEFL, DEFL], np.uint8)
    csrc = np.frombuffer(w[:32] + bytes(32), np.uint8).copy()
    passes = [[[(1, 0, C, w[20:])], [(1, RSV1, B, w), (1, RSV1, B, w)]]]
    state = open_state([B, 0], [1, 0])
    d = mm.Decoded(passes[0], pad=0xFF)
    t = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, state, ext)
    got = cm.run_messages(engine, d, state, ext)
    mm.assert_tables_equal(got, t)
    for tag, off, length, src_bytes, n_conns, count in (
            ("off its boundary", 8, 20, 64, 2, 1),
            ("past carry_src_bytes", 16, 20, 32, 2, 1),
            ("off beyond the arena", 1 << 40, 20, 64, 2, 1),
            ("length beyond the arena", 0, (1 << 64) - 1, 64, 2, 1),
            ("conn == n_conns", 0, 20, 64, 1, 2)):
        cin = np.zeros(n_conns, cm.CARRY_DTYPE)
        cin[0] = (off, length, B, OPENZ, 0, [0] * 13)
        for with_ctx in (False, True):
            ctx = it.slots_to_device([it.Slot() for _ in range(n_conns)], got["dev"]["frames"].device)
            inf = icm.run_inflate_carry(engine, got, BIG, 4096, ext[:n_conns] if with_ctx else None,
                                        ctx if with_ctx else None, n_conns, cin, csrc, src_bytes)
            want = icm.model_inflate_carry(d, t, BIG, None, None, None, n_conns, cin, csrc, src_bytes)
            assert want == dict(invalid=count), tag
            icm.assert_invalid(inf, count, tag)
            assert not ctx.any() and inf["state"].tobytes() == got["state"].tobytes(), tag
    # a bad record of a connection without a message in the batch is not the inflate's business
    cin = np.zeros(3, cm.CARRY_DTYPE)
    cin[0], cin[2] = (0, 20, B, OPENZ, 0, [0] * 13), (8, 1 << 40, B, OPENZ, 0, [0] * 13)
    inf = icm.run_inflate_carry(engine, got, BIG, 4096, None, None, 3, cin, csrc, 64)
    assert int(inf["summary"]["status"]) == 0 and int(inf["summary"]["frames"]) == 3
    # an unknown carry_flags bit fails the call; the known one does not
    for flags, ok in ((2, False), (3, False), (1 << 31, False), (1, True)):
        try:
            icm.run_join_carry_ext(engine, got["dev"], 2, BIG, jm.JOIN_ALL, 1 << 14, 1 << 12, carry_flags=flags)
            assert ok, flags
        except RuntimeError:
            assert not ok, flags


# ---------------------------------------------------------------------------- 10. the NULL calls
def test_null_calls_are_the_old_calls(engine):
    import torch
    rng = np.random.default_rng(0x1CA00A)
    n_conns = 64
    conns, ext, _ = icm.random_streams(rng, n_conns)
    for c in range(0, n_conns, 7):
        conns[c][-1] = (0,) + conns[c][-1][1:]   # some messages stay open
    d = mm.Decoded(conns, pad=0xFF)
    got = cm.run_messages(engine, d, None, ext)
    dev = got["dev"]["frames"].device
    t = got["dev"]
    assert t["n_messages"] >= 100
    junk_rec = mm._dev(np.full(n_conns * 32, 0x5A, np.uint8), dev)   # never looked at
    junk_src = mm._dev(np.zeros(64, np.uint8), dev)
    outs = []
    for call in ("ctx", "carry, no records", "carry, no arena"):
        ctx = it.slots_to_device([it.Slot() for _ in range(n_conns)], dev)
        st = t["state"].clone()
        inf, out, summ = (torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
                          for n in (t["n_messages"] * 32, (1 << 20) + 64, 64))
        args = (t["frames"], t["n_frames"], t["messages"], t["n_messages"], t["msg_of"], t["summary"], t["payload"],
                BIG, st, inf, out, 1 << 20, summ, mm._dev(ext, dev, 1), ctx, n_conns)
        if call == "ctx":
            engine.inflate_ctx_async(*args)
        elif call == "carry, no records":
            engine.inflate_carry_async(*args, None, junk_src, 64)
        else:
            engine.inflate_carry_async(*args, junk_rec, None, 64)
        torch.cuda.synchronize(engine.device)
        outs.append([x.cpu().numpy() for x in (inf, out, summ, st, ctx)])
    assert int(outs[0][2].view(mm.SUMMARY_DTYPE)[0]["frames"]) >= 50
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))
    # gevws_join_carry_ext_async with carry_flags 0 == gevws_join_carry_async, slots and FILL guards included
    inf_rec, inf_sum = mm._dev(outs[0][0], dev, 32), mm._dev(outs[0][2], dev, 64)
    cin = np.zeros(n_conns, cm.CARRY_DTYPE)
    oc, cc = 1 << 21, 1 << 18
    a = cm.run_join_carry(engine, t, n_conns, BIG, jm.JOIN_ALL, oc, cc, cin, None, None, inf_rec, inf_sum)
    b = icm.run_join_carry_ext(engine, t, n_conns, BIG, jm.JOIN_ALL, oc, cc, cin, None, None, inf_rec, inf_sum,
                               carry_flags=0)
    for k in ("bodies_raw", "out", "carry_raw", "carry_dst"):
        assert np.array_equal(a[k], b[k]), k
    assert a["summary"].tobytes() == b["summary"].tobytes()
    assert a["carry_summary"].tobytes() == b["carry_summary"].tobytes()
    assert int(a["carry_summary"]["frames"]) >= 1 and np.any(a["carry"]["flags"] == icm.LOST)
    assert not np.any(a["carry"]["flags"] & icm.COMPRESSED)


def test_without_the_flag_compressed_messages_still_end_lost(engine):
    """The stream of test_compressed_messages_are_lost_not_carried through the
    new entry points with carry_flags 0."""
    rng = np.random.default_rng(0xCA7709)
    hello, again = b"Hello, a whole compressed message", b"another whole one " * 9
    openz = icm.z(b"a compressed message that spans two passes")
    ext = np.array([DEFL, 0], np.uint8)
    passes = [
        [[(1, RSV1, T, icm.z(hello)), (0, 0, B, rnd(rng, 33)), (1, 0, C, rnd(rng, 2)), (0, RSV1, T, openz[:7])],
         [(0, 0, B, b"plain, open")]],
        [[(1, 0, C, openz[7:]), (0, RSV1, B, icm.z(again)[:4]), (1, 0, C, icm.z(again)[4:]), (1, 0, B, rnd(rng, 20))],
         [(1, 0, C, b" and closed")]]]
    res = icm.chain_device(engine, passes, ext, 1 << 20, BIG, carry_flags=0)
    assert rec(res[0][1], 0) == (0, T, icm.LOST, 0) and rec(res[0][1], 1) == (11, B, icm.OPEN, 0)
    assert [int(x) for x in res[1][0]["inflated"]["flags"]] == [gm.INF_PENDING, gm.INF_DONE, 0, 0]
    fl = [int(x) for x in res[1][1]["bodies"]["flags"]]
    assert fl == [0, jm.WHOLE | jm.INFLATED, jm.WHOLE | jm.JOINED, jm.WHOLE | jm.JOINED]
    # ... and with the flag the same stream delivers it
    res = icm.chain_device(engine, passes, ext, 1 << 20, BIG)
    assert rec(res[0][1], 0) == (7, T, OPENZ, 0)
    assert icm.sequences(2, [g for _, g, _ in res])[0][2] == (T, b"a compressed message that spans two passes")


# ---------------------------------------------------------------------------- 11. end to end
def test_end_to_end_through_engine(engine):
    import torch
    rng = np.random.default_rng(0x1CA00B)
    dev = torch.device("cuda", engine.device)
    text = ("a compressed text message over three passes: é€ " * 300).encode()
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    wire_z = (co.compress(text) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]
    a, b = len(wire_z) // 3, 2 * len(wire_z) // 3

    def wire(data, op, fin, rsv=0):
        return wo.encode_frame(data, op, fin, rsv, True, rnd(rng, 4))
    streams = [[wire(wire_z[:a], T, False, RSV1), wire(b"one", T, True)],
               [wire(wire_z[a:b], C, False) + wire(b"", PING, True), wire(b"two", T, True)],
               [wire(wire_z[b:], C, True), b""]]
    ext_h = np.array([gev_amd.EXT_DEFLATE, 0], np.uint8)
    ext = mm._dev(ext_h, dev, 1)
    state = torch.zeros((2, 8), dtype=torch.uint8, device=dev)
    carry = gev_amd.Carry(engine, 2, 1 << 20, compressed=True)
    for p, ss in enumerate(streams):
        batch = gpu_decode(engine, *pack_streams(ss))
        msgs = engine.messages(batch, state, conn_ext=ext)
        assert not msgs.conn_msg_host()["error"].any()
        inf = engine.inflate(batch, msgs, 1 << 20, state, carry=carry)
        bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL, carry=carry)
        echo = engine.echo_messages(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext)
        plain = echo.plain_wire.cpu().numpy().tobytes()
        if p < 2:
            assert list(echo.plain_conn) == [1] and plain == wo.encode_frame((b"one", b"two")[p], 1, True, 0, False)
            assert len(echo.def_conn) == 0
            r = carry.records_host()[0]
            kept = (a, b)[p]
            assert (int(r["flags"]), int(r["length"]), int(r["opcode"])) == \
                (gev_amd.CARRY_OPEN | gev_amd.CARRY_COMPRESSED, kept, T)
            assert carry.carried_bytes(0) == wire_z[:kept]
        else:
            assert bodies.body_bytes(0) == text
            dfl = wo.decode_stream(echo.def_wire.cpu().numpy().tobytes())
            assert dfl.status == wo.OK and len(dfl.frames) == 1 and list(echo.def_conn) == [0]
            f = dfl.frames[0]
            assert f.header.fin and f.header.rsv == 4 and f.header.opcode == 1
            assert zlib.decompressobj(-15).decompress(f.payload + b"\x00\x00\xff\xff") == text
            assert not carry.records_host().view(np.uint8).any() and carry.used == 0


# ---------------------------------------------------------------------------- a carried message on an old connection
def test_carried_message_on_relocated_slots(engine):
    """A compressed message that began in an earlier pass, carried and inflated at its FIN, on the slots of
    connections that have been open for a long time (tests/_takeover_far.py): `total` is raised so that the
    carried message crosses 2^31, 2^32 and 2^62.  The device against the models, as everywhere here; the
    payloads are zlib's with the history as its dictionary, so the expected bytes are the messages."""
    from tests import _takeover_far as far
    rng = far.rng_of(0x1CA0FA)
    hist = far.history_messages(rng)
    history = b"".join(hist[:3])
    base = it.Slot()
    base.append(history)
    cases = dict(far.far_cases(base.total, far.U_INF))
    shifts = [0, cases["below 2^31"], cases["below 2^32"], cases["on 2^32"], cases["near 2^62"]]
    slots = [base.relocated(s) for s in shifts]
    one = history[-900:-200]
    two = far.message(rng, history + one, "text")
    three = two[-300:]
    ch = far.peer_chain(history, [one, two, three])
    assert it.empty_window_differs(ch[1], two) and it.empty_window_differs(ch[2], three)
    cuts = (1, 1025, len(ch[1]) // 2, len(ch[1]) - 1, 17)
    passes = [[[(1, RSV1, B, ch[0]), (0, RSV1, B, ch[1][:k])] for k in cuts],
              [[(1, 0, C, ch[1][k:]), (1, RSV1, B, ch[2])] for k in cuts]]
    res, ctx = icm.chain_device(engine, passes, np.full(len(shifts), TAKE, np.uint8), BIG, BIG, slots=slots,
                                tag="carried, relocated")
    dev = it.slots_from_device(ctx)
    assert dev == [s.image() for s in slots]
    assert icm.sequences(len(shifts), [g for _, g, _ in res]) == [[(B, one), (B, two), (B, three)]] * len(shifts)
    near = it.Slot(dev[0])
    for c, s in enumerate(shifts):
        far_slot = it.Slot(dev[c])
        assert (far_slot.total, far_slot.broken, far_slot.ring) == (near.total + s, 0, near.ring), c
    assert near.total == 70001 + len(one) + len(two) + len(three)
