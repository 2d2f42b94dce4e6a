"""GPU checks of the join step (gevws_join_async) through the C ABI, bit-exact
against tests/_join_model.py: d_bodies field by field, the summary, and the
WHOLE of d_out -- the copied bodies, their zeroed pads, and every other byte
still the 0xEE it was prefilled with.  The hand-built arenas pad every slot
with 0xBF, so a read past hdr.length shows.  Unless a test says otherwise
out_cap is exactly the need: every batch's last body ends at out_cap."""
import zlib

import numpy as np
import pytest

import gev_amd
from tests import _inflate_gpu_model as gm
from tests import _join_model as jm
from tests import _messages_model as mm

pytestmark = pytest.mark.gpu

T, B, C, PING, PONG = 1, 2, 0, 9, 10
RSV1 = 4
SIZE_BLOCK = 256  # k_join_size / k_join_place: messages a workgroup (kWalkBlock)


def rnd(rng, n: int) -> bytes:
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def message(rng, lengths, op=B, between=None):
    """One message as frames of the given fragment lengths; `between(i)` = the
    frames to put behind fragment i (not the last)."""
    out = []
    for i, n in enumerate(lengths):
        last = i == len(lengths) - 1
        out.append((1 if last else 0, 0, op if i == 0 else C, rnd(rng, n)))
        if between is not None and not last:
            out.extend(between(i))
    return out


def join_both(engine, conns, flags=0, out_cap=None, state=None, tag=""):
    """Message pass + join on hand-built connections, both compared with the
    model; returns (device join, model, device message tables, Decoded)."""
    d = mm.Decoded(conns)
    got = gm.run_messages_ext(engine, d, None, state)
    t = d.model(state)
    mm.assert_tables_equal(got, t, tag)
    w = jm.join_model(d.frames, d.arena, t["messages"], t["msg_of"], flags, out_cap)
    cap = w["out"].size
    g = jm.run_join(engine, got["dev"], flags, cap)
    jm.assert_join(g, w, cap, tag)
    return g, w, got, d


# ---------------------------------------------------------------------------- the copy's shapes
def test_every_shift(engine):
    """Two-fragment messages, the first length 0..33 (every byte shift of the
    second fragment, twice over) x the second in {0, 1, 15, 16, 17, 31, 32, 33}."""
    rng = np.random.default_rng(0x6A6F01)
    conns = [message(rng, [a, b]) for a in range(34) for b in (0, 1, 15, 16, 17, 31, 32, 33)]
    g, w, _, _ = join_both(engine, conns)
    assert int(g["summary"]["frames"]) == 34 * 8 and np.all(g["bodies"]["flags"] == jm.WHOLE | jm.JOINED)
    # several messages of one connection, so bodies of one connection follow each other too
    join_both(engine, [sum((message(rng, [a, 17 - a]) for a in range(18)), [])], tag="one connection")


def test_tiny_fragments(engine):
    rng = np.random.default_rng(0x6A6F02)
    conns = [
        message(rng, [1] * 40),                  # a store vector spans 16 fragments
        message(rng, list(range(1, 21))),
        message(rng, [0, 3, 0, 4, 0]),           # empty fragments first, middle and last
        message(rng, [0, 0, 0]),                 # only empty fragments: delivered, no space
        message(rng, [0, 0, 1]),
        message(rng, [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 15, 1]),
        message(rng, [5, 0, 11, 0, 0, 16, 1]),   # a fragment that ends on the vector's end
    ]
    g, w, _, _ = join_both(engine, conns)
    b = g["bodies"]
    assert int(b["length"][3]) == 0 and int(b["flags"][3]) == jm.WHOLE | jm.JOINED
    assert int(b["off"][3]) == int(b["off"][4])  # the empty body takes no space


def test_tile_boundaries(engine):
    rng = np.random.default_rng(0x6A6F03)
    conns = [
        message(rng, [4095, 10]), message(rng, [4096, 10]), message(rng, [4097, 10]),
        message(rng, [4095, 1, 1, 100]),
        message(rng, [4097, 4097, 4095]),        # 12 289 bytes in fragments of 4 097
        message(rng, [7, 4089, 4096, 1]),
    ]
    assert sum(len(f[3]) for f in conns[4]) == 12289
    join_both(engine, conns)


def test_one_mebibyte_body_spans_many_workgroups(engine):
    rng = np.random.default_rng(0x6A6F04)
    total = (1 << 20) + 5
    lens = [int(x) | 1 for x in rng.integers(20000, 60000, 16)]
    lens.append(total - sum(lens))
    assert len(lens) == 17 and all(x % 2 == 1 and x > 0 for x in lens) and len(set(lens)) == 17
    g, w, _, _ = join_both(engine, [message(rng, [33, 2]), message(rng, lens), message(rng, [3, 3])])
    assert int(g["bodies"]["length"][1]) == total


def test_control_frames_between_fragments(engine):
    rng = np.random.default_rng(0x6A6F05)

    def ctl(i):
        return [(1, 0, PING if (i + k) % 2 else PONG, rnd(rng, int(rng.integers(0, 126))))
                for k in range(int(rng.integers(1, 4)))]
    conns = [message(rng, [int(x) for x in rng.integers(0, 300, int(rng.integers(2, 9)))], between=ctl)
             for _ in range(40)]
    conns.append([(1, 0, PING, b"only control frames")])
    conns.append(message(rng, [2000, 3000, 5000], op=T, between=ctl))
    conns[-1] = [(f, r, o, bytes(x & 0x7F for x in p) if o in (T, C) else p) for f, r, o, p in conns[-1]]  # ASCII
    join_both(engine, conns)


# ---------------------------------------------------------------------------- what is delivered
def test_not_delivered(engine):
    rng = np.random.default_rng(0x6A6F06)
    conns = [
        [(0, 0, B, b"open"), (0, 0, C, b"still open")],             # no END
        [(1, 0, C, b"tail of an earlier pass")],                     # continued from a carried state: no BEGIN
        [(0, 0, T, b"abc"), (1, 0, C, b"\xff tail")],               # UTF-8 failure in the second fragment
        message(rng, [3, 4]) + [(1, RSV1, B, b"rsv")] + message(rng, [5, 6]),  # ERR_RSV after one whole message
        (mm.ERR_LEN_MSB, message(rng, [7, 8])),                      # status < 0
        message(rng, [9, 10]),
    ]
    st = np.zeros(len(conns), mm.MSG_STATE_DTYPE)
    st["opcode"][1] = B
    g, w, got, _ = join_both(engine, conns, jm.JOIN_ALL, state=st)
    b = g["bodies"]
    assert [int(x) for x in b["flags"]] == [0, 0, 0, jm.WHOLE | jm.JOINED, jm.WHOLE | jm.JOINED]
    assert [int(x) for x in b["status"]] == [0, 0, mm.ERR_UTF8, 0, 0]
    assert [int(x) for x in b["conn"]] == [0, 1, 2, 3, 5]
    assert [int(x) for x in got["conn_msg"]["error"]] == [0, 0, mm.ERR_UTF8, mm.ERR_RSV, 0, 0]
    assert (int(g["summary"]["frames"]), int(g["summary"]["payload_len"])) == (2, 7 + 19)


def test_flags(engine):
    rng = np.random.default_rng(0x6A6F07)
    conns = [message(rng, [20]), message(rng, [0]), message(rng, [5, 6]), message(rng, [100]),
             message(rng, [1, 1, 1]) + message(rng, [4096])]
    # without JOIN_ALL: single-frame bodies point into d_payload, and no byte of d_out changes for them
    g, w, got, d = join_both(engine, conns)
    b = g["bodies"]
    single = np.flatnonzero(b["flags"] == jm.WHOLE)
    assert list(single) == [0, 1, 3, 5]
    first = d.model()["messages"]["first_frame"]
    assert np.array_equal(b["off"][single], d.frames["payload_off"][first[single]])
    assert int(g["summary"]["payload_bytes"]) == 16 + 16 and int(g["summary"]["frames"]) == 6
    # with it everything is in d_out
    g2, _, _, _ = join_both(engine, conns, jm.JOIN_ALL)
    assert np.all(g2["bodies"]["flags"] == jm.WHOLE | jm.JOINED)
    assert int(g2["summary"]["payload_bytes"]) == 32 + 0 + 16 + 112 + 16 + 4096
    # an unknown flag bit fails the call
    t, o = got["dev"], g["dev"]
    for bad in (2, 4, 0x80000000, jm.JOIN_ALL | 8):
        st = gev_amd.lib.gevws_join_async(engine._ctx, None, t["frames"].data_ptr(), t["n_frames"],
                                          t["messages"].data_ptr(), t["n_messages"], t["msg_of"].data_ptr(),
                                          t["summary"].data_ptr(), t["payload"].data_ptr(), None, None, bad,
                                          o["bodies"].data_ptr(), o["out"].data_ptr(), 1 << 20,
                                          o["summary"].data_ptr())
        assert st == gev_amd.ERR_INVALID, bad


# ---------------------------------------------------------------------------- behind the inflate
def comp(co, data: bytes) -> bytes:
    x = co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH)
    assert x.endswith(b"\x00\x00\xff\xff")
    return x[:-4]


def one_shot(data: bytes) -> bytes:
    return comp(zlib.compressobj(6, zlib.DEFLATED, -15), data)


def cut(payload: bytes, op: int, cuts, rsv=RSV1):
    edges = [0, *cuts, len(payload)]
    return [(1 if i == len(edges) - 2 else 0, rsv if i == 0 else 0, op if i == 0 else C,
             payload[edges[i]:edges[i + 1]]) for i in range(len(edges) - 1)]


def test_with_the_inflate(engine):
    import torch
    rng = np.random.default_rng(0x6A6F08)
    text = [(b"message %d of a takeover connection, " % i) * (3 + i) for i in range(3)]
    tk = zlib.compressobj(6, zlib.DEFLATED, -15)
    big = bytes(rng.integers(0, 8, 9000, dtype=np.uint8))
    conns = [
        cut(one_shot(b"Hello, one frame"), T, ()) + message(rng, [100, 200]),          # compressed, then plain
        cut(one_shot(big), B, (17, 1000, 1001)),                                        # compressed, fragmented
        [f for x in text for f in cut(comp(tk, x), T, (5,))],                           # takeover, three messages
        message(rng, [4000, 97, 1]) + cut(b"\x07garbage", B, ()) + message(rng, [1, 2]),  # ERR_DEFLATE in between
        message(rng, [31, 33]) + cut(one_shot(b"never finished")[:6], B, ())[:1],       # ... see below: PENDING
        message(rng, [50]),                                                             # a single plain frame
    ]
    conns[4][-1] = (0, RSV1, B, conns[4][-1][3])  # no FIN: the compressed message stays open
    ext = np.array([1, 1, 3, 1, 1, 0], np.uint8)
    d = mm.Decoded(conns, pad=0xFF)
    dev = torch.device("cuda", engine.device)
    batch = gev_amd.Batch(frames=mm._dev(d.frames, dev, 32).view(-1, 32), payload=mm._dev(d.arena, dev),
                          conn_out=mm._dev(d.conn_out, dev, 32).view(-1, 32), summary=mm._dev(d.summary, dev, 64),
                          n_conns=len(conns))
    d_ext = mm._dev(ext, dev, 1)
    state = torch.zeros((len(conns), 8), dtype=torch.uint8, device=dev)
    ctxs = torch.zeros((len(conns), gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev)
    msgs = engine.messages(batch, state, conn_ext=d_ext)
    want_t = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, None, ext)
    assert msgs.messages_host().tobytes() == want_t["messages"].tobytes()
    assert np.array_equal(msgs.msg_of_host(), want_t["msg_of"])
    n = want_t["messages"].shape[0]
    plain_need = sum(jm.round16(int(r["length"])) for r in want_t["messages"] if not int(r["flags"]) & gm.COMPRESSED)
    inf_need = sum(jm.round16(len(x)) for x in (b"Hello, one frame", big, *text))
    cap = inf_need + plain_need
    inf = engine.inflate(batch, msgs, 1 << 24, state, out_cap=cap, conn_ext=d_ext, contexts=ctxs)
    isum, irec = inf.summary_host(), inf.inflated_host()
    assert (int(isum["frames"]), int(isum["errors"]), int(isum["payload_bytes"])) == (5, 1, inf_need)
    by_conn = {c: [m for m in range(n) if int(want_t["messages"]["conn"][m]) == c] for c in range(len(conns))}
    assert inf.message_bytes(by_conn[0][0]) == b"Hello, one frame" and inf.message_bytes(by_conn[1][0]) == big
    assert [inf.message_bytes(m) for m in by_conn[2]] == text
    bad_m, pend_m = by_conn[3][1], by_conn[4][1]
    assert int(irec["status"][bad_m]) == gev_amd.MSG_ERR_DEFLATE and int(irec["flags"][pend_m]) == gev_amd.INF_PENDING
    # the join on the inflate's own buffer: out_cap is the whole of it
    before = inf.out.cpu().numpy()
    tables = dict(frames=batch.frames, n_frames=msgs.n_frames, messages=msgs.messages, n_messages=n,
                  msg_of=msgs.msg_of, summary=msgs.summary, payload=batch.payload)
    for flags in (jm.JOIN_ALL, 0):
        out = inf.out.clone()
        w = jm.join_model(d.frames, d.arena, want_t["messages"], want_t["msg_of"], flags, out.numel(), irec,
                          dict(payload_bytes=int(isum["payload_bytes"]), status=0), out_image=before)
        g = jm.run_join(engine, tables, flags, out.numel(), inf.inflated, inf.summary, out=out)
        assert np.array_equal(g["out"][: out.numel()], w["out"])
        assert w["base"] == inf_need and np.array_equal(g["out"][:inf_need], before[:inf_need])  # the inflate's bytes
        gb, wb = g["bodies"], w["bodies"]
        assert gb.tobytes() == wb.tobytes(), flags
        assert summary_of(g) == tuple(w["summary"].values())
        infl = np.flatnonzero(gb["flags"] == jm.WHOLE | jm.INFLATED)
        assert list(infl) == [by_conn[0][0], by_conn[1][0], *by_conn[2]]
        assert np.array_equal(gb["off"][infl], irec["out_off"][infl]) and \
            np.array_equal(gb["length"][infl], irec["length"][infl])
        assert int(gb["flags"][bad_m]) == 0 and int(gb["status"][bad_m]) == gev_amd.MSG_ERR_DEFLATE
        assert int(gb["flags"][pend_m]) == 0
        if flags:
            assert int(g["summary"]["payload_bytes"]) == cap == out.numel()  # the last body ends at out_cap
            assert np.all(gb["off"][gb["flags"] == jm.WHOLE | jm.JOINED] >= inf_need)
    # d_inflated == NULL: no compressed message is delivered, and the bodies start at 0
    w0 = jm.join_model(d.frames, d.arena, want_t["messages"], want_t["msg_of"], jm.JOIN_ALL, plain_need)
    g0 = jm.run_join(engine, tables, jm.JOIN_ALL, plain_need)
    jm.assert_join(g0, w0, plain_need, "no inflate records")
    comp_m = np.flatnonzero(want_t["messages"]["flags"] & gm.COMPRESSED)
    assert comp_m.size == 7 and not g0["bodies"]["flags"][comp_m].any()
    # Engine.join keeps the inflated bytes below base and reads every body from the right arena
    bodies = engine.join(batch, msgs, inf)
    assert bodies.body_bytes(by_conn[1][0]) == big and [bodies.body_bytes(m) for m in by_conn[2]] == text
    assert bodies.body_bytes(by_conn[5][0]) == conns[5][0][3] and bodies.body_bytes(bad_m) == b""
    assert bodies.body_bytes(by_conn[3][0]) == b"".join(f[3] for f in conns[3][:3])
    assert int(bodies.bodies_host()["flags"][by_conn[5][0]]) == jm.WHOLE  # left in the payload arena
    # ... and grows its arena once when out_cap is too small, the inflated bytes carried over
    grown = engine.join(batch, msgs, inf, flags=jm.JOIN_ALL, out_cap=64)
    assert grown.out_cap == cap and int(grown.summary_host()["payload_bytes"]) == cap
    assert grown.body_bytes(by_conn[1][0]) == big and [grown.body_bytes(m) for m in by_conn[2]] == text
    assert grown.body_bytes(by_conn[5][0]) == conns[5][0][3]
    assert int(grown.bodies_host()["flags"][by_conn[5][0]]) == jm.WHOLE | jm.JOINED


def summary_of(g):
    return jm.summary_tuple(g["summary"])


# ---------------------------------------------------------------------------- capacity and gates
def test_capacity_and_retry(engine):
    rng = np.random.default_rng(0x6A6F09)
    conns = [message(rng, [10, 20]), message(rng, [5000, 1]), message(rng, [16])]
    need = 32 + 5008 + 16
    g, w, _, _ = join_both(engine, conns, jm.JOIN_ALL, out_cap=need - 1, tag="one byte short")
    assert summary_of(g) == (3, need, 5047, 0, gev_amd.ERR_CAPACITY)
    assert np.all(g["bodies_raw"] == jm.FILL) and np.all(g["out"] == jm.FILL)
    g, _, _, _ = join_both(engine, conns, jm.JOIN_ALL, out_cap=need, tag="the retry")
    assert summary_of(g) == (3, need, 5047, 0, 0)


def poke(summary_dev, **fields):
    """A copy of a device summary with some fields replaced."""
    s = summary_dev.cpu().numpy().copy().view(mm.SUMMARY_DTYPE)
    for k, v in fields.items():
        s[k] = v
    return mm._dev(s, summary_dev.device, 64)


def test_gates_give_zero_summaries(engine):
    import torch
    rng = np.random.default_rng(0x6A6F0A)
    d = mm.Decoded([message(rng, [10, 20]), message(rng, [30])])
    got = gm.run_messages_ext(engine, d, None)
    t = dict(got["dev"])
    dev = t["frames"].device
    zero = (0, 0, 0, 0, 0)

    def untouched(g, tag):
        assert summary_of(g) == zero, tag
        assert np.all(g["bodies_raw"] == jm.FILL) and np.all(g["out"] == jm.FILL), tag
    t["summary"] = poke(got["dev"]["summary"], status=gev_amd.ERR_CAPACITY)
    untouched(jm.run_join(engine, t, jm.JOIN_ALL, 256), "a failed message summary")
    t["summary"] = poke(got["dev"]["summary"], frames=0)
    untouched(jm.run_join(engine, t, jm.JOIN_ALL, 256), "no messages")
    t["summary"] = got["dev"]["summary"]
    inf = torch.zeros(2 * 32, dtype=torch.uint8, device=dev)
    isum = mm._dev(np.zeros(1, mm.SUMMARY_DTYPE), dev, 64)
    untouched(jm.run_join(engine, t, jm.JOIN_ALL, 256, inf, poke(isum, status=gev_amd.ERR_CAPACITY, payload_bytes=40)),
              "a failed inflate summary")
    g = jm.run_join(engine, t, jm.JOIN_ALL, 256, inf, poke(isum, payload_bytes=40))  # ... and the same one, OK
    assert summary_of(g) == (2, 48 + 32 + 32, 60, 0, 0) and [int(x) for x in g["bodies"]["off"]] == [48, 80]
    assert np.all(g["out"][:48] == jm.FILL) and np.all(g["out"][112:] == jm.FILL)
    t["n_messages"] = 0  # max_messages == 0
    untouched(jm.run_join(engine, t, jm.JOIN_ALL, 256), "max_messages 0")
    # connections with control frames only: a message pass without messages
    join_both(engine, [[(1, 0, PING, b"p")], [(1, 0, PONG, b"")]], jm.JOIN_ALL, out_cap=64)


# ---------------------------------------------------------------------------- the scan, a random batch
def test_scan_across_blocks(engine):
    rng = np.random.default_rng(0x6A6F0B)
    n = 2 * SIZE_BLOCK + 88  # crosses the sizing kernel's block boundary twice
    conns = []
    for c in range(n // 5):
        conns.append(sum((message(rng, [2, 1]) for _ in range(5)), []))
    g, w, _, _ = join_both(engine, conns)
    assert int(g["summary"]["frames"]) == n and int(g["summary"]["payload_bytes"]) == 16 * n
    assert np.array_equal(g["bodies"]["off"], 16 * np.arange(n, dtype=np.uint64))
    # ... and with bodies that stay in place in between
    conns = [message(rng, [3]) + message(rng, [2, 1]) + message(rng, [0]) for _ in range(n // 2)]
    join_both(engine, conns, tag="mixed")


def test_random_batch(engine):
    rng = np.random.default_rng(0x6A6F0C)
    conns = []
    for c in range(300):
        conn = []
        for _ in range(int(rng.integers(1, 4))):
            total = int(rng.integers(0, 20001)) if rng.random() < 0.5 else int(rng.integers(0, 200))
            k = int(rng.integers(1, 9))
            cuts = sorted(int(x) for x in rng.integers(0, total + 1, k - 1))
            lens = [b - a for a, b in zip([0, *cuts], [*cuts, total])]
            conn += message(rng, lens, between=lambda i: [(1, 0, PING if i % 2 else PONG, rnd(rng, i % 126))]
                            if rng.random() < 0.3 else [])
        if c % 37 == 0:
            conn[-1] = (0,) + conn[-1][1:]  # the last message stays open
        conns.append(conn)
    for flags in (0, jm.JOIN_ALL):
        join_both(engine, conns, flags, tag=f"flags {flags}")
