"""GPU checks of permessage-deflate: the message pass with RSV1
(gevws_messages_ext_async) and the inflate step behind it
(gevws_inflate_async), on hand-built decoded batches and behind a real decode.
Every comparison is exact.  Expected bytes of well-formed streams are zlib's;
the Python model (tests/_inflate_model.py, pinned on the CPU against zlib)
gives the verdicts of small malformed streams; the tables come from
tests/_inflate_gpu_model.py.  Pad bytes of the hand-built arenas are 0xFF, so a
read past hdr.length changes the stream."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _inflate_corpus as ic
from tests import _inflate_gpu_model as gm
from tests import _inflate_model as im
from tests import _messages_model as mm
from tests._helpers import gpu_decode, pack_streams

pytestmark = pytest.mark.gpu

T, B, C, PING = 1, 2, 0, 9
RSV1, RSV2, RSV3 = 4, 2, 1
BIG = 1 << 24  # an output limit nothing here reaches


def frames_of(payload: bytes, op: int = B, cuts=(), between=None):
    """One compressed message as frames: the payload cut at `cuts`, RSV1 on the
    first frame only; `between` = a frame put after each fragment but the last."""
    edges = [0, *cuts, len(payload)]
    out = []
    for i in range(len(edges) - 1):
        last = i == len(edges) - 2
        out.append((1 if last else 0, RSV1 if i == 0 else 0, op if i == 0 else C, payload[edges[i]:edges[i + 1]]))
        if between is not None and not last:
            out.append(between)
    return out


def run_both(engine, conns, limit=BIG, out_cap=None, ext=None, state=None, tag=""):
    """Message pass + inflate step on hand-built connections (all deflate unless
    `ext` says otherwise), both compared with the model; returns (device, model)."""
    d = mm.Decoded(conns, pad=0xFF)
    ext = np.ones(len(conns), np.uint8) if ext is None else np.asarray(ext, np.uint8)
    got = gm.run_messages_ext(engine, d, ext, state)
    want = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, state, ext)
    mm.assert_tables_equal(got, want, tag)
    winf = gm.model_inflate(d, want, limit, want["state"])
    cap = winf["payload_bytes"] if out_cap is None else out_cap
    ginf = gm.run_inflate(engine, got, limit, cap)
    gm.assert_inflated(ginf, winf, cap, tag)
    return ginf, winf


# ---------------------------------------------------------------------------- 1. the message pass and RSV1
def test_rsv1_rules_per_connection(engine):
    hello = ic.deflate(b"Hello")
    conns = [
        [(1, RSV1, T, hello)],                                   # compressed text, one frame
        [(0, RSV1, B, hello[:3]), (1, 0, C, hello[3:])],         # fragmented: RSV1 on the first frame only
        [(0, RSV1, T, hello[:3]), (1, RSV1, C, hello[3:])],      # RSV1 on a continuation frame
        [(0, RSV1, T, hello[:3]), (1, RSV1, PING, b"")],         # RSV1 on a control frame
        [(1, RSV1 | RSV2, T, hello)],                            # RSV2
        [(1, RSV3, B, b"x")],                                    # RSV3
        [(1, 0, T, b"plain \xe2\x82\xac")],                      # a plain message on a deflate connection
        [(1, 0, T, b"\xff")],                                    # ... still UTF-8-checked
        [(1, RSV1, T, b"\xff\xff\xff")],                         # compressed text: no UTF-8 verdict here
        [(1, RSV1, T, hello)],                                   # a plain connection: RSV1 is an error
        [(1, RSV1, 3, hello)],                                   # RSV1 allowed, the opcode is not
    ]
    ext = [1] * 9 + [0, 1]
    d = mm.Decoded(conns, pad=0xFF)
    got = gm.run_messages_ext(engine, d, np.array(ext, np.uint8))
    want = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, None, np.array(ext, np.uint8))
    mm.assert_tables_equal(got, want)
    assert list(got["conn_msg"]["error"]) == [0, 0, mm.ERR_RSV, mm.ERR_RSV, mm.ERR_RSV, mm.ERR_RSV, 0, mm.ERR_UTF8, 0,
                                              mm.ERR_RSV, mm.ERR_OPCODE]
    flags = got["messages"]["flags"]
    assert flags[0] == flags[1] == mm.BEGIN | mm.END | gm.COMPRESSED
    assert int(got["summary"]["payload_len"]) == len(b"plain \xe2\x82\xac") + 1  # compressed text does not count


def test_compressed_flag_is_carried_by_the_state(engine):
    hello = ic.deflate(b"Hello, again and again and again")
    first = [[(0, RSV1, T, hello[:5])], [(0, 0, T, b"ab\xe2")], [(0, RSV1, B, hello[:2]), (1, 0, PING, b"p")]]
    second = [[(1, 0, C, hello[5:])], [(1, 0, C, b"\x82\xac")], [(1, 0, C, hello[2:])]]
    ext = np.ones(3, np.uint8)
    d1, d2 = mm.Decoded(first, pad=0xFF), mm.Decoded(second, pad=0xFF)
    g1 = gm.run_messages_ext(engine, d1, ext)
    w1 = gm.model_ext(d1.frames, d1.conn_out, d1.n_decoded, d1.arena, None, ext)
    mm.assert_tables_equal(g1, w1, "first pass")
    assert list(g1["state"]["reserved"][:, 0]) == [1, 0, 1] and list(g1["state"]["utf8_n"]) == [0, 1, 0]
    g2 = gm.run_messages_ext(engine, d2, ext, g1["state"])
    w2 = gm.model_ext(d2.frames, d2.conn_out, d2.n_decoded, d2.arena, w1["state"], ext)
    mm.assert_tables_equal(g2, w2, "second pass")
    assert list(g2["messages"]["flags"]) == [mm.END | gm.COMPRESSED, mm.END, mm.END | gm.COMPRESSED]
    assert not g2["state"].view(np.uint8).any()
    # neither half is whole in its pass: PENDING, nothing inflated
    for g, d, w in ((g1, d1, w1), (g2, d2, w2)):
        inf = gm.run_inflate(engine, g, BIG, 256)
        gm.assert_inflated(inf, gm.model_inflate(d, w, BIG, w["state"]), 256)
        assert list(inf["inflated"]["flags"]) == [gm.INF_PENDING, 0, gm.INF_PENDING]
    # the same state on a plain pass: the flag is ignored and dropped
    g3 = gm.run_messages_ext(engine, d2, None, g1["state"])
    mm.assert_tables_equal(g3, d2.model(g1["state"]), "plain pass")
    assert not (g3["messages"]["flags"] & gm.COMPRESSED).any() and not g3["state"]["reserved"].any()


def test_null_or_zero_ext_is_the_plain_pass(engine):
    rng = np.random.default_rng(0x706C61)
    conns = []
    for _ in range(200):
        conn = []
        for _ in range(int(rng.integers(1, 7))):
            conn.append((int(rng.random() < 0.7), int(rng.choice([0, 0, 0, 0, 4, 2, 1])),
                         int(rng.choice([0, 1, 2, 2, 9, 10, 3])), ic.sample(rng, int(rng.integers(0, 60)), 0)))
        conns.append(conn)
    d = mm.Decoded(conns, pad=0xFF)
    plain = mm.run_device(engine, d)
    mm.assert_tables_equal(plain, d.model())
    for ext in (None, np.zeros(len(conns), np.uint8)):
        got = gm.run_messages_ext(engine, d, ext)
        for k in ("messages", "msg_of", "conn_msg", "state"):
            assert got[k].tobytes() == plain[k].tobytes(), k
        assert got["summary"].tobytes() == plain["summary"].tobytes()


# ---------------------------------------------------------------------------- 2. block types and sizes
SIZES = [0, 1, 15, 16, 17, 257, 258, 259, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 70000, 300000]


def test_levels_strategies_and_sizes(engine):
    rng = np.random.default_rng(0x73697A)
    combos = [(lv, sg) for lv in ic.LEVELS for sg in ic.STRATEGIES]
    conns, k = [], 0
    for n in SIZES:
        # every level x strategy at the small sizes, four of them (rotating) at the large ones
        use = combos if n <= 4097 else [combos[(k + 5 * j) % 16] for j in range(4)] + [(0, zlib.Z_DEFAULT_STRATEGY)]
        for lv, sg in use:
            data = ic.sample(rng, n, k % 4)
            conns.append(frames_of(ic.deflate(data, lv, sg), T if k % 4 in (2, 3) else B))  # (ASCII kinds as text)
            k += 1
    ginf, winf = run_both(engine, conns)
    assert winf["errors"] == 0 and winf["frames"] == len(conns)
    assert sorted(set(int(x) for x in ginf["inflated"]["length"])) == sorted(SIZES)


# ---------------------------------------------------------------------------- 3. hand-assembled fixed-Huffman streams
class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):            # LSB first: header fields, extra bits
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):           # a Huffman code, MSB first
        self.bits += [(v >> i) & 1 for i in reversed(range(n))]

    def lit(self, s):               # the fixed literal / length code
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length, dist):
        ls = max(i for i, b in enumerate(im.LEN_BASE) if b <= length and (i < 28 or length == 258))
        self.lit(257 + ls)
        self.put(length - im.LEN_BASE[ls], im.LEN_EXTRA[ls])
        ds = max(i for i, b in enumerate(im.DIST_BASE) if b <= dist)
        self.code(ds, 5)
        self.put(dist - im.DIST_BASE[ds], im.DIST_EXTRA[ds])

    def fixed(self, final=0):
        self.put(final, 1), self.put(1, 2)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


def sync(w: BitWriter) -> bytes:
    """End of block, then the sync flush's empty stored block minus its tail."""
    w.lit(256)
    w.put(0, 3)
    return w.bytes()


def literals(w: BitWriter, data: bytes):
    for c in data:
        w.lit(c)


def test_hand_assembled_fixed_huffman_streams(engine):
    rng = np.random.default_rng(0x666978)
    conns, want = [], []

    def add(w, data, status=im.OK, raw=None):
        conns.append(frames_of(sync(w) if raw is None else raw))
        want.append((status, data))

    seed = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    # distance 32 768 exactly (zlib's compressor never emits it)
    w = BitWriter()
    w.fixed(), literals(w, seed)
    total = bytearray(seed)
    while len(total) < 32768:                      # runs of the last byte: distance 1
        w.match(258, 1)
        total += bytes([total[-1]]) * 258
    w.match(200, 32768)
    total += total[len(total) - 32768:][:200]
    add(w, bytes(total))
    # distance = bytes so far + 1
    w = BitWriter()
    w.fixed(), literals(w, seed[:40]), w.match(3, 41)
    add(w, b"", im.ERR_DEFLATE)
    # ... and = bytes so far, the longest legal reach
    w = BitWriter()
    w.fixed(), literals(w, seed[:40]), w.match(50, 40)
    add(w, seed[:40] + (seed[:40] * 3)[:50])
    # distance 1 with length 258
    w = BitWriter()
    w.fixed(), literals(w, b"z"), w.match(258, 1)
    add(w, b"z" * 259)
    # overlaps with distance 2, 3, 63, 64, 65 (a lane's stride) and length 258
    w = BitWriter()
    w.fixed(), literals(w, seed[:70])
    data = bytearray(seed[:70])
    for dist in (2, 3, 63, 64, 65, 7):
        w.match(258, dist)
        for _ in range(258):
            data.append(data[-dist])
    add(w, bytes(data))
    # a match that straddles the window wrap: the output passes 32 768 inside it
    w = BitWriter()
    w.fixed(), literals(w, seed)
    data = bytearray(seed)
    while len(data) + 258 <= 32768 - 100:
        w.match(258, 300)
        for _ in range(258):
            data.append(data[-300])
    literals(w, seed[: 32768 - 100 - len(data)])
    data += seed[: 32768 - 100 - len(data)]
    assert len(data) == 32768 - 100
    for dist in (300, 32768 - 100, 1):
        w.match(258, dist)
        for _ in range(258):
            data.append(data[-dist])
    add(w, bytes(data))
    # a BFINAL block followed by garbage
    w = BitWriter()
    w.fixed(final=1), literals(w, b"the end"), w.lit(256)
    add(w, b"the end", raw=w.bytes() + bytes(rng.integers(0, 256, 40, dtype=np.uint8)))
    # length symbols 286 / 287 and distance symbols 30 / 31
    for sym in (286, 287):
        w = BitWriter()
        w.fixed(), literals(w, b"abc"), w.lit(sym), w.code(0, 5)
        add(w, b"", im.ERR_DEFLATE)
    for ds in (30, 31):
        w = BitWriter()
        w.fixed(), literals(w, b"abc"), w.lit(257), w.code(ds, 5)
        add(w, b"", im.ERR_DEFLATE)
    # block type 3
    w = BitWriter()
    w.put(0, 1), w.put(3, 2)
    add(w, b"", im.ERR_DEFLATE, raw=w.bytes() + b"\0\0")

    for fr, (status, data) in zip(conns, want):  # the expectations themselves, against zlib
        raised, z = ic.zlib_inflate(fr[0][3])
        assert (raised, z) == (status != im.OK, data if status == im.OK else b"")
    ginf, winf = run_both(engine, conns)
    assert [int(s) for s in ginf["inflated"]["status"]] == [s for s, _ in want]
    assert [winf["bytes"][m] for m in range(len(want))] == [d for _, d in want]


# ---------------------------------------------------------------------------- 4. fragments
def test_fragment_boundaries(engine):
    data = b"fragmented frames, fragmented frames!"
    dyn = ic.deflate(data, 9)                                  # fixed or dynamic, about 30 bytes
    stored = ic.deflate(data, 0)                               # 00, LEN, NLEN, the bytes
    assert 20 <= len(dyn) <= 40 and stored[1:5] == bytes([len(data), 0, 255 - len(data), 255])
    ping = (1, 0, PING, b"ping!")
    conns = []
    for p in (dyn, stored):
        conns += [frames_of(p, T, [k]) for k in range(len(p) + 1)]           # in two at every byte (and empty halves)
    conns.append(frames_of(dyn, T, list(range(1, len(dyn)))))               # one-byte fragments
    conns.append(frames_of(stored, B, list(range(1, len(stored)))))
    conns.append(frames_of(dyn, T, [0, 0, 7, 7, 7, len(dyn), len(dyn)]))    # zero-length fragments
    conns.append(frames_of(dyn, T, [5, 11], between=ping))                  # a ping between fragments
    conns.append(frames_of(stored, T, [1, 2, 3, 4], between=ping))          # LEN / NLEN cut byte by byte
    big = ic.deflate(ic.sample(np.random.default_rng(4), 5000, 1), 0)       # refills inside a fragment: 1 KiB loads
    conns.append(frames_of(big, B, [1023, 1024, 1025, 2048, 3000]))
    conns.append(frames_of(big, B, [4097]))
    ginf, winf = run_both(engine, conns)
    assert winf["errors"] == 0 and all(winf["bytes"][m] == data for m in range(len(conns) - 2))
    # two messages on one connection, a ping between them
    run_both(engine, [frames_of(dyn, T) + [ping] + frames_of(stored, B, [9])], tag="two messages")


# ---------------------------------------------------------------------------- 5. malformed streams
def test_malformed_streams_match_the_model(engine):
    rng = np.random.default_rng(0x6D616C)
    streams = ic.malformed_streams(rng, 2000)
    conns = [frames_of(p, B if i % 3 else T) for i, p in enumerate(streams)]
    for limit in (BIG, 40):
        ginf, winf = run_both(engine, conns, limit=limit, tag=f"limit {limit}")
        st = winf["inflated"]["status"]
        assert (st == im.ERR_DEFLATE).sum() > 500 and (st == im.OK).sum() > 100
    assert (st == im.ERR_TOO_BIG).sum() > 100


# ---------------------------------------------------------------------------- 6. limits and tables
def test_max_message_bytes(engine):
    rng = np.random.default_rng(0x6C696D)
    for n, kind, level in ((3000, 0, 6), (3000, 1, 0), (70000, 2, 9), (1 << 20, None, 9)):
        data = bytes(n) if kind is None else ic.sample(rng, n, kind)
        conns = [frames_of(ic.deflate(data, level))]
        for limit, status in ((n, im.OK), (n - 1, im.ERR_TOO_BIG), (1, im.ERR_TOO_BIG)):
            ginf, _ = run_both(engine, conns, limit=limit, tag=f"{n} / {limit}")
            assert int(ginf["inflated"]["status"][0]) == status


def test_capacity_then_retry(engine):
    rng = np.random.default_rng(0x636170)
    conns = [frames_of(ic.deflate(ic.sample(rng, n, 0))) for n in (100, 1, 777, 16)]
    d = mm.Decoded(conns, pad=0xFF)
    ext = np.ones(len(conns), np.uint8)
    got = gm.run_messages_ext(engine, d, ext)
    want = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, None, ext)
    winf = gm.model_inflate(d, want, BIG, want["state"])
    need = winf["payload_bytes"]
    assert need == 112 + 16 + 784 + 16
    state_before = got["dev"]["state"].cpu().numpy().copy()
    short = gm.run_inflate(engine, got, BIG, need - 1)
    s = short["summary"]
    assert int(s["status"]) == gev_amd.ERR_CAPACITY and int(s["payload_bytes"]) == need
    assert np.all(short["out"] == 0xEE) and np.all(short["inflated"].view(np.uint8) == 0xEE)
    assert np.array_equal(got["dev"]["state"].cpu().numpy(), state_before)
    gm.assert_inflated(gm.run_inflate(engine, got, BIG, need), winf, need)


def test_state_failed_pending_and_plain_messages(engine):
    hello, bad = ic.deflate(b"Hello"), b"\x06garbage"
    latin = ic.deflate(b"caf\xe9")                                   # valid DEFLATE, invalid UTF-8 once inflated
    assert im.inflate(bad)[0] == im.ERR_DEFLATE
    conns = [
        frames_of(hello, T) + frames_of(bad, B) + frames_of(latin, T) + frames_of(hello, B),  # first failure wins
        frames_of(latin, T) + frames_of(bad, B),                     # ERR_UTF8 first; bytes kept
        frames_of(latin, B),                                         # binary: not text, OK
        [(1, 0, T, b"plain text")] + frames_of(hello, T),            # a plain message: untouched
        frames_of(hello, T) + [(0, RSV1, B, hello[:3])],             # the second has no END: PENDING
        [(1, 0, T, b"\xff")] + frames_of(hello, T),                  # failed in the message pass: nothing after it
    ]
    ginf, winf = run_both(engine, conns)
    inf = ginf["inflated"]
    assert [int(x) for x in inf["status"][:4]] == [0, im.ERR_DEFLATE, mm.ERR_UTF8, 0]
    assert [int(x) for x in ginf["state"]["failed"]] == [im.ERR_DEFLATE, mm.ERR_UTF8, 0, 0, 0, mm.ERR_UTF8]
    assert int(inf["length"][4]) == 4 and winf["bytes"][4] == b"caf\xe9"          # conn 1's ERR_UTF8 message
    assert [int(x) for x in inf["flags"][7:]] == [0, gm.INF_DONE, gm.INF_DONE, gm.INF_PENDING, 0]
    # without a state nothing is kept, the tables are the same
    d = mm.Decoded(conns, pad=0xFF)
    got = gm.run_messages_ext(engine, d, np.ones(len(conns), np.uint8))
    again = gm.run_inflate(engine, got, BIG, winf["payload_bytes"], use_state=False)
    assert again["inflated"].tobytes() == inf.tobytes() and again["state"] is None


def test_empty_and_failed_message_summary(engine):
    import torch
    hello = ic.deflate(b"Hello")
    d = mm.Decoded([frames_of(hello, T)], pad=0xFF)
    got = gm.run_messages_ext(engine, d, np.ones(1, np.uint8))
    for status, frames in ((gev_amd.ERR_CAPACITY, 1), (0, 0)):
        s = got["summary"].copy()
        s["status"], s["frames"] = status, frames
        got["dev"]["summary"].copy_(torch.from_numpy(np.frombuffer(s.tobytes(), np.uint8).copy()))
        inf = gm.run_inflate(engine, got, BIG, 64)
        assert not inf["summary"].tobytes().strip(b"\0"), status
        assert np.all(inf["out"] == 0xEE) and np.all(inf["inflated"].view(np.uint8) == 0xEE)
    # no messages at all: max_messages == 0
    none = gm.run_messages_ext(engine, mm.Decoded([[(1, 0, PING, b"")]], pad=0xFF), np.ones(1, np.uint8))
    assert none["dev"]["n_messages"] == 0
    inf = gm.run_inflate(engine, none, BIG, 64)
    assert not inf["summary"].tobytes().strip(b"\0") and np.all(inf["out"] == 0xEE)


# ---------------------------------------------------------------------------- 7. behind a real decode
def test_inflate_behind_a_decode(engine):
    import torch
    rng = np.random.default_rng(0x726561)
    streams, texts, ext = [], [], []
    for c in range(64):
        deflate = c % 4 != 3
        data = ic.sample(rng, int(rng.integers(0, 20000)), 0 if c % 2 else 2).decode("utf-8", "ignore").encode()
        payload = ic.deflate(data, int(rng.choice(ic.LEVELS))) if deflate else data
        cuts = sorted(int(x) for x in rng.integers(0, len(payload) + 1, int(rng.integers(0, 4))))
        s = b""
        for fin, rsv, op, part in frames_of(payload, T, cuts, between=(1, 0, PING, b"hb")):
            s += wo.encode_frame(part, op, bool(fin), rsv if deflate else 0, True,
                                 bytes(rng.integers(0, 256, 4, dtype=np.uint8)))
        streams.append(s), texts.append(data), ext.append(int(deflate))
    arena, table = pack_streams(streams)
    out = gpu_decode(engine, arena, table)
    dev = out.frames.device
    conn_ext = torch.from_numpy(np.array(ext, np.uint8)).to(dev)
    state = torch.zeros((len(streams), 8), dtype=torch.uint8, device=dev)
    msgs = engine.messages(out, state=state, conn_ext=conn_ext)
    m = msgs.messages_host()
    assert m.shape[0] == 64 and np.array_equal(m["flags"] & gm.COMPRESSED != 0, np.array(ext, bool))
    res = engine.inflate(out, msgs, 1 << 20, state=state, out_cap=64)       # grows once on ERR_CAPACITY
    inf = res.inflated_host()
    s = res.summary_host()
    assert int(s["frames"]) == sum(ext) and int(s["errors"]) == 0
    assert int(s["payload_len"]) == sum(len(t) for t, e in zip(texts, ext) if e)
    for c in range(64):
        if ext[c]:
            assert int(inf["flags"][c]) == gm.INF_DONE and res.message_bytes(c) == texts[c], c
        else:
            assert not inf[c].tobytes().strip(b"\0") and res.message_bytes(c) == b""
    assert not state.cpu().numpy().any()
