"""GPU checks of outbound fragmentation (gevws_fragment_async,
gevws_fragment_offsets_async) through the C ABI, bit-exact against
tests/_fragment_model.py -- the fragments, both tables, the summaries,
everything else still the 0xEE it was prefilled with -- and of the whole chain
with a frame size limit (Engine.respond / Engine.broadcast with
max_fragment_bytes): every connection's bytes are parsed with the oracle's
frame parser, reassembled and compared with the messages, and fed back through
the project's own decode -> messages -> inflate -> join."""
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _fragment_model as fm
from tests import _messages_model as mm
from tests._helpers import gpu_decode

pytestmark = pytest.mark.gpu

T, B, C, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
D, TK = gev_amd.EXT_DEFLATE, gev_amd.EXT_DEFLATE | gev_amd.EXT_SERVER_TAKEOVER
BLOCK = 256  # records a workgroup (kWalkBlock)


def filled(nbytes, dev):
    import torch
    return torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)


def run_fragment(engine, recs, F, max_frags, prev=None, max_records=None):
    """gevws_fragment_async over 0xEE-filled outputs: the raw bytes of (frags, first, summary)."""
    import torch
    dev = torch.device("cuda", engine.device)
    recs = np.ascontiguousarray(recs)
    n = len(recs) if max_records is None else max_records
    d_recs = mm._dev(recs, dev, 32)
    d_prev = None if prev is None else mm._dev(np.array([prev]), dev, 64)
    frags, first, summary = filled((max_frags + 1) * 32, dev), filled((n + 2) * 8, dev), filled(64, dev)
    engine.fragment_async(d_recs, n, d_prev, F, frags, max_frags, first, summary)
    torch.cuda.synchronize(engine.device)
    return frags.cpu().numpy(), first.cpu().numpy(), summary.cpu().numpy().view(fm.SUMMARY_DTYPE)[0]


def fragment_both(engine, recs, F, max_frags, prev=None, max_records=None, tag=""):
    """Device == model, byte for byte; what the contract does not name stays 0xEE."""
    want_f, want_first, want_s = fm.fragment(recs, F, max_frags, prev, max_records)
    frags, first, s = run_fragment(engine, recs, F, max_frags, prev, max_records)
    assert s.tobytes() == want_s.tobytes(), (tag, s, want_s)
    if want_f is None:
        assert (frags == 0xEE).all() and (first == 0xEE).all(), tag
        return s
    k, m = len(want_f) * 32, len(want_first) * 8
    assert frags[:k].tobytes() == want_f.tobytes(), tag
    assert (frags[k:] == 0xEE).all(), tag
    assert first[:m].tobytes() == want_first.tobytes() and (first[m:] == 0xEE).all(), tag
    return s


# ---------------------------------------------------------------------------- 1. the step against the model
@pytest.mark.parametrize("F", fm.LIMITS)
def test_step_matches_the_model(engine, F):
    rng = np.random.default_rng(0x67667200 + F)
    recs = fm.shape_records(F, rng)
    s = fragment_both(engine, recs, F, 1 << 12, tag=(F, "shapes"))
    need = int(s["frames"])
    assert int(s["status"]) == 0 and int(s["payload_bytes"]) >= 12 and need > len(recs)
    fragment_both(engine, recs, F, need, tag=(F, "exact room"))
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 1):   # across kWalkBlock and the block scan
        rr = fm.random_records(n, F, rng, max_len=3 * F + 7)
        s = fragment_both(engine, rr, F, 12 * n, tag=(F, n))
        assert int(s["status"]) == 0


def test_one_record_of_4097_fragments(engine):
    """The emit's bisection crosses workgroups inside one record, between one-fragment neighbours."""
    recs = np.array([fm.record(1, off=0), fm.record(0, off=16), fm.record(4097, opcode=2, rsv=4, off=32),
                     fm.record(1, opcode=2, off=8192), fm.record(300, opcode=9, off=8208)], fm.OUT_FRAME_DTYPE)
    s = fragment_both(engine, recs, 1, 5000, tag="4097")
    assert (int(s["frames"]), int(s["payload_bytes"])) == (4097 + 4, 1)
    fragment_both(engine, recs, 1, 4101, tag="4097 exact")


def test_gate(engine):
    rng = np.random.default_rng(0x67667210)
    recs = fm.random_records(300, 9, rng)
    # a count below max_records: only those records, d_first ends behind them
    s = fragment_both(engine, recs, 9, 4000, prev=fm.summary(frames=257), tag="count")
    assert int(s["frames"]) == int(fm.fragment(recs[:257], 9, 4000)[2]["frames"])
    fragment_both(engine, recs, 9, 4000, prev=fm.summary(frames=0), tag="no records")
    fragment_both(engine, recs, 9, 4000, prev=fm.summary(frames=1000), tag="more than max_records")
    # a failed step before: a zero summary, nothing else
    for st in (gev_amd.ERR_CAPACITY, gev_amd.ERR_INVALID):
        s = fragment_both(engine, recs, 9, 4000, prev=fm.summary(frames=300, status=st), tag=st)
        assert s.tobytes() == fm.summary().tobytes()


# ---------------------------------------------------------------------------- 2. capacity and malformed
def test_capacity_and_malformed(engine):
    rng = np.random.default_rng(0x67667220)
    recs = fm.random_records(600, 5, rng)
    need = int(fm.fragment(recs, 5, 1 << 20)[2]["frames"])
    s = fragment_both(engine, recs, 5, need - 1, tag="capacity")
    assert (int(s["status"]), int(s["frames"])) == (gev_amd.ERR_CAPACITY, need)
    s = fragment_both(engine, recs, 5, need, tag="fits")
    assert int(s["status"]) == 0
    s = fragment_both(engine, recs, 5, 0, tag="no room at all")
    assert (int(s["status"]), int(s["frames"])) == (gev_amd.ERR_CAPACITY, need)
    # 2^40 bytes at one byte a frame: malformed (no payload memory is needed, the step reads none)
    big = recs.copy()
    big[311] = fm.record(1 << 40, opcode=2, off=1 << 41)
    s = fragment_both(engine, big, 1, 1 << 12, tag="malformed")
    assert (int(s["status"]), int(s["errors"]), int(s["frames"]), int(s["payload_len"])) == \
        (gev_amd.ERR_INVALID, 1, 0, 0)
    # the same record is fine at a limit that leaves it 2^31 - 1 fragments at the most (then the room is short)
    s = fragment_both(engine, big, 1 << 10, 1 << 12, tag="2^30 fragments")
    assert (int(s["status"]), int(s["errors"])) == (gev_amd.ERR_CAPACITY, 0) and int(s["frames"]) > 1 << 30


# ---------------------------------------------------------------------------- 3. the offsets behind the encode
def run_offsets(engine, first, n, prev, fragged, frag_off, enc):
    import torch
    dev = torch.device("cuda", engine.device)
    d = lambda s: None if s is None else mm._dev(np.array([s]), dev, 64)  # noqa: E731
    d_first = mm._dev(np.asarray(first, np.uint64), dev, 16)
    d_off = mm._dev(np.asarray(frag_off, np.uint64), dev, 16)
    reply_off, rsum = filled((n + 1) * 8, dev), filled(64, dev)
    engine.fragment_offsets_async(d_first, n, d(prev), d(fragged), d_off, d(enc), reply_off, rsum)
    torch.cuda.synchronize(engine.device)
    return reply_off.cpu().numpy(), rsum.cpu().numpy().view(fm.SUMMARY_DTYPE)[0]


def offsets_both(engine, first, n, prev, fragged, frag_off, enc, tag=""):
    want_off, want_s = fm.offsets(first, n, prev, fragged, frag_off, enc)
    off, s = run_offsets(engine, first, n, prev, fragged, frag_off, enc)
    assert s.tobytes() == want_s.tobytes(), (tag, s, want_s)
    if want_off is None:
        assert (off == 0xEE).all(), tag
        return s
    k = len(want_off) * 8
    assert off[:k].tobytes() == want_off.tobytes() and (off[k:] == 0xEE).all(), tag
    return s


def synthetic(recs, F):
    """The fragment step's tables and an encode's as it would leave them (a 2-byte header a frame)."""
    frags, first, s = fm.fragment(recs, F, 1 << 20)
    sizes = [2 + int(x) for x in frags["payload_len"]]
    frag_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    enc = fm.summary(len(frags), int(sum(sizes)), int(frags["payload_len"].sum()))
    return first, s, frag_off, enc


def test_offsets_on_synthetic_tables(engine):
    rng = np.random.default_rng(0x67667230)
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5):
        recs = fm.random_records(n, 6, rng)
        first, s, frag_off, enc = synthetic(recs, 6)
        r = offsets_both(engine, first, n, None, s, frag_off, enc, tag=n)
        assert (int(r["status"]), int(r["frames"])) == (0, n)
    recs = fm.random_records(300, 6, rng)
    first, s, frag_off, enc = synthetic(recs, 6)
    n = 300
    # a count below max_records: the tables of those records alone fit it
    f7, s7, o7, e7 = synthetic(recs[:7], 6)
    offsets_both(engine, f7, n, fm.summary(frames=7), s7, o7, e7, tag="count")
    # each failed gate, the first failing status first
    cap, inv = gev_amd.ERR_CAPACITY, gev_amd.ERR_INVALID
    enc_cap = fm.summary(int(enc["frames"]), 987654, int(enc["payload_len"]), status=cap)
    r = offsets_both(engine, first, n, None, s, frag_off, enc_cap, tag="encode capacity")
    assert (int(r["status"]), int(r["payload_bytes"]), int(r["frames"])) == (cap, 987654, 0)
    enc_inv = fm.summary(int(enc["frames"]), 55, status=inv)
    assert int(offsets_both(engine, first, n, None, s, frag_off, enc_inv, tag="encode invalid")["payload_bytes"]) == 0
    s_cap = fm.summary(int(s["frames"]), 3, 99, status=cap)
    r = offsets_both(engine, first, n, None, s_cap, frag_off, enc_cap, tag="fragment capacity")
    assert r.tobytes() == fm.summary(status=cap).tobytes()
    s_inv = fm.summary(errors=2, status=inv)
    assert int(offsets_both(engine, first, n, None, s_inv, frag_off, enc_cap, tag="fragment invalid")["status"]) == inv
    prev_bad = fm.summary(frames=n, status=inv)
    r = offsets_both(engine, first, n, prev_bad, s_cap, frag_off, enc_cap, tag="prev")
    assert r.tobytes() == fm.summary(status=inv).tobytes()
    # tables that do not fit together: INVALID, d_frag_off never indexed (its entries would be far outside)
    wild = np.full(len(frag_off), 1 << 60, np.uint64)
    dec = first.copy()
    dec[130], dec[131] = dec[131], dec[130]
    r = offsets_both(engine, dec, n, None, s, wild, enc, tag="decreasing")
    assert int(r["status"]) == inv and int(r["errors"]) >= 1
    far = first.copy()
    far[200] = 1 << 50   # an index far outside d_frag_off
    r = offsets_both(engine, far, n, None, s, wild, enc, tag="outside")
    assert (int(r["status"]), int(r["errors"])) == (inv, 1)
    r = offsets_both(engine, first, n, None, fm.summary(int(s["frames"]) + 1), frag_off, enc, tag="total vs fragged")
    assert (int(r["status"]), int(r["errors"])) == (inv, 1)
    e2 = enc.copy()
    e2["frames"] = int(enc["frames"]) - 1
    r = offsets_both(engine, first, n, None, s, frag_off, e2, tag="total vs encode")
    assert (int(r["status"]), int(r["errors"])) == (inv, 1)
    nz = first.copy()
    nz[0] = 1
    assert int(offsets_both(engine, nz, n, None, s, frag_off, enc, tag="start")["errors"]) == 1


def parse(wire: bytes):
    # (the reference reads no header from fewer than 6 buffered bytes: three bare close frames behind the wire
    # let it read a short last frame, and are dropped again)
    got = wo.decode_stream(wire + b"\x88\x00" * 3)
    assert got.status == wo.OK
    frames = [f for f in got.frames if f.stream_pos < len(wire)]
    assert sum(f.header_len + f.header.length for f in frames) == len(wire)
    return frames


@pytest.mark.parametrize("F", (1, 125, 126, 300))
def test_offsets_behind_a_real_encode(engine, F):
    """fragment -> gevws_encode_replies_async -> offsets on real payload bytes:
    the wire holds the fragments' frames back to back, and reply k starts at
    d_reply_off[k]."""
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x67667240 + F)
    recs, off = [], 0
    for _ in range(BLOCK + 9):
        kind = int(rng.integers(0, 6))
        L = int(rng.integers(0, 3 * F + 8)) if kind < 5 else int(rng.integers(0, 126))
        if kind < 3:
            r = fm.record(L, opcode=int(rng.integers(1, 3)), rsv=int(rng.choice([0, 4])), off=off)
        elif kind == 3:
            r = fm.record(L, opcode=int(rng.integers(0, 3)), fin=0, off=off)
        elif kind == 4:
            r = fm.record(L, opcode=0, off=off)
        else:
            r = fm.record(L, opcode=int(rng.choice([8, 9, 10])), off=off)
        recs.append(r)
        off += (L + 15) // 16 * 16
    recs = np.array(recs, fm.OUT_FRAME_DTYPE)
    n, arena = len(recs), rng.integers(0, 256, off + 16, dtype=np.uint8)
    want_f, want_first, want_s = fm.fragment(recs, F, 1 << 20)
    nf = len(want_f)
    d_recs, payload = mm._dev(recs, dev, 32), mm._dev(arena, dev, 16)
    frags, first, fsum = filled((nf + 1) * 32, dev), filled((n + 2) * 8, dev), filled(64, dev)
    engine.fragment_async(d_recs, n, None, F, frags, nf, first, fsum)
    wcap = int(want_s["payload_len"]) + 14 * nf + 16
    wire = torch.zeros(wcap + 16, dtype=torch.uint8, device=dev)
    frag_off, esum = torch.zeros(nf, dtype=torch.int64, device=dev), filled(64, dev)
    engine.encode_replies_async(frags, nf, fsum, payload, wire, wcap, frag_off, esum)
    reply_off, rsum = filled((n + 1) * 8, dev), filled(64, dev)
    engine.fragment_offsets_async(first, n, None, fsum, frag_off, esum, reply_off, rsum)
    torch.cuda.synchronize(engine.device)
    assert frags.cpu().numpy()[: nf * 32].tobytes() == want_f.tobytes()
    es = esum.cpu().numpy().view(fm.SUMMARY_DTYPE)[0]
    assert (int(es["status"]), int(es["frames"]), int(es["payload_len"])) == (0, nf, int(want_s["payload_len"]))
    h_off = frag_off.cpu().numpy().view(np.uint64)
    want_off, want_r = fm.offsets(want_first, n, None, want_s, h_off, es)
    got = reply_off.cpu().numpy()
    assert got[: n * 8].tobytes() == want_off.tobytes() and (got[n * 8:] == 0xEE).all()
    assert rsum.cpu().numpy().tobytes() == want_r.tobytes()
    # the wire, parsed by the oracle: one frame a fragment, in order, with the fragment's header and bytes
    total = int(es["payload_bytes"])
    frames = parse(wire[:total].cpu().numpy().tobytes())
    assert len(frames) == nf
    for f, w, o in zip(frames, want_f, h_off):
        h = f.header
        assert (int(h.fin), h.rsv, h.opcode, h.length, f.stream_pos) == \
            (int(w["fin"]), int(w["rsv"]), int(w["opcode"]), int(w["payload_len"]), int(o))
        p0 = int(w["payload_off"])
        assert f.payload == arena[p0: p0 + int(w["payload_len"])].tobytes()
    ends = [int(x) for x in want_off[1:]] + [total]
    for k in range(n):   # reply k's span is exactly its fragments' frames
        fs = frames[int(want_first[k]): int(want_first[k + 1])]
        assert fs[0].stream_pos == int(want_off[k])
        assert sum(f.header_len + f.header.length for f in fs) == ends[k] - int(want_off[k])


# ---------------------------------------------------------------------------- 4.-6. the whole chain, echo
def ascii_bytes(rng, n):
    return bytes(rng.integers(0x20, 0x7F, n, dtype=np.uint8))


def comp(data: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]


class EchoCase:
    """Six connections and what each must be sent, in order: ("msg", bytes) /
    ("ctl", opcode, payload).  Every message is valid UTF-8 (the replies are
    text frames, and the round trip checks them as such)."""

    def __init__(self):
        rng = np.random.default_rng(0x67667250)
        key = lambda: bytes(rng.integers(0, 256, 4, dtype=np.uint8))  # noqa: E731

        def frames_of(data, op, cuts=(), rsv=0, ping=None):
            edges, s = [0, *cuts, len(data)], b""
            for i in range(len(edges) - 1):
                last = i == len(edges) - 2
                s += wo.encode_frame(data[edges[i]:edges[i + 1]], op if i == 0 else 0, last, rsv if i == 0 else 0,
                                     True, key())
                if ping is not None and i == 0 and not last:
                    s += wo.encode_frame(ping, PING, True, 0, True, key())
            return s

        big = ascii_bytes(rng, 70000)
        words = (b"the quick brown fox jumps over the lazy dog; " * 1600)[:70000]
        euro = "€".encode() * 100                 # three-byte characters: a limit of 3 k + 1 cuts inside one
        noise = ascii_bytes(rng, 3000)            # compresses little: the deflated wire is fragmented too
        mid = ascii_bytes(rng, 300)
        self.streams = [
            # 0 plain: a big binary message in three fragments with a ping between two of them, then small ones
            frames_of(big, B, (1000, 40000), ping=b"between") + frames_of(b"", T) + frames_of(b"x", B)
            + frames_of(mid, T, (150,)),
            # 1 deflate, no takeover
            frames_of(comp(euro), T, rsv=4) + frames_of(comp(words), B, (5,), rsv=4) + frames_of(comp(b""), T, rsv=4)
            + frames_of(comp(mid), T, rsv=4),
            # 2 deflate with server takeover: the window carries from message to message
            frames_of(comp(mid), T, rsv=4) + frames_of(comp(words[:30000]), T, rsv=4) + frames_of(comp(b"y"), B, rsv=4)
            + frames_of(comp(mid), T, rsv=4),
            # 3 plain text of three-byte characters
            frames_of(euro, T) + frames_of(euro * 7, T, (4,)),
            # 4 plain: fails UTF-8, the close is the last thing sent
            frames_of(b"fine", T, ping=None) + frames_of(b"pi", PING) + frames_of(b"\xff\xfe", T) + frames_of(b"late", T),
            # 5 deflate, no takeover: an uncompressed message among compressed ones
            frames_of(noise, B) + frames_of(comp(euro * 3), T, rsv=4),
        ]
        self.ext = np.array([0, D, TK, 0, 0, D], np.uint8)
        self.expect = [
            [("ctl", PONG, b"between"), ("msg", big), ("msg", b""), ("msg", b"x"), ("msg", mid)],
            [("msg", euro), ("msg", words), ("msg", b""), ("msg", mid)],
            [("msg", mid), ("msg", words[:30000]), ("msg", b"y"), ("msg", mid)],
            [("msg", euro), ("msg", euro * 7)],
            [("msg", b"fine"), ("ctl", PONG, b"pi"), ("ctl", CLOSE, (1007).to_bytes(2, "big"))],
            [("msg", noise), ("msg", euro * 3)],
        ]
        self.longest = 70000
        self.runs = {}

    def run(self, engine, F):
        """The chain from the decode on (respond rewrites the bodies in place), gathered; cached per limit."""
        if F in self.runs:
            return self.runs[F]
        import torch
        dev = torch.device("cuda", engine.device)
        nc = len(self.streams)
        lens = np.array([len(s) for s in self.streams], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        ext = mm._dev(self.ext, dev, 1)
        batch = gpu_decode(engine, b"".join(self.streams), np.stack([offs, lens], 1), aux_slots=nc)
        msgs = engine.messages(batch, conn_ext=ext)
        inf = engine.inflate(batch, msgs, 1 << 20)
        bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)
        ctxs = torch.zeros((nc, gev_amd.DEF_CTX_BYTES), dtype=torch.uint8, device=dev)
        res = engine.respond(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, None, ctxs, gather=True,
                             max_fragment_bytes=F)
        self.runs[F] = (res, ctxs)
        return self.runs[F]


@pytest.fixture(scope="module")
def echo_case():
    return EchoCase()


def replies_of(frames, F, c):
    """A connection's parsed frames as replies: control frames stand alone, a
    data reply is its first frame and the continuations up to the FIN.  ->
    [("ctl", opcode, payload) | ("msg", rsv of the first frame, [payloads])],
    the fragment pattern checked on the way."""
    out, cur = [], None
    for f in frames:
        h = f.header
        assert not h.masked, c
        if h.opcode & 8:
            assert cur is None, (c, "a control reply between a reply's fragments")
            assert h.fin and h.rsv == 0, c
            out.append(("ctl", h.opcode, f.payload))
            continue
        if cur is None:
            assert h.opcode == T, c
            cur = [h.rsv, []]
        else:
            assert h.opcode == C and h.rsv == 0, (c, "opcode and RSV1 on the first fragment only")
        cur[1].append(f.payload)
        if h.fin:
            parts = cur[1]
            total = sum(len(p) for p in parts)
            if F is not None:   # ceil(total / F) frames, all but the last full
                assert len(parts) == max(1, -(-total // F)), (c, total, len(parts))
                assert all(len(p) == F for p in parts[:-1]) and len(parts[-1]) <= F, c
                assert total <= F or len(parts[-1]) >= 1, c
            out.append(("msg", cur[0], parts))
            cur = None
    assert cur is None, (c, "a reply without its FIN")
    return out


def check_conn(case, res, c, F, z):
    """Connection c's bytes against case.expect[c]; z: its persistent decompressor (takeover) or None."""
    wire = res.conn_bytes(c)
    got = replies_of(parse(wire), F, c)
    want = case.expect[c]
    assert len(got) == len(want) == int(res.conn_send_host()["count"][c]), (c, len(got), len(want))
    for g, w in zip(got, want):
        assert g[0] == w[0], c
        if w[0] == "ctl":
            assert (g[1], g[2]) == (w[1], w[2]), c
            continue
        data = b"".join(g[2])
        if case.ext[c] & D:
            assert g[1] == 4, c    # compressed: RSV1, on the first fragment
            zz = z if z is not None else zlib.decompressobj(-15)
            assert zz.decompress(data + b"\x00\x00\xff\xff") == w[1], (c, len(w[1]))
        else:
            assert g[1] == 0 and data == w[1], (c, len(w[1]))
    return wire


@pytest.mark.parametrize("F", (3, 126, 1000))
def test_chain_echo(engine, echo_case, F):
    res, _ = echo_case.run(engine, F)
    cs = res.conn_send_host()
    S, FAIL = gev_amd.CTL_SHUTDOWN, gev_amd.CTL_SHUTDOWN | gev_amd.CTL_FAILED
    assert [int(x) for x in cs["flags"]] == [0, 0, 0, 0, FAIL, 0]
    sends = res.host_sends()
    split = 0
    for c in range(len(echo_case.streams)):
        z = zlib.decompressobj(-15) if echo_case.ext[c] & gev_amd.EXT_SERVER_TAKEOVER else None
        wire = check_conn(echo_case, res, c, F, z)
        assert bytes(sends[c]) == wire and len(wire) == int(cs["bytes"][c]), c   # the gather == the plan's entries
    # the tables for callers that want the fragments: per-reply offsets, first[k] .. first[k + 1] frames each
    e = res.echo
    for first, off, wire in ((e.plain_first, e.plain_off, e.plain_wire), (e.def_first, e.def_off, e.def_wire)):
        assert first is not None and len(first) == len(off) + 1 and first[0] == 0
        frames = parse(wire.cpu().numpy().tobytes())
        assert int(first[-1]) == len(frames)
        for k in range(len(off)):
            assert frames[int(first[k])].stream_pos == int(off[k]), k
            split += int(first[k + 1]) - int(first[k]) > 1
    assert split >= 3
    if F % 3 == 1:   # the limit cuts inside a three-byte character of connection 3's second message
        full = [f for f in parse(res.conn_bytes(3)) if f.header.length == F]
        assert full and not wo.utf8_valid(full[0].payload)


# ---------------------------------------------------------------------------- 5. a limit nobody reaches changes nothing
def test_identity(engine, echo_case):
    import torch
    base, base_ctx = echo_case.run(engine, None)
    for c in range(len(echo_case.streams)):
        z = zlib.decompressobj(-15) if echo_case.ext[c] & gev_amd.EXT_SERVER_TAKEOVER else None
        check_conn(echo_case, base, c, None, z)
    assert base.echo.plain_first is None and base.echo.def_first is None
    for F in (echo_case.longest, echo_case.longest + 1, 1 << 40):
        res, ctx = echo_case.run(engine, F)
        e, b = res.echo, base.echo
        assert torch.equal(e.plain_wire, b.plain_wire) and torch.equal(e.def_wire, b.def_wire)
        assert torch.equal(res.ctl_wire, base.ctl_wire)
        for name in ("plain_off", "def_off", "plain_conn", "def_conn", "reply_of"):
            assert np.array_equal(getattr(e, name), getattr(b, name)), name
        assert e.plain_first.tolist() == list(range(len(e.plain_off) + 1))
        assert e.def_first.tolist() == list(range(len(e.def_off) + 1))
        for name in ("send", "conn_send", "summary", "send_buf"):
            assert torch.equal(getattr(res, name), getattr(base, name)), name
        assert res.conn_buf.tobytes() == base.conn_buf.tobytes()
        assert res.gather_summary.tobytes() == base.gather_summary.tobytes()
        assert res.ctl_summary.tobytes() == base.ctl_summary.tobytes()
        for name in ("ctl_conn", "ctl_of", "msg_end", "conn_ctl"):
            assert np.array_equal(getattr(res, name), getattr(base, name)), name
        assert torch.equal(ctx, base_ctx)


# ---------------------------------------------------------------------------- 6. round trip on the device
@pytest.mark.parametrize("F", (3, 126, 1000))
def test_round_trip_on_the_device(engine, echo_case, F):
    """The plain and the no-takeover connections' gathered bytes as the input of
    a second pass: the project's own message layer accepts the fragments (a
    character split over two of them included) and the join gives the messages
    back."""
    import torch
    dev = torch.device("cuda", engine.device)
    res, _ = echo_case.run(engine, F)
    sends = res.host_sends()
    conns = [0, 1, 3, 5]
    # (the decode, as the reference, reads no header from fewer than 6 buffered bytes, and a last fragment of
    # at most 3 bytes is shorter: three bare pongs behind each stream let it be read -- the first of them is
    # decoded with it, a control frame the message layer passes over)
    streams = [bytes(sends[c]) + b"\x8a\x00" * 3 for c in conns]
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ext = mm._dev(echo_case.ext[conns], dev, 1)
    n_frames = sum(len(parse(bytes(sends[c]))) + 1 for c in conns)
    batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1), max_frames=n_frames)
    assert int(batch.summary_host()["frames"]) == n_frames and not batch.conn_out_host()["status"].any()
    msgs = engine.messages(batch, conn_ext=ext)
    inf = engine.inflate(batch, msgs, 1 << 20)
    bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)
    cm = msgs.conn_msg_host()
    assert not cm["error"].any()
    want = [w[1] for c in conns for w in echo_case.expect[c] if w[0] == "msg"]
    bh = bodies.bodies_host()
    assert len(bh) == len(want) == int(cm["nmessages"].sum())
    assert not bh["status"].any() and all(int(x) & gev_amd.BODY_WHOLE for x in bh["flags"])
    for i, w in enumerate(want):
        assert bodies.body_bytes(i) == w, (i, len(w))
    assert [int(x) for x in bh["opcode"]] == [T] * len(want)


# ---------------------------------------------------------------------------- 7. broadcast
@pytest.mark.parametrize("F", (7, 126))
def test_broadcast(engine, F):
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x67667270)

    def fr(payload, op, fin=True):
        return wo.encode_frame(payload, op, fin, 0, True, bytes(rng.integers(0, 256, 4, dtype=np.uint8)))

    euro = "€".encode() * 100
    words = b"the quick brown fox jumps over the lazy dog; " * 23
    noise = ascii_bytes(rng, 500)
    streams = [
        fr(euro[:100], T, False) + fr(b"between", PING) + fr(euro[100:], C),    # 0 room 0, takes plain
        fr(words, T) + fr(b"", T),                                              # 1 room 0, takes deflate
        fr(noise, B),                                                           # 2 room 0, takes deflate
        fr(b"room one " * 20, T) + fr((1000).to_bytes(2, "big"), CLOSE),        # 3 room 1, alone
        fr(b"nobody hears this", T) + fr(b"pi", PING),                          # 4 no room
    ]
    nc = len(streams)
    ext_h = np.array([0, D, D, 0, D], np.uint8)
    room_h = np.array([0, 0, 0, 1, gev_amd.ROOM_NONE], np.uint32)
    published = {0: [(0, euro), (1, words), (1, b""), (2, noise)], 1: [(3, b"room one " * 20)]}
    tails = {0: [(PONG, b"between")], 3: [(CLOSE, (1000).to_bytes(2, "big"))], 4: [(PONG, b"pi")]}
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ext = mm._dev(ext_h, dev, 1)
    rooms = gev_amd.Rooms.from_conn_room(room_h, dev)
    for flags in (0, gev_amd.ROOMS_SKIP_SENDER):
        batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1), aux_slots=nc)
        msgs = engine.messages(batch, conn_ext=ext)
        inf = engine.inflate(batch, msgs, 1 << 16)
        bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL)
        res = engine.broadcast(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, rooms, rooms_flags=flags,
                               gather=True, max_fragment_bytes=F)
        cs = res.conn_send_host()
        sends = res.host_sends()
        assert res.echo.plain_first is not None and res.echo.def_first is not None
        fragmented = 0
        for c in range(nc):
            wire = res.conn_bytes(c)
            assert bytes(sends[c]) == wire and len(wire) == int(cs["bytes"][c]), c
            got = replies_of(parse(wire), F, c)
            want = [x for s, x in published.get(int(room_h[c]), []) if not (flags and s == c)]
            tail = tails.get(c, [])
            assert len(got) == len(want) + len(tail) == int(cs["count"][c]), (flags, c, len(got))
            deflate = bool(ext_h[c] & D)
            for g, x in zip(got, want):     # every publication of its room once, fragmented, in frame order
                assert g[0] == "msg", c
                data = b"".join(g[2])
                fragmented += len(g[2]) > 1
                if deflate:
                    assert g[1] == 4 and zlib.decompressobj(-15).decompress(data + b"\x00\x00\xff\xff") == x, (c, len(x))
                else:
                    assert g[1] == 0 and data == x, (c, len(x))
            for g, (op, x) in zip(got[len(want):], tail):   # then its own control replies, whole
                assert g == ("ctl", op, x), c
        # at the least, with the sender skipped and F = 126: connection 0 is sent the 1 035 and the 500 plain
        # bytes, connection 1 the 500 random printable bytes compressed (over 6.5 bits a byte: above 400 bytes)
        assert fragmented >= 3
        assert int(cs["count"][4]) == 1
