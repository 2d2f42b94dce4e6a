"""Client context takeover (gevws_inflate_ctx_async, gevws_inflate_raw_ctx;
include/gevws.h) restated in plain Python on top of the no-takeover oracles.

Message k of a chain, with H_k the last min(32 768, total) inflated bytes of
the connection's earlier compressed messages, is judged as the stream
"H_k as stored blocks with BFINAL 0, then payload_k" under the no-takeover
rules with the limit raised by |H_k| and the first |H_k| output bytes dropped:
`oracle` evaluates exactly that through tests/_inflate_gpu_model.expect_stream
(zlib's bytes, the Python model's verdicts).  `Slot` is the context slot as the
header lays it out; `model_inflate_ctx` is gm.model_inflate with chains."""
from __future__ import annotations

import zlib

import numpy as np

from tests import _inflate_gpu_model as gm
from tests import _inflate_model as im
from tests import _messages_model as mm
from tests._inflate_corpus import TAIL

WIN = 32768
CTX_BYTES = WIN + 64
EXT_DEFLATE, EXT_TAKEOVER = 1, 2


def chain(datas, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY):
    """The payloads of `datas` from one persistent compressor, Z_SYNC_FLUSH per
    message, the tail stripped: what a client with context takeover sends."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = []
    for d in datas:
        s = c.compress(d) + c.flush(zlib.Z_SYNC_FLUSH)
        assert s.endswith(TAIL)
        out.append(s[:-4])
    return out


def stored(h: bytes) -> bytes:
    """h in stored blocks, BFINAL 0, at most 65 535 bytes each."""
    out = b""
    for i in range(0, len(h), 65535):
        part = h[i:i + 65535]
        out += b"\x00" + len(part).to_bytes(2, "little") + (len(part) ^ 0xFFFF).to_bytes(2, "little") + part
    return out


def oracle(h: bytes, payload: bytes, limit: int):
    """(status, bytes) of `payload` behind the window h, by the definition."""
    assert len(h) <= WIN
    try:
        st, out = gm.expect_stream(stored(h) + payload, limit + len(h))
    except zlib.error:  # a long stream that zlib rejects: the Python model's verdict (slow, but exact)
        st, out = im.inflate(stored(h) + payload, limit + len(h))
        assert st != im.OK
    assert st != im.OK or out[: len(h)] == h
    return st, out[len(h):]


def empty_window_differs(payload: bytes, data: bytes) -> bool:
    """Does an empty window reject the message or decode it differently?"""
    raised, z = zlib_inflate_dict(b"", payload)
    return raised or z != data


def zlib_inflate_dict(h: bytes, payload: bytes):
    """(raised, bytes) of zlib's raw inflate of payload + TAIL with the dictionary h."""
    d = zlib.decompressobj(-15, zdict=h) if h else zlib.decompressobj(-15)
    try:
        return False, d.decompress(payload + TAIL)
    except zlib.error:
        return True, b""


class Slot:
    """One connection's context slot: uint64 total, uint8 broken, zeros to 64
    bytes, then the ring image (stream byte i at ring[i & 32767])."""

    def __init__(self, image: bytes = None):
        self.total, self.broken, self.ring = 0, 0, bytearray(WIN)
        if image is not None:
            assert len(image) == CTX_BYTES and not any(image[9:64])
            self.total, self.broken = int.from_bytes(image[:8], "little"), image[8]
            self.ring = bytearray(image[64:])

    def copy(self) -> "Slot":
        return Slot(self.image())

    def relocated(self, shift: int) -> "Slot":
        """The slot of the same connection `shift` stream bytes later (a
        multiple of the ring's size): `total` raised, nothing else changed."""
        assert shift % WIN == 0 and 0 <= self.total + shift < 1 << 64
        s = self.copy()
        s.total += shift
        return s

    def window(self) -> bytes:
        n = min(self.total, WIN)
        first = (self.total - n) & (WIN - 1)
        return bytes((self.ring + self.ring)[first:first + n])

    def append(self, out: bytes) -> None:
        for i, c in enumerate(out[-WIN:], start=self.total + max(len(out) - WIN, 0)):
            self.ring[i & (WIN - 1)] = c
        self.total += len(out)

    def feed(self, payload: bytes, limit: int):
        """One compressed message: (status, bytes) and the slot's update."""
        if self.broken:
            return self.broken, b""
        st, out = oracle(self.window(), payload, limit)
        if st == im.OK:
            self.append(out)
        else:
            self.broken = st
        return st, out

    def image(self) -> bytes:
        return self.total.to_bytes(8, "little") + bytes([self.broken]) + bytes(55) + bytes(self.ring)


class Bits:
    """A hand-assembled fixed-Huffman message (as tests/test_gpu_inflate.py's)."""

    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):
        self.bits += [(v >> i) & 1 for i in reversed(range(n))]

    def lit(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


def match3_at_32768() -> bytes:
    """One fixed block: a match of length 3 at distance 32 768 (length symbol
    257; distance symbol 29 with extra bits 8 191), end of block, then the sync
    flush's empty stored block minus its tail."""
    w = Bits()
    w.put(0, 1), w.put(1, 2)
    w.lit(257), w.code(29, 5), w.put(8191, 13)
    w.lit(256)
    w.put(0, 3)
    return w.bytes()


def match_at(dist: int, length: int = 3) -> bytes:
    """One fixed block: a match of `length` (3..10) at distance `dist`, end of
    block, then the sync flush's empty stored block minus its tail."""
    assert 3 <= length <= 10 and 1 <= dist <= 32768
    w = Bits()
    w.put(0, 1), w.put(1, 2)
    w.lit(254 + length)
    y = dist - 1
    if y < 4:
        w.code(y, 5)
    else:
        e = y.bit_length() - 2
        w.code(2 * e + 2 + ((y >> e) & 1), 5), w.put(y & ((1 << e) - 1), e)
    w.lit(256)
    w.put(0, 3)
    return w.bytes()


def wrap_chain(rng):
    """The messages of a stream longer than the window whose later messages
    refer back over the ring's wrap: 300, 300, 5 000, 0, 40 000, 17, 2 000,
    2 000 and 70 000 random bytes, then 300 from 30 000 bytes back."""
    def r(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    a, x, y = r(300), r(2000), r(70000)
    datas = [a, a, r(5000), b"", r(40000), r(17), x, x, y, y[-30000:-29700]]
    assert [len(d) for d in datas] == [300, 300, 5000, 0, 40000, 17, 2000, 2000, 70000, 300]
    total = sum(len(d) for d in datas[:-1])
    assert (total & (WIN - 1)) < 30000 < total  # the last message's source lies across the ring's wrap
    return datas


def history_and_match(rng, n: int):
    """(payloads, datas or None for the failing second message, status of the
    second): n random bytes as a stored message, then match3_at_32768()."""
    h = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    first = (c.compress(h) + c.flush(zlib.Z_SYNC_FLUSH))[:-4]
    ok = n >= WIN
    return [first, match3_at_32768()], [h, h[-WIN:][:3] if ok else b""], im.OK if ok else im.ERR_DEFLATE


def model_inflate_ctx(d: mm.Decoded, tables: dict, limit: int, state, ext, slots):
    """gm.model_inflate with context takeover: `slots` (a list of Slot, one per
    connection) is updated in place the way the device must leave d_inf_ctx.
    The update is dropped by the caller when the call ends in CAPACITY."""
    msgs, msg_of = tables["messages"], tables["msg_of"]
    rec = np.zeros(msgs.shape[0], gm.INFLATED_DTYPE)
    data = [b""] * msgs.shape[0]
    st_out = None if state is None else state.copy()
    off = ok = total = errors = 0
    failed_conns, stopped = set(), set()
    for m in range(msgs.shape[0]):
        flags, c = int(msgs["flags"][m]), int(msgs["conn"][m])
        if not flags & gm.COMPRESSED:
            continue
        take = bool(int(ext[c]) & EXT_TAKEOVER)
        whole = flags & (mm.BEGIN | mm.END) == (mm.BEGIN | mm.END)
        if take and slots[c].broken:
            st, out = slots[c].broken, b""
        elif not whole or (take and c in stopped):
            rec[m]["flags"] = gm.INF_PENDING
            stopped.add(c)
            continue
        else:
            fs = np.flatnonzero(msg_of == m)
            payload = b"".join(d.arena[int(d.frames["payload_off"][f]):][: int(d.frames["length"][f])].tobytes()
                               for f in fs)
            st, out = slots[c].feed(payload, limit) if take else gm.expect_stream(payload, limit)
        if st == im.OK and int(msgs["opcode"][m]) == 1 and not gm.py_valid(out):
            st = mm.ERR_UTF8
        keep = st in (im.OK, mm.ERR_UTF8)
        rec[m]["flags"], rec[m]["status"], rec[m]["out_off"] = gm.INF_DONE, st, off
        if keep:
            rec[m]["length"], data[m] = len(out), out
            off += (len(out) + 15) // 16 * 16
            total += len(out)
        if st == im.OK:
            ok += 1
        else:
            errors += 1
            if c not in failed_conns and st_out is not None and int(st_out[c]["failed"]) == 0:
                st_out[c]["failed"] = st
            failed_conns.add(c)
    return dict(inflated=rec, bytes=data, state=st_out, frames=ok, payload_bytes=off, payload_len=total,
                errors=errors)


def run_inflate_ctx(engine, got: dict, limit: int, out_cap: int, ext, ctx, n_conns=None, use_state=True):
    """gevws_inflate_ctx_async behind gm.run_messages_ext's tables, as
    gm.run_inflate; ctx is the device tensor of slots (updated in place) or
    None, ext a numpy array or None."""
    import torch
    t = got["dev"]
    dev = t["frames"].device
    nm = t["n_messages"]
    inf = torch.full((max(nm, 1) * 32,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.full((out_cap + 64,), 0xEE, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    st = t["state"] if use_state else None
    d_ext = None if ext is None else mm._dev(np.asarray(ext, np.uint8), dev, 1)
    n_conns = got["conn_msg"].shape[0] if n_conns is None else n_conns
    engine.inflate_ctx_async(t["frames"], t["n_frames"], t["messages"], nm, t["msg_of"], t["summary"], t["payload"],
                             limit, st, inf, out, out_cap, summ, d_ext, ctx, n_conns)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0],
                inflated=inf[: nm * 32].cpu().numpy().view(gm.INFLATED_DTYPE), out=out.cpu().numpy(),
                state=None if st is None else st.cpu().numpy()[: got["conn_msg"].shape[0] * 8].view(mm.MSG_STATE_DTYPE))


def slots_to_device(slots, dev):
    import torch
    img = np.frombuffer(b"".join(s.image() for s in slots), np.uint8).copy()
    return torch.from_numpy(img).to(dev).reshape(len(slots), CTX_BYTES)


def slots_from_device(ctx):
    return [bytes(row) for row in ctx.cpu().numpy()]
