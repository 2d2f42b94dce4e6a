"""The message layer's contract (gevws_messages_async, include/gevws.h) restated
frame by frame in plain Python, and the helpers that hand-build a decoded
batch -- records, per-connection table, summary, payload arena -- for it.

The model is pinned on the CPU (tests/test_messages_model.py) against
bytes.decode and codecs' incremental decoder; the GPU tests compare the device
tables with it, field by field."""
from __future__ import annotations

import numpy as np

OK, ERR_RSV, ERR_OPCODE, ERR_CONTROL, ERR_CONTINUATION, ERR_INTERLEAVE, ERR_UTF8 = range(7)
BEGIN, END = 1, 2
NO_FRAME = 0xFFFFFFFFFFFFFFFF
ERR_LEN_MSB = -1

FRAME_DTYPE = np.dtype([("fin", "u1"), ("rsv", "u1"), ("opcode", "u1"), ("masked", "u1"),
                        ("mask", "u1", (4,)), ("length", "<i8"), ("payload_off", "<u8"), ("src_off", "<u8")])
CONN_OUT_DTYPE = np.dtype([("first_frame", "<u8"), ("consumed", "<u8"), ("payload_base", "<u8"),
                           ("nframes", "<u4"), ("status", "<i4")])
SUMMARY_DTYPE = np.dtype([("frames", "<u8"), ("payload_bytes", "<u8"), ("payload_len", "<u8"),
                          ("errors", "<u8"), ("status", "<i4"), ("flags", "<u4"), ("run_frames", "<u8"),
                          ("reserved", "<u8", (2,))])
MSG_STATE_DTYPE = np.dtype([("opcode", "u1"), ("failed", "u1"), ("utf8_n", "u1"), ("utf8", "u1", (3,)),
                            ("reserved", "u1", (2,))])
MESSAGE_DTYPE = np.dtype([("first_frame", "<u8"), ("length", "<u8"), ("conn", "<u4"), ("nframes", "<u4"),
                          ("opcode", "u1"), ("flags", "u1"), ("status", "u1"), ("reserved", "u1", (5,))])
CONN_MSG_DTYPE = np.dtype([("first_message", "<u8"), ("error_frame", "<u8"), ("nmessages", "<u4"),
                           ("error", "<i4"), ("reserved", "<u8")])


class Utf8:
    """Strict UTF-8 (unicode/utf8.Valid) as a byte-at-a-time machine: `need`
    continuation bytes outstanding, the next one within [lo, hi]; `pend` the
    bytes of the unfinished sequence."""

    def __init__(self, pend: bytes = b""):
        self.need, self.lo, self.hi, self.pend = 0, 0x80, 0xBF, bytearray()
        for c in pend:
            assert self.step(c), "a carried sequence is valid so far"

    def step(self, c: int) -> bool:
        if self.need == 0:
            if c < 0x80:
                return True
            self.lo, self.hi = 0x80, 0xBF
            if 0xC2 <= c <= 0xDF:
                self.need = 1
            elif 0xE0 <= c <= 0xEF:
                self.need = 2
                if c == 0xE0:
                    self.lo = 0xA0      # no overlong 3-byte forms
                if c == 0xED:
                    self.hi = 0x9F      # no surrogates
            elif 0xF0 <= c <= 0xF4:
                self.need = 3
                if c == 0xF0:
                    self.lo = 0x90      # no overlong 4-byte forms
                if c == 0xF4:
                    self.hi = 0x8F      # nothing above U+10FFFF
            else:
                return False            # a stray continuation byte, C0, C1, F5..FF
            self.pend = bytearray([c])
            return True
        if not self.lo <= c <= self.hi:
            return False
        self.lo, self.hi = 0x80, 0xBF
        self.need -= 1
        self.pend.append(c)
        if self.need == 0:
            self.pend = bytearray()
        return True

    def feed(self, data: bytes) -> bool:
        return all(self.step(c) for c in data)


def text_message_verdict(fragments, pend: bytes = b""):
    """(valid, failing fragment index or None) of one text message given as its
    fragments, the last one its FIN frame."""
    u = Utf8(pend)
    for i, frag in enumerate(fragments):
        if not u.feed(frag):
            return False, i
    if u.need:
        return False, len(fragments) - 1
    return True, None


def model(frames: np.ndarray, conn_out: np.ndarray, n_decoded: int, arena: np.ndarray, state=None):
    """The tables gevws_messages_async must produce for the first n_decoded
    records: dict(messages, msg_of, conn_msg, state, frames, payload_len, errors)."""
    n_conns = conn_out.shape[0]
    st_in = np.zeros(n_conns, MSG_STATE_DTYPE) if state is None else state.copy()
    st_out = st_in.copy()
    msgs = []
    msg_of = np.full(max(n_decoded, 0), -1, np.int64)
    conn_msg = np.zeros(n_conns, CONN_MSG_DTYPE)
    text_bytes = errors = 0
    for c in range(n_conns):
        first, nfr, status = int(conn_out["first_frame"][c]), int(conn_out["nframes"][c]), int(conn_out["status"][c])
        s = st_in[c]
        conn_msg[c]["first_message"] = len(msgs)
        conn_msg[c]["error_frame"] = NO_FRAME
        end = min(first + nfr, n_decoded)
        if n_decoded == 0 or status != 0 or end <= first or int(s["failed"]):
            conn_msg[c]["error"] = int(s["failed"]) if n_decoded else 0
            continue
        open_op = int(s["opcode"])
        utf = Utf8(bytes(s["utf8"][: int(s["utf8_n"])])) if open_op == 1 else Utf8()
        cur = None  # the open message's record, once it has a data frame in this batch
        err, err_frame = OK, NO_FRAME

        def flush(end_flag: bool):
            nonlocal cur
            if end_flag:
                cur["flags"] |= END
            msgs.append(cur)
            cur = None

        for f in range(first, end):
            fin, rsv, op, L = (int(frames[k][f]) for k in ("fin", "rsv", "opcode", "length"))
            if rsv:
                err = ERR_RSV
            elif 3 <= op <= 7 or op >= 0xB:
                err = ERR_OPCODE
            elif op & 8 and (not fin or L > 125):
                err = ERR_CONTROL
            elif op == 0 and not open_op:
                err = ERR_CONTINUATION
            elif op in (1, 2) and open_op:
                err = ERR_INTERLEAVE
            if err:
                err_frame = f
                break
            if op & 8:
                continue
            if op:
                open_op = op
                utf = Utf8()
            if op or cur is None:
                cur = dict(first_frame=f, length=0, conn=c, nframes=0, opcode=open_op, flags=BEGIN if op else 0,
                           status=OK)
            cur["length"] += L
            cur["nframes"] += 1
            msg_of[f] = len(msgs)
            if open_op == 1:
                off = int(frames["payload_off"][f])
                text_bytes += L
                if not utf.feed(arena[off:off + L].tobytes()) or (fin and utf.need):
                    err, err_frame = ERR_UTF8, f
                    cur["status"] = ERR_UTF8
                    break
            if fin:
                flush(True)
                open_op = 0
        if cur is not None:
            flush(False)
        conn_msg[c]["nmessages"] = len(msgs) - int(conn_msg[c]["first_message"])
        conn_msg[c]["error"] = err
        conn_msg[c]["error_frame"] = err_frame
        st_out[c] = np.zeros((), MSG_STATE_DTYPE)
        if err:
            errors += 1
            st_out[c]["failed"] = err
        else:
            st_out[c]["opcode"] = open_op
            if open_op == 1:
                st_out[c]["utf8_n"] = len(utf.pend)
                st_out[c]["utf8"][: len(utf.pend)] = list(utf.pend)
    out = np.zeros(len(msgs), MESSAGE_DTYPE)
    for i, m in enumerate(msgs):
        for k, v in m.items():
            out[i][k] = v
    return dict(messages=out, msg_of=msg_of, conn_msg=conn_msg, state=st_out, frames=len(msgs),
                payload_len=text_bytes, errors=errors)


# ---------------------------------------------------------------------------- hand-built decoded batches
class Decoded:
    """A decode's outputs built by hand: conns = a list of connections, each a
    list of (fin, rsv, opcode, payload bytes), or a (status, frames) pair.  The
    arena is laid out as a decode's (every payload on a 16-byte boundary); its
    pad bytes are `pad` -- a continuation byte by default, so a check that read
    past hdr.length would see a different text."""

    def __init__(self, conns, pad: int = 0xBF, summary_status: int = 0):
        recs, table, chunks, off = [], [], [], 0
        for conn in conns:
            status, frs = conn if isinstance(conn, tuple) else (0, conn)
            table.append((len(recs), len(frs), status, off))
            for fin, rsv, op, payload in frs:
                payload = bytes(payload)
                recs.append((fin, rsv, op, len(payload), off))
                padded = (len(payload) + 15) // 16 * 16
                chunks.append(payload + bytes([pad]) * (padded - len(payload)))
                off += padded
        self.frames = np.zeros(len(recs), FRAME_DTYPE)
        for i, (fin, rsv, op, L, o) in enumerate(recs):
            self.frames[i]["fin"], self.frames[i]["rsv"], self.frames[i]["opcode"] = int(bool(fin)), rsv, op
            self.frames[i]["length"], self.frames[i]["payload_off"] = L, o
        self.conn_out = np.zeros(len(table), CONN_OUT_DTYPE)
        for c, (first, nfr, status, base) in enumerate(table):
            self.conn_out[c] = (first, 0, base, nfr, status)
        self.arena = np.frombuffer(b"".join(chunks), np.uint8).copy() if chunks else np.zeros(0, np.uint8)
        self.summary = np.zeros(1, SUMMARY_DTYPE)
        self.summary["frames"], self.summary["payload_bytes"] = len(recs), off
        self.summary["payload_len"] = int(self.frames["length"].sum())
        self.summary["status"] = summary_status

    @classmethod
    def from_arrays(cls, frames, conn_out, arena):
        self = cls([])
        self.frames, self.conn_out, self.arena = frames, conn_out, arena
        self.summary["frames"], self.summary["payload_bytes"] = frames.shape[0], arena.size
        self.summary["payload_len"] = int(frames["length"].sum())
        return self

    @property
    def n_decoded(self) -> int:
        return int(self.summary["frames"][0]) if int(self.summary["status"][0]) == 0 else 0

    def model(self, state=None):
        return model(self.frames, self.conn_out, self.n_decoded, self.arena, state)


def _dev(np_arr, dev, min_bytes=16):
    import torch
    raw = np.ascontiguousarray(np_arr).view(np.uint8).reshape(-1)
    t = torch.zeros(max(raw.size, min_bytes), dtype=torch.uint8, device=dev)
    if raw.size:
        t[: raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return t


def run_device(engine, d: Decoded, state=None, max_messages=None, keep_state=True):
    """gevws_messages_async on a hand-built batch; the host copies of what it
    wrote: dict(messages, msg_of, conn_msg, state, summary).  state: numpy
    MSG_STATE_DTYPE carried in, or None for fresh connections (keep_state =
    False passes d_state = NULL)."""
    import torch
    dev = torch.device("cuda", engine.device)
    n_frames, n_conns = d.frames.shape[0], d.conn_out.shape[0]
    if max_messages is None:
        max_messages = n_frames
    fr, co, sm = _dev(d.frames, dev, 32), _dev(d.conn_out, dev, 32), _dev(d.summary, dev, 64)
    pay = _dev(d.arena, dev)
    st = None
    if keep_state:
        st = _dev(np.zeros(n_conns, MSG_STATE_DTYPE) if state is None else state, dev, 8)
    msgs = torch.full((max(max_messages, 1) * 32,), 0xEE, dtype=torch.uint8, device=dev)
    msg_of = torch.full((max(n_frames, 1),), 7777, dtype=torch.int64, device=dev)
    cm = torch.full((max(n_conns, 1) * 32,), 0xEE, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    engine.messages_async(fr, n_frames, co, n_conns, sm, pay, st, msgs, max_messages, msg_of, cm, summ)
    torch.cuda.synchronize(engine.device)
    s = summ.cpu().numpy().view(SUMMARY_DTYPE)[0]
    nm = min(int(s["frames"]), max_messages)
    return dict(summary=s, messages=msgs[: nm * 32].cpu().numpy().view(MESSAGE_DTYPE),
                msg_of=msg_of[:n_frames].cpu().numpy(),
                conn_msg=cm[: n_conns * 32].cpu().numpy().view(CONN_MSG_DTYPE),
                state=st[: n_conns * 8].cpu().numpy().view(MSG_STATE_DTYPE) if st is not None else None)


def assert_tables_equal(got: dict, want: dict, tag: str = "", state: bool = True) -> None:
    """The device tables == the model's, every field of every row."""
    s = got["summary"]
    assert int(s["status"]) == 0, tag
    assert (int(s["frames"]), int(s["payload_len"]), int(s["errors"])) == \
        (want["frames"], want["payload_len"], want["errors"]), tag
    assert int(s["payload_bytes"]) == 0 and int(s["flags"]) == 0, tag
    for k in ("error", "error_frame", "nmessages", "first_message", "reserved"):
        assert np.array_equal(got["conn_msg"][k], want["conn_msg"][k]), (tag, k)
    assert np.array_equal(got["msg_of"][: want["msg_of"].size], want["msg_of"]), tag
    assert got["messages"].tobytes() == want["messages"].tobytes(), tag
    if state and got["state"] is not None:
        assert got["state"].tobytes() == want["state"].tobytes(), tag
