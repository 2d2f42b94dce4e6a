"""gev_amd -- MI355X-native WebSocket frame-decode / payload-unmask engine.

Drop-in for the hot path of gev's websocket plugin
(plugins/websocket/protocol.go:27-64 ``Protocol.UnPacket``): the decode runs
in hand-written gfx950 HIP kernels (gev_amd/csrc/gevws_device.hip) behind the
C ABI of include/gevws.h.  This Python layer is a thin ctypes binding used by
the tests and bench; torch supplies device memory, streams and
torch.distributed (plumbing only).

Names mirror the reference: ``RingBuffer`` (github.com/Allenxuxu/ringbuffer as
gev uses it), ``Connection`` (gev.Connection's websocket context keys),
``Protocol.unpacket`` / ``Protocol.packet`` (websocket.Protocol),
``handler_protocol`` (Connection.handlerProtocol, connection.go:208-218).
"""
from __future__ import annotations

import ctypes
import atexit
import weakref
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._abi import (MSG_BEGIN, MSG_END, MSG_ERR_CONTINUATION, MSG_ERR_CONTROL, MSG_ERR_INTERLEAVE, MSG_ERR_OPCODE,
                   MSG_ERR_RSV, MSG_ERR_UTF8, MSG_OK)
from ._abi import EXT_DEFLATE, INF_DONE, INF_PENDING, MSG_COMPRESSED, MSG_ERR_DEFLATE, MSG_ERR_TOO_BIG
from ._abi import EXT_CLIENT_TAKEOVER, INF_CTX_BYTES, NEGOTIATE_CLIENT_TAKEOVER
from ._abi import DEFLATE_DYNAMIC, DEFLATE_PLAIN_IF_NOT_SMALLER
from ._abi import DEF_CTX_BYTES, EXT_SERVER_TAKEOVER, NEGOTIATE_SERVER_TAKEOVER
from ._abi import BODY_INFLATED, BODY_JOINED, BODY_WHOLE, JOIN_ALL
from ._abi import CARRY_COMPRESSED, CARRY_KEEP_COMPRESSED, CARRY_LOST, CARRY_OPEN
from ._abi import HANDLER_ECHO_BINARY, HANDLER_ECHO_TEXT, HANDLER_NONE
from ._abi import (CONTROL_NO_PING_FOR_PONG, CTL_FAILED, CTL_SHUTDOWN, MSG_ERR_CLOSED, WIRE_CONTROL, WIRE_DEFLATED,
                   WIRE_PLAIN)
from ._abi import ROOM_NONE, ROOMS_SKIP_SENDER
from ._abi import CHANGE_NONE, CHANGE_REJECTED, MSG_COMMAND
from ._abi import PUSH_ALL, PUSH_CONN, PUSH_ROOM
from ._abi import (ERR_CAPACITY, ERR_DEVICE, ERR_HANDSHAKE, ERR_INVALID, ERR_LEN_MSB, ERR_NOT_UPGRADED,
                   HANDSHAKE, IN_PAD, MEM_DEFAULT, MEM_FINE, MEM_UNCACHED, NEED_MORE, OK, PAYLOAD_ALIGN,
                   SUMMARY_UNORDERED, TILE, Header)

lib = _abi.load()

FRAME_DTYPE = np.dtype([("fin", "u1"), ("rsv", "u1"), ("opcode", "u1"), ("masked", "u1"),
                        ("mask", "u1", (4,)), ("length", "<i8"),
                        ("payload_off", "<u8"), ("src_off", "<u8")])
CONN_OUT_DTYPE = np.dtype([("first_frame", "<u8"), ("consumed", "<u8"), ("payload_base", "<u8"),
                           ("nframes", "<u4"), ("status", "<i4")])
SUMMARY_DTYPE = np.dtype([("frames", "<u8"), ("payload_bytes", "<u8"), ("payload_len", "<u8"),
                          ("errors", "<u8"), ("status", "<i4"), ("flags", "<u4"), ("run_frames", "<u8"),
                          ("reserved", "<u8", (2,))])
OUT_FRAME_DTYPE = np.dtype([("fin", "u1"), ("rsv", "u1"), ("opcode", "u1"), ("masked", "u1"),
                            ("mask", "u1", (4,)), ("length", "<i8"),
                            ("payload_off", "<u8"), ("payload_len", "<u8")])
SYNTH_DTYPE = np.dtype([("hdr_off", "<u8"), ("length", "<u8"), ("mask", "<u4"), ("b0", "u1"),
                        ("len_form", "u1"), ("masked", "u1"), ("pad", "u1")])
MSG_STATE_DTYPE = np.dtype([("opcode", "u1"), ("failed", "u1"), ("utf8_n", "u1"), ("utf8", "u1", (3,)),
                            ("reserved", "u1", (2,))])
MESSAGE_DTYPE = np.dtype([("first_frame", "<u8"), ("length", "<u8"), ("conn", "<u4"), ("nframes", "<u4"),
                          ("opcode", "u1"), ("flags", "u1"), ("status", "u1"), ("reserved", "u1", (5,))])
CONN_MSG_DTYPE = np.dtype([("first_message", "<u8"), ("error_frame", "<u8"), ("nmessages", "<u4"),
                           ("error", "<i4"), ("reserved", "<u8")])
INFLATED_DTYPE = np.dtype([("out_off", "<u8"), ("length", "<u8"), ("status", "u1"), ("flags", "u1"),
                           ("reserved", "u1", (14,))])
DEFLATE_MSG_DTYPE = np.dtype([("payload_off", "<u8"), ("length", "<u8"), ("opcode", "u1"), ("window_bits", "u1"),
                              ("reserved", "u1", (6,))])
BODY_DTYPE = np.dtype([("off", "<u8"), ("length", "<u8"), ("conn", "<u4"), ("opcode", "u1"), ("flags", "u1"),
                       ("status", "u1"), ("reserved", "u1", (9,))])
assert FRAME_DTYPE.itemsize == 32 and CONN_OUT_DTYPE.itemsize == 32 and INFLATED_DTYPE.itemsize == 32
CARRY_DTYPE = np.dtype([("off", "<u8"), ("length", "<u8"), ("opcode", "u1"), ("flags", "u1"), ("status", "u1"),
                        ("reserved", "u1", (13,))])
assert BODY_DTYPE.itemsize == 32 and CARRY_DTYPE.itemsize == 32
CONN_CTL_DTYPE = np.dtype([("cut_frame", "<u8"), ("close_code", "<u4"), ("flags", "<u4"), ("reserved", "<u8", (2,))])
SEND_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8"), ("frame", "<u8"), ("conn", "<u4"), ("wire", "<u4")])
CONN_SEND_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("bytes", "<u8"), ("flags", "<u4"),
                            ("reserved", "<u4")])
assert CONN_CTL_DTYPE.itemsize == 32 and SEND_DTYPE.itemsize == 32 and CONN_SEND_DTYPE.itemsize == 32
CONN_BUF_DTYPE = np.dtype([("off", "<u8"), ("bytes", "<u8"), ("flags", "<u4"), ("reserved", "<u4", (3,))])
assert CONN_BUF_DTYPE.itemsize == 32
ROOM_CHANGE_DTYPE = np.dtype([("conn", "<u4"), ("room", "<u4")])   # gevws_room_change
assert ROOM_CHANGE_DTYPE.itemsize == 8
PUSH_DTYPE = np.dtype([("off", "<u8"), ("length", "<u8"), ("target", "<u4"), ("kind", "u1"), ("opcode", "u1"),
                       ("reserved", "u1", (10,))])   # gevws_push
assert PUSH_DTYPE.itemsize == 32
assert DEFLATE_MSG_DTYPE.itemsize == 24 and OUT_FRAME_DTYPE.itemsize == 32
assert MSG_STATE_DTYPE.itemsize == 8 and MESSAGE_DTYPE.itemsize == 32 and CONN_MSG_DTYPE.itemsize == 32
assert SUMMARY_DTYPE.itemsize == 64 and SYNTH_DTYPE.itemsize == 24


def status_string(st: int) -> str:
    return lib.gevws_status_string(st).decode()


def device_count() -> int:
    return lib.gevws_device_count()


def utf8_valid(b: bytes) -> bool:
    """gevws_utf8_valid: unicode/utf8.Valid on host bytes (the rule the device pass applies)."""
    b = bytes(b)
    return bool(lib.gevws_utf8_valid(ctypes.c_char_p(b), len(b)))


def inflate_raw(b: bytes, cap: int) -> Tuple[int, bytes]:
    """gevws_inflate_raw: one message's compressed payload inflated on the host
    by the decoder the device runs; (MSG_OK / MSG_ERR_DEFLATE / MSG_ERR_TOO_BIG,
    the bytes produced before the verdict), at most cap of them."""
    b = bytes(b)
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(0)
    st = lib.gevws_inflate_raw(ctypes.c_char_p(b), len(b), out, cap, ctypes.byref(n))
    if st < 0:
        raise RuntimeError(f"gevws_inflate_raw: {status_string(st)}")
    return st, out.raw[: n.value]


def inflate_raw_ctx(b: bytes, cap: int, ctx: bytearray) -> Tuple[int, bytes]:
    """gevws_inflate_raw_ctx: inflate_raw over one connection's context slot
    (a bytearray of INF_CTX_BYTES, zeroed for a fresh connection, updated in
    place): the message is inflated behind the slot's window and appended to
    it; a failure marks the slot broken."""
    b = bytes(b)
    if not isinstance(ctx, bytearray) or len(ctx) != INF_CTX_BYTES:
        raise ValueError("ctx: a bytearray of INF_CTX_BYTES")
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(0)
    slot = (ctypes.c_uint8 * INF_CTX_BYTES).from_buffer(ctx)
    st = lib.gevws_inflate_raw_ctx(ctypes.c_char_p(b), len(b), out, cap, ctypes.byref(n), slot)
    if st < 0:
        raise RuntimeError(f"gevws_inflate_raw_ctx: {status_string(st)}")
    return st, out.raw[: n.value]


def deflate_negotiate_ext(value: bytes, flags: int = 0) -> Tuple[bytes, int]:
    """gevws_deflate_negotiate_flags: (the answer, the connection's conn_ext
    byte).  With NEGOTIATE_CLIENT_TAKEOVER the client may keep its window
    unless its offer said otherwise: the byte then carries EXT_CLIENT_TAKEOVER."""
    value = bytes(value)
    out = ctypes.create_string_buffer(256)
    n = ctypes.c_uint64(0)
    ext = ctypes.c_uint8(0)
    st = lib.gevws_deflate_negotiate_flags(ctypes.c_char_p(value), len(value), flags, out, len(out), ctypes.byref(n),
                                           ctypes.byref(ext))
    if st != OK:
        raise RuntimeError(f"gevws_deflate_negotiate_flags: {status_string(st)}")
    return out.raw[: n.value], int(ext.value)


def deflate_bound(n: int) -> int:
    """gevws_deflate_bound: the most bytes a message of n plain bytes can become."""
    return int(lib.gevws_deflate_bound(n))


def deflate_raw(b: bytes, window_bits: int = 0, flags: int = 0) -> bytes:
    """gevws_deflate_raw_flags: one message compressed on the host by the
    compressor the device runs -- the payload gevws_deflate_async writes for
    the same bytes, window_bits (0 = 15, else 8..15) and flags (0 or
    DEFLATE_DYNAMIC), byte for byte."""
    b = bytes(b)
    cap = deflate_bound(len(b))
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64(0)
    st = lib.gevws_deflate_raw_flags(ctypes.c_char_p(b), len(b), window_bits, flags, out, cap, ctypes.byref(n))
    if st != OK:
        raise RuntimeError(f"gevws_deflate_raw_flags: {status_string(st)}")
    return out.raw[: n.value]


def deflate_raw_ctx(b: bytes, ctx: bytearray, window_bits: int = 0, flags: int = 0) -> bytes:
    """gevws_deflate_raw_ctx: deflate_raw over one connection's context slot (a
    bytearray of DEF_CTX_BYTES, zeroed for a fresh connection, updated in
    place): the message is compressed with the connection's earlier messages
    as history and appended to the slot -- the payload gevws_deflate_ctx_async
    writes for it, byte for byte."""
    b = bytes(b)
    if not isinstance(ctx, bytearray) or len(ctx) != DEF_CTX_BYTES:
        raise ValueError("ctx: a bytearray of DEF_CTX_BYTES")
    cap = deflate_bound(len(b))
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64(0)
    slot = (ctypes.c_uint8 * DEF_CTX_BYTES).from_buffer(ctx)
    st = lib.gevws_deflate_raw_ctx(ctypes.c_char_p(b), len(b), window_bits, flags, out, cap, ctypes.byref(n), slot)
    if st != OK:
        raise RuntimeError(f"gevws_deflate_raw_ctx: {status_string(st)}")
    return out.raw[: n.value]


def deflate_negotiate_takeover(value: bytes, flags: int = 0) -> Tuple[bytes, int]:
    """gevws_deflate_negotiate_takeover: (the answer, the connection's conn_ext
    byte).  NEGOTIATE_CLIENT_TAKEOVER as in deflate_negotiate_ext; with
    NEGOTIATE_SERVER_TAKEOVER the server may keep its window unless the offer
    said otherwise: the byte then carries EXT_SERVER_TAKEOVER."""
    value = bytes(value)
    out = ctypes.create_string_buffer(256)
    n = ctypes.c_uint64(0)
    ext = ctypes.c_uint8(0)
    st = lib.gevws_deflate_negotiate_takeover(ctypes.c_char_p(value), len(value), flags, out, len(out),
                                              ctypes.byref(n), ctypes.byref(ext))
    if st != OK:
        raise RuntimeError(f"gevws_deflate_negotiate_takeover: {status_string(st)}")
    return out.raw[: n.value], int(ext.value)


def deflate_negotiate(value: bytes) -> bytes:
    """gevws_deflate_negotiate: the Sec-WebSocket-Extensions answer to the first
    permessage-deflate offer in `value` that the device inflate can serve
    (no context takeover), b"" when there is none."""
    value = bytes(value)
    out = ctypes.create_string_buffer(256)
    n = ctypes.c_uint64(0)
    st = lib.gevws_deflate_negotiate(ctypes.c_char_p(value), len(value), out, len(out), ctypes.byref(n))
    if st != OK:
        raise RuntimeError(f"gevws_deflate_negotiate: {status_string(st)}")
    return out.raw[: n.value]


def fragment_records(records: np.ndarray, max_fragment_bytes: int,
                     max_frags: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """gevws_fragment_records: the fragment step on host records
    (OUT_FRAME_DTYPE) -> (the fragments, first[n + 1], the summary).  Records
    longer than max_fragment_bytes become fragments by the rule the device
    applies.  max_frags: room for this many (None: what is needed).  The
    step's own failures (ERR_CAPACITY, ERR_INVALID for malformed records) come
    back in the summary's status, with no fragment and first left as it was
    (zeros)."""
    records = np.ascontiguousarray(records, dtype=OUT_FRAME_DTYPE).reshape(-1)
    n = int(records.size)
    F = int(max_fragment_bytes)
    first = np.zeros(n + 1, np.uint64)
    summary = np.zeros(1, SUMMARY_DTYPE)

    def call(room: int) -> np.ndarray:
        frags = np.zeros(max(room, 1), OUT_FRAME_DTYPE)
        st = lib.gevws_fragment_records(records.ctypes.data if n else None, n, F, frags.ctypes.data, room,
                                        first.ctypes.data, summary.ctypes.data)
        if st != OK:
            raise RuntimeError(f"gevws_fragment_records: {status_string(st)}")
        return frags

    if max_frags is None:  # sized by the step itself: a call with no room reports the need
        call(0)
        max_frags = min(int(summary[0]["frames"]), 0xFFFFFFFF)
    frags = call(int(max_frags))
    s = summary[0]
    return frags[: int(s["frames"]) if int(s["status"]) == OK else 0], first, s


def room_command_parse(body: bytes, n_rooms: int) -> Tuple[int, int]:
    """gevws_room_command_parse: what gevws_room_commands_async makes of a
    delivered text message of these bytes -> (class, room): class 0 no
    command, 1 a change ("/join N" with N < n_rooms: room N; "/leave": room
    ROOM_NONE), 2 a rejected join; room is ROOM_NONE unless the class is 1."""
    body = bytes(body)
    room = ctypes.c_uint32(0)
    st = lib.gevws_room_command_parse(ctypes.c_char_p(body), len(body), int(n_rooms), ctypes.byref(room))
    if st < 0:
        raise RuntimeError(f"gevws_room_command_parse: {status_string(st)}")
    return st, int(room.value)


def push_check(records: np.ndarray, n_conns: int, n_rooms: int, src_bytes: int) -> int:
    """gevws_push_check: how many of the PUSH_DTYPE records the push pass would
    call malformed (a bad kind, target, opcode, range, reserved byte or a key
    below the previous record's), by the device's rule."""
    records = np.ascontiguousarray(records, dtype=PUSH_DTYPE).reshape(-1)
    n = int(records.size)
    r = lib.gevws_push_check(records.ctypes.data if n else None, n, int(n_conns), int(n_rooms), int(src_bytes))
    if r < 0:
        raise RuntimeError(f"gevws_push_check: {status_string(int(r))}")
    return int(r)


def push_records(items) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The push list of `items`, a sequence of (kind, target, opcode, bytes) ->
    (records, arena, perm).  The bodies are laid into `arena` (uint8) in item
    order, each on a PAYLOAD_ALIGN boundary, with IN_PAD zero bytes behind the
    last one: the slack the encoder's and the deflate step's vector loads need
    (the readable bytes are arena.size - IN_PAD).  `records` (PUSH_DTYPE) are
    stable-sorted by (kind, target), as gevws_push_lists_async wants them:
    records[k] is items[perm[k]], so pushes of one key keep their order."""
    items = list(items)
    n = len(items)
    recs = np.zeros(n, PUSH_DTYPE)
    at, bodies = 0, []
    for i, (kind, target, opcode, body) in enumerate(items):
        body = bytes(body)
        recs[i]["off"], recs[i]["length"] = at, len(body)
        recs[i]["target"], recs[i]["kind"], recs[i]["opcode"] = int(target), int(kind), int(opcode)
        bodies.append((at, body))
        at += (len(body) + PAYLOAD_ALIGN - 1) // PAYLOAD_ALIGN * PAYLOAD_ALIGN
    arena = np.zeros(at + IN_PAD, np.uint8)
    for off, body in bodies:
        arena[off: off + len(body)] = np.frombuffer(body, np.uint8)
    key = (recs["kind"].astype(np.uint64) << np.uint64(32)) | recs["target"].astype(np.uint64)
    perm = np.argsort(key, kind="stable")
    return recs[perm], arena, perm.astype(np.int64)


def _torch():
    import torch
    return torch


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        return _torch().cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


@dataclass
class Batch:
    """Device-resident result of one batch decode (all tensors on the GPU)."""
    frames: "object"      # uint8 [max_frames, 32]  (gevws_frame records)
    payload: "object"     # uint8 [payload_cap + 16]
    conn_out: "object"    # uint8 [n_conns, 32]     (gevws_conn_out)
    summary: "object"     # uint8 [64]              (gevws_summary)
    n_conns: int
    aux_slots: int = 0    # close-reply slots reserved after the payload arena (alloc_batch)

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def frames_host(self) -> np.ndarray:
        n = int(self.summary_host()["frames"])
        return self.frames[:n].cpu().numpy().reshape(-1).view(FRAME_DTYPE)

    def conn_out_host(self) -> np.ndarray:
        return self.conn_out[: self.n_conns].cpu().numpy().reshape(-1).view(CONN_OUT_DTYPE)

    def payload_host(self) -> np.ndarray:
        n = int(self.summary_host()["payload_bytes"])
        return self.payload[:n].cpu().numpy()


@dataclass
class Messages:
    """Device-resident result of one message pass (Engine.messages)."""
    messages: "object"    # uint8 [max_messages, 32] (gevws_message records)
    msg_of: "object"      # int64 [max_frames]       (frame -> message, -1: none)
    conn_msg: "object"    # uint8 [n_conns, 32]      (gevws_conn_msg)
    state: "object"       # uint8 [n_conns, 8]       (gevws_msg_state after the pass) or None
    summary: "object"     # uint8 [64]               (gevws_summary)
    n_conns: int
    n_frames: int

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def messages_host(self) -> np.ndarray:
        n = int(self.summary_host()["frames"])
        return self.messages[:n].cpu().numpy().reshape(-1).view(MESSAGE_DTYPE)

    def msg_of_host(self) -> np.ndarray:
        return self.msg_of[: self.n_frames].cpu().numpy()

    def conn_msg_host(self) -> np.ndarray:
        return self.conn_msg[: self.n_conns].cpu().numpy().reshape(-1).view(CONN_MSG_DTYPE)

    def state_host(self) -> Optional[np.ndarray]:
        if self.state is None:
            return None
        return self.state[: self.n_conns].cpu().numpy().reshape(-1).view(MSG_STATE_DTYPE)


@dataclass
class Inflated:
    """Device-resident result of one inflate step (Engine.inflate)."""
    inflated: "object"    # uint8 [n_messages, 32]   (gevws_inflated records)
    out: "object"         # uint8 [out_cap]          (the inflated messages, each on a 16-byte boundary)
    summary: "object"     # uint8 [64]               (gevws_summary)
    n_messages: int

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def inflated_host(self) -> np.ndarray:
        return self.inflated[: self.n_messages].cpu().numpy().reshape(-1).view(INFLATED_DTYPE)

    def message_bytes(self, i: int) -> bytes:
        """The inflated bytes of message i (b"" when it has none)."""
        r = self.inflated_host()[i]
        off, n = int(r["out_off"]), int(r["length"])
        return self.out[off: off + n].cpu().numpy().tobytes() if n else b""


@dataclass
class Deflated:
    """Device-resident result of one deflate step (Engine.deflate)."""
    frames: "object"      # uint8 [n_messages, 32]   (gevws_out_frame records, ready for encode_async)
    out: "object"         # uint8 [out_cap + OUT_PAD] (the payloads, each on a 16-byte boundary)
    summary: "object"     # uint8 [64]               (gevws_summary)
    n_messages: int

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def frames_host(self) -> np.ndarray:
        n = int(self.summary_host()["frames"])
        return self.frames[:n].cpu().numpy().reshape(-1).view(OUT_FRAME_DTYPE)

    def payload(self, i: int) -> bytes:
        """The wire payload of message i."""
        r = self.frames_host()[i]
        off, n = int(r["payload_off"]), int(r["payload_len"])
        return self.out[off: off + n].cpu().numpy().tobytes() if n else b""


@dataclass
class Bodies:
    """Device-resident result of one join step (Engine.join)."""
    bodies: "object"      # uint8 [n_messages, 32]   (gevws_body records)
    out: "object"         # uint8 [out_cap + IN_PAD] (the inflated bytes below `base`, the joined bodies behind)
    summary: "object"     # uint8 [64]               (gevws_summary)
    payload: "object"     # the decode's payload arena (bodies that were left in place point into it)
    n_messages: int
    out_cap: int
    carry_summary: "object" = None   # uint8 [64], a join with a carry: the carry side's gevws_summary

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def carry_summary_host(self) -> Optional[np.ndarray]:
        return None if self.carry_summary is None else self.carry_summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def bodies_host(self) -> np.ndarray:
        return self.bodies[: self.n_messages].cpu().numpy().reshape(-1).view(BODY_DTYPE)

    def body_bytes(self, i: int) -> bytes:
        """The bytes of message i, from the arena its record points into (b"" when not delivered)."""
        r = self.bodies_host()[i]
        off, n, fl = int(r["off"]), int(r["length"]), int(r["flags"])
        if not fl & BODY_WHOLE or n == 0:
            return b""
        arena = self.out if fl & (BODY_JOINED | BODY_INFLATED) else self.payload
        return arena[off: off + n].cpu().numpy().tobytes()


class Carry:
    """The join step's carry between passes (Engine.join(carry=...)): every
    connection's open plain message, its record and its bytes so far, on the
    device.  Two sides that Engine.join swaps after each pass that succeeded:
    `records` / `arena` hold the state behind the last pass.  compressed: open
    permessage-deflate messages are kept too, as compressed bytes
    (CARRY_KEEP_COMPRESSED), for Engine.inflate(carry=...) to finish."""

    def __init__(self, engine: "Engine", n_conns: int, max_message_bytes: int, arena_bytes: int = 0,
                 compressed: bool = False):
        torch = _torch()
        self.device = torch.device("cuda", engine.device)
        self.n_conns, self.max_message_bytes = n_conns, max_message_bytes
        self.carry_flags = CARRY_KEEP_COMPRESSED if compressed else 0
        self.records = [torch.zeros((max(n_conns, 1), 32), dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.arenas = [self._arena(arena_bytes) for _ in range(2)]
        self.used = 0     # bytes of `arena` the records point into
        self.side = 0     # the side the next pass reads

    def _arena(self, nbytes: int):
        torch = _torch()
        return torch.zeros((max(nbytes, 0) + 15) // 16 * 16 + IN_PAD, dtype=torch.uint8, device=self.device)

    @property
    def records_in(self):
        return self.records[self.side]

    @property
    def arena(self):
        return self.arenas[self.side]

    def cap(self, side: int) -> int:
        return int(self.arenas[side].numel()) - IN_PAD

    def records_host(self) -> np.ndarray:
        return self.records_in[: self.n_conns].cpu().numpy().reshape(-1).view(CARRY_DTYPE)

    def carried_bytes(self, c: int) -> bytes:
        """The bytes kept of connection c's open message (b"" when none are)."""
        r = self.records_host()[c]
        off, n = int(r["off"]), int(r["length"])
        if not int(r["flags"]) & CARRY_OPEN or n == 0:
            return b""
        return self.arena[off: off + n].cpu().numpy().tobytes()


@dataclass
class Echo:
    """What Engine.echo_messages sends: the compressed replies' wire bytes and
    the plain replies' (device tensors), each with its per-reply connection and
    wire offset (numpy), and reply_of[m] = message m's index in its list or -1."""
    def_wire: "object"
    def_conn: np.ndarray
    def_off: np.ndarray
    plain_wire: "object"
    plain_conn: np.ndarray
    plain_off: np.ndarray
    reply_of: np.ndarray
    deflated: Optional["Deflated"] = None   # the deflate step's records and payloads
    # with max_fragment_bytes: reply k's frames in its wire are fragments [first[k], first[k + 1]) of the
    # list that was encoded (uint64 [replies + 1]); plain_off / def_off stay per reply
    plain_first: Optional[np.ndarray] = None
    def_first: Optional[np.ndarray] = None


@dataclass
class Responses:
    """What Engine.respond sends: the three wire buffers (the Echo's two and
    the control replies'), the control step's tables (numpy) and the send plan
    (device tensors): send[k] says which bytes of which wire go out k-th,
    conn_send[c] which entries are connection c's."""
    echo: "Echo"
    ctl_wire: "object"        # uint8: the control replies' wire bytes
    ctl_conn: np.ndarray      # uint32 [replies]
    ctl_of: np.ndarray        # int64 [frames]: frame -> control reply or -1
    msg_end: np.ndarray       # uint64 [messages]: the message's last data frame, or 2^64 - 1
    conn_ctl: np.ndarray      # CONN_CTL_DTYPE [n_conns]
    ctl_summary: np.ndarray   # SUMMARY_DTYPE: the control step's
    send: "object"            # uint8 [max_sends, 32] (gevws_send records)
    conn_send: "object"       # uint8 [n_conns, 32]   (gevws_conn_send)
    summary: "object"         # uint8 [64]            (the plan's gevws_summary)
    n_conns: int
    # with respond(gather=True): every connection's bytes in one buffer (gevws_send_gather_async)
    send_buf: Optional["object"] = None           # uint8, cut to the gather's payload_bytes
    conn_buf: Optional[np.ndarray] = None         # CONN_BUF_DTYPE [n_conns]
    gather_summary: Optional[np.ndarray] = None   # SUMMARY_DTYPE: the gather's
    # from Engine.broadcast: message m's index in the plain list / the deflate list or -1 (echo.reply_of: the plain one)
    plain_of: Optional[np.ndarray] = None
    def_of: Optional[np.ndarray] = None
    # from Engine.broadcast(commands=True): the pass's room commands, for Rooms.update(changes=...)
    room_changes: Optional["RoomChanges"] = None

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def host_sends(self) -> List[memoryview]:
        """What the host writes to each socket: one device-to-host copy of the
        send buffer, then connection c's span of it as element c (empty: nothing
        to send).  Needs respond(gather=True)."""
        if self.send_buf is None or self.conn_buf is None:
            raise ValueError("host_sends: the pass was not gathered (respond(gather=True))")
        host = memoryview(self.send_buf.cpu().numpy())
        return [host[int(b["off"]): int(b["off"]) + int(b["bytes"])] for b in self.conn_buf]

    def send_host(self) -> np.ndarray:
        n = int(self.summary_host()["frames"])
        return self.send[:n].cpu().numpy().reshape(-1).view(SEND_DTYPE)

    def conn_send_host(self) -> np.ndarray:
        return self.conn_send[: self.n_conns].cpu().numpy().reshape(-1).view(CONN_SEND_DTYPE)

    def conn_bytes(self, c: int) -> bytes:
        """The bytes to write to connection c's socket: its plan entries' segments in order."""
        wires = [w.cpu().numpy() for w in (self.echo.plain_wire, self.echo.def_wire, self.ctl_wire)]
        cs, send = self.conn_send_host()[c], self.send_host()
        first, count = int(cs["first"]), int(cs["count"])
        return b"".join(wires[int(e["wire"])][int(e["off"]): int(e["off"]) + int(e["len"])].tobytes()
                        for e in send[first: first + count])


@dataclass
class RoomChanges:
    """What gevws_room_commands_async made of a pass's bodies, on the device:
    the {conn, room} change records in message order, change_of[m] = message
    m's change, CHANGE_NONE or CHANGE_REJECTED, and the step's summary (frames
    = the changes).  Rooms.update(changes=...) hands the records, their
    capacity and the summary to gevws_rooms_update_async, so neither the
    records nor their count visit the host."""
    changes: "object"        # uint8 [max_changes, 8] (gevws_room_change records)
    change_of: "object"      # int64 [max(n_messages, 1)]
    summary: "object"        # uint8 [64] (gevws_summary)
    max_changes: int
    n_messages: int

    def summary_host(self) -> np.ndarray:
        return self.summary.cpu().numpy().view(SUMMARY_DTYPE)[0]

    def host(self) -> np.ndarray:
        """The change records written (ROOM_CHANGE_DTYPE); none unless the step's status is OK."""
        s = self.summary_host()
        n = min(int(s["frames"]), self.max_changes) if int(s["status"]) == OK else 0
        return self.changes[:n].cpu().numpy().reshape(-1).view(ROOM_CHANGE_DTYPE)

    def change_of_host(self) -> np.ndarray:
        return self.change_of[: self.n_messages].cpu().numpy()


@dataclass
class Rooms:
    """The room tables of gevws_reply_rooms_async / gevws_room_plan_async, owned
    by the host as the reference's server owns `sessions`: conn_room[c] is
    connection c's room or ROOM_NONE, room_first / room_members its inverse in
    CSR form (int32 device tensors holding the uint32 values).  from_conn_room
    builds them on the host; build / update make them on the device
    (gevws_rooms_update_async), so they can stay there from pass to pass."""
    conn_room: "object"      # [n_conns]
    room_first: "object"     # [n_rooms + 1]
    room_members: "object"   # [n_members]
    n_rooms: int

    @property
    def n_members(self) -> int:
        return int(self.room_members.numel())

    @staticmethod
    def csr(conn_room, n_rooms: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, int]:
        """(room_first, room_members, n_rooms) of a conn_room array, on the
        host: a stable argsort keeps a room's members in increasing order."""
        cr = np.asarray(conn_room, dtype=np.uint32).reshape(-1)
        has = np.flatnonzero(cr != ROOM_NONE)
        if n_rooms is None:
            n_rooms = int(cr[has].max()) + 1 if has.size else 0
        if has.size and int(cr[has].max()) >= n_rooms:
            raise ValueError("Rooms: a room id is not below n_rooms")
        members = has[np.argsort(cr[has], kind="stable")].astype(np.uint32)
        first = np.zeros(n_rooms + 1, np.uint32)
        first[1:] = np.cumsum(np.bincount(cr[has], minlength=n_rooms))[:n_rooms]
        return first, members, n_rooms

    @classmethod
    def from_conn_room(cls, conn_room, device, n_rooms: Optional[int] = None) -> "Rooms":
        torch = _torch()
        cr = np.ascontiguousarray(np.asarray(conn_room, dtype=np.uint32).reshape(-1))
        first, members, n_rooms = cls.csr(cr, n_rooms)
        up = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(device)  # noqa: E731
        return cls(conn_room=up(cr), room_first=up(first), room_members=up(members), n_rooms=n_rooms)

    def host(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        h = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        return h(self.conn_room), h(self.room_first), h(self.room_members)

    @staticmethod
    def _updated(engine: "Engine", conn_room, n_rooms: int, changes, closed, stream, what: str) -> "Rooms":
        """gevws_rooms_update_async over the device tensor conn_room: new
        tables in tensors of their own."""
        torch = _torch()
        dev = torch.device("cuda", engine.device)
        n_conns = int(conn_room.numel())
        d_changes, n_changes, prev = None, 0, None
        if changes is not None:
            if isinstance(changes, RoomChanges):   # the room-command step's: the count stays on the device
                d_changes, n_changes, prev = changes.changes, changes.max_changes, changes.summary
            elif isinstance(changes, torch.Tensor):   # gevws_room_change records in device memory
                nbytes = changes.numel() * changes.element_size()
                if nbytes % 8 or not changes.is_contiguous():
                    raise ValueError(f"{what}: changes: a contiguous tensor of 8-byte {{conn, room}} records")
                d_changes, n_changes = changes, nbytes // 8
            else:
                ch = np.asarray(changes)
                if ch.dtype != ROOM_CHANGE_DTYPE:
                    if ch.size and (ch.ndim != 2 or ch.shape[1] != 2 or ch.dtype.kind not in "iu"):
                        raise ValueError(f"{what}: changes: ROOM_CHANGE_DTYPE records or an (n, 2) integer array")
                    if ch.size and (ch.min() < 0 or ch.max() > 0xFFFFFFFF):
                        raise ValueError(f"{what}: changes: a value outside 32 bits")
                    ch = np.ascontiguousarray(ch.reshape(-1, 2).astype(np.uint32)).view(ROOM_CHANGE_DTYPE)
                ch = np.ascontiguousarray(ch.reshape(-1))
                n_changes = int(ch.shape[0])
                if n_changes:
                    d_changes = torch.from_numpy(ch.view(np.uint8).copy()).to(dev)
        conn_send = plan_summary = None
        if closed is not None:
            if closed.n_conns != n_conns:
                raise ValueError(f"{what}: closed is a pass of {closed.n_conns} connections, the rooms have {n_conns}")
            conn_send, plan_summary = closed.conn_send, closed.summary
        out = torch.empty(max(n_conns, 1), dtype=torch.int32, device=dev)
        first = torch.empty(n_rooms + 1, dtype=torch.int32, device=dev)
        members = torch.empty(max(n_conns, 1), dtype=torch.int32, device=dev)
        summary = torch.zeros(64, dtype=torch.uint8, device=dev)
        engine.rooms_update_async(conn_room if n_conns else None, n_conns, n_rooms, d_changes, n_changes, prev,
                                  conn_send, plan_summary, 0, out, first, members, summary, stream)
        torch.cuda.synchronize(engine.device)
        s = summary.cpu().numpy().view(SUMMARY_DTYPE)[0]
        if int(s["status"]) != OK:
            raise RuntimeError(f"{what}: {status_string(int(s['status']))} ({int(s['errors'])} records)")
        return Rooms(conn_room=out[:n_conns], room_first=first, room_members=members[: int(s["frames"])],
                     n_rooms=n_rooms)

    @classmethod
    def build(cls, engine: "Engine", conn_room, n_rooms: int, stream=None) -> "Rooms":
        """from_conn_room on the device: conn_room (a device tensor of 32-bit
        room ids, or an array that is uploaded) copied, its CSR inverse built by
        gevws_rooms_update_async without changes."""
        torch = _torch()
        if not isinstance(conn_room, torch.Tensor):
            cr = np.ascontiguousarray(np.asarray(conn_room, dtype=np.uint32).reshape(-1))
            conn_room = torch.from_numpy(cr.view(np.int32).copy()).to(torch.device("cuda", engine.device))
        if conn_room.element_size() != 4 or not conn_room.is_contiguous():
            raise ValueError("Rooms.build: conn_room: a contiguous tensor of 32-bit room ids")
        return cls._updated(engine, conn_room.reshape(-1), int(n_rooms), None, None, stream, "Rooms.build")

    def update(self, engine: "Engine", changes=None, closed: Optional["Responses"] = None,
               n_rooms: Optional[int] = None, stream=None) -> "Rooms":
        """New tables after membership changes, made on the device
        (gevws_rooms_update_async); this object stays valid.  changes: {conn,
        room} records applied in order, the last one of a connection wins, room
        ROOM_NONE leaves -- a ROOM_CHANGE_DTYPE array or an (n, 2) integer array
        (uploaded), a device tensor of such records, or the RoomChanges of
        Engine.broadcast(commands=True) (its summary gates the call and gives
        the count on the device).  closed: the pass's
        Responses; every connection it shut down (CTL_SHUTDOWN in its device
        conn_send) leaves its room, whatever `changes` says.  n_rooms: a larger room space (None: unchanged)."""
        return self._updated(engine, self.conn_room, self.n_rooms if n_rooms is None else int(n_rooms), changes,
                             closed, stream, "Rooms.update")


class _DevAddr:
    """A bare device address with the one method the launch wrappers read."""
    __slots__ = ("addr",)

    def __init__(self, addr: int):
        self.addr = addr

    def data_ptr(self) -> int:
        return self.addr


class PinnedArena:
    """Page-locked host memory mapped into the device (gevws_pinned_alloc):
    `host` is a numpy uint8 view for the CPU, `at(off)` a device address a
    decode can take as its payload arena, so the unmask kernel writes the
    plaintext straight into host memory (host-ingress helper, not on the
    reference path)."""

    def __init__(self, nbytes: int):
        h, d = ctypes.c_void_p(), ctypes.c_void_p()
        st = lib.gevws_pinned_alloc(nbytes, ctypes.byref(h), ctypes.byref(d))
        if st != OK:
            raise RuntimeError(f"gevws_pinned_alloc({nbytes}): {status_string(st)}")
        self.nbytes = nbytes
        self._h, self._d = h.value, d.value
        self.host = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(self._h))

    def at(self, offset: int = 0) -> _DevAddr:
        if not 0 <= offset <= self.nbytes:
            raise ValueError(f"PinnedArena.at({offset}): outside {self.nbytes} bytes")
        return _DevAddr(self._d + offset)

    def data_ptr(self) -> int:
        return self._d

    def close(self) -> None:
        if self._h:
            self.host = None
            lib.gevws_pinned_free(self._h)
            self._h = self._d = None

    def __del__(self, _free=lib.gevws_pinned_free):  # bound now: module globals are gone at exit
        if getattr(self, "_h", None):
            _free(self._h)


# Objects still alive at interpreter exit (e.g. held by a failed test's
# traceback) are freed in dependency order -- protocols, then engines -- from
# an atexit hook, while the HIP runtime is still up; the garbage collector's
# order at shutdown is arbitrary, and a protocol freed after its engine would
# synchronise a destroyed stream.
_LIVE_PROTOCOLS: "weakref.WeakSet" = weakref.WeakSet()
_LIVE_ENGINES: "weakref.WeakSet" = weakref.WeakSet()


def _close_live() -> None:
    for p in list(_LIVE_PROTOCOLS):
        p.close()
    for e in list(_LIVE_ENGINES):
        e.close()


atexit.register(_close_live)


class Engine:
    """One gevws_ctx (one per event loop / rank) on one GPU."""

    def __init__(self, device: int = 0):
        if device_count() <= device:
            raise RuntimeError(f"gev_amd.Engine: no HIP device {device} (found {device_count()}); "
                               "the decode path has no CPU fallback")
        self.device = device
        self._ctx = lib.gevws_ctx_create(device)
        if not self._ctx:
            raise RuntimeError("gevws_ctx_create failed")
        _LIVE_ENGINES.add(self)

    def close(self):
        if self._ctx:
            lib.gevws_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- tuning
    def set_tuning(self, key: int, value: int) -> None:
        st = lib.gevws_ctx_set_tuning(self._ctx, key, value)
        if st != OK:
            raise ValueError(f"set_tuning({key}, {value}): {status_string(st)}")

    # -------------------------------------------------------------- stream ordering
    def order_after_last(self, stream=None) -> None:
        """Make `stream` (default: torch's current stream) wait for this
        context's last call, whichever stream it ran on."""
        st = lib.gevws_ctx_order_after_last(self._ctx, _stream_handle(stream))
        if st != OK:
            raise RuntimeError(f"gevws_ctx_order_after_last: {status_string(st)}")

    @property
    def last_unmask_grid(self) -> int:
        """Workgroups of the last multi-kernel decode's unmask launch."""
        return int(lib.gevws_ctx_last_unmask_grid(self._ctx))

    @property
    def last_split_lanes(self) -> int:
        """Lanes per connection of the last multi-kernel decode's header walk (1 = not split)."""
        return int(lib.gevws_ctx_last_split_lanes(self._ctx))

    @property
    def last_split_fallbacks(self) -> int:
        """Connections the last multi-kernel decode's split walk re-walked
        serially after a missed guess (0 when not split; waits for the decode)."""
        return int(lib.gevws_ctx_last_split_fallbacks(self._ctx))

    @staticmethod
    def variant_name(i: int, key: int = _abi.TUNE_UNMASK_VARIANT) -> Optional[str]:
        n = lib.gevws_tuning_name(key, i)
        return n.decode() if n else None

    @staticmethod
    def variants(key: int = _abi.TUNE_UNMASK_VARIANT) -> List[int]:
        """Every valid value of a variant knob (GEVWS_TUNE_UNMASK_VARIANT / _WALK_VARIANT)."""
        out = []
        while Engine.variant_name(len(out), key) is not None:
            out.append(len(out))
        return out

    # -------------------------------------------------------------- timing
    def set_timing(self, enable: bool):
        lib.gevws_ctx_set_timing(self._ctx, int(enable))

    def timing(self) -> Tuple[Tuple[float, float, float, float], int]:
        """(summed ms per phase [walk-count, scan, walk-emit, unmask], calls) since the last query."""
        ms = (ctypes.c_float * 4)()
        calls = ctypes.c_uint32()
        st = lib.gevws_ctx_timing(self._ctx, ms, ctypes.byref(calls))
        if st != OK:
            raise RuntimeError(status_string(st))
        return tuple(ms), calls.value

    # -------------------------------------------------------------- decode
    def alloc_batch(self, n_conns: int, max_frames: int, payload_cap: int, aux_slots: int = 0) -> Batch:
        """Output buffers; aux_slots reserves room after the payload arena for
        close-reply bodies (Engine.serve)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        extra = (aux_slots * _abi.AUX_SLOT + 128) if aux_slots else 0
        return Batch(frames=torch.empty((max(max_frames, 1), 32), dtype=torch.uint8, device=dev),
                     payload=torch.empty(payload_cap + 16 + extra, dtype=torch.uint8, device=dev),
                     conn_out=torch.empty((max(n_conns, 1), 32), dtype=torch.uint8, device=dev),
                     summary=torch.zeros(64, dtype=torch.uint8, device=dev), n_conns=n_conns, aux_slots=aux_slots)

    def decode_async(self, arena, in_bytes: int, conns, n_conns: int, out: Batch, max_frames: int,
                     payload_cap: int, stream=None) -> None:
        """gevws_decode_batch_async on device tensors (arena: uint8 with IN_PAD slack;
        conns: int64 [n,2] = (off, len))."""
        st = lib.gevws_decode_batch_async(
            self._ctx, _stream_handle(stream), arena.data_ptr(), in_bytes,
            conns.data_ptr() if n_conns else None, n_conns, out.frames.data_ptr(), max_frames,
            out.payload.data_ptr(), payload_cap, out.conn_out.data_ptr(), out.summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_decode_batch_async: {status_string(st)}")

    def decode_post(self, arena, in_bytes: int, conns, n_conns: int, out: Batch, max_frames: int,
                    payload_cap: int) -> None:
        """gevws_decode_batch_post: a live pass on the context's stream, posted
        to the resident decode service when it is on (set_service) and the
        pass fits it, else launched; completion_seq tells which word to wait for."""
        st = lib.gevws_decode_batch_post(
            self._ctx, arena.data_ptr(), in_bytes, conns.data_ptr() if n_conns else None, n_conns,
            out.frames.data_ptr(), max_frames, out.payload.data_ptr(), payload_cap, out.conn_out.data_ptr(),
            out.summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_decode_batch_post: {status_string(st)}")

    def set_service(self, on: bool) -> None:
        """gevws_ctx_set_service: the resident decode service (False stops it)."""
        st = lib.gevws_ctx_set_service(self._ctx, 1 if on else 0)
        if st != OK:
            raise RuntimeError(f"gevws_ctx_set_service: {status_string(st)}")

    def service_stop(self) -> None:
        """gevws_ctx_service_stop: end the live instance (the next post starts another)."""
        lib.gevws_ctx_service_stop(self._ctx)

    def set_direct(self, on: bool) -> None:
        """gevws_ctx_set_direct: live passes written into the context's own AQL queue."""
        st = lib.gevws_ctx_set_direct(self._ctx, 1 if on else 0)
        if st != OK:
            raise RuntimeError(f"gevws_ctx_set_direct: {status_string(st)}")

    @property
    def direct_dispatches(self) -> int:
        """gevws_ctx_direct_dispatches: passes written into the context's own queue so far."""
        return int(lib.gevws_ctx_direct_dispatches(self._ctx))

    def synchronize(self) -> None:
        """gevws_ctx_synchronize: everything the context enqueued (stream, own queue, service)."""
        st = lib.gevws_ctx_synchronize(self._ctx)
        if st != OK:
            raise RuntimeError(f"gevws_ctx_synchronize: {status_string(st)}")

    def service_stats(self) -> dict:
        """gevws_ctx_service_stats: service instances launched, passes posted to them."""
        la, po = ctypes.c_int64(), ctypes.c_int64()
        lib.gevws_ctx_service_stats(self._ctx, ctypes.byref(la), ctypes.byref(po))
        return {"launches": la.value, "posts": po.value}

    def decode(self, arena, in_bytes: int, conns, n_conns: int, max_frames: Optional[int] = None,
               payload_cap: Optional[int] = None, stream=None, aux_slots: int = 0) -> Batch:
        """Decode a device-resident batch; grows capacities once on ERR_CAPACITY.
        aux_slots reserves close-reply space for a following Engine.serve."""
        torch = _torch()
        if max_frames is None:
            max_frames = min(in_bytes // 2 + 1, 0xFFFFFFFF)
        if payload_cap is None:
            payload_cap = in_bytes + 16 * min(max_frames, in_bytes // 64 + 64) + 64
        for attempt in range(2):
            out = self.alloc_batch(n_conns, max_frames, payload_cap, aux_slots)
            self.decode_async(arena, in_bytes, conns, n_conns, out, max_frames, payload_cap, stream)
            torch.cuda.synchronize(self.device)
            s = out.summary_host()
            if int(s["status"]) == ERR_CAPACITY and attempt == 0:
                max_frames = max(int(s["frames"]), 1)
                payload_cap = max(int(s["payload_bytes"]), 16)
                continue
            if int(s["status"]) != OK:
                raise RuntimeError(f"decode: {status_string(int(s['status']))}")
            return out
        raise RuntimeError("decode: capacity retry failed")

    def encode_async(self, frames_dev, n: int, payload, out, out_cap: int, out_off, summary, stream=None) -> None:
        """gevws_encode_batch_async: FrameToBytes for n records (OUT_FRAME_DTYPE rows as a
        uint8 [n, 32] device tensor) into `out` (>= out_cap + OUT_PAD bytes)."""
        st = lib.gevws_encode_batch_async(self._ctx, _stream_handle(stream), frames_dev.data_ptr() if n else None,
                                          n, payload.data_ptr(), out.data_ptr(), out_cap,
                                          out_off.data_ptr(), summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_encode_batch_async: {status_string(st)}")

    def encode(self, frames: np.ndarray, payload, out_cap: Optional[int] = None):
        """Encode host records (OUT_FRAME_DTYPE) whose payloads live in the device
        tensor `payload`; returns (wire device tensor [total], out_off numpy)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(frames.shape[0])
        if out_cap is None:
            out_cap = int(frames["payload_len"].sum()) + 14 * n
        fr = torch.from_numpy(np.ascontiguousarray(frames).view(np.uint8).reshape(-1, 32).copy()).to(dev) \
            if n else torch.zeros((1, 32), dtype=torch.uint8, device=dev)
        out = torch.empty(out_cap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
        off = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        self.encode_async(fr, n, payload, out, out_cap, off, summ)
        torch.cuda.synchronize(self.device)
        s = summ.cpu().numpy().view(SUMMARY_DTYPE)[0]
        if int(s["status"]) != OK:
            raise RuntimeError(f"encode: {status_string(int(s['status']))}")
        return out[: int(s["payload_bytes"])], off[:n].cpu().numpy().astype(np.uint64)

    def dispatch_async(self, frames_dev, n: int, policy: int, payload, aux_off: int, aux_cap: int, replies,
                       reply_of, summary, stream=None) -> None:
        """gevws_dispatch_async: HandlerWrap.OnMessage replies for n decoded frames."""
        st = lib.gevws_dispatch_async(self._ctx, _stream_handle(stream), frames_dev.data_ptr() if n else None, n,
                                      policy, payload.data_ptr(), aux_off, aux_cap,
                                      replies.data_ptr(), reply_of.data_ptr(), summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_dispatch_async: {status_string(st)}")

    def serve(self, out: "Batch", policy: int, aux_slots: Optional[int] = None):
        """One server step after a decode: dispatch (wrap.go:38-90) + encode of
        the replies.  `out.payload` must have room for the close-reply bodies
        after the decoded payloads (see alloc_batch(aux_slots=...)).  Returns
        (wire device tensor, reply_of numpy, summary of the dispatch)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        s = out.summary_host()
        n = int(s["frames"])
        aux_off = (int(s["payload_bytes"]) + 127) // 128 * 128
        aux_cap = out.payload.numel() - 16 - aux_off
        replies = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=dev)
        reply_of = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        dsum = torch.zeros(64, dtype=torch.uint8, device=dev)
        self.dispatch_async(out.frames, n, policy, out.payload, aux_off, max(aux_cap, 0), replies, reply_of, dsum)
        torch.cuda.synchronize(self.device)
        ds = dsum.cpu().numpy().view(SUMMARY_DTYPE)[0]
        if int(ds["status"]) != OK:
            raise RuntimeError(f"dispatch: {status_string(int(ds['status']))}")
        nr = int(ds["frames"])
        rep_host = replies[:nr].cpu().numpy().reshape(-1).view(OUT_FRAME_DTYPE)
        wire, _ = self.encode(rep_host, out.payload, int(rep_host["payload_len"].sum()) + 14 * nr)
        return wire, reply_of[:n].cpu().numpy(), ds

    # -------------------------------------------------------------- message layer
    def messages_async(self, frames, max_frames: int, conn_out, n_conns: int, decoded, payload, state, messages,
                       max_messages: int, msg_of, conn_msg, summary, stream=None) -> None:
        """gevws_messages_async on device tensors: fragment assembly, the RFC
        6455 frame checks and the UTF-8 check of text messages behind a decode
        (state: uint8 [n_conns, 8] read and rewritten, or None = all fresh)."""
        st = lib.gevws_messages_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, conn_out.data_ptr(), n_conns,
            decoded.data_ptr(), payload.data_ptr(), state.data_ptr() if state is not None else None,
            messages.data_ptr(), max_messages, msg_of.data_ptr(), conn_msg.data_ptr(), summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_messages_async: {status_string(st)}")

    def messages_ext_async(self, frames, max_frames: int, conn_out, n_conns: int, decoded, payload, state, messages,
                           max_messages: int, msg_of, conn_msg, summary, conn_ext, stream=None) -> None:
        """gevws_messages_ext_async: the message pass with one extension byte
        per connection (conn_ext: uint8 [n_conns], EXT_DEFLATE, or None)."""
        st = lib.gevws_messages_ext_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, conn_out.data_ptr(), n_conns,
            decoded.data_ptr(), payload.data_ptr(), state.data_ptr() if state is not None else None,
            messages.data_ptr(), max_messages, msg_of.data_ptr(), conn_msg.data_ptr(), summary.data_ptr(),
            conn_ext.data_ptr() if conn_ext is not None else None)
        if st != OK:
            raise RuntimeError(f"gevws_messages_ext_async: {status_string(st)}")

    def inflate_async(self, frames, max_frames: int, messages, max_messages: int, msg_of, msg_summary, payload,
                      max_message_bytes: int, state, inflated, out, out_cap: int, summary, stream=None) -> None:
        """gevws_inflate_async on device tensors: the compressed messages of a
        message pass inflated into `out` (state: the pass's uint8 [n_conns, 8],
        or None)."""
        st = lib.gevws_inflate_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, messages.data_ptr(), max_messages,
            msg_of.data_ptr(), msg_summary.data_ptr(), payload.data_ptr(), max_message_bytes,
            state.data_ptr() if state is not None else None, inflated.data_ptr(), out.data_ptr(), out_cap,
            summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_inflate_async: {status_string(st)}")

    def inflate_ctx_async(self, frames, max_frames: int, messages, max_messages: int, msg_of, msg_summary, payload,
                          max_message_bytes: int, state, inflated, out, out_cap: int, summary, conn_ext, contexts,
                          n_conns: int, stream=None) -> None:
        """gevws_inflate_ctx_async: inflate_async with client context takeover
        -- conn_ext: uint8 [n_conns] (EXT_DEFLATE | EXT_CLIENT_TAKEOVER),
        contexts: uint8 [n_conns, INF_CTX_BYTES], zeroed for fresh connections
        and carried from pass to pass.  Either None is inflate_async."""
        st = lib.gevws_inflate_ctx_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, messages.data_ptr(), max_messages,
            msg_of.data_ptr(), msg_summary.data_ptr(), payload.data_ptr(), max_message_bytes,
            state.data_ptr() if state is not None else None, inflated.data_ptr(), out.data_ptr(), out_cap,
            summary.data_ptr(), conn_ext.data_ptr() if conn_ext is not None else None,
            contexts.data_ptr() if contexts is not None else None, n_conns)
        if st != OK:
            raise RuntimeError(f"gevws_inflate_ctx_async: {status_string(st)}")

    def inflate_carry_async(self, frames, max_frames: int, messages, max_messages: int, msg_of, msg_summary, payload,
                            max_message_bytes: int, state, inflated, out, out_cap: int, summary, conn_ext, contexts,
                            n_conns: int, carry_in, carry_src, carry_src_bytes: int, stream=None) -> None:
        """gevws_inflate_carry_async: inflate_ctx_async plus the `in` side of
        the join's carry (carry_in: uint8 [n_conns, 32] records, carry_src:
        their arena) -- a continued compressed message whose record is
        CARRY_OPEN | CARRY_COMPRESSED is inflated behind its carried bytes.
        n_conns is required; conn_ext / contexts may be None.  carry_in or
        carry_src None is inflate_ctx_async."""
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_inflate_carry_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, messages.data_ptr(), max_messages,
            msg_of.data_ptr(), msg_summary.data_ptr(), payload.data_ptr(), max_message_bytes, p(state),
            inflated.data_ptr(), out.data_ptr(), out_cap, summary.data_ptr(), p(conn_ext), p(contexts), n_conns,
            p(carry_in), p(carry_src), carry_src_bytes)
        if st != OK:
            raise RuntimeError(f"gevws_inflate_carry_async: {status_string(st)}")

    def inflate(self, out: "Batch", msgs: "Messages", max_message_bytes: int, state=None,
                out_cap: Optional[int] = None, stream=None, conn_ext=None, contexts=None,
                carry: Optional["Carry"] = None) -> "Inflated":
        """The inflate step behind Engine.messages(out, conn_ext=...): every
        whole compressed message of the pass inflated.  Grows the output once
        on ERR_CAPACITY (nothing is written and the state is untouched by the
        call that did not fit).  With conn_ext and contexts (uint8 [n_conns,
        INF_CTX_BYTES], the caller's, carried from pass to pass) connections
        with EXT_CLIENT_TAKEOVER keep their window between messages; the call
        that did not fit leaves the contexts untouched too.  With carry (a
        Carry(compressed=True), before the pass's join) a compressed message
        that began in an earlier pass and ends in this one is inflated behind
        its carried bytes; the carry is only read."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(msgs.summary_host()["frames"])
        if out_cap is None:
            out_cap = 4 * int(out.summary_host()["payload_bytes"]) + 16 * n
            if carry is not None:
                out_cap += 4 * carry.used
        for attempt in range(2):
            res = Inflated(inflated=torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev),
                           out=torch.empty(max(out_cap, 16), dtype=torch.uint8, device=dev),
                           summary=torch.zeros(64, dtype=torch.uint8, device=dev), n_messages=n)
            if carry is not None:
                with_ctx = conn_ext is not None and contexts is not None
                self.inflate_carry_async(out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary,
                                         out.payload, max_message_bytes, state, res.inflated, res.out, out_cap,
                                         res.summary, conn_ext if with_ctx else None, contexts if with_ctx else None,
                                         carry.n_conns, carry.records_in, carry.arena, carry.used, stream)
            elif conn_ext is not None and contexts is not None:
                self.inflate_ctx_async(out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary,
                                       out.payload, max_message_bytes, state, res.inflated, res.out, out_cap,
                                       res.summary, conn_ext, contexts, int(contexts.shape[0]), stream)
            else:
                self.inflate_async(out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary,
                                   out.payload, max_message_bytes, state, res.inflated, res.out, out_cap,
                                   res.summary, stream)
            torch.cuda.synchronize(self.device)
            s = res.summary_host()
            if int(s["status"]) == ERR_CAPACITY and attempt == 0:
                out_cap = int(s["payload_bytes"])
                continue
            if int(s["status"]) != OK:
                raise RuntimeError(f"inflate: {status_string(int(s['status']))}")
            return res
        raise RuntimeError("inflate: capacity retry failed")

    def deflate_async(self, msgs, max_msgs: int, prev, src, src_bytes: int, flags: int, out_frames, out,
                      out_cap: int, summary, stream=None) -> None:
        """gevws_deflate_async on device tensors: the messages of `msgs`
        (DEFLATE_MSG_DTYPE rows as a uint8 [n, 24] tensor, their bytes in `src`)
        compressed into `out` (>= out_cap + OUT_PAD bytes) with their
        gevws_out_frame records in `out_frames`; prev: a producing step's
        summary that gates the count, or None."""
        st = lib.gevws_deflate_async(
            self._ctx, _stream_handle(stream), msgs.data_ptr() if max_msgs else None, max_msgs,
            prev.data_ptr() if prev is not None else None, src.data_ptr() if max_msgs else None, src_bytes, flags,
            out_frames.data_ptr() if max_msgs else None, out.data_ptr() if max_msgs else None, out_cap,
            summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_deflate_async: {status_string(st)}")

    def deflate_ctx_async(self, msgs, max_msgs: int, prev, src, src_bytes: int, flags: int, out_frames, out,
                          out_cap: int, summary, msg_conn, conn_ext, contexts, n_conns: int, stream=None) -> None:
        """gevws_deflate_ctx_async: deflate_async with server context takeover
        -- msg_conn: uint32 [max_msgs] (each message's connection), conn_ext:
        uint8 [n_conns] (EXT_DEFLATE | EXT_SERVER_TAKEOVER), contexts: uint8
        [n_conns, DEF_CTX_BYTES], zeroed for fresh connections and carried from
        call to call.  Any of the three None is deflate_async."""
        st = lib.gevws_deflate_ctx_async(
            self._ctx, _stream_handle(stream), msgs.data_ptr() if max_msgs else None, max_msgs,
            prev.data_ptr() if prev is not None else None, src.data_ptr() if max_msgs else None, src_bytes, flags,
            out_frames.data_ptr() if max_msgs else None, out.data_ptr() if max_msgs else None, out_cap,
            summary.data_ptr(), msg_conn.data_ptr() if msg_conn is not None else None,
            conn_ext.data_ptr() if conn_ext is not None else None,
            contexts.data_ptr() if contexts is not None else None, n_conns)
        if st != OK:
            raise RuntimeError(f"gevws_deflate_ctx_async: {status_string(st)}")

    def deflate(self, msgs: np.ndarray, src, src_bytes: int, flags: int = 0, out_cap: Optional[int] = None,
                stream=None, msg_conn=None, conn_ext=None, contexts=None) -> "Deflated":
        """The deflate step over host records (DEFLATE_MSG_DTYPE) whose bytes
        live in the device tensor `src` (src_bytes + IN_PAD long).  Grows the
        output once on ERR_CAPACITY (nothing is written by the call that did
        not fit).  With msg_conn (uint32 [n], host or device), conn_ext and
        contexts (uint8 [n_conns, DEF_CTX_BYTES], the caller's, carried from
        call to call) connections with EXT_SERVER_TAKEOVER keep their window
        between messages; the call that did not fit leaves the contexts
        untouched too."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(msgs.shape[0])
        d_msgs = torch.from_numpy(np.ascontiguousarray(msgs).view(np.uint8).reshape(-1, 24).copy()).to(dev) \
            if n else torch.zeros((1, 24), dtype=torch.uint8, device=dev)
        with_ctx = msg_conn is not None and conn_ext is not None and contexts is not None
        d_conn = None
        if with_ctx:
            d_conn = msg_conn if hasattr(msg_conn, "data_ptr") else \
                torch.from_numpy(np.ascontiguousarray(msg_conn, dtype=np.uint32).view(np.int32).copy()).to(dev)
        if out_cap is None:  # text compresses several-fold; the retry covers what does not
            out_cap = int(msgs["length"].sum()) // 2 + 16 * n
        for attempt in range(2):
            res = Deflated(frames=torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev),
                           out=torch.empty(out_cap + _abi.OUT_PAD, dtype=torch.uint8, device=dev),
                           summary=torch.zeros(64, dtype=torch.uint8, device=dev), n_messages=n)
            if with_ctx:
                self.deflate_ctx_async(d_msgs, n, None, src, src_bytes, flags, res.frames, res.out, out_cap,
                                       res.summary, d_conn, conn_ext, contexts, int(contexts.shape[0]), stream)
            else:
                self.deflate_async(d_msgs, n, None, src, src_bytes, flags, res.frames, res.out, out_cap, res.summary,
                                   stream)
            torch.cuda.synchronize(self.device)
            s = res.summary_host()
            if int(s["status"]) == ERR_CAPACITY and attempt == 0:
                out_cap = int(s["payload_bytes"])
                continue
            if int(s["status"]) != OK:
                raise RuntimeError(f"deflate: {status_string(int(s['status']))}")
            return res
        raise RuntimeError("deflate: capacity retry failed")

    # -------------------------------------------------------------- join / reply
    def join_async(self, frames, max_frames: int, messages, max_messages: int, msg_of, msg_summary, payload, inflated,
                   inflate_summary, flags: int, bodies, out, out_cap: int, summary, stream=None) -> None:
        """gevws_join_async on device tensors: one contiguous body per whole
        message of a message pass; fragmented ones are gathered into `out`
        behind the inflate's bytes (inflated / inflate_summary: the inflate
        step's records and summary, or None)."""
        st = lib.gevws_join_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, messages.data_ptr(), max_messages,
            msg_of.data_ptr(), msg_summary.data_ptr(), payload.data_ptr(),
            inflated.data_ptr() if inflated is not None else None,
            inflate_summary.data_ptr() if inflate_summary is not None else None, flags, bodies.data_ptr(),
            out.data_ptr(), out_cap, summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_join_async: {status_string(st)}")

    def join_carry_async(self, frames, max_frames: int, messages, max_messages: int, msg_of, msg_summary, payload,
                         inflated, inflate_summary, flags: int, bodies, out, out_cap: int, summary, conn_msg,
                         n_conns: int, max_message_bytes: int, carry_in, carry_src, carry_src_bytes: int, carry_out,
                         carry_dst, carry_cap: int, carry_summary, stream=None) -> None:
        """gevws_join_carry_async on device tensors: join_async plus the carry
        of open plain messages from pass to pass (carry_in / carry_src: the
        previous pass's carry_out / carry_dst, or None).  With conn_msg,
        carry_out, carry_dst or carry_summary None it is join_async."""
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_join_carry_async(
            self._ctx, _stream_handle(stream), p(frames), max_frames, p(messages), max_messages, p(msg_of),
            p(msg_summary), p(payload), p(inflated), p(inflate_summary), flags, p(bodies), p(out), out_cap,
            p(summary), p(conn_msg), n_conns, max_message_bytes, p(carry_in), p(carry_src), carry_src_bytes,
            p(carry_out), p(carry_dst), carry_cap, p(carry_summary))
        if st != OK:
            raise RuntimeError(f"gevws_join_carry_async: {status_string(st)}")

    def join_carry_ext_async(self, frames, max_frames: int, messages, max_messages: int, msg_of, msg_summary, payload,
                             inflated, inflate_summary, flags: int, bodies, out, out_cap: int, summary, conn_msg,
                             n_conns: int, max_message_bytes: int, carry_in, carry_src, carry_src_bytes: int,
                             carry_out, carry_dst, carry_cap: int, carry_summary, carry_flags: int,
                             stream=None) -> None:
        """gevws_join_carry_ext_async: join_carry_async plus carry_flags --
        with CARRY_KEEP_COMPRESSED open compressed messages are carried as
        compressed bytes (records CARRY_OPEN | CARRY_COMPRESSED) and a
        continued one that the inflate finished is delivered INFLATED.
        carry_flags 0 is join_carry_async."""
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_join_carry_ext_async(
            self._ctx, _stream_handle(stream), p(frames), max_frames, p(messages), max_messages, p(msg_of),
            p(msg_summary), p(payload), p(inflated), p(inflate_summary), flags, p(bodies), p(out), out_cap,
            p(summary), p(conn_msg), n_conns, max_message_bytes, p(carry_in), p(carry_src), carry_src_bytes,
            p(carry_out), p(carry_dst), carry_cap, p(carry_summary), carry_flags)
        if st != OK:
            raise RuntimeError(f"gevws_join_carry_ext_async: {status_string(st)}")

    def _join_with_carry(self, out: "Batch", msgs: "Messages", inflated, flags: int, out_cap: Optional[int], stream,
                         conn_msg, carry: "Carry") -> "Bodies":
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(msgs.summary_host()["frames"])
        inf_bytes = int(inflated.summary_host()["payload_bytes"]) if inflated is not None else 0
        if out_cap is None:  # the frames' slots, and a continued message's carried bytes in front
            out_cap = (inf_bytes + 15) // 16 * 16 + int(out.summary_host()["payload_bytes"]) + carry.used + 16
        src, dst = carry.side, 1 - carry.side
        need = carry.used + int(out.summary_host()["payload_bytes"])  # every byte kept or carried on
        if carry.cap(dst) < need:
            carry.arenas[dst] = carry._arena(need)
        for attempt in range(2):
            arena = torch.empty(max(out_cap, 16) + IN_PAD, dtype=torch.uint8, device=dev)
            if inf_bytes and inf_bytes <= out_cap:
                arena[:inf_bytes] = inflated.out[:inf_bytes]
            res = Bodies(bodies=torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev), out=arena,
                         summary=torch.zeros(64, dtype=torch.uint8, device=dev), payload=out.payload, n_messages=n,
                         out_cap=out_cap, carry_summary=torch.zeros(64, dtype=torch.uint8, device=dev))
            args = (out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary, out.payload,
                    inflated.inflated if inflated is not None else None,
                    inflated.summary if inflated is not None else None, flags, res.bodies, arena,
                    out_cap, res.summary, conn_msg, carry.n_conns, carry.max_message_bytes,
                    carry.records[src], carry.arenas[src], carry.used, carry.records[dst],
                    carry.arenas[dst], carry.cap(dst), res.carry_summary)
            if carry.carry_flags:
                self.join_carry_ext_async(*args, carry.carry_flags, stream)
            else:
                self.join_carry_async(*args, stream)
            torch.cuda.synchronize(self.device)
            s, cs = res.summary_host(), res.carry_summary_host()
            short = [x for x in (s, cs) if int(x["status"]) == ERR_CAPACITY]
            if short and attempt == 0:  # neither side was written: grow what did not fit, same inputs again
                if int(s["status"]) == ERR_CAPACITY:
                    out_cap = int(s["payload_bytes"])
                if int(cs["status"]) == ERR_CAPACITY:
                    carry.arenas[dst] = carry._arena(int(cs["payload_bytes"]))
                continue
            for x in (s, cs):
                if int(x["status"]) != OK:
                    raise RuntimeError(f"join: {status_string(int(x['status']))}")
            carry.side, carry.used = dst, int(cs["payload_bytes"])  # (only now: a failed call keeps the old carry)
            return res
        raise RuntimeError("join: capacity retry failed")

    def join(self, out: "Batch", msgs: "Messages", inflated: Optional["Inflated"] = None, flags: int = 0,
             out_cap: Optional[int] = None, stream=None, *, conn_msg=None, carry: Optional["Carry"] = None) -> "Bodies":
        """The join step behind Engine.messages (and Engine.inflate): every
        whole message's bytes as one (off, length).  With `inflated` the
        inflated bytes are kept below `base` of the returned arena and the
        joined bodies follow them.  Grows the arena once on ERR_CAPACITY
        (nothing is written by the call that did not fit).  With `carry` (a
        Carry; conn_msg: the message pass's table, msgs.conn_msg by default) a
        plain message that spans passes is kept in the carry and delivered with
        its FIN frame (a Carry(compressed=True): a compressed one too, inflated
        by Engine.inflate(carry=...) before this call); the carry's sides are
        swapped after a call that succeeded."""
        if carry is not None:
            return self._join_with_carry(out, msgs, inflated, flags, out_cap, stream,
                                         msgs.conn_msg if conn_msg is None else conn_msg, carry)
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(msgs.summary_host()["frames"])
        inf_bytes = int(inflated.summary_host()["payload_bytes"]) if inflated is not None else 0
        if out_cap is None:  # a joined body never takes more than its frames' slots
            out_cap = (inf_bytes + 15) // 16 * 16 + int(out.summary_host()["payload_bytes"])
        for attempt in range(2):
            arena = torch.empty(max(out_cap, 16) + IN_PAD, dtype=torch.uint8, device=dev)
            if inf_bytes and inf_bytes <= out_cap:  # (a smaller out_cap fails with the need, and the retry copies)
                arena[:inf_bytes] = inflated.out[:inf_bytes]
            res = Bodies(bodies=torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev), out=arena,
                         summary=torch.zeros(64, dtype=torch.uint8, device=dev), payload=out.payload, n_messages=n,
                         out_cap=out_cap)
            self.join_async(out.frames, msgs.n_frames, msgs.messages, n, msgs.msg_of, msgs.summary, out.payload,
                            inflated.inflated if inflated is not None else None,
                            inflated.summary if inflated is not None else None, flags, res.bodies, arena, out_cap,
                            res.summary, stream)
            torch.cuda.synchronize(self.device)
            s = res.summary_host()
            if int(s["status"]) == ERR_CAPACITY and attempt == 0:
                out_cap = int(s["payload_bytes"])
                continue
            if int(s["status"]) != OK:
                raise RuntimeError(f"join: {status_string(int(s['status']))}")
            return res
        raise RuntimeError("join: capacity retry failed")

    def reply_bodies_async(self, bodies, max_messages: int, msg_summary, join_summary, policy: int, conn_ext,
                           window_bits, n_conns: int, def_msgs, def_conn, def_summary, plain, plain_conn,
                           plain_summary, reply_of, stream=None) -> None:
        """gevws_reply_bodies_async on device tensors: the delivered bodies as
        the deflate step's message list (connections with EXT_DEFLATE in
        conn_ext) and the encoder's frame list (the others)."""
        st = lib.gevws_reply_bodies_async(
            self._ctx, _stream_handle(stream), bodies.data_ptr(), max_messages, msg_summary.data_ptr(),
            join_summary.data_ptr(), policy, conn_ext.data_ptr() if conn_ext is not None else None,
            window_bits.data_ptr() if window_bits is not None else None, n_conns, def_msgs.data_ptr(),
            def_conn.data_ptr(), def_summary.data_ptr(), plain.data_ptr(), plain_conn.data_ptr(),
            plain_summary.data_ptr(), reply_of.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_reply_bodies_async: {status_string(st)}")

    def encode_replies_async(self, replies, max_replies: int, dispatched, payload, out, out_cap: int, out_off,
                             summary, stream=None) -> None:
        """gevws_encode_replies_async: encode_async with the count read on the
        device from the producing step's summary."""
        st = lib.gevws_encode_replies_async(self._ctx, _stream_handle(stream), replies.data_ptr(), max_replies,
                                            dispatched.data_ptr(), payload.data_ptr(), out.data_ptr(), out_cap,
                                            out_off.data_ptr(), summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_encode_replies_async: {status_string(st)}")

    def fragment_async(self, records, max_records: int, prev, max_fragment_bytes: int, frags, max_frags: int, first,
                       summary, flags: int = 0, stream=None) -> None:
        """gevws_fragment_async on device tensors: every record longer than
        max_fragment_bytes as its fragments in `frags`, first[k] = record k's
        first fragment (max_records + 1 entries).  prev: the summary of the step
        that made the records, or None."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_fragment_async(self._ctx, _stream_handle(stream), ptr(records), max_records, ptr(prev),
                                      max_fragment_bytes, flags, ptr(frags), max_frags, ptr(first), ptr(summary))
        if st != OK:
            raise RuntimeError(f"gevws_fragment_async: {status_string(st)}")

    def fragment_offsets_async(self, first, max_records: int, prev, fragged, frag_off, frag_encoded, reply_off,
                               reply_encoded, stream=None) -> None:
        """gevws_fragment_offsets_async on device tensors, behind the encode of
        the fragments: one wire offset per reply and the summary that goes with
        it, for the send plan or the room plan."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_fragment_offsets_async(self._ctx, _stream_handle(stream), ptr(first), max_records, ptr(prev),
                                              ptr(fragged), ptr(frag_off), ptr(frag_encoded), ptr(reply_off),
                                              ptr(reply_encoded))
        if st != OK:
            raise RuntimeError(f"gevws_fragment_offsets_async: {status_string(st)}")

    def _fragmented_wire(self, recs, cap: int, gate, payload, k: int, total: int, max_fragment_bytes: int, stream,
                         who: str):
        """One record list's wire under a frame size limit: fragment -> encode
        -> offsets.  cap: the list's capacity, k its count, total its payload
        bytes.  -> ((the wire, host offsets per reply), (device offsets per
        reply, their summary), host first[k + 1]); the fragment step's
        ERR_CAPACITY is retried once from the need."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        F = int(max_fragment_bytes)
        if F < 1:
            raise ValueError(f"{who}: max_fragment_bytes must be at least 1")
        host = lambda t: t.cpu().numpy().view(SUMMARY_DTYPE)[0]  # noqa: E731
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        first, fsum = z(cap + 1, dt=torch.int64), z(64)
        max_frags = max(k, 1)
        for attempt in range(2):
            frags = z(max_frags, 32)
            self.fragment_async(recs, cap, gate, F, frags, max_frags, first, fsum, 0, stream)
            torch.cuda.synchronize(self.device)
            fs = host(fsum)
            if int(fs["status"]) == ERR_CAPACITY and attempt == 0:
                max_frags = int(fs["frames"])
                continue
            break
        if int(fs["status"]) != OK:
            raise RuntimeError(f"{who}: fragment: {status_string(int(fs['status']))} ({int(fs['errors'])})")
        wcap = total + 14 * int(fs["frames"]) + 16
        wire = torch.empty(wcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
        frag_off, esum = z(max_frags, dt=torch.int64), z(64)
        self.encode_replies_async(frags, max_frags, fsum, payload, wire, wcap, frag_off, esum, stream)
        off, rsum = z(cap, dt=torch.int64), z(64)
        self.fragment_offsets_async(first, cap, gate, fsum, frag_off, esum, off, rsum, stream)
        torch.cuda.synchronize(self.device)
        es, rs = host(esum), host(rsum)
        if int(es["status"]) != OK or int(rs["status"]) != OK:
            raise RuntimeError(f"{who}: encode {status_string(int(es['status']))}, offsets "
                               f"{status_string(int(rs['status']))} ({int(rs['errors'])})")
        return ((wire[: int(es["payload_bytes"])], off[:k].cpu().numpy().astype(np.uint64)), (off, rsum),
                first[: k + 1].cpu().numpy().astype(np.uint64))

    def echo_messages(self, out: "Batch", msgs: "Messages", bodies: "Bodies", policy: int, conn_ext,
                      window_bits=None, contexts=None, flags: int = 0, stream=None,
                      max_fragment_bytes: Optional[int] = None) -> "Echo":
        """A message-level echo with the lists built on the device: reply ->
        deflate (with contexts: deflate_ctx) -> the two encodes, all on
        `bodies.out`.  conn_ext / window_bits: uint8 [n_conns] device tensors
        (or None), contexts: uint8 [n_conns, DEF_CTX_BYTES] for connections with
        EXT_SERVER_TAKEOVER, flags: the deflate step's.  The bodies come from a
        join with JOIN_ALL.  max_fragment_bytes: no frame of a reply carries
        more payload than this (fragment -> encode -> offsets for each list;
        Echo.plain_first / def_first name the fragments); None: one frame a
        reply."""
        return self._echo_chain(out, msgs, bodies, policy, conn_ext, window_bits, contexts, flags, stream,
                                max_fragment_bytes)[0]

    def _echo_chain(self, out: "Batch", msgs: "Messages", bodies: "Bodies", policy: int, conn_ext, window_bits,
                    contexts, flags: int, stream, max_fragment_bytes: Optional[int] = None):
        """echo_messages' chain; beside the Echo, what the send plan reads of it
        on the device: (reply_of, [(offset table, encode summary) of the deflated
        wire, of the plain wire])."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n, n_conns = bodies.n_messages, out.n_conns
        cap = max(n, 1)
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        def_msgs, def_conn, def_sum = z(cap, 24), z(cap, dt=torch.int32), z(64)
        plain, plain_conn, plain_sum = z(cap, 32), z(cap, dt=torch.int32), z(64)
        reply_of = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        empty = Echo(z(0), np.zeros(0, np.uint32), np.zeros(0, np.uint64), z(0), np.zeros(0, np.uint32),
                     np.zeros(0, np.uint64), np.zeros(0, np.int64))
        if n == 0:
            return empty, reply_of, [(torch.zeros(1, dtype=torch.int64, device=dev), z(64)) for _ in range(2)]
        self.reply_bodies_async(bodies.bodies, n, msgs.summary, bodies.summary, policy, conn_ext, window_bits, n_conns,
                                def_msgs, def_conn, def_sum, plain, plain_conn, plain_sum, reply_of, stream)
        torch.cuda.synchronize(self.device)
        ds = def_sum.cpu().numpy().view(SUMMARY_DTYPE)[0]
        ps = plain_sum.cpu().numpy().view(SUMMARY_DTYPE)[0]
        if int(ds["status"]) != OK or int(ps["status"]) != OK:
            raise RuntimeError(f"reply_bodies: {status_string(int(ds['status']))} ({int(ds['errors'])} records)")
        nd, npl = int(ds["frames"]), int(ps["frames"])
        src_bytes = int(bodies.summary_host()["payload_bytes"])
        # the deflate step: gevws_deflate_bound per message holds whatever the bytes are
        dm = def_msgs[:nd].cpu().numpy().reshape(-1).view(DEFLATE_MSG_DTYPE)
        dcap = int(sum((deflate_bound(int(x)) + 15) // 16 * 16 for x in dm["length"])) + 16
        res = Deflated(frames=z(cap, 32), out=torch.empty(dcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev),
                       summary=z(64), n_messages=nd)
        if contexts is not None and conn_ext is not None:
            self.deflate_ctx_async(def_msgs, n, def_sum, bodies.out, src_bytes, flags, res.frames, res.out, dcap,
                                   res.summary, def_conn, conn_ext, contexts, int(contexts.shape[0]), stream)
        else:
            self.deflate_async(def_msgs, n, def_sum, bodies.out, src_bytes, flags, res.frames, res.out, dcap,
                               res.summary, stream)
        torch.cuda.synchronize(self.device)
        s = res.summary_host()
        if int(s["status"]) != OK:
            raise RuntimeError(f"echo_messages: deflate: {status_string(int(s['status']))}")
        wires, tables, firsts = [], [], [None, None]
        for recs, gate, payload, total in (
                (res.frames, res.summary, res.out, int(s["payload_len"])),
                (plain, plain_sum, bodies.out,
                 int(plain[:npl].cpu().numpy().reshape(-1).view(OUT_FRAME_DTYPE)["payload_len"].sum()))):
            k = int(gate.cpu().numpy().view(SUMMARY_DTYPE)[0]["frames"])
            if max_fragment_bytes is not None:
                w, t, firsts[len(wires)] = self._fragmented_wire(recs, n, gate, payload, k, total, max_fragment_bytes,
                                                                 stream, "echo_messages")
                wires.append(w)
                tables.append(t)
                continue
            wcap = total + 14 * k + 16
            wire = torch.empty(wcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
            off = torch.zeros(cap, dtype=torch.int64, device=dev)
            esum = z(64)
            self.encode_replies_async(recs, n, gate, payload, wire, wcap, off, esum, stream)
            torch.cuda.synchronize(self.device)
            es = esum.cpu().numpy().view(SUMMARY_DTYPE)[0]
            if int(es["status"]) != OK:
                raise RuntimeError(f"echo_messages: encode: {status_string(int(es['status']))}")
            wires.append((wire[: int(es["payload_bytes"])], off[:k].cpu().numpy().astype(np.uint64)))
            tables.append((off, esum))
        return Echo(def_wire=wires[0][0], def_conn=def_conn[:nd].cpu().numpy().view(np.uint32), def_off=wires[0][1],
                    plain_wire=wires[1][0], plain_conn=plain_conn[:npl].cpu().numpy().view(np.uint32),
                    plain_off=wires[1][1], reply_of=reply_of[:n].cpu().numpy(), deflated=res, plain_first=firsts[1],
                    def_first=firsts[0]), reply_of, tables

    def control_async(self, frames, max_frames: int, conn_out, n_conns: int, decoded, payload, aux_off: int,
                      aux_cap: int, msg_of, messages, max_messages: int, conn_msg, msg_summary, bodies, join_summary,
                      flags: int, ctl, ctl_conn, ctl_of, msg_end, conn_ctl, summary, stream=None) -> None:
        """gevws_control_async on device tensors: the control replies and the
        failure closes up to each connection's cut, the bodies behind it
        stripped in place."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_control_async(
            self._ctx, _stream_handle(stream), frames.data_ptr(), max_frames, conn_out.data_ptr(), n_conns,
            decoded.data_ptr(), payload.data_ptr(), aux_off, aux_cap, msg_of.data_ptr(), ptr(messages), max_messages,
            conn_msg.data_ptr(), msg_summary.data_ptr(), ptr(bodies), join_summary.data_ptr(), flags, ctl.data_ptr(),
            ctl_conn.data_ptr(), ctl_of.data_ptr(), ptr(msg_end), conn_ctl.data_ptr(), summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_control_async: {status_string(st)}")

    def send_plan_async(self, max_frames: int, decoded, conn_out, n_conns: int, msg_of, msg_end, reply_of,
                        max_messages: int, msg_summary, join_summary, conn_ext, ctl_of, conn_ctl, ctl_summary,
                        plain_off, plain_encoded, def_off, def_encoded, ctl_off, ctl_encoded, send, max_sends: int,
                        conn_send, summary, stream=None) -> None:
        """gevws_send_plan_async on device tensors: which bytes of the three
        wire buffers go to which connection, in send order."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_send_plan_async(
            self._ctx, _stream_handle(stream), max_frames, decoded.data_ptr(), conn_out.data_ptr(), n_conns,
            msg_of.data_ptr(), ptr(msg_end), ptr(reply_of), max_messages, msg_summary.data_ptr(),
            join_summary.data_ptr(), ptr(conn_ext), ctl_of.data_ptr(), conn_ctl.data_ptr(), ctl_summary.data_ptr(),
            plain_off.data_ptr(), plain_encoded.data_ptr(), def_off.data_ptr(), def_encoded.data_ptr(),
            ctl_off.data_ptr(), ctl_encoded.data_ptr(), ptr(send), max_sends, conn_send.data_ptr(),
            summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_send_plan_async: {status_string(st)}")

    def send_gather_async(self, send, max_sends: int, conn_send, n_conns: int, plan_summary, wires, wire_bytes,
                          buf, buf_cap: int, conn_buf, summary, flags: int = 0, stream=None) -> None:
        """gevws_send_gather_async on device tensors: every connection's plan
        entries copied back to back into its 16-aligned span of `buf` (device
        memory or a PinnedArena address).  wires: the three wire buffers (plain,
        deflated, control; None: an empty one), wire_bytes: the readable bytes
        of each."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        bases = (ctypes.c_void_p * 3)(*[ptr(w) for w in wires])
        nbytes = (ctypes.c_uint64 * 3)(*[int(x) for x in wire_bytes])
        st = lib.gevws_send_gather_async(
            self._ctx, _stream_handle(stream), ptr(send), max_sends, conn_send.data_ptr(), n_conns,
            plan_summary.data_ptr(), ctypes.addressof(bases), ctypes.addressof(nbytes), flags, ptr(buf), buf_cap,
            conn_buf.data_ptr(), summary.data_ptr())
        if st != OK:
            raise RuntimeError(f"gevws_send_gather_async: {status_string(st)}")

    def _gather(self, send, max_sends: int, conn_send, n_conns: int, plan_sum, plan_bytes: int, wires, stream):
        """respond's last step: the buffer sized from the plan's summary, grown
        once on ERR_CAPACITY.  -> (send_buf, conn_buf, the gather's summary)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        cap = (plan_bytes + 16 * n_conns + 15) // 16 * 16
        conn_buf = torch.zeros((max(n_conns, 1), 32), dtype=torch.uint8, device=dev)
        gsum = torch.zeros(64, dtype=torch.uint8, device=dev)
        for attempt in range(2):
            buf = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
            self.send_gather_async(send, max_sends, conn_send, n_conns, plan_sum, wires,
                                   [int(w.numel()) for w in wires], buf, cap, conn_buf, gsum, 0, stream)
            torch.cuda.synchronize(self.device)
            gs = gsum.cpu().numpy().view(SUMMARY_DTYPE)[0]
            if int(gs["status"]) == ERR_CAPACITY and attempt == 0:
                cap = int(gs["payload_bytes"])
                continue
            if int(gs["status"]) != OK:
                raise RuntimeError(f"respond: gather: {status_string(int(gs['status']))} ({int(gs['errors'])})")
            return (buf[: int(gs["payload_bytes"])],
                    conn_buf[:n_conns].cpu().numpy().reshape(-1).view(CONN_BUF_DTYPE), gs)
        raise RuntimeError("respond: gather: capacity retry failed")

    def respond(self, out: "Batch", msgs: "Messages", bodies: "Bodies", policy: int, conn_ext, window_bits=None,
                contexts=None, flags: int = 0, control_flags: int = 0, stream=None,
                gather: bool = False, max_fragment_bytes: Optional[int] = None) -> "Responses":
        """Everything a pass sends: control -> reply -> deflate (with contexts:
        deflate_ctx) -> the three encodes -> plan.  The arguments are
        echo_messages'; control_flags: the control step's.  `bodies` (from a join
        with JOIN_ALL) is rewritten in place: messages behind a connection's cut
        are no longer delivered.  The close bodies go into the aux slots
        alloc_batch reserved, one per connection at the most.  gather=True ends
        the chain with the gather: send_buf / conn_buf / gather_summary hold
        every connection's bytes in one buffer (Responses.host_sends).
        max_fragment_bytes: the replies' frame size limit (echo_messages);
        control replies are never fragmented."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n_conns, nf, nm = out.n_conns, msgs.n_frames, bodies.n_messages
        if out.aux_slots < n_conns:
            raise ValueError(f"respond: the batch reserves {out.aux_slots} aux slots for {n_conns} connections")
        aux_cap = _abi.AUX_SLOT * out.aux_slots
        aux_off = (out.payload.numel() - 16 - aux_cap) // 16 * 16
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        capf, capm, capc = max(nf, 1), max(nm, 1), max(n_conns, 1)
        ctl, ctl_conn, ctl_sum = z(capf, 32), z(capf, dt=torch.int32), z(64)
        ctl_of = torch.full((capf,), -1, dtype=torch.int64, device=dev)
        msg_end = torch.full((capm,), -1, dtype=torch.int64, device=dev)
        conn_ctl = z(capc, 32)
        conn_ctl.view(torch.int64)[:, 0] = -1  # no cut
        self.control_async(out.frames, nf, out.conn_out, n_conns, out.summary, out.payload, aux_off, aux_cap,
                           msgs.msg_of, msgs.messages, nm, msgs.conn_msg, msgs.summary, bodies.bodies, bodies.summary,
                           control_flags, ctl, ctl_conn, ctl_of, msg_end, conn_ctl, ctl_sum, stream)
        torch.cuda.synchronize(self.device)
        cs = ctl_sum.cpu().numpy().view(SUMMARY_DTYPE)[0]
        if int(cs["status"]) != OK:
            raise RuntimeError(f"respond: control: {status_string(int(cs['status']))} ({int(cs['errors'])})")
        echo, reply_of, tables = self._echo_chain(out, msgs, bodies, policy, conn_ext, window_bits, contexts, flags,
                                                  stream, max_fragment_bytes)
        nr = int(cs["frames"])
        total = int(ctl[:nr].cpu().numpy().reshape(-1).view(OUT_FRAME_DTYPE)["payload_len"].sum())
        wcap = total + 14 * nr + 16
        ctl_wire = torch.empty(wcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
        ctl_off, ctl_enc = torch.zeros(capf, dtype=torch.int64, device=dev), z(64)
        self.encode_replies_async(ctl, nf, ctl_sum, out.payload, ctl_wire, wcap, ctl_off, ctl_enc, stream)
        send, conn_send, plan_sum = z(capf, 32), z(capc, 32), z(64)
        (def_off, def_enc), (plain_off, plain_enc) = tables
        self.send_plan_async(nf, out.summary, out.conn_out, n_conns, msgs.msg_of, msg_end, reply_of, nm, msgs.summary,
                             bodies.summary, conn_ext, ctl_of, conn_ctl, ctl_sum, plain_off, plain_enc, def_off,
                             def_enc, ctl_off, ctl_enc, send, nf, conn_send, plan_sum, stream)
        torch.cuda.synchronize(self.device)
        es = ctl_enc.cpu().numpy().view(SUMMARY_DTYPE)[0]
        ps = plan_sum.cpu().numpy().view(SUMMARY_DTYPE)[0]
        if int(es["status"]) != OK or int(ps["status"]) != OK:
            raise RuntimeError(f"respond: encode {status_string(int(es['status']))}, plan "
                               f"{status_string(int(ps['status']))} ({int(ps['errors'])})")
        send_buf = conn_buf = gsum = None
        if gather:
            wires = (echo.plain_wire, echo.def_wire, ctl_wire[: int(es["payload_bytes"])])
            send_buf, conn_buf, gsum = self._gather(send, nf, conn_send, n_conns, plan_sum, int(ps["payload_bytes"]),
                                                    wires, stream)
        return Responses(echo=echo, ctl_wire=ctl_wire[: int(es["payload_bytes"])],
                         ctl_conn=ctl_conn[:nr].cpu().numpy().view(np.uint32), ctl_of=ctl_of[:nf].cpu().numpy(),
                         msg_end=msg_end[:nm].cpu().numpy().view(np.uint64),
                         conn_ctl=conn_ctl[:n_conns].cpu().numpy().reshape(-1).view(CONN_CTL_DTYPE), ctl_summary=cs,
                         send=send, conn_send=conn_send, summary=plan_sum, n_conns=n_conns, send_buf=send_buf,
                         conn_buf=conn_buf, gather_summary=gsum)

    def reply_rooms_async(self, bodies, max_messages: int, msg_summary, join_summary, policy: int, conn_ext,
                          window_bits, n_conns: int, rooms: "Rooms", flags: int, def_msgs, def_conn, def_summary,
                          plain, plain_conn, plain_summary, plain_of, def_of, stream=None) -> None:
        """gevws_reply_rooms_async on device tensors: every delivered body once
        in the plain list and once in the deflate list, as its room's members
        need it (flags: ROOMS_SKIP_SENDER)."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_reply_rooms_async(
            self._ctx, _stream_handle(stream), ptr(bodies), max_messages, ptr(msg_summary), ptr(join_summary), policy,
            ptr(conn_ext), ptr(window_bits), n_conns, ptr(rooms.conn_room), ptr(rooms.room_first),
            ptr(rooms.room_members), rooms.n_rooms, rooms.n_members, flags, ptr(def_msgs), ptr(def_conn),
            ptr(def_summary), ptr(plain), ptr(plain_conn), ptr(plain_summary), ptr(plain_of), ptr(def_of))
        if st != OK:
            raise RuntimeError(f"gevws_reply_rooms_async: {status_string(st)}")

    def room_plan_async(self, max_frames: int, decoded, conn_out, n_conns: int, msg_of, msg_end, plain_of, def_of,
                        max_messages: int, msg_summary, join_summary, conn_ext, ctl_of, conn_ctl, ctl_summary,
                        plain_off, plain_encoded, def_off, def_encoded, ctl_off, ctl_encoded, rooms: "Rooms",
                        flags: int, send, max_sends: int, conn_send, summary, stream=None) -> None:
        """gevws_room_plan_async on device tensors: the send plan with every
        published frame named once per recipient of its room."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_room_plan_async(
            self._ctx, _stream_handle(stream), max_frames, ptr(decoded), ptr(conn_out), n_conns, ptr(msg_of),
            ptr(msg_end), ptr(plain_of), ptr(def_of), max_messages, ptr(msg_summary), ptr(join_summary),
            ptr(conn_ext), ptr(ctl_of), ptr(conn_ctl), ptr(ctl_summary), ptr(plain_off), ptr(plain_encoded),
            ptr(def_off), ptr(def_encoded), ptr(ctl_off), ptr(ctl_encoded), ptr(rooms.conn_room),
            ptr(rooms.room_first), ptr(rooms.room_members), rooms.n_rooms, rooms.n_members, flags, ptr(send),
            max_sends, ptr(conn_send), ptr(summary))
        if st != OK:
            raise RuntimeError(f"gevws_room_plan_async: {status_string(st)}")

    def rooms_update_async(self, conn_room_in, n_conns: int, n_rooms: int, changes, max_changes: int, prev,
                           conn_send, plan_summary, flags: int, conn_room_out, room_first_out, room_members_out,
                           summary, stream=None) -> None:
        """gevws_rooms_update_async on device tensors: the changes (and the
        closes of conn_send) applied to conn_room_in, the new rooms and their
        CSR inverse written to the three outputs."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_rooms_update_async(
            self._ctx, _stream_handle(stream), ptr(conn_room_in), n_conns, n_rooms, ptr(changes), max_changes,
            ptr(prev), ptr(conn_send), ptr(plan_summary), flags, ptr(conn_room_out), ptr(room_first_out),
            ptr(room_members_out), ptr(summary))
        if st != OK:
            raise RuntimeError(f"gevws_rooms_update_async: {status_string(st)}")

    def room_commands_async(self, bodies, max_messages: int, msg_summary, join_summary, ctl_summary, out,
                            src_bytes: int, n_conns: int, n_rooms: int, flags: int, changes, max_changes: int,
                            change_of, summary, stream=None) -> None:
        """gevws_room_commands_async on device tensors: "/join N" and "/leave"
        in delivered text bodies become {conn, room} records in `changes`, and
        those bodies are stripped in place (status MSG_COMMAND)."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = lib.gevws_room_commands_async(
            self._ctx, _stream_handle(stream), ptr(bodies), max_messages, ptr(msg_summary), ptr(join_summary),
            ptr(ctl_summary), ptr(out), src_bytes, n_conns, n_rooms, flags, ptr(changes), max_changes,
            ptr(change_of), ptr(summary))
        if st != OK:
            raise RuntimeError(f"gevws_room_commands_async: {status_string(st)}")

    def broadcast(self, out: "Batch", msgs: "Messages", bodies: "Bodies", policy: int, conn_ext, rooms: "Rooms",
                  window_bits=None, flags: int = 0, rooms_flags: int = 0, control_flags: int = 0,
                  gather: bool = False, stream=None, max_fragment_bytes: Optional[int] = None,
                  commands: bool = False) -> "Responses":
        """Everything a pass sends when a message goes to its sender's room:
        control -> reply_rooms -> deflate -> the three encodes -> room plan ->
        (gather).  The arguments are respond's, without contexts (a broadcast
        payload is shared, so no connection's window can hold it); rooms: the
        room tables, rooms_flags: ROOMS_SKIP_SENDER or 0, flags: the deflate
        step's.  The result is respond's: conn_bytes(c) and host_sends() work
        unchanged; echo.def_conn / echo.plain_conn name the senders.
        max_fragment_bytes: one frame size limit for every recipient (a
        message is framed once).  commands=True puts the room-command step
        between the control step and the reply step: "/join N" and "/leave"
        messages leave the broadcast and come back as room_changes, for
        Rooms.update(changes=res.room_changes, closed=res) behind the pass."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n_conns, nf, nm = out.n_conns, msgs.n_frames, bodies.n_messages
        if out.aux_slots < n_conns:
            raise ValueError(f"broadcast: the batch reserves {out.aux_slots} aux slots for {n_conns} connections")
        aux_cap = _abi.AUX_SLOT * out.aux_slots
        aux_off = (out.payload.numel() - 16 - aux_cap) // 16 * 16
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        host = lambda t: t.cpu().numpy().view(SUMMARY_DTYPE)[0]  # noqa: E731
        capf, capm, capc = max(nf, 1), max(nm, 1), max(n_conns, 1)
        ctl, ctl_conn, ctl_sum = z(capf, 32), z(capf, dt=torch.int32), z(64)
        ctl_of = torch.full((capf,), -1, dtype=torch.int64, device=dev)
        msg_end = torch.full((capm,), -1, dtype=torch.int64, device=dev)
        conn_ctl = z(capc, 32)
        conn_ctl.view(torch.int64)[:, 0] = -1  # no cut
        self.control_async(out.frames, nf, out.conn_out, n_conns, out.summary, out.payload, aux_off, aux_cap,
                           msgs.msg_of, msgs.messages, nm, msgs.conn_msg, msgs.summary, bodies.bodies, bodies.summary,
                           control_flags, ctl, ctl_conn, ctl_of, msg_end, conn_ctl, ctl_sum, stream)
        room_changes = None
        if commands:
            room_changes = RoomChanges(changes=z(capm, 8), change_of=torch.full((capm,), -1, dtype=torch.int64,
                                                                                device=dev),
                                       summary=z(64), max_changes=nm, n_messages=nm)
            if nm:
                self.room_commands_async(bodies.bodies, nm, msgs.summary, bodies.summary, ctl_sum, bodies.out,
                                         int(bodies.summary_host()["payload_bytes"]), n_conns, rooms.n_rooms, 0,
                                         room_changes.changes, nm, room_changes.change_of, room_changes.summary,
                                         stream)
        def_msgs, def_conn, def_sum = z(capm, 24), z(capm, dt=torch.int32), z(64)
        plain, plain_conn, plain_sum = z(capm, 32), z(capm, dt=torch.int32), z(64)
        plain_of = torch.full((capm,), -1, dtype=torch.int64, device=dev)
        def_of = torch.full((capm,), -1, dtype=torch.int64, device=dev)
        self.reply_rooms_async(bodies.bodies, nm, msgs.summary, bodies.summary, policy, conn_ext, window_bits, n_conns,
                               rooms, rooms_flags, def_msgs, def_conn, def_sum, plain, plain_conn, plain_sum, plain_of,
                               def_of, stream)
        torch.cuda.synchronize(self.device)
        cs, ds, ps = host(ctl_sum), host(def_sum), host(plain_sum)
        if int(cs["status"]) != OK:
            raise RuntimeError(f"broadcast: control: {status_string(int(cs['status']))} ({int(cs['errors'])})")
        if room_changes is not None and int(room_changes.summary_host()["status"]) != OK:
            rs = room_changes.summary_host()
            raise RuntimeError(f"broadcast: room_commands: {status_string(int(rs['status']))} ({int(rs['errors'])})")
        if int(ds["status"]) != OK or int(ps["status"]) != OK:
            raise RuntimeError(f"broadcast: reply_rooms: {status_string(int(ds['status']))} ({int(ds['errors'])} records)")
        nd, npl, nr = int(ds["frames"]), int(ps["frames"]), int(cs["frames"])
        src_bytes = int(bodies.summary_host()["payload_bytes"]) if nm else 0
        dm = def_msgs[:nd].cpu().numpy().reshape(-1).view(DEFLATE_MSG_DTYPE)
        dcap = int(sum((deflate_bound(int(x)) + 15) // 16 * 16 for x in dm["length"])) + 16
        res = Deflated(frames=z(capm, 32), out=torch.empty(dcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev),
                       summary=z(64), n_messages=nd)
        if nm:
            self.deflate_async(def_msgs, nm, def_sum, bodies.out, src_bytes, flags, res.frames, res.out, dcap,
                               res.summary, stream)
            torch.cuda.synchronize(self.device)
        s = res.summary_host()
        if int(s["status"]) != OK:
            raise RuntimeError(f"broadcast: deflate: {status_string(int(s['status']))}")
        lens = lambda recs, k: int(recs[:k].cpu().numpy().reshape(-1).view(OUT_FRAME_DTYPE)["payload_len"].sum())  # noqa: E731
        wires, tables, firsts = [], [], [None, None, None]
        for recs, cap, gate, payload, k, total in (
                (plain, capm, plain_sum, bodies.out if nm else out.payload, npl, lens(plain, npl)),
                (res.frames, capm, res.summary, res.out, nd, int(s["payload_len"])),
                (ctl, capf, ctl_sum, out.payload, nr, lens(ctl, nr))):
            if max_fragment_bytes is not None and len(wires) < 2:  # (the control replies stay whole)
                w, t, firsts[len(wires)] = self._fragmented_wire(recs, cap, gate, payload, k, total,
                                                                 max_fragment_bytes, stream, "broadcast")
                wires.append(w)
                tables.append(t)
                continue
            wcap = total + 14 * k + 16
            wire = torch.empty(wcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
            off, esum = torch.zeros(cap, dtype=torch.int64, device=dev), z(64)
            self.encode_replies_async(recs, cap, gate, payload, wire, wcap, off, esum, stream)
            torch.cuda.synchronize(self.device)
            es = host(esum)
            if int(es["status"]) != OK:
                raise RuntimeError(f"broadcast: encode: {status_string(int(es['status']))}")
            wires.append((wire[: int(es["payload_bytes"])], off[:k].cpu().numpy().astype(np.uint64)))
            tables.append((off, esum))
        (plain_off, plain_enc), (def_off, def_enc), (ctl_off, ctl_enc) = tables
        conn_send, plan_sum = z(capc, 32), z(64)
        max_sends = capf
        for attempt in range(2):
            send = z(max(max_sends, 1), 32)
            self.room_plan_async(nf, out.summary, out.conn_out, n_conns, msgs.msg_of, msg_end, plain_of, def_of, nm,
                                 msgs.summary, bodies.summary, conn_ext, ctl_of, conn_ctl, ctl_sum, plain_off,
                                 plain_enc, def_off, def_enc, ctl_off, ctl_enc, rooms, rooms_flags, send, max_sends,
                                 conn_send, plan_sum, stream)
            torch.cuda.synchronize(self.device)
            pls = host(plan_sum)
            if int(pls["status"]) == ERR_CAPACITY and attempt == 0:   # a fan-out: more entries than frames
                max_sends = int(pls["frames"])
                continue
            break
        if int(pls["status"]) != OK:
            raise RuntimeError(f"broadcast: plan: {status_string(int(pls['status']))} ({int(pls['errors'])})")
        echo = Echo(def_wire=wires[1][0], def_conn=def_conn[:nd].cpu().numpy().view(np.uint32), def_off=wires[1][1],
                    plain_wire=wires[0][0], plain_conn=plain_conn[:npl].cpu().numpy().view(np.uint32),
                    plain_off=wires[0][1], reply_of=plain_of[:nm].cpu().numpy(), deflated=res,
                    plain_first=firsts[0], def_first=firsts[1])
        send_buf = conn_buf = gsum = None
        if gather:
            send_buf, conn_buf, gsum = self._gather(send, max_sends, conn_send, n_conns, plan_sum,
                                                    int(pls["payload_bytes"]),
                                                    (wires[0][0], wires[1][0], wires[2][0]), stream)
        return Responses(echo=echo, ctl_wire=wires[2][0], ctl_conn=ctl_conn[:nr].cpu().numpy().view(np.uint32),
                         ctl_of=ctl_of[:nf].cpu().numpy(), msg_end=msg_end[:nm].cpu().numpy().view(np.uint64),
                         conn_ctl=conn_ctl[:n_conns].cpu().numpy().reshape(-1).view(CONN_CTL_DTYPE), ctl_summary=cs,
                         send=send, conn_send=conn_send, summary=plan_sum, n_conns=n_conns, send_buf=send_buf,
                         conn_buf=conn_buf, gather_summary=gsum, plain_of=plain_of[:nm].cpu().numpy(),
                         def_of=def_of[:nm].cpu().numpy(), room_changes=room_changes)

    def push_lists_async(self, pushes, max_pushes: int, prev, src_bytes: int, conn_ext, window_bits, live,
                         n_conns: int, rooms: Optional["Rooms"], flags: int, def_msgs, def_summary, plain,
                         plain_summary, plain_of, def_of, stream=None) -> None:
        """gevws_push_lists_async on device tensors: every push once in the
        plain list and once in the deflate list, as its live recipients need it.
        rooms None: no room tables (a ROOM push is then malformed); prev: the
        summary of whatever made the list on the device, or None."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        tabs = (None, None, None, 0, 0) if rooms is None else (
            ptr(rooms.conn_room), ptr(rooms.room_first), ptr(rooms.room_members), rooms.n_rooms, rooms.n_members)
        st = lib.gevws_push_lists_async(
            self._ctx, _stream_handle(stream), ptr(pushes), max_pushes, ptr(prev), src_bytes, ptr(conn_ext),
            ptr(window_bits), ptr(live), n_conns, *tabs, flags, ptr(def_msgs), ptr(def_summary), ptr(plain),
            ptr(plain_summary), ptr(plain_of), ptr(def_of))
        if st != OK:
            raise RuntimeError(f"gevws_push_lists_async: {status_string(st)}")

    def push_plan_async(self, pushes, max_pushes: int, prev, src_bytes: int, plain_summary, def_summary, plain_of,
                        def_of, plain_off, plain_encoded, def_off, def_encoded, conn_ext, live, n_conns: int,
                        rooms: Optional["Rooms"], flags: int, send, max_sends: int, conn_send, summary,
                        stream=None) -> None:
        """gevws_push_plan_async on device tensors: every push's one encoded
        frame named once per live recipient, each recipient's in list order."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        tabs = (None, None, None, 0, 0) if rooms is None else (
            ptr(rooms.conn_room), ptr(rooms.room_first), ptr(rooms.room_members), rooms.n_rooms, rooms.n_members)
        st = lib.gevws_push_plan_async(
            self._ctx, _stream_handle(stream), ptr(pushes), max_pushes, ptr(prev), src_bytes, ptr(plain_summary),
            ptr(def_summary), ptr(plain_of), ptr(def_of), ptr(plain_off), ptr(plain_encoded), ptr(def_off),
            ptr(def_encoded), ptr(conn_ext), ptr(live), n_conns, *tabs, flags, ptr(send), max_sends, ptr(conn_send),
            ptr(summary))
        if st != OK:
            raise RuntimeError(f"gevws_push_plan_async: {status_string(st)}")

    def push(self, pushes, src, conn_ext, rooms: Optional["Rooms"] = None, window_bits=None, live=None,
             flags: int = 0, gather: bool = False, max_fragment_bytes: Optional[int] = None, stream=None, *,
             n_conns: Optional[int] = None) -> "Responses":
        """A push pass, messages the host originates: push_lists -> deflate (no
        contexts) -> the two encodes -> push plan -> (gather).  pushes: the
        sorted PUSH_DTYPE records and src their body arena, as push_records
        returns them (numpy, uploaded; or device tensors: uint8 [n, 32] and a
        uint8 arena whose last IN_PAD bytes are slack).  conn_ext / window_bits
        / live: uint8 [n_conns] device tensors or None (no deflate-taker /
        window 15 / every connection a live session); rooms: the room tables or
        None; flags: the deflate step's.  n_conns: the connection table's size,
        by default that of the first table given.  The result is respond's, with
        an empty control wire: conn_bytes(c) and host_sends() work unchanged,
        send[k].frame is the push's index in the list and plain_of / def_of its
        place in the two lists.  max_fragment_bytes: one frame size limit for
        every recipient; pings and pongs stay whole."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if n_conns is None:
            tabs = [t for t in (conn_ext, live, window_bits, rooms.conn_room if rooms is not None else None)
                    if t is not None]
            if not tabs:
                raise ValueError("push: n_conns is needed when no connection table is given")
            n_conns = int(tabs[0].numel())
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        host = lambda t: t.cpu().numpy().view(SUMMARY_DTYPE)[0]  # noqa: E731
        if not isinstance(pushes, torch.Tensor):
            recs = np.ascontiguousarray(pushes, dtype=PUSH_DTYPE).reshape(-1)
            pushes = torch.from_numpy(recs.view(np.uint8).reshape(-1, 32).copy()).to(dev)
        if not isinstance(src, torch.Tensor):
            src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.uint8).copy()).to(dev)
        n = int(pushes.numel()) // 32
        src_bytes = int(src.numel()) - IN_PAD
        if src_bytes < 0:
            raise ValueError("push: src is shorter than its IN_PAD bytes of slack")
        cap, capc = max(n, 1), max(n_conns, 1)
        def_msgs, def_sum, plain, plain_sum = z(cap, 24), z(64), z(cap, 32), z(64)
        plain_of = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        def_of = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        self.push_lists_async(pushes, n, None, src_bytes, conn_ext, window_bits, live, n_conns, rooms, 0, def_msgs,
                              def_sum, plain, plain_sum, plain_of, def_of, stream)
        torch.cuda.synchronize(self.device)
        ds, ps = host(def_sum), host(plain_sum)
        if int(ds["status"]) != OK or int(ps["status"]) != OK:
            raise RuntimeError(f"push: push_lists: {status_string(int(ds['status']))} ({int(ds['errors'])} records)")
        nd, npl = int(ds["frames"]), int(ps["frames"])
        dm = def_msgs[:nd].cpu().numpy().reshape(-1).view(DEFLATE_MSG_DTYPE)
        dcap = int(sum((deflate_bound(int(x)) + 15) // 16 * 16 for x in dm["length"])) + 16
        res = Deflated(frames=z(cap, 32), out=torch.empty(dcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev),
                       summary=z(64), n_messages=nd)
        if n:
            self.deflate_async(def_msgs, n, def_sum, src, src_bytes, flags, res.frames, res.out, dcap, res.summary,
                               stream)
            torch.cuda.synchronize(self.device)
        s = res.summary_host()
        if int(s["status"]) != OK:
            raise RuntimeError(f"push: deflate: {status_string(int(s['status']))}")
        total0 = int(plain[:npl].cpu().numpy().reshape(-1).view(OUT_FRAME_DTYPE)["payload_len"].sum())
        wires, tables, firsts = [], [], [None, None]
        for recs, gate, payload, k, total in ((plain, plain_sum, src, npl, total0),
                                              (res.frames, res.summary, res.out, nd, int(s["payload_len"]))):
            if max_fragment_bytes is not None:
                w, t, firsts[len(wires)] = self._fragmented_wire(recs, cap, gate, payload, k, total,
                                                                 max_fragment_bytes, stream, "push")
                wires.append(w)
                tables.append(t)
                continue
            wcap = total + 14 * k + 16
            wire = torch.empty(wcap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
            off, esum = torch.zeros(cap, dtype=torch.int64, device=dev), z(64)
            self.encode_replies_async(recs, cap, gate, payload, wire, wcap, off, esum, stream)
            torch.cuda.synchronize(self.device)
            es = host(esum)
            if int(es["status"]) != OK:
                raise RuntimeError(f"push: encode: {status_string(int(es['status']))}")
            wires.append((wire[: int(es["payload_bytes"])], off[:k].cpu().numpy().astype(np.uint64)))
            tables.append((off, esum))
        (plain_off, plain_enc), (def_off, def_enc) = tables
        conn_send, plan_sum = z(capc, 32), z(64)
        max_sends = cap
        for attempt in range(2):
            send = z(max(max_sends, 1), 32)
            self.push_plan_async(pushes, n, None, src_bytes, plain_sum, def_sum, plain_of, def_of, plain_off,
                                 plain_enc, def_off, def_enc, conn_ext, live, n_conns, rooms, 0, send, max_sends,
                                 conn_send, plan_sum, stream)
            torch.cuda.synchronize(self.device)
            pls = host(plan_sum)
            if int(pls["status"]) == ERR_CAPACITY and attempt == 0:   # a fan-out: more entries than pushes
                max_sends = int(pls["frames"])
                continue
            break
        if int(pls["status"]) != OK:
            raise RuntimeError(f"push: plan: {status_string(int(pls['status']))} ({int(pls['errors'])})")
        none32 = np.zeros(0, np.uint32)
        echo = Echo(def_wire=wires[1][0], def_conn=none32, def_off=wires[1][1], plain_wire=wires[0][0],
                    plain_conn=none32, plain_off=wires[0][1], reply_of=plain_of[:n].cpu().numpy(), deflated=res,
                    plain_first=firsts[0], def_first=firsts[1])
        ctl_wire = z(0)
        send_buf = conn_buf = gsum = None
        if gather:
            send_buf, conn_buf, gsum = self._gather(send, max_sends, conn_send, n_conns, plan_sum,
                                                    int(pls["payload_bytes"]), (wires[0][0], wires[1][0], ctl_wire),
                                                    stream)
        return Responses(echo=echo, ctl_wire=ctl_wire, ctl_conn=none32, ctl_of=np.zeros(0, np.int64),
                         msg_end=np.zeros(0, np.uint64), conn_ctl=np.zeros(n_conns, CONN_CTL_DTYPE),
                         ctl_summary=np.zeros(1, SUMMARY_DTYPE)[0], send=send, conn_send=conn_send, summary=plan_sum,
                         n_conns=n_conns, send_buf=send_buf, conn_buf=conn_buf, gather_summary=gsum,
                         plain_of=plain_of[:n].cpu().numpy(), def_of=def_of[:n].cpu().numpy())

    def messages(self, out: "Batch", state=None, max_messages: Optional[int] = None, stream=None, *,
                 conn_ext=None) -> "Messages":
        """The message pass over a decoded batch; `state` (uint8 [n_conns, 8]
        device tensor) carries open messages from pass to pass and is updated
        in place.  Grows the message table once on ERR_CAPACITY (the state is
        untouched by the pass that did not fit).  conn_ext (uint8 [n_conns]
        device tensor of EXT_DEFLATE bytes) marks the connections that
        negotiated permessage-deflate."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(out.summary_host()["frames"]) if int(out.summary_host()["status"]) == OK else 0
        if max_messages is None:
            max_messages = n
        for attempt in range(2):
            res = Messages(messages=torch.empty((max(max_messages, 1), 32), dtype=torch.uint8, device=dev),
                           msg_of=torch.empty(max(n, 1), dtype=torch.int64, device=dev),
                           conn_msg=torch.zeros((max(out.n_conns, 1), 32), dtype=torch.uint8, device=dev),
                           state=state, summary=torch.zeros(64, dtype=torch.uint8, device=dev),
                           n_conns=out.n_conns, n_frames=n)
            self.messages_ext_async(out.frames, n, out.conn_out, out.n_conns, out.summary, out.payload, state,
                                    res.messages, max_messages, res.msg_of, res.conn_msg, res.summary, conn_ext,
                                    stream)
            torch.cuda.synchronize(self.device)
            s = res.summary_host()
            if int(s["status"]) == ERR_CAPACITY and attempt == 0:
                max_messages = int(s["frames"])
                continue
            if int(s["status"]) != OK:
                raise RuntimeError(f"messages: {status_string(int(s['status']))}")
            return res
        raise RuntimeError("messages: capacity retry failed")

    def set_completion_flag(self, arena: Optional["PinnedArena"], offset: int = 0) -> None:
        """gevws_ctx_set_completion_flag: the one-launch kernels store their
        sequence number into the 32-bit word at arena.host[offset:offset+4]
        (None: off)."""
        addr = arena.at(offset).data_ptr() if arena is not None else None
        st = lib.gevws_ctx_set_completion_flag(self._ctx, addr)
        if st != OK:
            raise RuntimeError(f"gevws_ctx_set_completion_flag: {status_string(st)}")

    def set_timeline_ticks(self, arena: Optional["PinnedArena"], offset: int = 0) -> None:
        """gevws_ctx_set_timeline_ticks: the one-launch kernels stamp their start /
        end ticks (GPU constant-rate clock) into 4 u64 at arena.host[offset:offset+32]
        before they signal (None: off)."""
        addr = arena.at(offset).data_ptr() if arena is not None else None
        st = lib.gevws_ctx_set_timeline_ticks(self._ctx, addr)
        if st != OK:
            raise RuntimeError(f"gevws_ctx_set_timeline_ticks: {status_string(st)}")

    @property
    def completion_seq(self) -> int:
        """gevws_ctx_completion_seq: the number the last call's last kernel
        stores into the completion word, -1 when it does not signal."""
        return int(lib.gevws_ctx_completion_seq(self._ctx))

    def handle_decoded(self, out: "Batch", policy: int, max_frames: int, aux_slots: int, out_cap: int):
        """gevws_handle_decoded_async: dispatch + encode of the replies chained
        behind the decode with no host round trip (one launch when max_frames
        <= 1 024).  Returns (wire device tensor, reply_of numpy, dispatch
        summary, encode summary)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        # the close bodies go into the slots alloc_batch reserved behind the
        # payload arena, never over decoded payloads the replies still read
        if not 0 <= aux_slots <= out.aux_slots:
            raise ValueError(f"handle_decoded: aux_slots {aux_slots} outside the batch's {out.aux_slots} reserved slots")
        aux_off = (out.payload.numel() - 16 - 128 * aux_slots) // 16 * 16
        n = max(int(max_frames), 1)
        replies = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        reply_of = torch.full((n,), -7, dtype=torch.int64, device=dev)
        sums = torch.zeros(128, dtype=torch.uint8, device=dev)
        wire = torch.zeros(out_cap + _abi.OUT_PAD, dtype=torch.uint8, device=dev)
        off = torch.empty(n, dtype=torch.int64, device=dev)
        st = lib.gevws_handle_decoded_async(self._ctx, None, out.frames.data_ptr(), int(max_frames),
                                            out.summary.data_ptr(), int(policy), out.payload.data_ptr(), aux_off,
                                            128 * aux_slots, replies.data_ptr(), reply_of.data_ptr(),
                                            sums.data_ptr(), wire.data_ptr(), int(out_cap), off.data_ptr(),
                                            sums.data_ptr() + 64)
        if st != OK:
            raise RuntimeError(f"gevws_handle_decoded_async: {status_string(st)}")
        torch.cuda.synchronize(self.device)
        ss = sums.cpu().numpy().view(SUMMARY_DTYPE)
        nf = int(out.summary_host()["frames"])
        return wire[: int(ss[1]["payload_bytes"])], reply_of[:nf].cpu().numpy(), ss[0], ss[1]

    def cipher_(self, buf, mask: bytes, offset: int = 0, nbytes: Optional[int] = None,
                byte_offset: int = 0, stream=None) -> None:
        """ws.Cipher (cipher.go:14-53) in place on a device uint8 tensor region."""
        m = (ctypes.c_uint8 * 4)(*mask)
        n = buf.numel() - byte_offset if nbytes is None else nbytes
        st = lib.gevws_cipher_async(self._ctx, _stream_handle(stream), buf.data_ptr() + byte_offset, n, m,
                                    offset)
        if st != OK:
            raise RuntimeError(status_string(st))

    def copy_(self, dst, src, nbytes: int, dst_offset: int = 0, src_offset: int = 0, grid: int = 0,
              stream=None) -> None:
        """gevws_copy_async: the streaming-copy ceiling kernel (measurement only)."""
        assert dst_offset + nbytes <= dst.numel() and src_offset + nbytes <= src.numel()
        st = lib.gevws_copy_async(self._ctx, _stream_handle(stream), dst.data_ptr() + dst_offset,
                                  src.data_ptr() + src_offset, nbytes, grid)
        if st != OK:
            raise RuntimeError(status_string(st))

    def synth(self, arena, desc_dev, n_frames: int, seed: int, stream=None) -> None:
        st = lib.gevws_synth_async(self._ctx, _stream_handle(stream), arena.data_ptr(), desc_dev.data_ptr(),
                                   n_frames, seed)
        if st != OK:
            raise RuntimeError(status_string(st))

    def verify(self, desc_dev, n_frames: int, seed: int, out: Batch, mismatch_dev, stream=None) -> None:
        if out.frames.shape[0] < n_frames:
            raise ValueError("verify: batch holds fewer frame records than the layout")
        st = lib.gevws_synth_verify_async(self._ctx, _stream_handle(stream), desc_dev.data_ptr(), n_frames,
                                          seed, out.frames.data_ptr(), out.payload.data_ptr(),
                                          out.payload.numel() - 16, mismatch_dev.data_ptr())
        if st != OK:
            raise RuntimeError(status_string(st))


# ====================================================================== host mirror
class RingBuffer:
    """ringbuffer.RingBuffer as gev uses it (New / Write / Length / PeekAll / Retrieve)."""

    def __init__(self, size: int = 4096):
        self._p = lib.gevws_ring_new(size)

    def __del__(self, _free=lib.gevws_ring_free):  # bound now: module globals are gone at exit
        if getattr(self, "_p", None):
            _free(self._p)
            self._p = None

    def write(self, data: bytes) -> int:
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data) if data else None
        return lib.gevws_ring_write(self._p, buf, len(data))

    def length(self) -> int:
        return lib.gevws_ring_length(self._p)

    def capacity(self) -> int:
        return lib.gevws_ring_capacity(self._p)

    def is_empty(self) -> bool:
        return self.length() == 0

    def peek_all(self) -> Tuple[bytes, bytes]:
        a, b = _abi.U8P(), _abi.U8P()
        na, nb = ctypes.c_uint64(), ctypes.c_uint64()
        lib.gevws_ring_peek_all(self._p, ctypes.byref(a), ctypes.byref(na), ctypes.byref(b), ctypes.byref(nb))
        first = ctypes.string_at(a, na.value) if na.value else b""
        end = ctypes.string_at(b, nb.value) if nb.value else b""
        return first, end

    def retrieve(self, n: int) -> None:
        lib.gevws_ring_retrieve(self._p, n)


_CONNS: "weakref.WeakValueDictionary[int, Connection]" = weakref.WeakValueDictionary()


class Connection:
    """The per-connection context keys of the websocket plugin (protocol.go:11-14)."""

    def __init__(self, upgraded: bool = True):
        self._p = lib.gevws_conn_new()
        _CONNS[self._p] = self
        self.set_upgraded(upgraded)

    def __del__(self, _free=lib.gevws_conn_free):  # bound now: module globals are gone at exit
        if getattr(self, "_p", None):
            _free(self._p)
            self._p = None

    def handshake(self) -> "HandshakeInfo":
        """The last handshake's ws.Handshake and error (after UnPacket ran it)."""
        hs = _abi.Handshake()
        lib.gevws_conn_handshake(self._p, ctypes.byref(hs))
        return HandshakeInfo._from(hs)

    def set_upgraded(self, v: bool) -> None:
        lib.gevws_conn_set_upgraded(self._p, int(v))

    @property
    def upgraded(self) -> bool:
        return bool(lib.gevws_conn_upgraded(self._p))

    def pending(self) -> int:
        return lib.gevws_conn_pending(self._p)


class RejectError(Exception):
    """ws.RejectConnectionError(RejectionStatus(code), RejectionReason(reason),
    RejectionHeader(header)) (plugins/websocket/ws/errors.go:81-129).  Raise it
    from an Upgrader hook; any other exception is a plain Go error (HTTP 500,
    ws.go:325-333)."""

    def __init__(self, reason: str = "", code: int = 0, header: bytes = b""):
        super().__init__(reason)
        self.reason, self.code, self.header = reason, code, header


class HandshakeError(Exception):
    """A failed Upgrader.Upgrade: kind = GEVWS_HS_*, reason = err.Error()."""

    def __init__(self, kind: int, reason: str, http_code: int):
        super().__init__(reason)
        self.kind, self.reason, self.http_code = kind, reason, http_code


@dataclass
class HandshakeInfo:
    """ws.Handshake (ws/ws.go:40-47) plus the error of the call."""
    protocol: bytes
    extensions: bytes
    error: int
    http_code: int
    reason: str

    @staticmethod
    def _from(hs: "_abi.Handshake") -> "HandshakeInfo":
        return HandshakeInfo(ctypes.string_at(hs.protocol, hs.protocol_len) if hs.protocol_len else b"",
                             ctypes.string_at(hs.extensions, hs.extensions_len) if hs.extensions_len else b"",
                             hs.error, hs.http_code, (hs.reason or b"").decode())


def accept_key(nonce: bytes) -> bytes:
    """initAcceptFromNonce (ws/nonce.go:23-39) through the C ABI."""
    assert len(nonce) == 24
    out = ctypes.create_string_buffer(28)
    lib.gevws_accept_key(nonce, out)
    return out.raw


class Upgrader:
    """ws.Upgrader (plugins/websocket/ws/ws.go:49-154) over the C ABI.

    Hooks take the reference's arguments (bytes for []byte):
      protocol(token) -> bool;  protocol_custom(conn, value) -> (selected, ok);
      extension(name, [(key, value or None)]) -> bool;
      extension_custom(conn, value, selected_so_far) -> (selected, ok);
      on_request(conn, uri), on_host(conn, host), on_header(conn, key, value):
        return None to accept, raise RejectError / Exception to reject;
      on_before_upgrade(conn) -> extra response header bytes or None, or raise.
    ``header`` is Upgrader.Header (raw "Key: value\\r\\n" lines)."""

    def __init__(self, header: bytes = b"", **hooks):
        self._p = lib.gevws_upgrader_new()
        self._keep: list = []
        if header:
            lib.gevws_upgrader_set_header(self._p, header, len(header))
        unknown = set(hooks) - {"protocol", "protocol_custom", "extension", "extension_custom", "on_request",
                                "on_host", "on_header", "on_before_upgrade"}
        if unknown:
            raise TypeError(f"unknown Upgrader hooks {sorted(unknown)}")
        self._hooks = hooks
        h = _abi.UpgraderHooks()
        for name, fn in hooks.items():
            if fn is not None:
                setattr(h, name, getattr(self, "_c_" + name)())
        self._cstruct = h
        lib.gevws_upgrader_set_hooks(self._p, ctypes.byref(h))

    def __del__(self, _free=lib.gevws_upgrader_free):  # bound now: module globals are gone at exit
        if getattr(self, "_p", None):
            _free(self._p)
            self._p = None

    # -- C trampolines (each keeps its own ctypes callback object alive)
    def _hold(self, b: bytes) -> int:
        buf = ctypes.create_string_buffer(b, len(b) + 1)
        self._keep.append(buf)
        return ctypes.addressof(buf)

    def _reject(self, rej, e: Exception) -> int:
        r = rej.contents
        if isinstance(e, RejectError):
            reason = e.reason.encode()
            r.code, r.plain = e.code, 0
            if e.header:
                r.header, r.header_len = self._hold(e.header), len(e.header)
        else:
            reason = str(e).encode()
            r.code, r.plain = 0, 1
        r.reason, r.reason_len = self._hold(reason), len(reason)
        return 1

    @staticmethod
    def _b(p, n) -> bytes:
        return ctypes.string_at(p, n) if n else b""

    def _c_protocol(self):
        fn = self._hooks["protocol"]
        return _abi.HOOK_PROTOCOL(lambda u, t, n: int(bool(fn(self._b(t, n)))))

    def _c_protocol_custom(self):
        fn = self._hooks["protocol_custom"]

        def cb(u, c, v, n, sel, sel_n):
            got, ok = fn(_CONNS.get(c), self._b(v, n))
            got = got.encode() if isinstance(got, str) else (got or b"")
            sel[0], sel_n[0] = (self._hold(got) if got else None), len(got)
            return int(bool(ok))
        return _abi.HOOK_PROTOCOL_CUSTOM(cb)

    def _c_extension(self):
        fn = self._hooks["extension"]

        def cb(u, name, n, params, npar):
            ps = [(self._b(params[i].key, params[i].key_len),
                   None if not params[i].value else self._b(params[i].value, params[i].value_len))
                  for i in range(npar)]
            return int(bool(fn(self._b(name, n), ps)))
        return _abi.HOOK_EXTENSION(cb)

    def _c_extension_custom(self):
        fn = self._hooks["extension_custom"]

        def cb(u, c, v, n, cur, cur_n, sel, sel_n):
            got, ok = fn(_CONNS.get(c), self._b(v, n), self._b(cur, cur_n))
            got = got or b""
            sel[0], sel_n[0] = (self._hold(got) if got else None), len(got)
            return int(bool(ok))
        return _abi.HOOK_EXTENSION_CUSTOM(cb)

    def _value_hook(self, name):
        fn = self._hooks[name]

        def cb(u, c, v, n, rej):
            try:
                fn(_CONNS.get(c), self._b(v, n))
                return 0
            except Exception as e:  # noqa: BLE001 -- every hook error is a rejection
                return self._reject(rej, e)
        return _abi.HOOK_ON_VALUE(cb)

    def _c_on_request(self):
        return self._value_hook("on_request")

    def _c_on_host(self):
        return self._value_hook("on_host")

    def _c_on_header(self):
        fn = self._hooks["on_header"]

        def cb(u, c, k, kn, v, vn, rej):
            try:
                fn(_CONNS.get(c), self._b(k, kn), self._b(v, vn))
                return 0
            except Exception as e:  # noqa: BLE001
                return self._reject(rej, e)
        return _abi.HOOK_ON_HEADER(cb)

    def _c_on_before_upgrade(self):
        fn = self._hooks["on_before_upgrade"]

        def cb(u, c, hdr, hdr_len, rej):
            try:
                extra = fn(_CONNS.get(c))
                if extra:
                    hdr[0], hdr_len[0] = self._hold(extra), len(extra)
                return 0
            except Exception as e:  # noqa: BLE001
                return self._reject(rej, e)
        return _abi.HOOK_ON_BEFORE_UPGRADE(cb)

    def upgrade(self, c: "Connection", buffer: "RingBuffer") -> Tuple[bytes, HandshakeInfo, Optional[HandshakeError]]:
        """Upgrade(c, in) -> (out, hs, err) (ws.go:158-343)."""
        self._keep.clear()
        out = _abi.U8P()
        n = ctypes.c_uint64()
        hs = _abi.Handshake()
        st = lib.gevws_upgrader_upgrade(self._p, c._p, buffer._p, ctypes.byref(out), ctypes.byref(n),
                                        ctypes.byref(hs))
        if st not in (OK, ERR_HANDSHAKE):
            raise RuntimeError(f"upgrade: {status_string(st)}")
        info = HandshakeInfo._from(hs)
        data = ctypes.string_at(out, n.value) if n.value else b""
        err = None if st == OK else HandshakeError(info.error, info.reason, info.http_code)
        return data, info, err


class DeviceArena:
    """gevws_device_alloc: zeroed device memory of a chosen kind (default,
    fine-grained or uncached); `data_ptr()` / `at(off)` for the launch
    wrappers (measurement helper: where the input arena lives)."""

    def __init__(self, device: int, nbytes: int, kind: int = 0):
        p = ctypes.c_void_p()
        st = lib.gevws_device_alloc(device, nbytes, kind, ctypes.byref(p))
        if st != OK:
            raise RuntimeError(f"gevws_device_alloc({nbytes}, kind {kind}): {status_string(st)}")
        self.device, self.nbytes, self.kind, self._p = device, nbytes, kind, p.value

    def data_ptr(self) -> int:
        return self._p

    def at(self, offset: int = 0) -> _DevAddr:
        if not 0 <= offset <= self.nbytes:
            raise ValueError(f"DeviceArena.at({offset}): outside {self.nbytes} bytes")
        return _DevAddr(self._p + offset)

    def close(self) -> None:
        if getattr(self, "_p", None):
            lib.gevws_device_free(self.device, self._p)
            self._p = None

    def __del__(self, _free=lib.gevws_device_free):
        if getattr(self, "_p", None):
            _free(self.device, self._p)


class Comm:
    """gevws_comm: an RCCL communicator over several GPUs of ONE process (a gev
    server whose event loops are placed on the node's devices round-robin) and
    the decode path's one collective, the all-reduce(sum) of every device's
    decoded {frames, payload bytes, errors}."""

    def __init__(self, devices: Sequence[int]):
        arr = (ctypes.c_int * len(devices))(*devices)
        self._p = lib.gevws_comm_create(arr, len(devices))
        if not self._p:
            raise RuntimeError(f"gevws_comm_create({list(devices)}) failed (RCCL missing or device not visible)")
        self.devices = list(devices)

    def __del__(self, _free=lib.gevws_comm_destroy):
        if getattr(self, "_p", None):
            _free(self._p)
            self._p = None

    def size(self) -> int:
        return int(lib.gevws_comm_size(self._p))

    def allreduce_counts(self, engines: Sequence["Engine"], batches: Sequence["Batch"]) -> Tuple[int, int, int]:
        """gevws_counts_allreduce over each device's last decode summary; every
        device's batch gets the totals in `counts` (int64[3] on its device);
        returns (frames, payload_len, errors) summed over the devices."""
        import torch
        n = len(self.devices)
        if len(engines) != n or len(batches) != n:
            raise ValueError("one engine and one batch per device of the communicator")
        # written only by the contexts' streams (no fill on torch's stream); the
        # blocks may have been freed by work still queued on torch's current
        # stream, so that stream is drained first (this is the synchronous form)
        counts = [torch.empty(3, dtype=torch.int64, device=torch.device("cuda", e.device)) for e in engines]
        for e in engines:
            torch.cuda.current_stream(torch.device("cuda", e.device)).synchronize()
        ctxs = (ctypes.c_void_p * n)(*[e._ctx for e in engines])
        sums = (ctypes.c_void_p * n)(*[b.summary.data_ptr() for b in batches])
        cnts = (ctypes.c_void_p * n)(*[c.data_ptr() for c in counts])
        tot = (ctypes.c_int64 * 3)()
        st = lib.gevws_counts_allreduce(self._p, ctxs, sums, cnts, tot)
        if st != OK:
            raise RuntimeError(f"gevws_counts_allreduce: {status_string(st)}")
        for b, c in zip(batches, counts):
            b.counts = c
        return int(tot[0]), int(tot[1]), int(tot[2])


class Protocol:
    """websocket.Protocol (plugins/websocket/protocol.go:16-69) over the device engine."""

    def __init__(self, engine: Engine, upgrader: Optional[Upgrader] = None):
        self.engine = engine
        self._p = lib.gevws_protocol_new(engine._ctx)
        _LIVE_PROTOCOLS.add(self)
        self.upgrader = upgrader
        if upgrader is not None:
            lib.gevws_protocol_set_upgrader(self._p, upgrader._p)

    def __del__(self, _free=lib.gevws_protocol_free):  # bound now: module globals are gone at exit
        if getattr(self, "_p", None):
            _free(self._p)
            self._p = None

    def close(self) -> None:
        """Free the protocol (it synchronises its engine's stream, so it must go
        before the engine: _close_live does protocols first at exit)."""
        if getattr(self, "_p", None):
            lib.gevws_protocol_free(self._p)
            self._p = None

    def unpacket(self, c: Connection, buffer: RingBuffer) -> Tuple[Optional[Header], Optional[bytes]]:
        """UnPacket(c, buffer) -> (ctx, out): one frame; (None, response) for
        the handshake (protocol.go:29-37); or (None, None)."""
        if self.upgrader is not None:
            self.upgrader._keep.clear()
        h = Header()
        out = _abi.U8P()
        n = ctypes.c_uint64()
        st = lib.gevws_protocol_unpacket(self._p, c._p, buffer._p, ctypes.byref(h), ctypes.byref(out),
                                         ctypes.byref(n))
        self.last_status = st
        if st in (HANDSHAKE, ERR_HANDSHAKE):
            return None, (ctypes.string_at(out, n.value) if n.value else None)
        if st != OK:
            return None, None
        return h, (ctypes.string_at(out, n.value) if n.value else b"")

    def unpacket_batch(self, conns: Sequence[Connection], buffers: Sequence[RingBuffer]) -> int:
        n = len(conns)
        cs = (ctypes.c_void_p * n)(*[c._p for c in conns])
        rs = (ctypes.c_void_p * n)(*[b._p for b in buffers])
        r = lib.gevws_protocol_unpacket_batch(self._p, cs, rs, n)
        if r < 0:
            raise RuntimeError(f"unpacket_batch: {status_string(int(r))}")
        return int(r)

    def unpacket_batch_begin(self, conns: Sequence[Connection], buffers: Sequence[RingBuffer]) -> int:
        """gevws_protocol_unpacket_batch_begin: stage and enqueue the pass, do not wait;
        returns the connections in it."""
        n = len(conns)
        cs = (ctypes.c_void_p * n)(*[c._p for c in conns])
        rs = (ctypes.c_void_p * n)(*[b._p for b in buffers])
        # the C side keeps the raw pointers until _end: hold the Python objects
        # too, so no Connection / RingBuffer is freed under a pass in flight
        self._pending = (cs, rs, list(conns), list(buffers))
        r = lib.gevws_protocol_unpacket_batch_begin(self._p, cs, rs, n)
        if r < 0:
            raise RuntimeError(f"unpacket_batch_begin: {status_string(int(r))}")
        return int(r)

    def unpacket_batch_end(self) -> int:
        """gevws_protocol_unpacket_batch_end: wait for the pass in flight and queue its frames."""
        r = lib.gevws_protocol_unpacket_batch_end(self._p)
        self._pending = None
        if r < 0:
            raise RuntimeError(f"unpacket_batch_end: {status_string(int(r))}")
        return int(r)

    def set_handler(self, policy: int) -> None:
        """gevws_protocol_set_handler: HandlerWrap.OnMessage on the device for
        every frame a pass decodes (GEVWS_HANDLER_*; -1 = off)."""
        st = lib.gevws_protocol_set_handler(self._p, int(policy))
        if st != OK:
            raise ValueError(f"set_handler({policy}): {status_string(st)}")

    def reply(self, c: Connection) -> Tuple[Optional[bytes], bool]:
        """gevws_protocol_reply: (reply wire bytes or None, ShutdownWrite) -- the
        device handler's answer for the frame unpacket() last returned on c."""
        out = _abi.U8P()
        n = ctypes.c_uint64()
        sh = ctypes.c_int()
        st = lib.gevws_protocol_reply(self._p, c._p, ctypes.byref(out), ctypes.byref(n), ctypes.byref(sh))
        if st != OK:
            raise RuntimeError(f"reply: {status_string(st)}")
        return (ctypes.string_at(out, n.value) if n.value else None), bool(sh.value)

    def set_service(self, on: bool) -> None:
        """gevws_protocol_set_service: zero-copy passes without a handler step
        go to the context's resident decode service (no launch call)."""
        st = lib.gevws_protocol_set_service(self._p, 1 if on else 0)
        if st != OK:
            raise RuntimeError(f"gevws_protocol_set_service: {status_string(st)}")

    def set_direct(self, on: bool) -> None:
        """gevws_protocol_set_direct: zero-copy passes without a handler step
        are written into the context's own AQL queue (no HIP launch call)."""
        st = lib.gevws_protocol_set_direct(self._p, 1 if on else 0)
        if st != OK:
            raise RuntimeError(f"gevws_protocol_set_direct: {status_string(st)}")

    def set_zero_copy_max(self, nbytes: int) -> None:
        """gevws_protocol_set_zero_copy_max: batched passes over at most
        `nbytes` of input run on mapped host memory with no copies (0 = never)."""
        lib.gevws_protocol_set_zero_copy_max(self._p, int(nbytes))

    def stats(self) -> dict:
        """Host-ingress counters (gevws_protocol_get_stats): device passes,
        connections and bytes staged, UnPacket calls answered by the host gate,
        passes run zero-copy."""
        s = _abi.ProtocolStats()
        lib.gevws_protocol_get_stats(self._p, ctypes.byref(s))
        return {k: int(getattr(s, k)) for k, _ in _abi.ProtocolStats._fields_}

    def timeline(self) -> dict:
        """Where the batched passes' time went (gevws_protocol_get_timeline):
        host ns per phase summed over the passes, and the one-launch kernels'
        GPU ns for passes answered by the completion flag."""
        t = _abi.ProtocolTimeline()
        lib.gevws_protocol_get_timeline(self._p, ctypes.byref(t))
        return {k: int(getattr(t, k)) for k, _ in _abi.ProtocolTimeline._fields_}

    def decode_host(self, segments: Sequence[Tuple[bytes, bytes]]):
        """gevws_decode_host_batch: [(first, end)] host segments per connection ->
        (frames, payload arena, conn_out, summary) as numpy arrays (the FFI form)."""
        n = len(segments)
        keep = []
        hc = (_abi.HostConn * max(n, 1))()
        total = 0
        for i, (a, b) in enumerate(segments):
            ba = np.frombuffer(a, np.uint8) if a else np.zeros(0, np.uint8)
            bb = np.frombuffer(b, np.uint8) if b else np.zeros(0, np.uint8)
            keep += [ba, bb]
            hc[i].seg0, hc[i].n0 = (ba.ctypes.data if ba.size else None), ba.size
            hc[i].seg1, hc[i].n1 = (bb.ctypes.data if bb.size else None), bb.size
            total += ba.size + bb.size
        max_frames = total // 2 + 1
        cap = total + 16 * max_frames + 16
        for _ in range(2):
            frames = np.zeros(max_frames, FRAME_DTYPE)
            payload = np.zeros(cap, np.uint8)
            cout = np.zeros(max(n, 1), CONN_OUT_DTYPE)
            s = _abi.Summary()
            r = lib.gevws_decode_host_batch(self._p, hc, n, frames.ctypes.data, max_frames, payload.ctypes.data,
                                            cap, cout.ctypes.data, ctypes.byref(s))
            if r == ERR_CAPACITY:
                max_frames, cap = max(s.frames, 1), max(s.payload_bytes, 16)
                continue
            if r < 0:
                raise RuntimeError(f"decode_host: {status_string(int(r))}")
            return frames[:s.frames], payload[:s.payload_bytes], cout[:n], s
        raise RuntimeError("decode_host: capacity retry failed")

    def packet(self, c: Connection, data: bytes) -> bytes:
        """Packet(c, data) -> data (protocol.go:67-69)."""
        return data


def handler_protocol(protocol: Protocol, c: Connection, buffer: RingBuffer,
                     on_message: Callable[[Connection, Optional[Header], bytes], Optional[bytes]]) -> List[bytes]:
    """Connection.handlerProtocol (connection.go:208-218): UnPacket until (nil, nil),
    handing each frame to on_message and collecting Packet'ed replies."""
    replies: List[bytes] = []
    ctx, data = protocol.unpacket(c, buffer)
    while ctx is not None or (data is not None and len(data) != 0):
        send = on_message(c, ctx, data)
        if send is not None:
            replies.append(protocol.packet(c, send))
        ctx, data = protocol.unpacket(c, buffer)
    return replies


__all__ = ["Engine", "Batch", "Comm", "RingBuffer", "Connection", "Protocol", "Header", "handler_protocol",
           "Upgrader", "RejectError", "HandshakeError", "HandshakeInfo", "accept_key", "HANDSHAKE", "ERR_HANDSHAKE",
           "status_string", "device_count", "lib", "FRAME_DTYPE", "CONN_OUT_DTYPE", "SUMMARY_DTYPE",
           "SYNTH_DTYPE", "OUT_FRAME_DTYPE", "OK", "NEED_MORE", "ERR_LEN_MSB", "ERR_CAPACITY", "ERR_INVALID", "ERR_DEVICE",
           "ERR_NOT_UPGRADED", "IN_PAD", "PAYLOAD_ALIGN", "TILE", "SUMMARY_UNORDERED",
           "DEFLATE_MSG_DTYPE", "DEFLATE_PLAIN_IF_NOT_SMALLER", "DEFLATE_DYNAMIC", "Deflated", "deflate_raw", "deflate_bound",
           "deflate_raw_ctx", "deflate_negotiate_takeover", "DEF_CTX_BYTES", "EXT_SERVER_TAKEOVER",
           "NEGOTIATE_SERVER_TAKEOVER", "Carry", "CARRY_DTYPE", "CARRY_OPEN", "CARRY_LOST",
           "CARRY_COMPRESSED", "CARRY_KEEP_COMPRESSED", "Rooms", "ROOM_NONE", "ROOMS_SKIP_SENDER",
           "ROOM_CHANGE_DTYPE", "RoomChanges", "room_command_parse", "MSG_COMMAND", "CHANGE_NONE", "CHANGE_REJECTED"]
