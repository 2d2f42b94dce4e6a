"""The room-command step's contract (gevws_room_commands_async, include/gevws.h)
restated in plain Python, and the command session built on tests/_session.py.

Three parts.  parse() is the rule on a body's bytes, independent of
gev_amd/csrc/gevws_room_command.hpp.  commands_model() / run_commands() are the
step on synthetic tables: what it must write, and the device call on host arrays
with every output prefilled with 0xEE.  command_traffic() / command_view() /
run_command_session() are a whole session in which membership moves only by what
clients send: the traffic, the client's view of it per pass with the room table
behind every pass, and the driver (Engine.broadcast(commands=True) and
Rooms.update(changes=res.room_changes, closed=res)).  No torch at import time."""
from __future__ import annotations

import functools
import zlib
from collections import Counter
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import gev_amd
from tests import _messages_model as mm
from tests import _rooms_model as ro
from tests import _session as s

ROOM_NONE = ro.ROOM_NONE
ERR_CAPACITY, ERR_INVALID = -2, -3
FILL = ro.FILL
NONE, CHANGE, REJECTED = 0, 1, 2          # parse's classes
OF_NONE, OF_REJECTED = -1, -2             # d_change_of
MSG_COMMAND = 10
WHOLE, JOINED, INFLATED = 1, 2, 4         # GEVWS_BODY_*
BODY_DTYPE = gev_amd.BODY_DTYPE
CHANGE_DTYPE = np.dtype([("conn", "<u4"), ("room", "<u4")])
SUMMARY_FIELDS = ("frames", "payload_bytes", "payload_len", "errors", "status")


# ---------------------------------------------------------------------------- the rule
def parse(body: bytes, n_rooms: int):
    """(class, room) of a delivered text message of these bytes."""
    body = bytes(body)
    if not 6 <= len(body) <= 16:
        return NONE, ROOM_NONE
    if body == b"/leave":
        return CHANGE, ROOM_NONE
    digits = body[6:]
    if body[:6] != b"/join " or not digits or any(not 0x30 <= b <= 0x39 for b in digits):
        return NONE, ROOM_NONE
    value = int(digits.decode("ascii"))
    return (CHANGE, value) if value < n_rooms else (REJECTED, ROOM_NONE)


# ---------------------------------------------------------------------------- the step on tables
def zero_summary() -> dict:
    return dict(frames=0, payload_bytes=0, payload_len=0, errors=0, status=0)


def commands_model(bodies, out, src_bytes, n_conns, n_rooms, max_messages=None, max_changes=None, msg=None,
                   join_status=0, ctl_status=None):
    """What the call must produce: dict(summary, changes, change_of, bodies);
    the three tables are None where nothing may be written (bodies: where
    d_bodies must stay byte for byte).  msg: the message pass's summary as a dict
    (frames, status), None: every body, status OK."""
    bodies = np.asarray(bodies, BODY_DTYPE).reshape(-1)
    out = np.asarray(out, np.uint8).reshape(-1)
    nothing = dict(changes=None, change_of=None, bodies=None)
    if max_messages is None:
        max_messages = bodies.size
    n = max_messages
    if msg is not None:
        n = min(n, int(msg["frames"])) if int(msg["status"]) == 0 else 0
    if join_status != 0 or (ctl_status is not None and ctl_status != 0) or n == 0:
        return dict(nothing, summary=zero_summary())
    b = bodies[:n]
    fl = b["flags"].astype(np.int64)
    delivered = fl & WHOLE != 0
    bad = delivered & ((fl & (JOINED | INFLATED) == 0) | (b["conn"].astype(np.int64) >= n_conns))
    looked = delivered & ~bad & (b["opcode"] == 1) & (b["length"] >= 6) & (b["length"] <= 16)
    off, length = b["off"].astype(object), b["length"].astype(object)       # (no 64-bit wrap in the model)
    cls = np.zeros(n, np.int64)
    room = np.full(n, ROOM_NONE, np.int64)
    seen = {}
    for m in np.flatnonzero(looked).tolist():
        o, k = int(off[m]), int(length[m])
        if o % 16 or o + k > src_bytes:
            bad[m] = True
            continue
        key = out[o: o + k].tobytes()
        if key not in seen:
            seen[key] = parse(key, n_rooms)
        cls[m], room[m] = seen[key]
    if bad.any():
        return dict(nothing, summary=dict(zero_summary(), errors=int(bad.sum()), status=ERR_INVALID))
    is_change = cls == CHANGE
    need = int(is_change.sum())
    if max_changes is None:
        max_changes = need
    if need > max_changes:
        return dict(nothing, summary=dict(zero_summary(), frames=need, status=ERR_CAPACITY))
    changes = np.zeros(need, CHANGE_DTYPE)
    changes["conn"] = b["conn"][is_change]
    changes["room"] = room[is_change].astype(np.uint32)
    change_of = np.full(n, OF_NONE, np.int64)
    change_of[is_change] = np.arange(need)
    change_of[cls == REJECTED] = OF_REJECTED
    new = bodies.copy()
    strip = np.flatnonzero(cls != NONE)
    new["off"][strip] = 0
    new["length"][strip] = 0
    new["flags"][strip] = 0
    new["status"][strip] = MSG_COMMAND
    summary = dict(zero_summary(), frames=need, payload_len=int(strip.size), payload_bytes=int((cls == REJECTED).sum()))
    return dict(summary=summary, changes=changes, change_of=change_of, bodies=new)


def summary_np(frames=0, status=0) -> np.ndarray:
    sm = np.zeros(1, mm.SUMMARY_DTYPE)
    sm["frames"], sm["status"] = frames, status
    return sm


def run_commands(engine, bodies, out, src_bytes, n_conns, n_rooms, max_messages=None, max_changes=None, msg=None,
                 join_status=0, ctl_status=None):
    """gevws_room_commands_async on host arrays: host copies of everything it
    may write -- d_changes, d_change_of and the summary prefilled with FILL, and
    d_bodies after the call.  out is uploaded into an allocation that ends with
    its last aligned vector."""
    import torch
    dev = torch.device("cuda", engine.device)
    bodies = np.ascontiguousarray(np.asarray(bodies, BODY_DTYPE).reshape(-1))
    out = np.asarray(out, np.uint8).reshape(-1)
    if max_messages is None:
        max_messages = bodies.size
    if max_changes is None:
        max_changes = max_messages
    padded = np.zeros((out.size + 15) // 16 * 16, np.uint8)
    padded[: out.size] = out
    d_bodies = mm._dev(bodies, dev, 32)
    d_out = mm._dev(padded, dev, 16)
    frames = bodies.size if msg is None else int(msg["frames"])
    d_msg = mm._dev(summary_np(frames, 0 if msg is None else int(msg["status"])), dev, 64)
    d_join = mm._dev(summary_np(0, join_status), dev, 64)
    d_ctl = None if ctl_status is None else mm._dev(summary_np(0, ctl_status), dev, 64)
    f = lambda nbytes: torch.full((max(nbytes, 8),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    changes, change_of, summ = f(max_changes * 8), f(max_messages * 8), f(64)
    engine.room_commands_async(d_bodies, max_messages, d_msg, d_join, d_ctl, d_out, src_bytes, n_conns, n_rooms, 0,
                               changes, max_changes, change_of, summ)
    torch.cuda.synchronize(engine.device)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(changes=h(changes), change_of=h(change_of), summary=h(summ).view(mm.SUMMARY_DTYPE)[0],
                bodies=h(d_bodies)[: bodies.size * 32], out=h(d_out)[: padded.size], out_in=padded)


def assert_commands(got: dict, want: dict, bodies, tag="") -> None:
    """Device == model on every output byte: the summary, the changes,
    d_change_of and d_bodies; what is not an output entry is still FILL; d_out
    is unchanged."""
    sm, w = got["summary"], want["summary"]
    have = tuple(int(sm[k]) for k in SUMMARY_FIELDS)
    assert have == tuple(int(w[k]) for k in SUMMARY_FIELDS), (tag, "summary", have, w)
    assert int(sm["flags"]) == 0 and int(sm["run_frames"]) == 0 and not sm["reserved"].any(), (tag, "summary tail")
    assert np.array_equal(got["out"], got["out_in"]), (tag, "d_out written")
    before = np.ascontiguousarray(np.asarray(bodies, BODY_DTYPE).reshape(-1)).view(np.uint8)
    if want["changes"] is None:
        assert np.all(got["changes"] == FILL) and np.all(got["change_of"] == FILL), (tag, "written by a call that wrote nothing")
        assert np.array_equal(got["bodies"], before), (tag, "d_bodies written by a call that wrote nothing")
        return
    for k in ("changes", "change_of"):
        w8 = np.ascontiguousarray(want[k]).view(np.uint8)
        g8 = got[k]
        assert np.array_equal(g8[: w8.size], w8), (tag, k)
        assert np.all(g8[w8.size:] == FILL), (tag, k, "written behind its end")
    w8 = np.ascontiguousarray(want["bodies"]).view(np.uint8)
    if not np.array_equal(got["bodies"], w8):
        m = int(np.flatnonzero(got["bodies"] != w8)[0]) // 32
        raise AssertionError((tag, "d_bodies", m, got["bodies"].view(BODY_DTYPE)[m], want["bodies"][m]))


# ---------------------------------------------------------------------------- synthetic batches
SLOT = 32   # bytes of d_out a synthetic body owns: its vector and a pad


def batch_of(entries, conns, n_conns=None):
    """A batch from per-body (bytes, length, opcode, flags, status): body m's
    bytes at off 32 m of d_out (the bytes may be longer than `length`: the pad),
    conn from `conns`.  An undelivered body (flags 0) gets off = length = 0."""
    n = len(entries)
    bodies = np.zeros(n, BODY_DTYPE)
    out = np.zeros(n * SLOT, np.uint8)
    for m, (data, length, opcode, flags, status) in enumerate(entries):
        out[m * SLOT: m * SLOT + len(data)] = np.frombuffer(bytes(data), np.uint8)
        if flags & WHOLE:
            bodies[m]["off"], bodies[m]["length"] = m * SLOT, length
        bodies[m]["opcode"], bodies[m]["flags"], bodies[m]["status"] = opcode, flags, status
    bodies["conn"] = conns
    bodies["reserved"] = 0xC3          # a strip keeps what it does not name
    return bodies, out


def batch_from_palette(pal, idx, conns):
    """batch_of for body m = pal[idx[m]] (palette()'s entries), without a loop over the bodies."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    mat = np.zeros((len(pal), SLOT), np.uint8)
    for k, e in enumerate(pal):
        mat[k, : len(e[1])] = np.frombuffer(e[1], np.uint8)
    col = lambda j, dt: np.array([e[j] for e in pal], dt)[idx] if idx.size else np.zeros(0, dt)  # noqa: E731
    flags = col(4, np.uint8)
    delivered = flags & WHOLE != 0
    bodies = np.zeros(idx.size, BODY_DTYPE)
    bodies["off"] = np.where(delivered, np.arange(idx.size, dtype=np.uint64) * SLOT, 0)
    bodies["length"] = np.where(delivered, col(2, np.uint64), 0)
    bodies["opcode"], bodies["flags"], bodies["status"] = col(3, np.uint8), flags, col(5, np.uint8)
    bodies["conn"] = conns
    bodies["reserved"] = 0xC3
    return bodies, (mat[idx].reshape(-1) if idx.size else np.zeros(0, np.uint8))


def palette(n_rooms: int):
    """Bodies of every class: (name, bytes with pad, length, opcode, flags, status)."""
    J, I = WHOLE | JOINED, WHOLE | INFLATED
    big = str(n_rooms - 1).encode()
    p = [
        ("join", b"/join 0", 7, 1, J, 0), ("join the last room", b"/join " + big, 6 + len(big), 1, J, 0),
        ("join, leading zeros", b"/join 000000000" + big[-1:], 16, 1, J, 0),
        ("join, inflated", b"/join 1", 7, 1, I, 0), ("leave", b"/leave", 6, 1, J, 0),
        ("leave, inflated", b"/leave", 6, 1, I, 0),
        ("join, digits in the pad", b"/join 1" + b"234567890123", 7, 1, J, 0),
        ("leave, digits in the pad", b"/leave" + b"0123456789", 6, 1, J, 0),
        ("rejected: n_rooms", b"/join " + str(n_rooms).encode(), 6 + len(str(n_rooms)), 1, J, 0),
        ("rejected: 2^32 - 1", b"/join 4294967295", 16, 1, J, 0), ("rejected: 2^32", b"/join 4294967296", 16, 1, J, 0),
        ("rejected: ten nines", b"/join 9999999999", 16, 1, I, 0),
        ("near: no digits", b"/join ", 6, 1, J, 0), ("near: a newline", b"/join 3\n", 8, 1, J, 0),
        ("near: upper case", b"/JOIN 3", 7, 1, J, 0), ("near: leave and a space", b"/leave ", 7, 1, J, 0),
        ("near: eleven digits", b"/join 00000000001", 17, 1, J, 0), ("near: /join", b"/join", 5, 1, J, 0),
        ("near: a sign", b"/join +1", 8, 1, J, 0), ("near: two spaces", b"/join  1", 8, 1, J, 0),
        ("near: the digit is in the pad", b"/join 1", 6, 1, J, 0), ("near: leave cut short", b"/leave", 5, 1, J, 0),
        ("binary join", b"/join 1", 7, 2, J, 0), ("binary leave", b"/leave", 6, 2, I, 0),
        ("undelivered", b"/join 1", 7, 1, 0, 0), ("undelivered: utf-8", b"/leave", 6, 1, 0, 6),
        ("closed", b"/join 1", 7, 1, 0, 9), ("empty", b"", 0, 1, J, 0), ("empty, inflated", b"", 0, 2, I, 0),
        ("text", b"hello, room", 11, 1, J, 0), ("long text", b"x" * 30, 30, 1, J, 0),
    ]
    return p


# ---------------------------------------------------------------------------- the command session
N_ROOMS = 7
SEED = 0x5EC0DE
# binary messages of a command's bytes are broadcast; no text message of the session spells a room this way
BINARY_LOOKALIKES = (b"/join 02", b"/join 002")


@dataclass
class CommandCase:
    conns: List[s.Conn]
    cuts: list
    passes: int
    n_rooms: int
    rooms0: np.ndarray


def message_frames(conn: s.Conn, i: int) -> List[int]:
    """The data frames of the message whose FIN frame is frame i."""
    out = [i]
    while conn.frames[out[0]].header.opcode == s.C:
        j = out[0] - 1
        while conn.frames[j].header.opcode & 8:
            j -= 1
        out.insert(0, j)
    return out


def command_traffic(seed: int = SEED, n_conns: int = 300, n_rooms: int = N_ROOMS, passes: int = 4) -> CommandCase:
    """The broadcast session's shape (s.broadcast_traffic) with clients that
    send commands: random ones on every kind of connection, and scripted
    connections, each named by what it is for, whose marks fix their cuts."""
    rng = np.random.default_rng(seed)
    classes = ((0, 0), (s.D, 0), (s.D, 0), (s.D | s.ST, 12), (s.D | s.CT, 0))
    T, PING, PONG = s.T, s.PING, s.PONG
    scripts = {}

    def script(name, ext, room):
        b = s.Builder(rng, ext, 0, heavy="cmd: " + name)
        scripts[name] = (b, room)
        return b

    here = lambda b: b.mark().mark().mark()      # noqa: E731  everything so far in pass 0, the rest in the last pass
    # a join out of no room; what it sends in the same pass goes nowhere, in the next pass to room 3
    script("join, then publish", 0, ROOM_NONE).message(b"/join 3", T).message(b"to nobody yet", T).mark().message(
        b"hello room 3", T).mark().mark().message(b"still in room 3", T)
    script("move", s.D, 1).message(b"/join 2", T).message(b"to the old room 1", T).mark().message(
        b"to the new room 2", T).mark().mark()
    script("leave", 0, 4).message(b"to room 4", T).message(b"/leave", T).mark().message(b"to nobody", T).mark().mark()
    script("rejected", 0, 5).message(b"/join 7", T).message(b"/join 4294967295", T).message(
        b"/join 99999999999", T).mark().message(b"still in room 5", T).mark().mark()
    script("1-byte fragments", 0, ROOM_NONE).message(b"/join 6", T, [1, 2, 3, 4, 5, 6], between=[(PING, b"in it")]
                                                      ).mark().message(b"in room 6 now", T).mark().mark()
    script("cut between fragments", 0, 0).frame(b"/joi", T, False).mark().frame(b"n 1", s.C, True).mark().message(
        b"in room 1 now", T).mark()
    script("cut inside a frame", s.D, 2).message(b"/leave", T, compress=False).mark(3).message(b"a last word", T
                                                                                                  ).mark().mark()
    script("compressed", s.D, ROOM_NONE).message(b"/join 5", T, compress=True).mark().message(
        b"compressed, in room 5", T, compress=True).mark().mark()
    script("compressed, client takeover", s.D | s.CT, 3).message(b"/join 4", T, compress=True).message(
        b"/join 4", T, 3, compress=True).mark().message(b"/leave", T, compress=True).mark().mark()
    script("near misses", 0, 6).message(b"/join 3\n", T).message(b"/JOIN 3", T).message(b"/leave ", T).message(
        b"/join", T).message(b"/join ", T).message(BINARY_LOOKALIKES[0], s.B).message(BINARY_LOOKALIKES[1], s.B).mark(
        ).mark().mark()
    here(script("behind a close", 0, 2).message(b"bye", T).close(1000, b"bye").message(b"/join 4", T))
    here(script("in front of a close", s.D, 1).message(b"/join 3", T).close(1000))
    here(script("two commands disagree", 0, 0).message(b"/join 1", T).message(b"between", T).message(b"/join 2", T))
    here(script("join, then leave", 0, ROOM_NONE).message(b"/join 4", T).message(b"/leave", T))
    slots = sorted(int(x) for x in rng.choice(n_conns - 1, len(scripts) - 1, replace=False)) + [n_conns - 1]
    at = dict(zip(slots, scripts))
    free = [c for c in range(n_conns) if c not in at]
    closers = set(int(x) for x in rng.choice(free, 3, replace=False))
    big = set(int(x) for x in rng.choice([c for c in free if c not in closers], 2, replace=False))
    rooms0 = rng.integers(0, n_rooms, n_conns).astype(np.uint32)
    rooms0[rng.choice(n_conns, 25, replace=False)] = ROOM_NONE
    for c in closers | big:
        rooms0[c] = c % n_rooms
    conns = []
    for c in range(n_conns):
        if c in at:
            b, rooms0[c] = scripts[at[c]]
            conns.append(b.done())
            continue
        b = s.Builder(rng, *classes[int(rng.integers(0, len(classes)))])
        for _ in range(int(rng.integers(0, 4))):
            k = rng.random()
            if k < 0.25:        # a command: a room (two of them out of range), or a leave
                g = int(rng.integers(0, n_rooms + 3))
                data = b"/leave" if g == n_rooms + 2 else b"/join %d" % g
                frags = 1 + int(rng.random() < 0.3)
            else:
                data = s.text_of(rng, int(rng.integers(0, 120)), 0.3)
                frags = 1 + int(rng.random() < 0.3)
            b.message(data, T, frags, compress=bool(b.c.ext & s.D) and rng.random() < 0.6,
                      between=[(PING, b"pi")] if rng.random() < 0.2 else [])
            if rng.random() < 0.15:
                b.ctl(PONG if rng.random() < 0.3 else PING, b"between messages")
        if c in big:
            b.message(s.text_of(rng, 40000, 0.5), T, 4, between=[(PING, b"in the big one")])
        if c in closers:
            b.c.heavy = "closes"
            if c == min(closers):
                b.message(b"ok \xff not", T).message(b"/join 1", T)
            else:
                b.message(b"/join %d" % ((c + 1) % n_rooms), T).close(1000, b"bye").message(b"/leave", T)
            for _ in range(3):      # a long tail nobody reads
                b.message(s.text_of(rng, 1500), T)
        conns.append(b.done())
    cuts, _ = s.make_cuts(conns, passes, seed ^ 0x5A5A)
    return CommandCase(conns, cuts, passes, n_rooms, rooms0)


@functools.lru_cache(maxsize=None)
def command_case() -> CommandCase:
    return command_traffic()


def as_broadcast(case: CommandCase) -> s.BroadcastCase:
    """The same traffic for a server without the command step: no change record at all."""
    return s.BroadcastCase(case.conns, case.cuts, case.passes, case.n_rooms, case.rooms0,
                           [np.zeros((0, 2), np.int64)] * case.passes)


def command_view(case: CommandCase, flags: int):
    """s.broadcast_view for a server with the command step, from the contract
    in include/gevws.h: per pass and recipient the expected replies, the room
    table behind every pass, and a tally of the cases the traffic holds.

    A delivered text message that parse() takes for a command is sent to nobody;
    its change is applied behind the pass, in message order (by connection, then
    stream order), and a connection the pass shut down ends in no room."""
    n = len(case.conns)
    room = case.rooms0.copy()
    alive = [True] * n
    ends = [s.pass_ends(case.cuts[c], case.passes, len(case.conns[c].wire)) for c in range(n)]
    views, tables, tally = [], [], Counter()
    joined_before = {}
    for p in range(case.passes):
        mine: List[List] = [[] for _ in range(n)]
        changes = []
        for c, conn in enumerate(case.conns):
            if not alive[c]:
                continue
            lo = conn.fed_frames(ends[c][p - 1]) if p else 0
            hi = conn.fed_frames(ends[c][p])
            dies = conn.dead_at is not None and hi > conn.dead_at
            own = []
            for i, k, x in conn.items:
                if not lo <= i < hi:
                    continue
                if k != "echo":
                    mine[c].append((k, x))
                    continue
                fr = message_frames(conn, i)
                text = conn.frames[fr[0]].header.opcode == s.T
                cls, g = parse(x, case.n_rooms) if text else (NONE, ROOM_NONE)
                if cls == NONE:
                    mine[c].append((k, x))
                    if x[:5].lower() in (b"/join", b"/leav"):
                        tally["a near-miss that is broadcast"] += 1
                    if c in joined_before and joined_before[c] == p - 1 and room[c] != ROOM_NONE and (
                            np.count_nonzero(room == room[c]) > 1):
                        tally["joins, then publishes in the next pass"] += 1
                    continue
                # a command: stripped, never sent
                tally["commands"] += 1
                if cls == REJECTED:
                    tally["a rejected join"] += 1
                else:
                    own.append(g)
                    changes.append((c, g))
                if len(fr) >= len(x) and all(conn.frames[j].header.length == 1 for j in fr):
                    tally["split into 1-byte fragments"] += 1
                if p and conn.frames[fr[0]].stream_pos < ends[c][p - 1]:
                    tally["cut across two passes"] += 1
                if conn.info[i][1]:
                    tally["compressed"] += 1
                if dies:
                    tally["in front of a close in the same pass"] += 1
            if len(set(own)) > 1:
                tally["two commands in one pass disagree"] += 1
            if dies:    # what lies behind the cut and was fed with it: the control step stripped it
                for j in range(conn.dead_at + 1, len(conn.frames)):
                    f = conn.frames[j]
                    if conn.frame_end(j) <= ends[c][p] and f.header.fin and f.header.opcode == s.T and not f.header.rsv \
                            and parse(f.payload, case.n_rooms)[0] != NONE:
                        tally["behind a close in the same pass"] += 1
        view: List[List] = [[] for _ in range(n)]
        for r in range(n):
            if not alive[r]:
                continue
            if room[r] != ROOM_NONE:
                for sender in np.flatnonzero(room == room[r]):
                    if flags & s.SKIP_SENDER and sender == r:
                        continue
                    view[r] += [(k, x) for k, x in mine[int(sender)] if k == "echo"]
            view[r] += [(k, x) for k, x in mine[r] if k != "echo"]
        views.append(view)
        for c, g in changes:
            old = int(room[c])
            if g == ROOM_NONE:
                tally["a leave"] += 1
            elif old == ROOM_NONE:
                tally["a join"] += 1
            elif old != g:
                tally["a move"] += 1
            room[c] = g
            if g != ROOM_NONE:
                joined_before[c] = p
        for c, conn in enumerate(case.conns):
            if alive[c] and conn.dead_at is not None and conn.fed_frames(ends[c][p]) > conn.dead_at:
                alive[c] = False
            if not alive[c]:
                room[c] = ROOM_NONE
        tables.append(room.copy())
    return views, tables, tally


COVERAGE = ("a join", "a move", "a leave", "a rejected join", "split into 1-byte fragments", "cut across two passes",
            "compressed", "a near-miss that is broadcast", "behind a close in the same pass",
            "in front of a close in the same pass", "two commands in one pass disagree",
            "joins, then publishes in the next pass")


def received_messages(conn: s.Conn, wire: bytes, F: Optional[int]) -> List[bytes]:
    """The data messages in what a recipient was sent in one pass, inflated."""
    deflate = bool(conn.ext & s.D)
    out = []
    for r in s.replies_of(s.parse_wire(bytes(wire)), F, deflate):
        if r[0] != "msg":
            continue
        data = b"".join(r[2])
        out.append(zlib.decompressobj(-15).decompress(data + s.TAIL) if r[1] == s.RSV1 else data)
    return out


def check_command_session(case: CommandCase, views, sent, F: Optional[int], tally: Optional[Counter] = None) -> None:
    """sent[p][r] against the view, and no command text among what anyone
    received (the binary look-alikes are no commands and do arrive)."""
    bc = as_broadcast(case)
    for r in range(len(case.conns)):
        s.check_broadcast_conn(bc, views, r, [sent[p][r] for p in range(case.passes)], F, tally)
        for p in range(case.passes):
            for data in received_messages(case.conns[r], sent[p][r], F):
                if parse(data, case.n_rooms)[0] != NONE and data not in BINARY_LOOKALIKES:
                    raise s.CheckError("pass %d, recipient %d was sent the command %r" % (p, r, data))


def reference_command_server(case: CommandCase, flags: int, F: Optional[int]):
    """sent[p][r]: the bytes a correct host server with the command rule sends recipient r in pass p."""
    views, _, _ = command_view(case, flags)
    return [[b"".join(s.encode_replies(v, F, s.takes_deflate_broadcast(case.conns[r].ext))) for r, v in enumerate(view)]
            for view in views]


def run_command_session(engine, case: CommandCase, F: Optional[int] = None, rooms_flags: int = 0,
                        commands: bool = True) -> s.SessionRun:
    """s.run_session's broadcast wiring with the command step: decode ->
    messages -> inflate -> join(carry) -> broadcast(commands=True), gathered,
    and Rooms.update(changes=res.room_changes, closed=res) between the passes.
    run.changes[p]: the pass's change records as the device wrote them.
    commands=False: today's broadcast, no change record at all."""
    import torch

    from tests._helpers import gpu_decode, pack_streams
    dev = torch.device("cuda", engine.device)
    conns, cuts, passes = case.conns, case.cuts, case.passes
    n = len(conns)
    ext = mm._dev(np.array([c.ext for c in conns], np.uint8), dev, 1)
    wb = mm._dev(np.array([c.window_bits for c in conns], np.uint8), dev, 1)
    state = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
    inf_ctx = torch.zeros((n, gev_amd.INF_CTX_BYTES), dtype=torch.uint8, device=dev)
    carry = gev_amd.Carry(engine, n, s.LIMIT, compressed=True)
    rooms = gev_amd.Rooms.build(engine, case.rooms0, case.n_rooms)
    ends = [s.pass_ends(cuts[c], passes, len(conns[c].wire)) for c in range(n)]
    run = s.SessionRun(consumed=[0] * n, leftover=[b""] * n, cuts=cuts)
    run.changes, run.bodies = [], []
    pos = [0] * n
    for p in range(passes):
        bufs = []
        for c in range(n):
            if c in run.shutdown_pass:
                bufs.append(b"")
                continue
            bufs.append(run.leftover[c] + conns[c].wire[pos[c]: ends[c][p]])
            pos[c] = ends[c][p]
        batch = gpu_decode(engine, *pack_streams(bufs), aux_slots=n)
        co = batch.conn_out_host()
        assert not (co["status"] < 0).any()
        for c in range(n):
            if c not in run.shutdown_pass:
                k = int(co["consumed"][c])
                run.consumed[c] += k
                run.leftover[c] = bufs[c][k:]
        msgs = engine.messages(batch, state, conn_ext=ext)
        inf = engine.inflate(batch, msgs, s.LIMIT, state, conn_ext=ext, contexts=inf_ctx, carry=carry)
        bodies = engine.join(batch, msgs, inf, flags=gev_amd.JOIN_ALL, carry=carry)
        res = engine.broadcast(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, ext, rooms, window_bits=wb,
                               rooms_flags=rooms_flags, gather=True, max_fragment_bytes=F, commands=commands)
        if commands:
            run.changes.append(res.room_changes.host().copy())
            rooms = rooms.update(engine, changes=res.room_changes, closed=res)
        else:
            assert res.room_changes is None
            rooms = rooms.update(engine, closed=res)
        run.bodies.append(bodies.bodies_host().copy())
        run.room_tables.append(rooms.host())
        sent = s.all_conn_bytes(res)
        run.sent.append(sent)
        run.gathered.append([bytes(m) for m in res.host_sends()])
        for c in np.flatnonzero(res.conn_send_host()["flags"] & gev_amd.CTL_SHUTDOWN):
            run.shutdown_pass.setdefault(int(c), p)
    return run
