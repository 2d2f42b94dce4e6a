"""The room broadcast's contracts (gevws_reply_rooms_async,
gevws_room_plan_async; include/gevws.h) restated in plain Python over the tables
of tests/_join_model.py and tests/_respond_model.py, and the helpers that run
both device steps on hand-built tables.

The model is pinned on the CPU (tests/test_rooms_model.py) by hand-written
expectations; the GPU tests compare every output of the device with it, byte for
byte."""
from __future__ import annotations

import numpy as np

from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm

ROOM_NONE = 0xFFFFFFFF
SKIP_SENDER = 1
EXT_DEFLATE, EXT_SERVER_TAKEOVER = 1, 4
ERR_CAPACITY, ERR_INVALID = rm.ERR_CAPACITY, rm.ERR_INVALID
FILL = jm.FILL
zero_summary = rm.zero_summary


def csr_of(conn_room, n_rooms=None):
    """(conn_room, first, members) as uint32 arrays: the CSR by a stable argsort."""
    cr = np.asarray(conn_room, np.uint32)
    has = np.flatnonzero(cr != ROOM_NONE)
    if n_rooms is None:
        n_rooms = int(cr[has].max()) + 1 if has.size else 0
    members = has[np.argsort(cr[has], kind="stable")].astype(np.uint32)
    first = np.zeros(n_rooms + 1, np.uint32)
    first[1:] = np.cumsum(np.bincount(cr[has], minlength=n_rooms))[:n_rooms]
    return cr, first, members


def takes_deflate(conn_ext, c: int) -> bool:
    if conn_ext is None:
        return False
    e = int(conn_ext[c])
    return bool(e & EXT_DEFLATE) and not e & EXT_SERVER_TAKEOVER


def _slot_room(first, i: int) -> int:
    """The room a lane finds for member slot i: the last room that starts at or
    before i, by the bisection the device runs (defined for any table)."""
    lo, hi = 0, len(first) - 2
    while lo < hi:
        mid = lo + ((hi - lo + 1) >> 1)
        if int(first[mid]) <= i:
            lo = mid
        else:
            hi = mid - 1
    return lo


def check_tables(rooms, n_conns: int, conn_ext=None, window_bits=None, windows=False) -> int:
    """The number of bad records: the n_rooms + 1 entries of `first`, the member
    slots, the connections, and one more for a wrong number of roomed
    connections.  windows: a deflate-taking member's window byte outside
    {0, 8..15} makes its slot bad (the reply step)."""
    cr, first, members = rooms
    n_rooms, n_members = len(first) - 1, len(members)
    bad = 0
    for i in range(n_rooms + 1):
        b = i == 0 and int(first[0]) != 0
        if i < n_rooms:
            b |= int(first[i]) > int(first[i + 1])
        else:
            b |= int(first[i]) != n_members or n_members > n_conns
        bad += bool(b)
    for i in range(n_members):
        if n_rooms == 0:
            bad += 1
            continue
        g = _slot_room(first, i)
        a, e = int(first[g]), int(first[g + 1])
        m = int(members[i])
        b = not a <= i < e
        if m >= n_conns:
            b = True
        else:
            b |= int(cr[m]) != g
            if windows and takes_deflate(conn_ext, m) and window_bits is not None:
                b |= int(window_bits[m]) not in (0, 8, 9, 10, 11, 12, 13, 14, 15)
        if a < i:
            b |= int(members[i - 1]) >= m
        bad += bool(b)
    roomed = 0
    for c in range(n_conns):
        g = int(cr[c])
        roomed += g != ROOM_NONE
        bad += g != ROOM_NONE and g >= n_rooms
    return bad + (roomed != n_members)


def members_of(rooms, g: int):
    _, first, members = rooms
    return [int(x) for x in members[int(first[g]): int(first[g + 1])]]


def reply_rooms_model(bodies, policy, conn_ext, window_bits, n_conns, rooms, flags=0, msg_status=0, join_status=0):
    """What gevws_reply_rooms_async must produce: dict(def_msgs, def_conn,
    plain, plain_conn, plain_of, def_of, def_summary, plain_summary); the lists
    are None where nothing may be written."""
    n = bodies.shape[0] if msg_status == 0 and join_status == 0 else 0
    nothing = dict(def_msgs=None, def_conn=None, plain=None, plain_conn=None, plain_of=None, def_of=None)
    if n == 0:
        return dict(nothing, def_summary=zero_summary(), plain_summary=zero_summary())
    cr, first, members = rooms
    n_rooms = len(first) - 1
    plain_of, def_of = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    dmsgs, dconn, plain, pconn = [], [], [], []
    op = 1 if policy == jm.HANDLER_ECHO_TEXT else 2
    bad = check_tables(rooms, n_conns, conn_ext, window_bits, True) if policy != jm.HANDLER_NONE else 0
    for m in range(n if policy != jm.HANDLER_NONE else 0):
        b = bodies[m]
        fl, c = int(b["flags"]), int(b["conn"])
        if not fl & jm.WHOLE:
            continue
        if not fl & (jm.JOINED | jm.INFLATED) or c >= n_conns:
            bad += 1
            continue
        if bad:
            continue
        g = int(cr[c])
        if g >= n_rooms:
            continue
        recips = [r for r in members_of(rooms, g) if not (flags & SKIP_SENDER and r == c)]
        if any(not takes_deflate(conn_ext, r) for r in recips):
            plain_of[m] = len(plain)
            plain.append((int(b["off"]), int(b["length"])))
            pconn.append(c)
        if any(takes_deflate(conn_ext, r) for r in recips):
            wb = min(int(window_bits[r]) or 15 if window_bits is not None else 15
                     for r in members_of(rooms, g) if takes_deflate(conn_ext, r))
            def_of[m] = len(dmsgs)
            dmsgs.append((int(b["off"]), int(b["length"]), op, wb))
            dconn.append(c)
    if bad:
        s = dict(zero_summary(), errors=bad, status=ERR_INVALID)
        return dict(nothing, def_summary=s, plain_summary=dict(s))
    dm = np.zeros(len(dmsgs), jm.DEFLATE_MSG_DTYPE)
    for k, (off, length, o, wb) in enumerate(dmsgs):
        dm[k]["payload_off"], dm[k]["length"], dm[k]["opcode"], dm[k]["window_bits"] = off, length, o, wb
    pl = np.zeros(len(plain), jm.OUT_FRAME_DTYPE)
    for k, (off, length) in enumerate(plain):
        pl[k]["fin"], pl[k]["opcode"], pl[k]["length"] = 1, op, length
        pl[k]["payload_off"], pl[k]["payload_len"] = off, length
    return dict(def_msgs=dm, def_conn=np.array(dconn, np.uint32), plain=pl, plain_conn=np.array(pconn, np.uint32),
                plain_of=plain_of, def_of=def_of, def_summary=dict(zero_summary(), frames=len(dmsgs)),
                plain_summary=dict(zero_summary(), frames=len(plain)))


def room_plan_model(n_decoded, conn_out, msg_of, msg_end, plain_of, def_of, n_messages, conn_ext, ctl_of, conn_ctl,
                    wires, rooms, flags=0, max_sends=None, gate_ok=True):
    """What gevws_room_plan_async must produce: dict(send, conn_send, summary).
    wires: three (offset table, count, wire total), plain / deflated / control;
    gate_ok False: one of the input summaries failed.  max_sends None: enough."""
    n_conns = conn_out.shape[0]
    if not gate_ok or n_decoded == 0 or n_conns == 0:
        return dict(send=None, conn_send=None, summary=zero_summary())
    n = n_decoded
    cr, first, members = rooms
    n_rooms = len(first) - 1
    bad = check_tables(rooms, n_conns)

    def rng(wire, idx):
        tab, cnt, total = wires[wire]
        if idx >= cnt:
            return None
        off = int(tab[idx])
        nxt = int(tab[idx + 1]) if idx + 1 < cnt else total
        return None if nxt < off else (off, nxt - off)

    pubs = {}   # (room, wire) -> [(frame, off, len, sender)]
    ctls = {}   # connection -> [(frame, off, len)]
    owned = np.zeros(n, bool)
    for c in range(n_conns):
        lo = min(int(conn_out["first_frame"][c]), n)
        hi = min(lo + int(conn_out["nframes"][c]), n)
        owned[lo:hi] = True
    for f in np.flatnonzero(~owned):   # a frame of no connection that would send something
        m = int(msg_of[f])
        if int(ctl_of[f]) >= 0:
            bad += 1
        elif m >= 0:
            bad += m >= n_messages or (int(msg_end[m]) == f and (int(plain_of[m]) >= 0 or int(def_of[m]) >= 0))
    for c in range(n_conns):
        lo = min(int(conn_out["first_frame"][c]), n)
        hi = min(lo + int(conn_out["nframes"][c]), n)
        g = int(cr[c])
        for f in range(lo, hi):
            k = int(ctl_of[f])
            if k >= 0:
                r = rng(2, k)
                if r is None:
                    bad += 1
                else:
                    ctls.setdefault(c, []).append((f, *r))
                continue
            m = int(msg_of[f])
            if m < 0:
                continue
            if m >= n_messages:
                bad += 1
                continue
            if int(msg_end[m]) != f or g >= n_rooms:
                continue
            ok = True
            for wire, idx in ((0, int(plain_of[m])), (1, int(def_of[m]))):
                if idx < 0:
                    continue
                r = rng(wire, idx)
                if r is None:
                    ok = False
                else:
                    pubs.setdefault((g, wire), []).append((f, *r, c))
            bad += not ok
    if bad:
        return dict(send=None, conn_send=None, summary=dict(zero_summary(), errors=bad, status=ERR_INVALID))
    entries, conn_send = [], np.zeros(n_conns, rm.CONN_SEND_DTYPE)
    for r in range(n_conns):
        start, nbytes = len(entries), 0
        g = int(cr[r])
        if g < n_rooms:
            wire = 1 if takes_deflate(conn_ext, r) else 0
            for f, off, ln, sender in sorted(pubs.get((g, wire), [])):
                if flags & SKIP_SENDER and sender == r:
                    continue
                entries.append((off, ln, f, r, wire))
                nbytes += ln
        for f, off, ln in ctls.get(r, []):
            entries.append((off, ln, f, r, 2))
            nbytes += ln
        conn_send[r] = (start, len(entries) - start, nbytes, conn_ctl["flags"][r], 0)
    shut = int(np.count_nonzero(conn_ctl["flags"][:n_conns] & rm.SHUTDOWN))
    total = int(sum(e[1] for e in entries))
    summary = dict(frames=len(entries), payload_bytes=total, payload_len=0, errors=shut, status=0)
    if max_sends is not None and len(entries) > max_sends:
        summary["status"] = ERR_CAPACITY
        return dict(send=None, conn_send=None, summary=summary)
    send = np.zeros(len(entries), rm.SEND_DTYPE)
    for k, e in enumerate(entries):
        send[k] = e
    return dict(send=send, conn_send=conn_send, summary=summary)


def synthetic_wires(rep: dict, ctl: dict):
    """Offset tables and encode summaries as the three encodes would leave them
    (a 2-byte header and the payload, frames back to back; the deflated wire's
    payloads taken as long as the plain bytes): (the model's triples, the
    device's (table, summary) pairs), plain / deflated / control."""
    sizes = [[2 + int(x) for x in rep["plain"]["payload_len"]], [2 + int(x) for x in rep["def_msgs"]["length"]],
             [2 + int(x) for x in ctl["ctl"]["payload_len"]]]
    tabs = [np.concatenate([[0], np.cumsum(s)[:-1]]).astype(np.uint64) if s else np.zeros(0, np.uint64) for s in sizes]
    model = [(tab, len(s), int(sum(s))) for tab, s in zip(tabs, sizes)]
    dev = [(tab, rm.summary_np(frames=len(s), payload_bytes=int(sum(s)))) for tab, s in zip(tabs, sizes)]
    return model, dev


def chain_model(d: mm.Decoded, t: dict, conn_ext, window_bits, rooms, flags=0, policy=jm.HANDLER_ECHO_BINARY):
    """The control model, the room reply model and synthetic wires of a
    hand-built batch: dict(ctl, rep, wires, dev_wires)."""
    nc = d.conn_out.shape[0]
    ctl = rm.control_model(d.frames, d.conn_out, d.n_decoded, d.arena, t["msg_of"], t["messages"], t["conn_msg"],
                           t["bodies"])
    rep = reply_rooms_model(ctl["bodies"], policy, conn_ext, window_bits, nc, rooms, flags)
    wires, dev_wires = synthetic_wires(rep, ctl)
    return dict(ctl=ctl, rep=rep, wires=wires, dev_wires=dev_wires)


def plan_of_chain(d: mm.Decoded, t: dict, ch: dict, conn_ext, rooms, flags=0, max_sends=None, gate_ok=True):
    ctl, rep = ch["ctl"], ch["rep"]
    return room_plan_model(d.n_decoded, d.conn_out, t["msg_of"], ctl["msg_end"], rep["plain_of"], rep["def_of"],
                           t["messages"].shape[0], conn_ext, ctl["ctl_of"], ctl["conn_ctl"], ch["wires"], rooms, flags,
                           max_sends, gate_ok)


# ---------------------------------------------------------------------------- device runs
class DevRooms:
    """Hand-built (possibly malformed) tables as the object Engine's wrappers read."""

    def __init__(self, rooms, dev):
        cr, first, members = rooms
        up = lambda a: mm._dev(np.ascontiguousarray(a, dtype=np.uint32), dev, 4)  # noqa: E731
        self.conn_room, self.room_first, self.room_members = up(cr), up(first), up(members)
        self.n_rooms, self.n_members = len(first) - 1, len(members)


def run_reply_rooms(engine, bodies_np, msg_status, join_status, policy, conn_ext, window_bits, n_conns, rooms, flags):
    """gevws_reply_rooms_async on host records: host copies of everything it
    may write, each prefilled with FILL."""
    import torch
    dev = torch.device("cuda", engine.device)
    nm = bodies_np.shape[0]
    cap = max(nm, 1)
    bodies = mm._dev(bodies_np, dev, 32)
    msum = mm._dev(rm.summary_np(frames=nm, status=msg_status), dev, 64)
    jsum = mm._dev(rm.summary_np(frames=nm, status=join_status), dev, 64)
    ext = None if conn_ext is None else mm._dev(np.asarray(conn_ext, np.uint8), dev, 1)
    wb = None if window_bits is None else mm._dev(np.asarray(window_bits, np.uint8), dev, 1)
    f = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    dm, dc, ds, pl, pc, ps = f(cap * 24), f(cap * 4), f(64), f(cap * 32), f(cap * 4), f(64)
    po, do = f(cap * 8), f(cap * 8)
    engine.reply_rooms_async(bodies, nm, msum, jsum, policy, ext, wb, n_conns, DevRooms(rooms, dev), flags, dm, dc, ds,
                             pl, pc, ps, po, do)
    torch.cuda.synchronize(engine.device)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(def_msgs=h(dm), def_conn=h(dc), def_summary=h(ds).view(mm.SUMMARY_DTYPE)[0], plain=h(pl),
                plain_conn=h(pc), plain_summary=h(ps).view(mm.SUMMARY_DTYPE)[0], plain_of=h(po), def_of=h(do))


def assert_reply_rooms(got: dict, want: dict, tag="") -> None:
    for k in ("def_summary", "plain_summary"):
        s = got[k]
        assert jm.summary_tuple(s) == tuple(want[k][x] for x in ("frames", "payload_bytes", "payload_len", "errors",
                                                                 "status")), (tag, k, jm.summary_tuple(s), want[k])
        assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), (tag, k)
    names = ("def_msgs", "def_conn", "plain", "plain_conn", "plain_of", "def_of")
    if want["def_msgs"] is None:
        for k in names:
            assert np.all(got[k] == FILL), (tag, k, "written by a call that wrote nothing")
        return
    for k in names:
        rm._same(got[k], want[k], (tag, k))


def run_room_plan(engine, n_frames, decoded, conn_out, msg_of, msg_end, plain_of, def_of, n_messages, msg_summary,
                  join_summary, conn_ext, ctl_of, conn_ctl, ctl_summary, wires, rooms, flags, max_sends):
    """gevws_room_plan_async on host tables (as tests/_respond_model.run_plan):
    host copies of what it may write, prefilled with FILL."""
    import torch
    dev = torch.device("cuda", engine.device)
    nc = conn_out.shape[0]
    D = lambda a, mn=8: mm._dev(a, dev, mn)  # noqa: E731
    f = lambda nbytes: torch.full((max(nbytes, 8),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    send, cs, summ = f(max_sends * 32), f(nc * 32), f(64)
    ext = None if conn_ext is None else D(np.asarray(conn_ext, np.uint8), 1)
    w = [(D(np.asarray(tab, np.uint64)), D(s, 64)) for tab, s in wires]
    engine.room_plan_async(n_frames, D(decoded, 64), D(conn_out, 32), nc, D(np.asarray(msg_of, np.int64)),
                           D(np.asarray(msg_end, np.uint64)), D(np.asarray(plain_of, np.int64)),
                           D(np.asarray(def_of, np.int64)), n_messages, D(msg_summary, 64), D(join_summary, 64), ext,
                           D(np.asarray(ctl_of, np.int64)), D(conn_ctl, 32), D(ctl_summary, 64), w[0][0], w[0][1],
                           w[1][0], w[1][1], w[2][0], w[2][1], DevRooms(rooms, dev), flags, send, max_sends, cs, summ)
    torch.cuda.synchronize(engine.device)
    return dict(send=send.cpu().numpy(), conn_send=cs.cpu().numpy(),
                summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0])


assert_plan = rm.assert_plan
