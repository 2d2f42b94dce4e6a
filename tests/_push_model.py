"""The push pass's contracts (gevws_push_lists_async, gevws_push_plan_async,
gevws_push_check; include/gevws.h, "Server push") restated in plain Python over
explicit recipient lists, and the helpers that run both device steps on
hand-built tables.

The model is pinned on the CPU (tests/test_push_model.py) by its own properties
and against gevws_push_check; the GPU tests compare every output of the device
with it, byte for byte."""
from __future__ import annotations

import numpy as np

import gev_amd
from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm
from tests import _rooms_model as ro

ALL, ROOM, CONN = 0, 1, 2
TEXT, BINARY, PING, PONG = 1, 2, 9, 10
ROOM_NONE = ro.ROOM_NONE
EXT_DEFLATE, EXT_SERVER_TAKEOVER = ro.EXT_DEFLATE, ro.EXT_SERVER_TAKEOVER
ERR_CAPACITY, ERR_INVALID = ro.ERR_CAPACITY, ro.ERR_INVALID
FILL = ro.FILL
PUSH_DTYPE = gev_amd.PUSH_DTYPE
WINDOWS = (0, 8, 9, 10, 11, 12, 13, 14, 15)
zero_summary = ro.zero_summary
takes_deflate = ro.takes_deflate


def keys(recs) -> np.ndarray:
    return (recs["kind"].astype(np.uint64) << np.uint64(32)) | recs["target"].astype(np.uint64)


def records_bad(recs, n_conns: int, n_rooms: int, src_bytes: int) -> np.ndarray:
    """Per record: is it malformed (each counts once, whatever is wrong)."""
    recs = np.asarray(recs, PUSH_DTYPE).reshape(-1)
    bad = np.zeros(recs.size, bool)
    k = keys(recs)
    for i, r in enumerate(recs):
        kind, target, op = int(r["kind"]), int(r["target"]), int(r["opcode"])
        off, length = int(r["off"]), int(r["length"])
        b = kind > CONN
        b |= kind == ALL and target != 0
        b |= kind == ROOM and target >= n_rooms
        b |= kind == CONN and target >= n_conns
        b |= op not in (TEXT, BINARY, PING, PONG)
        b |= off % 16 != 0
        b |= length > 0xFFFFFFFF or off + length > src_bytes      # (Python integers: the sum cannot wrap)
        b |= op in (PING, PONG) and length > 125
        b |= bool(r["reserved"].any())
        b |= i > 0 and int(k[i]) < int(k[i - 1])
        bad[i] = b
    return bad


def is_live(live, c: int) -> bool:
    return live is None or bool(live[c])


def window_of(window_bits, c: int) -> int:
    return (int(window_bits[c]) or 15) if window_bits is not None else 15


def table_bad(rooms, n_conns: int, conn_ext=None, window_bits=None, live=None) -> int:
    """Bad table records: the rooms' (tests/_rooms_model.check_tables; none
    without tables), and every live deflate-taking connection with a window
    byte outside {0, 8..15} whose record is not bad already."""
    bad = ro.check_tables(rooms, n_conns) if rooms is not None else 0
    if window_bits is None:
        return bad
    n_rooms = len(rooms[1]) - 1 if rooms is not None else 0
    for c in range(n_conns):
        if is_live(live, c) and takes_deflate(conn_ext, c) and int(window_bits[c]) not in WINDOWS:
            g = int(rooms[0][c]) if rooms is not None else ROOM_NONE
            bad += not (g != ROOM_NONE and g >= n_rooms)
    return bad


def recipients(rec, n_conns: int, rooms, live):
    """The connections push `rec` (well formed, over well-formed tables) goes to, increasing."""
    kind, target = int(rec["kind"]), int(rec["target"])
    if kind == ALL:
        return [c for c in range(n_conns) if is_live(live, c)]
    if kind == ROOM:
        return [c for c in ro.members_of(rooms, target) if is_live(live, c)]
    return [target] if is_live(live, target) else []


def _recipient_cache(recs, n_conns, rooms, live):
    cache = {}
    out = []
    for r in recs:
        k = (int(r["kind"]), int(r["target"]))
        if k not in cache:
            cache[k] = recipients(r, n_conns, rooms, live)
        out.append(cache[k])
    return out


def lists_model(recs, src_bytes, conn_ext, window_bits, live, n_conns, rooms, prev=None, max_pushes=None):
    """What gevws_push_lists_async must produce: dict(def_msgs, plain, plain_of,
    def_of, def_summary, plain_summary); the tables are None where nothing may be
    written.  prev: d_prev as a dict(frames, status) or None."""
    recs = np.asarray(recs, PUSH_DTYPE).reshape(-1)
    n = recs.size if max_pushes is None else min(max_pushes, recs.size)
    if prev is not None:
        n = 0 if prev["status"] != 0 else min(n, prev["frames"])
    nothing = dict(def_msgs=None, plain=None, plain_of=None, def_of=None)
    if n == 0:
        return dict(nothing, def_summary=zero_summary(), plain_summary=zero_summary())
    recs = recs[:n]
    n_rooms = len(rooms[1]) - 1 if rooms is not None else 0
    bad = table_bad(rooms, n_conns, conn_ext, window_bits, live) + int(records_bad(recs, n_conns, n_rooms,
                                                                                src_bytes).sum())
    if bad:
        s = dict(zero_summary(), errors=bad, status=ERR_INVALID)
        return dict(nothing, def_summary=s, plain_summary=dict(s))
    plain_of, def_of = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    dmsgs, plain = [], []
    for p, (r, R) in enumerate(zip(recs, _recipient_cache(recs, n_conns, rooms, live))):
        op, ctl = int(r["opcode"]), int(r["opcode"]) in (PING, PONG)
        if any(ctl or not takes_deflate(conn_ext, c) for c in R):
            plain_of[p] = len(plain)
            plain.append((int(r["off"]), int(r["length"]), op))
        takers = [c for c in R if takes_deflate(conn_ext, c)]
        if takers and not ctl:
            def_of[p] = len(dmsgs)
            dmsgs.append((int(r["off"]), int(r["length"]), op, min(window_of(window_bits, c) for c in takers)))
    dm = np.zeros(len(dmsgs), jm.DEFLATE_MSG_DTYPE)
    for k, (off, length, op, wb) in enumerate(dmsgs):
        dm[k]["payload_off"], dm[k]["length"], dm[k]["opcode"], dm[k]["window_bits"] = off, length, op, wb
    pl = np.zeros(len(plain), jm.OUT_FRAME_DTYPE)
    for k, (off, length, op) in enumerate(plain):
        pl[k]["fin"], pl[k]["opcode"], pl[k]["length"] = 1, op, length
        pl[k]["payload_off"], pl[k]["payload_len"] = off, length
    return dict(def_msgs=dm, plain=pl, plain_of=plain_of, def_of=def_of,
                def_summary=dict(zero_summary(), frames=len(dmsgs)),
                plain_summary=dict(zero_summary(), frames=len(plain)))


def plan_model(recs, src_bytes, plain_of, def_of, wires, conn_ext, live, n_conns, rooms, max_sends=None,
               gate_ok=True, prev=None, max_pushes=None):
    """What gevws_push_plan_async must produce: dict(send, conn_send, summary).
    wires: two (offset table, count, wire total), plain / deflated; gate_ok
    False: a list or encode summary failed.  With bad tables or records only
    those are counted (the index checks need recipients)."""
    recs = np.asarray(recs, PUSH_DTYPE).reshape(-1)
    n = recs.size if max_pushes is None else min(max_pushes, recs.size)
    if prev is not None:
        n = 0 if prev["status"] != 0 else min(n, prev["frames"])
    if not gate_ok or n == 0 or n_conns == 0:
        return dict(send=None, conn_send=None, summary=zero_summary())
    recs = recs[:n]
    n_rooms = len(rooms[1]) - 1 if rooms is not None else 0
    bad = table_bad(rooms, n_conns) + int(records_bad(recs, n_conns, n_rooms, src_bytes).sum())
    if bad:
        return dict(send=None, conn_send=None, summary=dict(zero_summary(), errors=bad, status=ERR_INVALID))

    def rng(wire, idx):
        tab, cnt, total = wires[wire]
        if idx >= cnt:
            return None
        off = int(tab[idx])
        nxt = int(tab[idx + 1]) if idx + 1 < cnt else total
        return None if nxt < off else (off, nxt - off)

    per_conn = [[] for _ in range(n_conns)]
    for p, R in enumerate(_recipient_cache(recs, n_conns, rooms, live)):
        ip, idf = int(plain_of[p]), int(def_of[p])
        r0 = rng(0, ip) if ip >= 0 else None
        r1 = rng(1, idf) if idf >= 0 else None
        b = (ip >= 0 and r0 is None) or (idf >= 0 and r1 is None)
        for c in R:
            if takes_deflate(conn_ext, c):
                b |= idf < 0 and ip < 0
            else:
                b |= ip < 0
        if b:
            bad += 1
            continue
        for c in R:
            wire = 1 if takes_deflate(conn_ext, c) and idf >= 0 else 0
            per_conn[c].append((*(r1 if wire else r0), p, c, wire))
    if bad:
        return dict(send=None, conn_send=None, summary=dict(zero_summary(), errors=bad, status=ERR_INVALID))
    entries, conn_send = [], np.zeros(n_conns, rm.CONN_SEND_DTYPE)
    for c in range(n_conns):
        conn_send[c] = (len(entries), len(per_conn[c]), sum(e[1] for e in per_conn[c]), 0, 0)
        entries += per_conn[c]
    summary = dict(frames=len(entries), payload_bytes=int(sum(e[1] for e in entries)), payload_len=0, errors=0,
                   status=0)
    if max_sends is not None and len(entries) > max_sends:
        summary["status"] = ERR_CAPACITY
        return dict(send=None, conn_send=None, summary=summary)
    send = np.zeros(len(entries), rm.SEND_DTYPE)
    for k, e in enumerate(entries):
        send[k] = e
    return dict(send=send, conn_send=conn_send, summary=summary)


def synthetic_wires(lists: dict):
    """Offset tables and encode summaries as the two encodes would leave them
    (a 2-byte header and the payload, frames back to back; the deflated wire's
    payloads taken as long as the plain bytes): (the model's triples, the
    device's (table, summary) pairs), plain / deflated."""
    sizes = [[], []] if lists["plain"] is None else [[2 + int(x) for x in lists["plain"]["payload_len"]],
                                                     [2 + int(x) for x in lists["def_msgs"]["length"]]]
    tabs = [np.concatenate([[0], np.cumsum(s)[:-1]]).astype(np.uint64) if s else np.zeros(0, np.uint64) for s in sizes]
    model = [(tab, len(s), int(sum(s))) for tab, s in zip(tabs, sizes)]
    dev = [(tab, rm.summary_np(frames=len(s), payload_bytes=int(sum(s)))) for tab, s in zip(tabs, sizes)]
    return model, dev


def client_view(recs, arena, conn_ext, live, n_conns, rooms):
    """What each connection must receive: [(opcode, body, compressed)] per
    connection, in list order."""
    recs = np.asarray(recs, PUSH_DTYPE).reshape(-1)
    out = [[] for _ in range(n_conns)]
    for r, R in zip(recs, _recipient_cache(recs, n_conns, rooms, live)):
        op, off, ln = int(r["opcode"]), int(r["off"]), int(r["length"])
        body = bytes(arena[off: off + ln])
        for c in R:
            out[c].append((op, body, takes_deflate(conn_ext, c) and op in (TEXT, BINARY)))
    return out


# ---------------------------------------------------------------------------- shapes
LENGTHS = (0, 1, 15, 16, 17, 125, 126, 65535, 65536)   # every header size class, both sides of each edge
N_ROOMS, EMPTY_ROOM, SINGLE_ROOM, DEAD_ROOM = 7, 2, 4, 5


def base_shape(seed=0x70757368, n_conns=300):
    """The tests' connection table: n_conns connections (two blocks of 256) in
    7 rooms -- one empty, one with a single member, one whose members are all
    dead -- about a ninth in no room, extension bytes plain / deflate / server
    takeover, window bytes {0, 9, 15}, about a tenth dead.
    -> dict(n_conns, rooms, conn_room, ext, wb, live)."""
    rng = np.random.default_rng(seed)
    cr = rng.integers(0, 9, n_conns).astype(np.uint32)
    cr[cr >= 7] = ROOM_NONE
    cr[cr == EMPTY_ROOM] = 3
    cr[cr == SINGLE_ROOM] = 6
    cr[17] = SINGLE_ROOM
    ext = rng.choice(np.array([0, EXT_DEFLATE, EXT_DEFLATE, EXT_DEFLATE | EXT_SERVER_TAKEOVER], np.uint8), n_conns)
    wb = rng.choice(np.array([0, 9, 15], np.uint8), n_conns)
    live = (rng.random(n_conns) >= 0.1).astype(np.uint8)
    live[cr == DEAD_ROOM] = 0
    live[17] = 1
    rooms = ro.csr_of(cr, n_rooms=N_ROOMS)
    assert ro.check_tables(rooms, n_conns) == 0 and len(ro.members_of(rooms, EMPTY_ROOM)) == 0
    assert ro.members_of(rooms, SINGLE_ROOM) == [17] and len(ro.members_of(rooms, DEAD_ROOM)) > 0
    return dict(n_conns=n_conns, rooms=rooms, conn_room=cr, ext=ext, wb=wb, live=live)


def random_items(rng, n, n_conns, n_rooms=N_ROOMS, lengths=LENGTHS, all_max=None):
    """n items for gev_amd.push_records: the three kinds mixed, opcodes 1 / 2 /
    9 / 10 (pings and pongs of at most 125 bytes), lengths from `lengths`.
    all_max: the longest body of an ALL push (None: any)."""
    items = []
    for i in range(n):
        kind = int(rng.integers(0, 3))
        target = 0 if kind == ALL else int(rng.integers(0, n_rooms if kind == ROOM else n_conns))
        op = int(rng.choice([TEXT, TEXT, BINARY, BINARY, PING, PONG]))
        ok = [x for x in lengths if (op < 8 or x <= 125) and (kind != ALL or all_max is None or x <= all_max)]
        ln = int(ok[i % len(ok)]) if i < 2 * len(ok) else int(rng.choice(ok))
        if op == TEXT:
            body = bytes(rng.integers(0x20, 0x7F, ln, dtype=np.uint8))
        else:
            body = bytes(rng.integers(0, 256, ln, dtype=np.uint8)) if ln < 4096 else bytes(ln // 7) + bytes(
                rng.integers(0, 256, ln - ln // 7, dtype=np.uint8))
        items.append((kind, target, op, body))
    return items


# ---------------------------------------------------------------------------- device runs
def _u8(a, dev):
    return None if a is None else mm._dev(np.asarray(a, np.uint8), dev, 1)


def _rooms(rooms, dev):
    return None if rooms is None else ro.DevRooms(rooms, dev)


def run_lists(engine, recs, src_bytes, conn_ext, window_bits, live, n_conns, rooms, prev=None, max_pushes=None):
    """gevws_push_lists_async on host records: host copies of everything it may
    write, each prefilled with FILL.  prev: a SUMMARY_DTYPE array or None."""
    import torch
    dev = torch.device("cuda", engine.device)
    recs = np.ascontiguousarray(np.asarray(recs, PUSH_DTYPE).reshape(-1))
    n = recs.size if max_pushes is None else max_pushes
    cap = max(recs.size, 1)
    f = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    dm, ds, pl, ps, po, do = f(cap * 24), f(64), f(cap * 32), f(64), f(cap * 8), f(cap * 8)
    engine.push_lists_async(mm._dev(recs, dev, 32), n, None if prev is None else mm._dev(prev, dev, 64), src_bytes,
                            _u8(conn_ext, dev), _u8(window_bits, dev), _u8(live, dev), n_conns, _rooms(rooms, dev), 0,
                            dm, ds, pl, ps, po, do)
    torch.cuda.synchronize(engine.device)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(def_msgs=h(dm), def_summary=h(ds).view(mm.SUMMARY_DTYPE)[0], plain=h(pl),
                plain_summary=h(ps).view(mm.SUMMARY_DTYPE)[0], plain_of=h(po), def_of=h(do))


def assert_lists(got: dict, want: dict, tag="") -> None:
    for k in ("def_summary", "plain_summary"):
        s = got[k]
        assert jm.summary_tuple(s) == tuple(want[k][x] for x in ("frames", "payload_bytes", "payload_len", "errors",
                                                                 "status")), (tag, k, jm.summary_tuple(s), want[k])
        assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), (tag, k)
    names = ("def_msgs", "plain", "plain_of", "def_of")
    if want["def_msgs"] is None:
        for k in names:
            assert np.all(got[k] == FILL), (tag, k, "written by a call that wrote nothing")
        return
    for k in names:
        rm._same(got[k], want[k], (tag, k))


def run_plan(engine, recs, src_bytes, plain_summary, def_summary, plain_of, def_of, wires, conn_ext, live, n_conns,
             rooms, max_sends, prev=None, max_pushes=None):
    """gevws_push_plan_async on host tables: host copies of what it may write,
    prefilled with FILL.  wires: two (offset table, encode summary)."""
    import torch
    dev = torch.device("cuda", engine.device)
    recs = np.ascontiguousarray(np.asarray(recs, PUSH_DTYPE).reshape(-1))
    n = recs.size if max_pushes is None else max_pushes
    D = lambda a, mn=8: mm._dev(a, dev, mn)  # noqa: E731
    f = lambda nbytes: torch.full((max(nbytes, 8),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    send, cs, summ = f(max_sends * 32), f(n_conns * 32), f(64)
    w = [(D(np.asarray(tab, np.uint64)), D(s, 64)) for tab, s in wires]
    engine.push_plan_async(D(recs, 32), n, None if prev is None else D(prev, 64), src_bytes, D(plain_summary, 64),
                           D(def_summary, 64), D(np.asarray(plain_of, np.int64)), D(np.asarray(def_of, np.int64)),
                           w[0][0], w[0][1], w[1][0], w[1][1], _u8(conn_ext, dev), _u8(live, dev), n_conns,
                           _rooms(rooms, dev), 0, send, max_sends, cs, summ)
    torch.cuda.synchronize(engine.device)
    return dict(send=send.cpu().numpy(), conn_send=cs.cpu().numpy(),
                summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0])


assert_plan = rm.assert_plan
