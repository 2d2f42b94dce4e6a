"""GPU checks of the membership update (gevws_rooms_update_async) through the C
ABI, bit-exact against tests/_rooms_update_model.py: d_conn_room_out,
d_room_first_out, d_room_members_out and the summary, every byte that is not an
output entry still the 0xEE it was prefilled with, the input unchanged -- and of
the tables in use: the room reply step's own check accepts them, and a second
Engine.broadcast over Rooms.update's tables sends what the host-built ones send."""
import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm
from tests import _rooms_model as ro
from tests import _rooms_update_model as um
from tests._helpers import gpu_decode

pytestmark = pytest.mark.gpu

NONE = um.ROOM_NONE
S, F = um.CTL_SHUTDOWN, um.CTL_FAILED
B = 1024          # kRuKeys: the sort's keys per workgroup (four rounds of a 256-lane workgroup)
BLOCK = 256       # kWalkBlock: the lanes of the per-change and per-connection kernels
LDS_ROOMS = 4096  # kRuLdsRooms: up to this many rooms are counted in LDS
N_BIG = 3 * B + 37
T, C, CLOSE = 1, 0, 8


def check(engine, conn_room, n_rooms, tag="", **kw):
    """One call on the device and in the model: equal bit for bit."""
    want = um.update_model(conn_room, n_rooms, **kw)
    got = um.run_update(engine, conn_room, n_rooms, **kw)
    um.assert_update(got, want, conn_room, tag)
    return got, want


def random_rooms(rng, n_conns, n_rooms):
    """Random rooms, about a quarter of the connections in none."""
    cr = rng.integers(0, max(n_rooms, 1), n_conns).astype(np.uint32)
    cr[rng.random(n_conns) < 0.25] = NONE
    if n_rooms == 0:
        cr[:] = NONE
    return cr


# ---------------------------------------------------------------------------- 1. the pure build
@pytest.mark.parametrize("n_rooms", [0, 1, 2, 256, 257, 65536, 65537])
def test_pure_build(engine, n_rooms):
    """No changes, no closes: Rooms.csr on the device, at every workgroup edge of
    the sort and every pass count (n_rooms 0: no pass; 1, 2, 256: one; 257,
    65 536: two; 65 537: three)."""
    rng = np.random.default_rng(0x72753100 + n_rooms)
    for n_conns in (0, 1, 65, B - 1, B, B + 1, N_BIG):
        cr = random_rooms(rng, n_conns, n_rooms)
        if n_rooms > 1 and n_conns > 2:
            cr[0], cr[n_conns - 1] = n_rooms - 1, 0   # the largest room id first, the smallest last
        got, want = check(engine, cr, n_rooms, tag=(n_conns, n_rooms))
        assert int(got["summary"]["frames"]) == np.count_nonzero(cr != NONE)
        assert ro.check_tables((want["conn_room"], want["first"], want["members"]), n_conns) == 0


def test_pure_build_four_passes(engine):
    """n_rooms = 2^24 + 1: every byte of the room id is a digit.  The
    connections sit in low and in high rooms, some ids differing in the top
    byte alone."""
    rng = np.random.default_rng(0x72753104)
    n_rooms = (1 << 24) + 1
    low = rng.integers(0, 300, N_BIG)
    high = n_rooms - 1 - rng.integers(0, 70000, N_BIG)
    cr = np.where(rng.random(N_BIG) < 0.5, low, high).astype(np.uint32)
    cr[rng.random(N_BIG) < 0.25] = NONE
    cr[5], cr[6], cr[7] = 1 << 24, 0, 1 << 24
    got, _ = check(engine, cr, n_rooms, tag="2^24 + 1 rooms")
    assert int(got["summary"]["frames"]) > 2 * B


@pytest.mark.parametrize("n_rooms", [LDS_ROOMS, LDS_ROOMS + 1])
def test_room_count_threshold(engine, n_rooms):
    """Up to LDS_ROOMS rooms a workgroup counts its rooms in LDS, above that in
    device memory: both sides of the threshold, with changes and closes, the
    last room used and more than one workgroup of connections."""
    rng = np.random.default_rng(0x72753105 + n_rooms)
    cr = random_rooms(rng, N_BIG, n_rooms)
    cr[[0, B, N_BIG - 1]] = n_rooms - 1
    pairs = [(int(c), int(g)) for c, g in zip(rng.integers(0, N_BIG, 500), rng.integers(0, n_rooms, 500))]
    flags = ((rng.random(N_BIG) < 0.05) * S).astype(np.uint32)
    flags[B] = 0
    got, want = check(engine, cr, n_rooms, changes=um.changes_np(pairs + [(B, n_rooms - 1)]), conn_flags=flags,
                      tag=n_rooms)
    assert int(want["first"][n_rooms]) - int(want["first"][n_rooms - 1]) >= 1


# ---------------------------------------------------------------------------- 2. order
@pytest.mark.parametrize("shape", ["one room", "two rooms alternating", "reversed", "equal low bytes"])
def test_order_stress(engine, shape):
    c = np.arange(N_BIG, dtype=np.uint32)
    if shape == "one room":          # the members are arange: every term of a key's rank is exercised
        cr, n_rooms = np.zeros(N_BIG, np.uint32), 1
    elif shape == "two rooms alternating":
        cr, n_rooms = c % 2, 2
    elif shape == "reversed":        # every key moves, no two are equal
        cr, n_rooms = N_BIG - 1 - c, N_BIG
    else:                            # the first pass leaves them where they are, the second orders them
        cr, n_rooms = ((c * 7) % 251) << 8 | 0x5A, 65537
    got, want = check(engine, cr.astype(np.uint32), n_rooms, tag=shape)
    assert int(got["summary"]["frames"]) == N_BIG
    if shape == "one room":
        assert want["members"].tolist() == list(range(N_BIG))
    if shape == "reversed":
        assert want["members"].tolist() == list(range(N_BIG - 1, -1, -1))


# ---------------------------------------------------------------------------- 3. changes
def test_join_move_leave_and_stay(engine):
    rng = np.random.default_rng(0x72753301)
    n_conns, n_rooms = B + 77, 9
    cr = random_rooms(rng, n_conns, n_rooms)
    cr[:8] = [NONE, 0, 1, 2, NONE, 3, 4, 5]
    pairs = [(0, 4), (1, 5), (2, NONE), (3, 2), (4, NONE)]      # join, move, leave, stay, leave nothing
    pairs += [(int(c), int(g)) for c, g in zip(rng.integers(8, n_conns, 300), rng.integers(0, n_rooms, 300))]
    pairs += [(n_conns - 1, 8), (0, 7)]                         # the first record's connection again in the last
    got, want = check(engine, cr, n_rooms, changes=um.changes_np(pairs), tag="mixed")
    assert want["conn_room"][:5].tolist() == [7, 5, NONE, 2, NONE] and int(want["conn_room"][-1]) == 8
    assert int(got["summary"]["payload_bytes"]) == len(pairs) and int(got["summary"]["payload_len"]) > 100


def test_one_connection_named_200_times(engine):
    """More change lanes than a wave holds, across a workgroup edge of them:
    the last record wins whichever lane's atomic retires last."""
    rng = np.random.default_rng(0x72753302)
    n_conns, n_rooms = 300, 300
    cr = random_rooms(rng, n_conns, n_rooms)
    k = BLOCK - 100
    pairs = [(int(c), int(g)) for c, g in zip(rng.integers(0, n_conns, k), rng.integers(0, n_rooms, k))]
    pairs += [(17, int(g)) for g in rng.permutation(n_rooms)[:200]]   # records 156 .. 355: lanes of two workgroups
    pairs[-1] = (17, 123)
    assert len(pairs) > BLOCK + 64
    got, want = check(engine, cr, n_rooms, changes=um.changes_np(pairs), tag="200 times")
    assert int(want["conn_room"][17]) == 123
    for _ in range(2):   # and a leave in the middle does not outlive a later join
        pairs[200] = (17, NONE)
        check(engine, cr, n_rooms, changes=um.changes_np(pairs), tag="200 times, a leave among them")


def test_the_count_comes_from_the_gate(engine):
    cr = np.array([0, 1, NONE, 2] * 20, np.uint32)
    ch = um.changes_np([(0, 2), (2, 1), (0, NONE), (0, 1), (3, 2), (1, NONE), (2, 0)])
    got, _ = check(engine, cr, 3, changes=ch, max_changes=7, prev=dict(frames=3, status=0), tag="3 of 7")
    assert int(got["summary"]["payload_bytes"]) == 3
    check(engine, cr, 3, changes=ch, max_changes=2, prev=dict(frames=100, status=0), tag="2 of 7")
    check(engine, cr, 3, changes=ch, max_changes=7, prev=dict(frames=0, status=0), tag="none of 7")
    check(engine, cr, 3, changes=ch, max_changes=0, tag="max_changes 0")
    # a failed gate: its status and nothing else -- even with records that are malformed
    bad = um.changes_np([(999, 999)])
    got, _ = check(engine, cr, 3, changes=bad, prev=dict(frames=1, status=gev_amd.ERR_CAPACITY), tag="failed d_prev")
    assert jm.summary_tuple(got["summary"]) == (0, 0, 0, 0, gev_amd.ERR_CAPACITY)


# ---------------------------------------------------------------------------- 4. closes
def test_closes(engine):
    rng = np.random.default_rng(0x72753401)
    n_conns, n_rooms = B + 5, 40
    cr = random_rooms(rng, n_conns, n_rooms)
    cr[:4] = [3, 3, NONE, 5]
    flags = np.zeros(n_conns, np.uint32)
    flags[rng.random(n_conns) < 0.1] = S
    flags[rng.random(n_conns) < 0.1] = S | F
    flags[:4] = [S, S | F, S, F]          # CTL_FAILED alone closes nothing
    got, want = check(engine, cr, n_rooms, conn_flags=flags, tag="closes alone")
    assert want["conn_room"][:4].tolist() == [NONE, NONE, NONE, 5] and int(got["summary"]["payload_bytes"]) == 0
    # a close beside a join of the same connection, and joins of others
    pairs = [(0, 7), (2, 7), (3, 7), (1, NONE)] + [(int(c), 7) for c in rng.integers(4, n_conns, 50)]
    got, want = check(engine, cr, n_rooms, changes=um.changes_np(pairs), conn_flags=flags, tag="a close beats a join")
    assert want["conn_room"][:4].tolist() == [NONE, NONE, NONE, 7]
    assert np.all(want["conn_room"][(flags & S) != 0] == NONE)
    # a plan that failed moves nobody
    for plan in (gev_amd.ERR_CAPACITY, gev_amd.ERR_INVALID):
        got, _ = check(engine, cr, n_rooms, changes=um.changes_np(pairs), conn_flags=flags, plan=dict(status=plan),
                       tag="failed plan")
        assert jm.summary_tuple(got["summary"]) == (0, 0, 0, 0, plan)
    check(engine, cr, n_rooms, changes=um.changes_np(pairs), conn_flags=flags, plan=dict(status=0),
          prev=dict(frames=10, status=0), tag="both gates open")


# ---------------------------------------------------------------------------- 5. malformed input
def test_malformed_input(engine):
    rng = np.random.default_rng(0x72753501)
    n_conns, n_rooms = B + 9, 12
    cr = random_rooms(rng, n_conns, n_rooms)
    good = [(int(c), int(g)) for c, g in zip(rng.integers(0, n_conns, 40), rng.integers(0, n_rooms, 40))]
    in_bad = cr.copy()
    in_bad[B + 3] = n_rooms
    several = cr.copy()
    several[[1, 700, n_conns - 1]] = [n_rooms, 0xFFFFFFFE, n_rooms + 5]
    cases = {
        "conn == n_conns": (cr, good + [(n_conns, 0)], 1),
        "room == n_rooms": (cr, [(5, n_rooms)] + good, 1),
        "in[c] == n_rooms": (in_bad, good, 1),
        "in[c] == n_rooms, no list": (in_bad, None, 1),
        "several at once": (several, good[:20] + [(n_conns, n_rooms), (0, 0xFFFFFFFE), (1, 0)] + good[20:]
                            + [(0xFFFFFFFF, 0)], 6),
    }
    for tag, (rooms, pairs, count) in cases.items():
        ch = None if pairs is None else um.changes_np(pairs)
        got, _ = check(engine, rooms, n_rooms, changes=ch, conn_flags=np.full(n_conns, S, np.uint32)
                       if tag == "several at once" else None, tag=tag)
        assert jm.summary_tuple(got["summary"]) == (0, 0, 0, count, gev_amd.ERR_INVALID), tag
        for k in ("conn_room", "first", "members"):
            assert np.all(got[k] == um.FILL), (tag, k)
    # n_rooms == 0: any room id is one too many
    got, _ = check(engine, np.array([NONE, 0, NONE], np.uint32), 0, tag="a room without rooms")
    assert jm.summary_tuple(got["summary"]) == (0, 0, 0, 1, gev_amd.ERR_INVALID)


def test_invalid_calls_with_a_live_context(engine):
    """The checks the call makes before any device work, each one alone behind
    a real context (tests/test_rooms_update_abi.py can only reach them with a
    NULL one): the call fails and every buffer keeps its fill."""
    import torch
    dev = torch.device("cuda", engine.device)
    n_conns, n_rooms = 70, 3
    cr = (np.arange(n_conns) % n_rooms).astype(np.uint32)
    f = lambda nbytes: torch.full((nbytes,), um.FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    d_in, d_ch = mm._dev(cr, dev, 4), mm._dev(um.changes_np([(0, 1)]), dev, 8)
    out, first, members, summ = f(n_conns * 4), f((n_rooms + 1) * 4), f(n_conns * 4), f(64)

    def call(**edit):
        a = dict(conn_room_in=d_in, n_conns=n_conns, n_rooms=n_rooms, changes=d_ch, max_changes=1, prev=None,
                 conn_send=None, plan_summary=None, flags=0, conn_room_out=out, room_first_out=first,
                 room_members_out=members, summary=summ)
        a.update(edit)
        engine.rooms_update_async(**a)
        torch.cuda.synchronize(engine.device)

    cases = [dict(flags=1), dict(flags=0x80000000), dict(conn_room_out=None), dict(room_first_out=None),
             dict(room_members_out=None), dict(summary=None), dict(conn_room_in=None), dict(conn_room_out=d_in),
             dict(max_changes=1 << 32), dict(max_changes=(1 << 64) - 1)]
    for edit in cases:
        with pytest.raises(RuntimeError, match="gevws_rooms_update_async"):
            call(**edit)
        for t in (out, first, members, summ):
            assert bool((t == um.FILL).all()), edit
        assert np.array_equal(d_in.cpu().numpy()[: n_conns * 4].view(np.uint32), cr), edit
    # the same call without an edit is valid; no input with no connections is valid too
    call()
    assert int(summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0]["status"]) == 0
    assert out.cpu().numpy().view(np.uint32).tolist() == [1] + cr[1:].tolist()
    call(conn_room_in=None, n_conns=0, changes=None, max_changes=0)
    s = summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0]
    assert jm.summary_tuple(s) == (0, 0, 0, 0, 0) and first.cpu().numpy().view(np.uint32).tolist() == [0] * 4


# ---------------------------------------------------------------------------- 6. a sequence, and the tables in use
def test_a_sequence_of_updates(engine):
    """Eight batches one after another, each call's output the next one's
    input on the device; then the room reply step takes the device-built
    tables: its own check (rooms_check) accepts them."""
    rng = np.random.default_rng(0x72753601)
    n_conns, n_rooms = BLOCK + 44, 6
    cr = np.full(n_conns, NONE, np.uint32)
    dev_in, got = None, None
    for step in range(8):
        k = int(rng.integers(1, 2 * n_conns))
        rooms = rng.integers(0, n_rooms, k).astype(np.uint32)
        rooms[rng.random(k) < 0.15] = NONE
        ch = um.changes_np(list(zip(rng.integers(0, n_conns, k).tolist(), rooms.tolist())))
        flags = ((rng.random(n_conns) < 0.04) * S).astype(np.uint32) if step % 3 == 2 else None
        if step == 4:
            n_rooms = 300   # the room space grows: two passes from here on
        want = um.update_model(cr, n_rooms, ch, conn_flags=flags)
        got = um.run_update(engine, cr, n_rooms, ch, conn_flags=flags, conn_room_dev=dev_in)
        um.assert_update(got, want, cr, f"step {step}")
        cr, dev_in = want["conn_room"], got["dev_out"]
    nm = int(got["summary"]["frames"])
    assert 50 < nm < n_conns and np.count_nonzero(np.diff(want["first"].astype(np.int64))) > 100
    dev_tables = (got["conn_room"].view(np.uint32)[:n_conns], got["first"].view(np.uint32)[: n_rooms + 1],
                  got["members"].view(np.uint32)[:nm])
    d = mm.Decoded([[(1, 0, 2, b"m%d" % c)] for c in range(n_conns)])
    t = rm.tables_of(d)
    ctl = rm.control_model(d.frames, d.conn_out, d.n_decoded, d.arena, t["msg_of"], t["messages"], t["conn_msg"],
                           t["bodies"])
    ext = (np.arange(n_conns) % 3 == 0).astype(np.uint8) * ro.EXT_DEFLATE
    runs = [ro.run_reply_rooms(engine, ctl["bodies"], 0, 0, jm.HANDLER_ECHO_BINARY, ext, None, n_conns, tabs, 0)
            for tabs in (dev_tables, ro.csr_of(cr, n_rooms))]
    model = ro.reply_rooms_model(ctl["bodies"], jm.HANDLER_ECHO_BINARY, ext, None, n_conns, ro.csr_of(cr, n_rooms))
    for r in runs:
        assert int(r["def_summary"]["status"]) == 0 and int(r["plain_summary"]["status"]) == 0
        ro.assert_reply_rooms(r, model, "device-built tables")
    assert int(runs[0]["plain_summary"]["frames"]) > 20 and int(runs[0]["def_summary"]["frames"]) > 20
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


# ---------------------------------------------------------------------------- 7. end to end
def test_broadcast_update_broadcast(engine):
    """A pass in which two connections send a close frame and one fails UTF-8,
    Rooms.update with that pass's Responses and a list of changes, then a second
    pass: every connection is sent what the host-updated tables send it, and the
    closed ones nothing."""
    import torch
    dev = torch.device("cuda", engine.device)
    rng = np.random.default_rng(0x72753701)
    nc, n_rooms = 40, 5

    def fr(payload, op, fin=True):
        return wo.encode_frame(payload, op, fin, 0, True, bytes(rng.integers(0, 256, 4, dtype=np.uint8)))

    def run_pass(streams, rooms):
        lens = np.array([len(s) for s in streams], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        batch = gpu_decode(engine, b"".join(streams), np.stack([offs, lens], 1), aux_slots=nc)
        msgs = engine.messages(batch)
        bodies = engine.join(batch, msgs, flags=gev_amd.JOIN_ALL)
        return engine.broadcast(batch, msgs, bodies, gev_amd.HANDLER_ECHO_TEXT, None, rooms)

    room_h = (np.arange(nc) % n_rooms).astype(np.uint32)
    room_h[[4, 9]] = NONE
    closers = {3: fr((1000).to_bytes(2, "big"), CLOSE), 17: fr(b"", CLOSE),
               26: fr(b"ok", T, False) + fr(b"\xff", C)}
    first = [closers.get(c, fr(b"first %d" % c, T)) for c in range(nc)]
    rooms0 = gev_amd.Rooms.build(engine, room_h, n_rooms)
    assert [a.tolist() for a in rooms0.host()] == [a.tolist() for a in ro.csr_of(room_h, n_rooms)]
    res = run_pass(first, rooms0)
    flags = res.conn_send_host()["flags"]
    assert {c: int(flags[c]) for c in np.flatnonzero(flags)} == {3: S, 17: S, 26: S | F}
    # joins, moves, leaves; a join of a connection that this pass closed
    changes = np.array([[4, 0], [9, 2], [0, 1], [1, NONE], [3, 2], [26, 0], [12, 4], [12, 3]], np.int64)
    rooms1 = rooms0.update(engine, changes, closed=res)
    want = um.update_model(room_h, n_rooms, um.changes_np(changes.tolist()), conn_flags=flags)
    assert want["conn_room"][[3, 17, 26, 4, 9, 0, 1, 12]].tolist() == [NONE, NONE, NONE, 0, 2, 1, NONE, 3]
    assert [a.tolist() for a in rooms1.host()] == [want[k].tolist() for k in ("conn_room", "first", "members")]
    assert rooms1.n_rooms == n_rooms and rooms1.n_members == int(want["summary"]["frames"]) == nc - 4
    assert [a.tolist() for a in rooms0.host()] == [a.tolist() for a in ro.csr_of(room_h, n_rooms)]   # still valid
    # the closes alone, as a record array and as a device tensor: the same tables
    recs = um.changes_np(changes.tolist())
    for ch in (recs, torch.from_numpy(recs.view(np.uint8).copy()).to(dev)):
        again = rooms0.update(engine, ch, closed=res)
        assert [a.tolist() for a in again.host()] == [a.tolist() for a in rooms1.host()]
    only = rooms0.update(engine, closed=res)
    assert only.host()[0].tolist() == um.update_model(room_h, n_rooms, conn_flags=flags)["conn_room"].tolist()
    # the second pass: everybody still open says something
    second = [b"" if c in closers else fr(b"second %d" % c, T) for c in range(nc)]
    got = run_pass(second, rooms1)
    ref = run_pass(second, gev_amd.Rooms.from_conn_room(want["conn_room"], dev, n_rooms))
    sent = [got.conn_bytes(c) for c in range(nc)]
    assert sent == [ref.conn_bytes(c) for c in range(nc)]
    for c in closers:
        assert sent[c] == b"" and len(sent[int(np.flatnonzero(want["conn_room"] == room_h[c])[0])]) > 0, c
    # a join is heard, a leaver hears nothing
    assert b"second 4" in sent[5] and b"second 9" in sent[2] and sent[1] == b""
    # a malformed change raises with the status and the count
    with pytest.raises(RuntimeError, match=r"Rooms.update: .*\(2 records\)"):
        rooms0.update(engine, [[nc, 0], [0, n_rooms]])
