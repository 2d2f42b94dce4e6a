"""CPU checks of the room broadcast's model (tests/_rooms_model.py) and of
gev_amd.Rooms' host side: the CSR round-trips, the table check counts what the
header says it counts, and the plan of one room of three is pinned entry by
entry.  No device compute is called here."""
import numpy as np

import gev_amd
from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm
from tests import _rooms_model as ro

NONE = ro.ROOM_NONE
B = 2


def test_csr_round_trips():
    cr = np.array([2, NONE, 0, 2, 0, NONE, 2, 3], np.uint32)   # room 1 is empty
    first, members, n_rooms = gev_amd.Rooms.csr(cr)
    assert n_rooms == 4
    assert first.tolist() == [0, 2, 2, 5, 6] and members.tolist() == [2, 4, 0, 3, 6, 7]
    assert first.dtype == members.dtype == np.uint32
    back = np.full(cr.size, NONE, np.uint32)
    for g in range(n_rooms):
        mine = members[first[g]: first[g + 1]]
        assert np.all(np.diff(mine.astype(np.int64)) > 0), g
        back[mine] = g
    assert back.tolist() == cr.tolist()
    m_cr, m_first, m_members = ro.csr_of(cr)
    assert m_first.tolist() == first.tolist() and m_members.tolist() == members.tolist()
    assert ro.check_tables((m_cr, m_first, m_members), cr.size) == 0
    # the tensors from_conn_room uploads hold the same tables
    r = gev_amd.Rooms.from_conn_room(cr, "cpu")
    h_cr, h_first, h_members = r.host()
    assert (r.n_rooms, r.n_members) == (4, 6)
    assert h_cr.tolist() == cr.tolist() and h_first.tolist() == first.tolist() and h_members.tolist() == members.tolist()
    # no room at all is well formed; more rooms than ids are empty rooms
    f0, m0, n0 = gev_amd.Rooms.csr(np.full(3, NONE, np.uint32))
    assert (f0.tolist(), m0.tolist(), n0) == ([0], [], 0)
    assert ro.check_tables((np.full(3, NONE, np.uint32), f0, m0), 3) == 0
    f5, _, n5 = gev_amd.Rooms.csr(cr, n_rooms=6)
    assert n5 == 6 and f5.tolist() == [0, 2, 2, 5, 6, 6, 6]


def test_check_tables_counts_bad_records():
    cr, first, members = ro.csr_of([0, 0, 1, NONE, 1])
    assert (first.tolist(), members.tolist()) == ([0, 2, 4], [0, 1, 2, 4])

    def bad(cr=cr, first=first, members=members, n=5, **kw):
        return ro.check_tables((np.array(cr, np.uint32), np.array(first, np.uint32), np.array(members, np.uint32)), n,
                               **kw)

    assert bad() == 0
    assert bad(members=[0, 9, 2, 4]) == 1                 # a member >= n_conns
    assert bad(members=[1, 0, 2, 4]) == 1                 # an out-of-order pair: the second slot
    assert bad(cr=[0, 1, 1, NONE, 1]) == 1                # conn_room disagrees with the CSR
    assert bad(cr=[0, 0, 1, 1, 1]) == 1                   # a roomed connection missing from the CSR: the count
    assert bad(cr=[0, 0, 7, NONE, 1]) == 2                # a room id >= n_rooms: the connection and its slot
    # a decreasing first: record 1, first[2] != n_members, slot 2 (now in room 0) and slot 3 (in no room)
    assert bad(first=[0, 3, 2]) == 4
    assert bad(first=[1, 2, 4]) == 2                      # first[0] != 0, and slot 0 lies in no room
    ext = np.array([1, 1, 5, 0, 0], np.uint8)
    wb = np.array([7, 0, 7, 7, 7], np.uint8)              # only connection 0 is a deflate-taking member
    assert bad(conn_ext=ext, window_bits=wb, windows=True) == 1
    assert bad(conn_ext=ext, window_bits=wb) == 0         # the plan reads no windows


def one_room_of_three():
    d = mm.Decoded([[(1, 0, B, b"a")], [(1, 0, B, b"bb")], [(1, 0, B, b"ccc")]])
    t = rm.tables_of(d)
    rooms = ro.csr_of([0, 0, 0])
    return d, t, rooms


def test_one_room_of_three_is_nine_entries():
    d, t, rooms = one_room_of_three()
    ch = ro.chain_model(d, t, None, None, rooms)
    rep = ch["rep"]
    assert rep["plain_of"].tolist() == [0, 1, 2] and rep["def_of"].tolist() == [-1, -1, -1]
    assert rep["plain_conn"].tolist() == [0, 1, 2] and rep["plain"]["payload_len"].tolist() == [1, 2, 3]
    assert [w[1:] for w in ch["wires"]] == [(3, 12), (0, 0), (0, 0)] and ch["wires"][0][0].tolist() == [0, 3, 7]
    p = ro.plan_of_chain(d, t, ch, None, rooms)
    assert p["summary"] == dict(frames=9, payload_bytes=36, payload_len=0, errors=0, status=0)
    assert [tuple(int(x) for x in e) for e in p["send"]] == [
        (0, 3, 0, 0, 0), (3, 4, 1, 0, 0), (7, 5, 2, 0, 0),
        (0, 3, 0, 1, 0), (3, 4, 1, 1, 0), (7, 5, 2, 1, 0),
        (0, 3, 0, 2, 0), (3, 4, 1, 2, 0), (7, 5, 2, 2, 0)]   # (off, len, frame, conn, wire)
    assert [(int(c["first"]), int(c["count"]), int(c["bytes"])) for c in p["conn_send"]] == [
        (0, 3, 12), (3, 3, 12), (6, 3, 12)]


def test_one_room_of_three_without_the_sender_is_six():
    d, t, rooms = one_room_of_three()
    ch = ro.chain_model(d, t, None, None, rooms, ro.SKIP_SENDER)
    assert ch["rep"]["plain_of"].tolist() == [0, 1, 2]
    p = ro.plan_of_chain(d, t, ch, None, rooms, ro.SKIP_SENDER)
    assert p["summary"] == dict(frames=6, payload_bytes=24, payload_len=0, errors=0, status=0)
    assert [tuple(int(x) for x in e) for e in p["send"]] == [
        (3, 4, 1, 0, 0), (7, 5, 2, 0, 0),
        (0, 3, 0, 1, 0), (7, 5, 2, 1, 0),
        (0, 3, 0, 2, 0), (3, 4, 1, 2, 0)]
    assert [(int(c["first"]), int(c["count"]), int(c["bytes"])) for c in p["conn_send"]] == [
        (0, 2, 9), (2, 2, 8), (4, 2, 7)]
    # one entry short: the need, nothing else
    short = ro.plan_of_chain(d, t, ch, None, rooms, ro.SKIP_SENDER, max_sends=5)
    assert short["send"] is None and short["summary"]["frames"] == 6 and short["summary"]["status"] == ro.ERR_CAPACITY


def test_kinds_lists_and_windows():
    """A plain member, a deflate member and a deflate + takeover member in one
    room; a loner in a room of its own; a connection in no room."""
    D, TK = ro.EXT_DEFLATE, ro.EXT_DEFLATE | ro.EXT_SERVER_TAKEOVER
    conns = [[(1, 0, B, b"p")], [(1, 0, B, b"dd")], [(1, 0, B, b"ttt")], [(1, 0, B, b"solo")], [(1, 0, B, b"none")]]
    d = mm.Decoded(conns)
    t = rm.tables_of(d)
    ext = np.array([0, D, TK, D, D], np.uint8)
    wb = np.array([9, 12, 8, 0, 10], np.uint8)   # only deflate-taking members count: 12 in room 0, 15 in room 1
    rooms = ro.csr_of([0, 0, 0, 1, NONE])
    rep = ro.reply_rooms_model(t["bodies"], jm.HANDLER_ECHO_TEXT, ext, wb, 5, rooms)
    assert rep["plain_of"].tolist() == [0, 1, 2, -1, -1] and rep["def_of"].tolist() == [0, 1, 2, 3, -1]
    assert rep["def_msgs"]["window_bits"].tolist() == [12, 12, 12, 15] and rep["def_conn"].tolist() == [0, 1, 2, 3]
    assert set(rep["def_msgs"]["opcode"].tolist()) == {1}
    skip = ro.reply_rooms_model(t["bodies"], jm.HANDLER_ECHO_TEXT, ext, wb, 5, rooms, ro.SKIP_SENDER)
    # without its sender, the deflate member's message has no deflate recipient, the loner's none at all
    assert skip["plain_of"].tolist() == [0, 1, 2, -1, -1] and skip["def_of"].tolist() == [0, -1, 1, -1, -1]
    assert skip["def_msgs"]["window_bits"].tolist() == [12, 12]   # the sender counts even when skipped
    ch = ro.chain_model(d, t, ext, wb, rooms, policy=jm.HANDLER_ECHO_TEXT)
    p = ro.plan_of_chain(d, t, ch, ext, rooms)
    assert [(int(e["frame"]), int(e["conn"]), int(e["wire"])) for e in p["send"]] == [
        (0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 1), (1, 1, 1), (2, 1, 1), (0, 2, 0), (1, 2, 0), (2, 2, 0), (3, 3, 1)]
    assert [int(c["count"]) for c in p["conn_send"]] == [3, 3, 3, 1, 0]
