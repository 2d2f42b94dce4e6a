"""The membership update's model (tests/_rooms_update_model.py) pinned on the
CPU: its tables are well formed by the room calls' own rule
(tests/_rooms_model.check_tables) over random sequences of updates, and
last-wins, close-beats-join, the gates, the counts and the bad records hold on
hand-written cases."""
import numpy as np

from tests import _rooms_model as ro
from tests import _rooms_update_model as um

NONE = um.ROOM_NONE
S, F = um.CTL_SHUTDOWN, um.CTL_FAILED


def tables(r):
    return r["conn_room"], r["first"], r["members"]


def summary(r):
    return tuple(r["summary"][k] for k in ("frames", "payload_bytes", "payload_len", "errors", "status"))


def test_random_sequences_stay_well_formed():
    rng = np.random.default_rng(0x72753031)
    for n_conns, n_rooms in ((0, 0), (1, 1), (37, 5), (300, 2), (300, 700)):
        cr = np.full(n_conns, NONE, np.uint32)
        for step in range(8):
            k = int(rng.integers(0, 2 * n_conns + 1)) if n_rooms else 0
            conns = rng.integers(0, max(n_conns, 1), k)
            rooms = rng.integers(0, max(n_rooms, 1), k).astype(np.uint32)
            rooms[rng.random(k) < 0.2] = NONE
            flags = None
            if step % 2:
                flags = (rng.random(n_conns) < 0.05).astype(np.uint32) * rng.choice([S, S | F], n_conns)
            if step == 5:
                n_rooms += 3   # the room space grows
            r = um.update_model(cr, n_rooms, um.changes_np(list(zip(conns.tolist(), rooms.tolist()))),
                                conn_flags=flags)
            assert r["summary"]["status"] == 0 and r["summary"]["errors"] == 0
            assert ro.check_tables(tables(r), n_conns) == 0, (n_conns, n_rooms, step)
            assert r["first"].size == n_rooms + 1 and r["summary"]["frames"] == r["members"].size
            assert r["summary"]["frames"] == np.count_nonzero(r["conn_room"] != NONE)
            assert r["summary"]["payload_len"] == np.count_nonzero(r["conn_room"] != cr)
            assert r["summary"]["payload_bytes"] == k
            if flags is not None:
                assert np.all(r["conn_room"][(flags & S) != 0] == NONE)
            cr = r["conn_room"]


def test_the_last_change_wins():
    cr = np.array([0, 1, NONE, 2], np.uint32)
    ch = um.changes_np([(0, 2), (2, 1), (0, NONE), (0, 1), (3, 2), (1, NONE), (2, 0)])
    r = um.update_model(cr, 3, ch)
    assert r["conn_room"].tolist() == [1, NONE, 0, 2]
    assert r["first"].tolist() == [0, 1, 2, 3] and r["members"].tolist() == [2, 0, 3]
    # join (2), move (0), leave (1); connection 3's change names the room it holds: not moved
    assert summary(r) == (3, 7, 3, 0, 0)
    # the count cuts the list: max_changes, or the gate's frames when that is smaller
    assert um.update_model(cr, 3, ch, max_changes=3)["conn_room"].tolist() == [NONE, 1, 1, 2]
    r = um.update_model(cr, 3, ch, max_changes=6, prev=dict(frames=1, status=0))
    assert r["conn_room"].tolist() == [2, 1, NONE, 2] and summary(r) == (3, 1, 1, 0, 0)
    r = um.update_model(cr, 3, ch, max_changes=2, prev=dict(frames=100, status=0))
    assert summary(r) == (4, 2, 2, 0, 0)
    # no list: a pure build, the twin of Rooms.csr
    r = um.update_model(cr, 3)
    assert r["conn_room"].tolist() == cr.tolist() and r["members"].tolist() == [0, 1, 3]
    assert summary(r) == (3, 0, 0, 0, 0)


def test_a_close_beats_a_join():
    cr = np.array([0, 0, 1, NONE, 1], np.uint32)
    ch = um.changes_np([(3, 1), (1, 1), (0, 1)])
    r = um.update_model(cr, 2, ch, conn_flags=[0, S, S | F, S, F])   # FAILED alone is no close
    assert r["conn_room"].tolist() == [1, NONE, NONE, NONE, 1]
    assert r["first"].tolist() == [0, 0, 2] and r["members"].tolist() == [0, 4]
    assert summary(r) == (2, 3, 3, 0, 0)   # 0 moved, 1 and 2 closed; 3 had no room before and has none after
    # closes alone: nothing uploaded
    r = um.update_model(cr, 2, None, conn_flags=[S, 0, 0, 0, 0])
    assert r["conn_room"].tolist() == [NONE, 0, 1, NONE, 1] and summary(r) == (3, 0, 1, 0, 0)


def test_gates_copy_the_status_and_nothing_else():
    cr = np.array([0, 1], np.uint32)
    ch = um.changes_np([(0, 1)])
    for kw in (dict(prev=dict(frames=1, status=ro.ERR_CAPACITY)), dict(plan=dict(status=ro.ERR_INVALID)),
               dict(prev=dict(frames=1, status=ro.ERR_CAPACITY), plan=dict(status=ro.ERR_INVALID))):
        r = um.update_model(cr, 2, ch, conn_flags=[S, 0], **kw)
        first = kw.get("prev", kw.get("plan"))["status"]
        assert summary(r) == (0, 0, 0, 0, first) and r["conn_room"] is None and r["members"] is None


def test_bad_records_are_counted_one_each():
    cr = np.array([0, 1, NONE], np.uint32)
    assert summary(um.update_model(cr, 2, um.changes_np([(3, 0)]))) == (0, 0, 0, 1, um.ERR_INVALID)
    assert summary(um.update_model(cr, 2, um.changes_np([(0, 2)]))) == (0, 0, 0, 1, um.ERR_INVALID)
    assert summary(um.update_model(cr, 1)) == (0, 0, 0, 1, um.ERR_INVALID)          # in[1] == n_rooms
    # a record counts once, whatever is wrong with it; a change that overwrites a bad room does not mend it
    r = um.update_model(np.array([0, 5, NONE, 7], np.uint32), 2, um.changes_np([(9, 9), (1, 0), (0, 2), (2, 1)]))
    assert summary(r) == (0, 0, 0, 4, um.ERR_INVALID) and r["first"] is None
    # a bad record behind the count is not read
    assert summary(um.update_model(cr, 2, um.changes_np([(0, 1), (3, 0)]), max_changes=1)) == (2, 1, 1, 0, 0)
