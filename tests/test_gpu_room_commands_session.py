"""Whole sessions in which membership moves only by what clients send: 300
connections, 7 rooms, 4 passes cut at any byte, Engine.broadcast(commands=True)
and Rooms.update(changes=res.room_changes, closed=res) between the passes
(tests/_room_commands_model.py on the harness of tests/_session.py).  The check
is the client's: what each recipient is sent per pass is the contract's view,
the room table behind every pass is the contract's, and no command text reaches
anybody.  The traffic's coverage is pinned on the CPU
(tests/test_room_commands_model.py)."""
from collections import Counter

import numpy as np
import pytest

import gev_amd
from tests import _room_commands_model as cm
from tests import _session as s

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags,F", ((0, None), (gev_amd.ROOMS_SKIP_SENDER, 1000)), ids=["all", "skip-sender-1000"])
def test_command_session(engine, flags, F):
    case = cm.command_case()
    n = len(case.conns)
    views, tables, tally = cm.command_view(case, flags)
    assert all(tally[k] > 0 for k in cm.COVERAGE), tally
    run = cm.run_command_session(engine, case, F, rooms_flags=flags)
    replies = Counter()
    cm.check_command_session(case, views, run.sent, F, replies)
    print("replies:", dict(replies), "cases:", {k: tally[k] for k in cm.COVERAGE})
    assert all(replies[k] > 0 for k in ("echo plain", "echo deflated", "pong", "close reply", "1007"))
    for p in range(case.passes):
        assert run.gathered[p] == run.sent[p], p
    # the room table behind every pass, and its CSR inverse
    for p in range(case.passes):
        conn_room, first, members = run.room_tables[p]
        assert conn_room.tolist() == tables[p].tolist(), p
        want_first, want_members, _ = gev_amd.Rooms.csr(tables[p], case.n_rooms)
        assert first.tolist() == want_first.tolist() and members.tolist() == want_members.tolist(), p
    # the change records are in message order, and every stripped body says so
    stripped = 0
    for p in range(case.passes):
        ch = run.changes[p]
        assert np.all(np.diff(ch["conn"].astype(np.int64)) >= 0), p
        assert np.all((ch["room"] < case.n_rooms) | (ch["room"] == gev_amd.ROOM_NONE)), p
        b = run.bodies[p]
        cmds = b["status"] == gev_amd.MSG_COMMAND
        assert not b["flags"][cmds].any() and not b["length"][cmds].any() and np.all(b["opcode"][cmds] == 1)
        stripped += int(cmds.sum())
    assert stripped == tally["commands"] and sum(len(c) for c in run.changes) == stripped - tally["a rejected join"]
    # the closes: nothing in later passes, and no room
    closers = {c for c in range(n) if case.conns[c].dead_at is not None}
    assert set(run.shutdown_pass) == closers
    for c, p0 in run.shutdown_pass.items():
        assert all(run.sent[p][c] == b"" for p in range(p0 + 1, case.passes)), c
        assert all(run.room_tables[p][0][c] == gev_amd.ROOM_NONE for p in range(p0, case.passes)), c


def test_without_commands_the_same_traffic_is_broadcast_as_before(engine):
    """commands=False: broadcast gives today's bytes -- command text is
    ordinary text and goes to the room, and nobody moves but the closed."""
    case = cm.command_case()
    bc = cm.as_broadcast(case)
    run = cm.run_command_session(engine, case, None, commands=False)
    views, tables = s.broadcast_view(bc, 0)
    for r in range(len(case.conns)):
        s.check_broadcast_conn(bc, views, r, [run.sent[p][r] for p in range(case.passes)], None)
    for p in range(case.passes):
        assert run.room_tables[p][0].tolist() == tables[p].tolist(), p
        assert not (run.bodies[p]["status"] == gev_amd.MSG_COMMAND).any()
    got = [d for p in range(case.passes) for r in range(len(case.conns))
           for d in cm.received_messages(case.conns[r], run.sent[p][r], None)]
    assert sum(1 for d in got if cm.parse(d, case.n_rooms)[0] != cm.NONE and d not in cm.BINARY_LOOKALIKES) > 100
    # the very bytes of the existing session driver on this traffic
    base = s.run_session(engine, bc.conns, bc.cuts, bc.passes, None, rooms=gev_amd.Rooms.build(engine, bc.rooms0, bc.n_rooms),
                         changes=bc.changes)
    assert base.sent == run.sent
