"""Session tests of the whole message chain on the device, from the client's
side: decode -> messages -> inflate -> join(carry) -> control -> reply /
reply_rooms -> deflate -> fragment -> encodes -> plan / room plan -> gather,
with Rooms.update between passes, over many passes of byte streams cut at any
byte.  However a connection's stream is cut into passes, the peer receives the
same thing: what tests/_session.py's host-side reading of RFC 6455 / RFC 7692
and include/gevws.h says it should (tests/test_session_model.py pins that
checker and the inputs on the CPU)."""
from collections import Counter

import numpy as np
import pytest

import gev_amd
from tests import _session as s
from tests._session import CT, ST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def echo_runs():
    return {}


def echo_run(engine, runs, passes, F, deflate_flags=0):
    key = (passes, F, deflate_flags)
    if key not in runs:
        runs[key] = s.run_session(engine, s.echo_conns(), s.echo_cuts(passes)[0], passes, F,
                                  deflate_flags=deflate_flags)
    return runs[key]


def round16(n: int) -> int:
    return (n + 15) // 16 * 16


@pytest.mark.parametrize("passes,F", s.CUTTINGS, ids=["%d-%s" % c for c in s.CUTTINGS])
def test_echo_session(engine, echo_runs, passes, F):
    check_echo_session(engine, echo_runs, passes, F)


def test_echo_session_dynamic_huffman(engine, echo_runs):
    """The three-pass cutting once more with GEVWS_DEFLATE_DYNAMIC in the deflate step's flags."""
    check_echo_session(engine, echo_runs, 3, None, gev_amd.DEFLATE_DYNAMIC)


def check_echo_session(engine, echo_runs, passes, F, deflate_flags=0):
    """320 connections of every extension class, about twenty of them heavy
    (tests/_session.py heavy_conns), echoed over `passes` passes.

    Two readings of the issue's end-of-session conditions, both forced by the
    contract: a connection that was shut down is fed nothing afterwards (DESIGN
    section 8 item 8), so what it left open -- the carry of a message a close
    frame interrupted, its message state, an inflate window that the one-pass
    run moved on over frames behind the close -- is the host's to drop and is
    not compared; every other connection is held to all of them."""
    conns = s.echo_conns()
    n = len(conns)
    run = echo_run(engine, echo_runs, passes, F, deflate_flags)
    # (a) per connection, everything it was sent over the session is the expected peer view
    tally, checked = Counter(), 0
    for c, conn in enumerate(conns):
        try:
            s.check_echo_conn(conn, run.wire(c), F, tally)
        except s.CheckError as e:
            raise AssertionError("connection %d (%s, ext %d): %s" % (c, conn.heavy or "light", conn.ext, e)) from None
        checked += 1
    assert checked == n                                      # the share left out is 0
    print("replies:", dict(tally))
    assert all(tally[k] > 0 for k in s.REPLY_KINDS), tally
    assert tally["needs the window"] > 0
    # (b) per pass, the gather is the plan's entries
    for p in range(passes):
        assert run.gathered[p] == run.sent[p], p
    # the host's view of the session: every live connection was read to its end, the others up to their cut
    for c, conn in enumerate(conns):
        if conn.dead_at is None:
            assert c not in run.shutdown_pass and run.consumed[c] == len(conn.wire) and not run.leftover[c], c
        else:
            assert c in run.shutdown_pass and run.consumed[c] >= conn.frame_end(conn.dead_at), c
    # (c) without a limit the bytes do not depend on the cutting
    base = echo_run(engine, echo_runs, 1, None, deflate_flags)
    live_ct = [c for c in range(n) if conns[c].ext & CT and conns[c].dead_at is None]
    assert len(live_ct) > 20
    if F is None:
        for c in range(n):
            assert run.wire(c) == base.wire(c), (c, conns[c].heavy)
    # (d) the end of the session
    recs = run.carries[-1]
    live = np.array([conns[c].dead_at is None for c in range(n)])
    assert not recs[live].view(np.uint8).any()
    still = recs[recs["flags"] & gev_amd.CARRY_OPEN != 0]
    assert run.carry_used[-1] == sum(round16(int(x)) for x in still["length"])
    print("carry records a shut-down connection left open:", len(still))
    if passes >= 3:     # the close between two fragments, cut off from the message's end: the record stays
        assert len(still) >= 1
    on_edge = [c for c in range(n) if live[c] and not (conns[c].info and conns[c].info[-1][0])]
    assert len(on_edge) > 250 and not run.state[on_edge].any()
    for c, conn in enumerate(conns):
        if conn.ext & ST:
            host_ctx = bytearray(gev_amd.DEF_CTX_BYTES)
            for k, x in conn.expected():
                if k == "echo":
                    gev_amd.deflate_raw_ctx(x, host_ctx, window_bits=conn.window_bits, flags=deflate_flags)
            assert run.def_ctx[c].tobytes() == bytes(host_ctx), (c, conn.heavy)
        else:
            assert not run.def_ctx[c].any(), c
    assert np.array_equal(run.inf_ctx[live_ct], base.inf_ctx[live_ct])
    assert run.inf_ctx[live_ct].any(axis=1).sum() > 10
    # what keeps the run from passing vacuously, from its own records
    if passes > 1:
        seen = s.observed_carries(run, conns, run.cuts, passes)
        print("carries:", dict(seen))
        assert all(seen[k] > 0 for k in s.CARRY_KINDS), seen
        assert seen == s.predicted_carries(conns, run.cuts, passes)


LEAD_BYTES = (1 << 32) + 4096


@pytest.mark.parametrize("F", (None, 1000), ids=["None", "1000"])
def test_echo_session_behind_a_payload_arena_past_4gib(engine, echo_runs, F):
    """The one-pass echo session once more with every payload offset, body
    offset and aux offset above 2^32: a leading connection holds one frame of
    2^32 + 4096 payload bytes with a reserved opcode (s.run_far_session), the
    320 connections follow it.  Whatever an offset cut to 32 bits would read
    is the 0xA5 fill of the frame's first MiB."""
    import torch
    free, _ = torch.cuda.mem_get_info(engine.device)
    if free < 12 << 30:
        pytest.skip(f"the far arena needs about 9 GiB of device memory, {free / 2**30:.1f} GiB are free")
    conns = s.echo_conns()
    n = len(conns)
    run = s.run_far_session(engine, conns, LEAD_BYTES, F)
    print("far session: %.2f s" % run.seconds)
    # the offsets really are far: the decode's arena, every record behind the leading frame, the aux region
    lead16 = (LEAD_BYTES + 15) // 16 * 16
    assert int(run.decode_summary["payload_bytes"]) > 1 << 32
    assert int(run.first_frame[1]) == 1 and int(run.payload_off[0]) == 0
    assert int(run.payload_off[1:].min()) == lead16 >= 1 << 32
    assert run.aux_off >= 1 << 32
    # the client's view: every connection is sent what the checker expects
    tally, checked = Counter(), 0
    for c, conn in enumerate(conns):
        try:
            s.check_echo_conn(conn, run.sent[c + 1], F, tally)
        except s.CheckError as e:
            raise AssertionError("connection %d (%s, ext %d): %s" % (c, conn.heavy or "light", conn.ext, e)) from None
        checked += 1
    assert checked == n == 320                                # the share left out is 0
    assert all(tally[k] > 0 for k in s.REPLY_KINDS), tally
    assert tally["needs the window"] > 0
    assert run.gathered == run.sent                           # the gather is the plan's entries
    # the leading connection: a reserved opcode is a protocol error
    assert run.sent[0] == bytes.fromhex("880203ea")
    assert int(run.conn_flags[0]) & (gev_amd.CTL_SHUTDOWN | gev_amd.CTL_FAILED) == gev_amd.CTL_SHUTDOWN | gev_amd.CTL_FAILED
    for c, conn in enumerate(conns):
        assert bool(int(run.conn_flags[c + 1]) & gev_amd.CTL_SHUTDOWN) == (conn.dead_at is not None), c
    # without a limit the bytes do not depend on the arena's layout: the same session without the leading frame
    if F is None:
        base = echo_run(engine, echo_runs, 1, None)
        for c in range(n):
            assert run.sent[c + 1] == base.wire(c), (c, conns[c].heavy)
    # the join without GEVWS_JOIN_ALL leaves single-frame plain bodies in the far arena: the same bytes there
    b0, b1 = run.bodies_in_place, run.bodies_copied
    whole = b1["flags"] & gev_amd.BODY_WHOLE != 0
    assert np.array_equal(b0["flags"] & gev_amd.BODY_WHOLE != 0, whole) and whole.sum() > 300
    assert np.array_equal(b0["length"], b1["length"]) and np.array_equal(b0["conn"], b1["conn"])
    placed = whole & (b0["flags"] & (gev_amd.BODY_JOINED | gev_amd.BODY_INFLATED) == 0)
    assert placed.sum() > 50 and int(b0["off"][placed & (b0["length"] > 0)].min()) >= 1 << 32
    assert np.all(b1["flags"][whole] & (gev_amd.BODY_JOINED | gev_amd.BODY_INFLATED) != 0)
    assert all(a == b for a, b in run.body_bytes)
    assert sum(len(a) for a, _ in run.body_bytes) > 50000
    del run
    torch.cuda.empty_cache()


def test_echo_session_cuts_everywhere(engine, echo_runs):
    """Over the cuttings that ran, a pass boundary fell in every place a frame has."""
    classes = Counter()
    for passes, F in s.CUTTINGS:
        run = echo_run(engine, echo_runs, passes, F)
        for conn, mine in zip(s.echo_conns(), run.cuts):
            for off in mine:
                classes.update(s.cut_classes(conn, off) & set(s.CUT_CLASSES))
    assert all(classes[k] > 0 for k in s.CUT_CLASSES), classes


@pytest.mark.parametrize("flags,F", ((0, None), (gev_amd.ROOMS_SKIP_SENDER, 1000)), ids=["all", "skip-sender-1000"])
def test_broadcast_session(engine, flags, F):
    """300 connections in 7 rooms (some in none) over 4 passes cut at any byte,
    with join / move / leave records and the passes' closes applied by
    Rooms.update between them: every recipient is sent, pass by pass, what the
    contract of gevws_reply_rooms_async / gevws_room_plan_async gives it."""
    case = s.broadcast_case()
    n = len(case.conns)
    rooms = gev_amd.Rooms.build(engine, case.rooms0, case.n_rooms)
    run = s.run_session(engine, case.conns, case.cuts, case.passes, F, rooms=rooms, changes=case.changes,
                        rooms_flags=flags)
    views, tables = s.broadcast_view(case, flags)
    tally = Counter()
    for r in range(n):
        s.check_broadcast_conn(case, views, r, [run.sent[p][r] for p in range(case.passes)], F, tally)
    print("replies:", dict(tally))
    assert all(tally[k] > 0 for k in ("echo plain", "echo deflated", "pong", "ping for pong", "close reply", "1007"))
    for p in range(case.passes):
        assert run.gathered[p] == run.sent[p], p
    # the closes: two close frames and a failure, nothing for them in later passes, and no room
    closers = {c for c in range(n) if case.conns[c].dead_at is not None}
    assert set(run.shutdown_pass) == closers and len(closers) == 3
    assert min(run.shutdown_pass.values()) < case.passes - 1
    for c, p0 in run.shutdown_pass.items():
        assert all(run.sent[p][c] == b"" for p in range(p0 + 1, case.passes)), c
        assert all(run.room_tables[p][0][c] == gev_amd.ROOM_NONE for p in range(p0, case.passes)), c
    # the tables behind every pass are the contract's
    for p in range(case.passes):
        conn_room, first, members = run.room_tables[p]
        assert conn_room.tolist() == tables[p].tolist(), p
        want_first, want_members, _ = gev_amd.Rooms.csr(tables[p], case.n_rooms)
        assert first.tolist() == want_first.tolist() and members.tolist() == want_members.tolist(), p
    # both carries were open behind some pass: the two long messages arrive over several
    seen = s.observed_carries(run, case.conns, case.cuts, case.passes)
    assert seen["plain"] > 0 and seen["compressed"] > 0, seen
    assert seen == s.predicted_carries(case.conns, case.cuts, case.passes)
    # a server-takeover member was sent a room's publication uncompressed
    assert any(case.conns[r].ext & ST and any(k == "echo" for k, _ in views[p][r])
               for p in range(case.passes) for r in range(n))
