"""The room-command rule and the command session, pinned on the CPU.

gev_amd.room_command_parse (the host twin of the device rule,
gev_amd/csrc/gevws_room_command.hpp) against tests/_room_commands_model.parse on
every edge the contract names; the step's table model on a hand-made batch; and
the command session's traffic: it holds every case the GPU session test is for,
and the checker accepts a correct host server and rejects one that lets a
command through or ignores one."""
from collections import Counter

import numpy as np
import pytest

import gev_amd
from tests import _room_commands_model as cm
from tests import _session as s

N_ROOMS_ALL = (0, 1, 10, 2 ** 32 - 1)


def both(body: bytes, n_rooms: int):
    want = cm.parse(body, n_rooms)
    got = gev_amd.room_command_parse(body, n_rooms)
    assert got == want, (body, n_rooms, got, want)
    assert want[1] == cm.ROOM_NONE or want[0] == cm.CHANGE
    return want


# ---------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("n_rooms", N_ROOMS_ALL)
def test_every_prefix_length(n_rooms):
    """Every length 0..17 of both keywords' prefixes, the text continued with
    digits, spaces and the keyword itself."""
    for full in (b"/leave" + b"0" * 11, b"/leave" + b" " * 11, b"/leave/leave/leave", b"/join " + b"0" * 11,
                 b"/join 12345678901", b"/join /join /join", b"/join 4294967294  "):
        for k in range(18):
            both(full[:k], n_rooms)
    assert both(b"/leave", 0) == (cm.CHANGE, cm.ROOM_NONE)
    assert both(b"/join ", 10) == (cm.NONE, cm.ROOM_NONE) and both(b"/join", 10) == (cm.NONE, cm.ROOM_NONE)
    assert both(b"/join 0", 0) == (cm.REJECTED, cm.ROOM_NONE) and both(b"/join 0", 1) == (cm.CHANGE, 0)


@pytest.mark.parametrize("text", (b"/leave", b"/join 0", b"/join 4294967295"))
def test_every_single_byte_mutation(text):
    changed = 0
    for n_rooms in (1, 2 ** 32 - 1):
        base = both(text, n_rooms)
        for i in range(len(text)):
            for v in range(256):
                if v == text[i]:
                    continue
                got = both(text[:i] + bytes([v]) + text[i + 1:], n_rooms)
                if i < 6:
                    assert got[0] == cm.NONE, (text, i, v)      # the keyword is exact
                changed += got != base
    assert changed > 0


def test_values_around_n_rooms():
    for n_rooms in N_ROOMS_ALL:
        for v in {0, 1, 9, 10, 11, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, max(n_rooms - 1, 0), n_rooms, n_rooms + 1}:
            text = b"/join %d" % v
            if len(text) > 16:
                continue
            want = both(text, n_rooms)
            assert want == ((cm.CHANGE, v) if v < n_rooms else (cm.REJECTED, cm.ROOM_NONE)), (v, n_rooms)
    assert both(b"/join 4294967295", 2 ** 32 - 1)[0] == cm.REJECTED      # GEVWS_ROOM_NONE is never a room
    assert both(b"/join 4294967294", 2 ** 32 - 1) == (cm.CHANGE, 2 ** 32 - 2)


def test_ten_digits_above_2_32():
    """The value is taken in 64 bits: ten digits never wrap into a small room."""
    for v in (2 ** 32, 2 ** 32 + 1, 2 ** 32 + 5, 4294967306, 8589934592, 8589934593, 9999999999):
        for n_rooms in (2, 11, 2 ** 32 - 1):
            assert both(b"/join %d" % v, n_rooms) == (cm.REJECTED, cm.ROOM_NONE), v
    assert both(b"/join 10000000000", 2 ** 32 - 1)[0] == cm.NONE          # eleven digits: 17 bytes, no command


def test_leading_zeros():
    assert both(b"/join 0000000009", 10) == (cm.CHANGE, 9)
    assert both(b"/join 0000000010", 10) == (cm.REJECTED, cm.ROOM_NONE)
    assert both(b"/join 00", 1) == (cm.CHANGE, 0) and both(b"/join 007", 8) == (cm.CHANGE, 7)
    assert both(b"/join 0000000000", 1) == (cm.CHANGE, 0)


def test_pad_bytes_behind_the_length_do_not_count():
    """The host twin reads body[0, length) alone; the same bytes with digits
    behind them are another, longer body."""
    import ctypes
    for text, n_rooms in ((b"/join 1", 2000), (b"/leave", 3), (b"/join ", 10), (b"/join 12", 13)):
        buf = text + b"234567890123"
        room = ctypes.c_uint32(7)
        got = gev_amd.lib.gevws_room_command_parse(ctypes.c_char_p(buf), len(text), n_rooms, ctypes.byref(room))
        assert (got, room.value) == cm.parse(text, n_rooms), text
    assert both(b"/join 1234", 2000) == (cm.CHANGE, 1234)
    # lengths outside 6..16 read nothing, not even a NULL body; a NULL room is allowed
    fn = gev_amd.lib.gevws_room_command_parse
    assert fn(None, 0, 5, None) == 0 and fn(None, 5, 5, None) == 0 and fn(None, 17, 5, None) == 0
    assert fn(None, 6, 5, None) == gev_amd.ERR_INVALID and fn(ctypes.c_char_p(b"/leave"), 6, 5, None) == 1


def test_random_bodies_agree():
    rng = np.random.default_rng(0xC0DE)
    alphabet = np.frombuffer(b"/joinleave 0123456789\nJ", np.uint8)
    hits = Counter()
    for _ in range(20000):
        k = int(rng.integers(0, 19))
        body = bytes(rng.choice(alphabet, k)) if rng.random() < 0.5 else (
            (b"/join " if rng.random() < 0.7 else b"/leave") + bytes(rng.choice(alphabet[11:], k)))[:18]
        hits[both(body, int(rng.choice([0, 1, 10, 1000, 2 ** 32 - 1])))[0]] += 1
    assert all(hits[k] > 50 for k in (cm.NONE, cm.CHANGE, cm.REJECTED)), hits


# ---------------------------------------------------------------------------- the step's model
def test_step_model_on_a_hand_made_batch():
    n_rooms = 12
    pal = cm.palette(n_rooms)
    bodies, out = cm.batch_of([e[1:] for e in pal], np.arange(len(pal)) // 3)
    want = cm.commands_model(bodies, out, out.size, 100, n_rooms)
    names = [e[0] for e in pal]
    of = dict(zip(names, want["change_of"].tolist()))
    accepted = [k for k in names if k.startswith(("join", "leave"))]
    assert [of[k] for k in accepted] == list(range(len(accepted))) and len(accepted) == 8
    assert all(of[k] == cm.OF_REJECTED for k in names if k.startswith("rejected"))
    assert all(of[k] == cm.OF_NONE for k in names if not k.startswith(("join", "leave", "rejected")))
    ch = dict(zip(accepted, want["changes"]["room"].tolist()))
    assert ch["join, digits in the pad"] == 1 and ch["leave, digits in the pad"] == cm.ROOM_NONE
    assert ch["join the last room"] == 11 and ch["join, leading zeros"] == 1
    assert want["summary"] == dict(frames=8, payload_bytes=4, payload_len=12, errors=0, status=0)
    new = want["bodies"]
    for m, k in enumerate(names):
        if of[k] == cm.OF_NONE:
            assert new[m].tobytes() == bodies[m].tobytes(), k
        else:
            assert (int(new[m]["off"]), int(new[m]["length"]), int(new[m]["flags"]), int(new[m]["status"])) == (
                0, 0, 0, cm.MSG_COMMAND), k
            assert new[m]["conn"] == bodies[m]["conn"] and new[m]["opcode"] == 1 and np.all(new[m]["reserved"] == 0xC3)
    # capacity, gates, malformed records
    cap = cm.commands_model(bodies, out, out.size, 100, n_rooms, max_changes=7)
    assert cap["summary"] == dict(cm.zero_summary(), frames=8, status=cm.ERR_CAPACITY) and cap["bodies"] is None
    for kw in (dict(join_status=-2), dict(ctl_status=-2), dict(msg=dict(frames=5, status=-3)),
               dict(msg=dict(frames=0, status=0)), dict(max_messages=0)):
        assert cm.commands_model(bodies, out, out.size, 100, n_rooms, **kw)["summary"] == cm.zero_summary(), kw
    bad = cm.commands_model(bodies, out, out.size, 3, n_rooms)     # conn >= 3 on the delivered bodies behind the ninth
    assert bad["summary"]["status"] == cm.ERR_INVALID and bad["summary"]["errors"] > 0 and bad["changes"] is None


# ---------------------------------------------------------------------------- the command session's traffic
def test_command_traffic_holds_its_cases():
    case = cm.command_case()
    assert len(case.conns) == 300 and case.n_rooms == 7 and case.passes == 4
    for flags in (0, s.SKIP_SENDER):
        views, tables, tally = cm.command_view(case, flags)
        assert all(tally[k] > 0 for k in cm.COVERAGE), {k: tally[k] for k in cm.COVERAGE}
        assert tally["commands"] > 60
    # membership moves by commands alone, and it does move
    moved = [int(np.count_nonzero(tables[p] != (tables[p - 1] if p else case.rooms0))) for p in range(case.passes)]
    assert sum(moved) > 30 and sum(1 for m in moved if m) >= 3, moved
    closers = [c for c, conn in enumerate(case.conns) if conn.dead_at is not None]
    assert len(closers) >= 5 and all(tables[-1][c] == cm.ROOM_NONE for c in closers)
    # the scripted connections end where their names say
    at = {conn.heavy[5:]: c for c, conn in enumerate(case.conns) if conn.heavy.startswith("cmd: ")}
    last = tables[-1]
    want = {"join, then publish": 3, "move": 2, "leave": cm.ROOM_NONE, "rejected": 5, "1-byte fragments": 6,
            "cut between fragments": 1, "cut inside a frame": cm.ROOM_NONE, "compressed": 5,
            "compressed, client takeover": cm.ROOM_NONE, "near misses": 6, "behind a close": cm.ROOM_NONE,
            "in front of a close": cm.ROOM_NONE, "two commands disagree": 2, "join, then leave": cm.ROOM_NONE}
    assert {k: int(last[at[k]]) for k in want} == want
    assert int(tables[0][at["cut between fragments"]]) == 0 and int(tables[1][at["cut between fragments"]]) == 1
    assert int(tables[0][at["cut inside a frame"]]) == 2 and int(tables[1][at["cut inside a frame"]]) == cm.ROOM_NONE
    assert int(tables[0][at["two commands disagree"]]) == 2
    # without the command step the same traffic broadcasts the command text
    plain_views, _ = s.broadcast_view(cm.as_broadcast(case), 0)
    assert any(cm.parse(x, 7)[0] != cm.NONE for view in plain_views for v in view for k, x in v if k == "echo")
    through = {x for view in views for v in view for k, x in v if k == "echo" and cm.parse(x, 7)[0] != cm.NONE}
    assert through == set(cm.BINARY_LOOKALIKES)          # binary messages of a command's bytes, and nothing else


@pytest.mark.parametrize("flags,F", ((0, None), (s.SKIP_SENDER, 1000)))
def test_checker_accepts_the_reference_command_server(flags, F):
    case = cm.command_case()
    views, _, _ = cm.command_view(case, flags)
    sent = cm.reference_command_server(case, flags, F)
    tally = Counter()
    cm.check_command_session(case, views, sent, F, tally)
    assert all(tally[k] > 0 for k in ("echo plain", "echo deflated", "pong", "close reply", "1007")), tally


def test_checker_rejects_a_server_without_the_command_step():
    """What today's broadcast sends on this traffic -- the command text to the
    room, the membership where it was -- is not what the checker accepts."""
    case = cm.command_case()
    views, _, _ = cm.command_view(case, 0)
    sent = s.reference_broadcast_server(cm.as_broadcast(case), 0, None)
    sent = [[b"".join(r) for r in row] for row in sent]
    with pytest.raises(s.CheckError):
        cm.check_command_session(case, views, sent, None)
