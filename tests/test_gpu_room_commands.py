"""GPU checks of the room-command step (gevws_room_commands_async) through the C
ABI on synthetic d_bodies / d_out, bit-exact against
tests/_room_commands_model.py: the change records, d_change_of, every byte of
d_bodies and the summary; everything that is not an output entry still the 0xEE
it was prefilled with, d_out unchanged."""
import numpy as np
import pytest

from tests import _room_commands_model as cm

pytestmark = pytest.mark.gpu

BLOCK = 256                     # kWalkBlock: a lane block of the count and emit kernels
COUNTS = (0, 1, 255, 256, 257, 262144, 262145)   # one lane block, its neighbours; 1 024 blocks and one body more
N_ROOMS, N_CONNS = 12, 5000
PAL = cm.palette(N_ROOMS)
NAMES = [e[0] for e in PAL]
COMMANDS = [k for k, n in enumerate(NAMES) if n.startswith(("join", "leave", "rejected"))]
OTHERS = [k for k, n in enumerate(NAMES) if not n.startswith(("join", "leave", "rejected"))]


def conns_of(rng, n):
    """Message order: by connection."""
    return np.sort(rng.integers(0, N_CONNS, n)).astype(np.uint32)


def check(engine, bodies, out, src_bytes=None, n_conns=N_CONNS, n_rooms=N_ROOMS, tag="", **kw):
    src_bytes = out.size if src_bytes is None else src_bytes
    want = cm.commands_model(bodies, out, src_bytes, n_conns, n_rooms, **kw)
    got = cm.run_commands(engine, bodies, out, src_bytes, n_conns, n_rooms,
                          **{**kw, "max_changes": kw.get("max_changes", int(want["summary"]["frames"]))})
    cm.assert_commands(got, want, bodies, tag)
    return got, want


# ---------------------------------------------------------------------------- 1. counts and placements
@pytest.mark.parametrize("placement", ["none", "every body", "block edges", "a random third"])
@pytest.mark.parametrize("n", COUNTS)
def test_counts_and_placements(engine, n, placement):
    """The changes keep the message order across lane blocks and across the
    scan's rounds; d_changes holds exactly the need."""
    rng = np.random.default_rng(0x7C0000 + n)
    m = np.arange(n)
    is_cmd = {"none": np.zeros(n, bool), "every body": np.ones(n, bool),
              "block edges": (m % BLOCK == 0) | (m % BLOCK == BLOCK - 1) | (m == n - 1),
              "a random third": rng.random(n) < 1 / 3}[placement]
    idx = np.where(is_cmd, rng.choice(COMMANDS, n), rng.choice(OTHERS, n)) if n else np.zeros(0, np.int64)
    bodies, out = cm.batch_from_palette(PAL, idx, conns_of(rng, n))
    got, want = check(engine, bodies, out, tag=(n, placement))
    s = want["summary"]
    assert s["status"] == 0 and s["payload_len"] == int(is_cmd.sum()) and s["frames"] + s["payload_bytes"] == s["payload_len"]
    if n >= 255 and placement in ("every body", "a random third"):
        assert s["frames"] > 20 and s["payload_bytes"] > 5      # (of 255 bodies a third: about 57 and 28)
    if n:
        assert np.all(np.diff(want["changes"]["conn"].astype(np.int64)) >= 0)   # message order: by connection
    if n == 0:   # no bodies by the count, and by the message pass's summary
        check(engine, *cm.batch_from_palette(PAL, rng.choice(COMMANDS, 4), conns_of(rng, 4)),
              msg=dict(frames=0, status=0), tag="no messages")


def test_fewer_messages_than_room(engine):
    """The bodies are the first min(d_msg_summary->frames, max_messages): what lies behind is neither read nor written."""
    rng = np.random.default_rng(0x7C0101)
    n = 3 * BLOCK + 9
    bodies, out = cm.batch_from_palette(PAL, rng.choice(COMMANDS, n), conns_of(rng, n))
    bodies["conn"][2 * BLOCK + 5:] = 0xFFFFFFF0          # malformed, but behind the count
    got, want = check(engine, bodies, out, msg=dict(frames=2 * BLOCK + 5, status=0), tag="frames < max_messages")
    assert want["summary"]["payload_len"] == 2 * BLOCK + 5
    check(engine, bodies[: BLOCK + 1], out, msg=dict(frames=n, status=0), tag="frames > max_messages")


# ---------------------------------------------------------------------------- 2. every class in one batch
def test_every_class_in_one_batch(engine):
    rng = np.random.default_rng(0x7C0200)
    idx = np.concatenate([np.arange(len(PAL)), rng.integers(0, len(PAL), 3 * BLOCK)])
    rng.shuffle(idx)
    bodies, out = cm.batch_from_palette(PAL, idx, conns_of(rng, idx.size))
    got, want = check(engine, bodies, out, tag="mix")
    of = want["change_of"]
    for k, name in enumerate(NAMES):
        at = np.flatnonzero(idx == k)
        if name.startswith(("join", "leave")):
            assert np.all(of[at] >= 0), name
        elif name.startswith("rejected"):
            assert np.all(of[at] == cm.OF_REJECTED), name
        else:
            assert np.all(of[at] == cm.OF_NONE), name
    rooms = dict(zip(of[of >= 0].tolist(), want["changes"]["room"].tolist()))
    for k, room in ((NAMES.index("join, digits in the pad"), 1), (NAMES.index("leave, digits in the pad"), cm.ROOM_NONE),
                    (NAMES.index("join the last room"), N_ROOMS - 1), (NAMES.index("join, inflated"), 1)):
        assert all(rooms[int(of[m])] == room for m in np.flatnonzero(idx == k)), NAMES[k]
    # n_rooms belongs to the call: none, one, and all of them
    for n_rooms in (0, 1, 2 ** 32 - 1):
        check(engine, bodies, out, n_rooms=n_rooms, tag=("n_rooms", n_rooms))


# ---------------------------------------------------------------------------- 3. capacity
@pytest.mark.parametrize("n", (1, 257, 2 * BLOCK + 77))
def test_capacity(engine, n):
    rng = np.random.default_rng(0x7C0300 + n)
    accepted = [k for k in COMMANDS if not NAMES[k].startswith("rejected")]
    idx = rng.choice(accepted, n) if n == 1 else np.where(rng.random(n) < 0.5, rng.choice(COMMANDS, n), rng.choice(OTHERS, n))
    bodies, out = cm.batch_from_palette(PAL, idx, conns_of(rng, n))
    need = int(cm.commands_model(bodies, out, out.size, N_CONNS, N_ROOMS)["summary"]["frames"])
    assert need >= 1
    got, want = check(engine, bodies, out, max_changes=need - 1, tag="one below the need")
    assert want["summary"] == dict(cm.zero_summary(), frames=need, status=cm.ERR_CAPACITY) and want["bodies"] is None
    check(engine, bodies, out, max_changes=need, tag="the need")          # the caller retries: the same inputs
    check(engine, bodies, out, max_changes=need + 5, tag="more than the need")


# ---------------------------------------------------------------------------- 4. gates
@pytest.mark.parametrize("gate", ["msg", "join", "ctl", "ctl ok", "no messages", "max_messages 0"])
def test_gates(engine, gate):
    rng = np.random.default_rng(0x7C0400)
    n = BLOCK + 3
    bodies, out = cm.batch_from_palette(PAL, rng.choice(COMMANDS, n), conns_of(rng, n))
    bodies["conn"][5] = 0xFFFFFFF0              # a closed gate reads nothing: not even a malformed record counts
    kw = {"msg": dict(msg=dict(frames=n, status=cm.ERR_CAPACITY)), "join": dict(join_status=cm.ERR_CAPACITY),
          "ctl": dict(ctl_status=cm.ERR_INVALID), "ctl ok": dict(ctl_status=0),
          "no messages": dict(msg=dict(frames=0, status=0)), "max_messages 0": dict(max_messages=0)}[gate]
    got, want = check(engine, bodies, out, tag=gate, max_changes=n, **kw)
    if gate == "ctl ok":
        assert want["summary"] == dict(cm.zero_summary(), errors=1, status=cm.ERR_INVALID)
    else:
        assert want["summary"] == cm.zero_summary() and want["changes"] is None


# ---------------------------------------------------------------------------- 5. malformed records
def malformed_batch(rng, n=BLOCK + 40):
    idx = np.where(rng.random(n) < 0.4, rng.choice(COMMANDS, n), rng.choice(OTHERS, n))
    idx[[3, 60, BLOCK - 1, BLOCK, n - 1]] = NAMES.index("join")      # looked-at bodies to break
    idx[[7, 61]] = NAMES.index("long text")                          # delivered, not looked at
    idx[[8, 62]] = NAMES.index("binary join")
    idx[9] = NAMES.index("undelivered")
    return cm.batch_from_palette(PAL, idx, conns_of(rng, n))


BREAK = {
    "neither joined nor inflated": lambda b, m, src: b["flags"].__setitem__(m, cm.WHOLE),
    "conn == n_conns": lambda b, m, src: b["conn"].__setitem__(m, N_CONNS),
    "conn 2^32 - 1": lambda b, m, src: b["conn"].__setitem__(m, 0xFFFFFFFF),
    "off % 16 == 8": lambda b, m, src: b["off"].__setitem__(m, int(b["off"][m]) + 8),
    "off % 16 == 1": lambda b, m, src: b["off"].__setitem__(m, int(b["off"][m]) + 1),
    "off behind d_out": lambda b, m, src: b["off"].__setitem__(m, src),
    "off + length wraps": lambda b, m, src: b["off"].__setitem__(m, 2 ** 64 - 16),
    "off far behind d_out": lambda b, m, src: b["off"].__setitem__(m, 1 << 40),
}


@pytest.mark.parametrize("kind", list(BREAK))
def test_each_malformed_kind_alone(engine, kind):
    rng = np.random.default_rng(0x7C0500)
    bodies, out = malformed_batch(rng)
    for m in (3, BLOCK):
        BREAK[kind](bodies, m, out.size)
    got, want = check(engine, bodies, out, tag=kind, max_changes=bodies.size)
    assert want["summary"] == dict(cm.zero_summary(), errors=2, status=cm.ERR_INVALID)


def test_malformed_kinds_mixed_and_what_is_not_malformed(engine):
    rng = np.random.default_rng(0x7C0501)
    bodies, out = malformed_batch(rng)
    n = bodies.size
    ok, _ = check(engine, bodies, out, tag="well formed", max_changes=n)
    assert int(ok["summary"]["status"]) == 0
    # not malformed: an undelivered body's conn, a misplaced body nobody looks at (binary, or longer than a command)
    fine = bodies.copy()
    fine["conn"][9] = 0xFFFFFFFF
    fine["off"][7] += 8
    fine["off"][8] = 1 << 40
    got, _ = check(engine, fine, out, tag="not malformed", max_changes=n)
    assert int(got["summary"]["status"]) == 0 and int(got["summary"]["frames"]) == int(ok["summary"]["frames"])
    bad = bodies.copy()
    for m, kind in zip((3, 60, BLOCK - 1, BLOCK, n - 1), ("neither joined nor inflated", "conn == n_conns", "off % 16 == 8",
                                                         "off + length wraps", "off behind d_out")):
        BREAK[kind](bad, m, out.size)
    bad["flags"][61], bad["conn"][61] = cm.WHOLE, 0xFFFFFFFF       # two things wrong with one record: it counts once
    bad["flags"][62] = cm.WHOLE                                    # a delivered body in its frame's slot, not looked at
    got, want = check(engine, bad, out, tag="mixed", max_changes=n)
    assert want["summary"] == dict(cm.zero_summary(), errors=7, status=cm.ERR_INVALID)


def test_the_last_vector_of_d_out(engine):
    """A looked-at body in the last vector of d_out with off + length ==
    src_bytes is valid; the same body one byte further is malformed."""
    rng = np.random.default_rng(0x7C0502)
    n = BLOCK + 1
    idx = rng.choice(OTHERS, n)
    idx[n - 1] = NAMES.index("join, digits in the pad")
    bodies, out = cm.batch_from_palette(PAL, idx, conns_of(rng, n))
    off, length = int(bodies["off"][n - 1]), int(bodies["length"][n - 1])
    src = off + length
    assert src % 16 == 7 and off == (n - 1) * cm.SLOT
    got, want = check(engine, bodies, out[:src], tag="ends with d_out")
    assert want["summary"] == dict(cm.zero_summary(), frames=1, payload_len=1) and want["changes"]["room"][0] == 1
    check(engine, bodies, out[: src - 1], tag="d_out one byte shorter")
    longer = bodies.copy()
    longer["length"][n - 1] = length + 1                            # "/join 12": a command, but for its last byte
    got, want = check(engine, longer, out[:src], src_bytes=src, tag="one byte further")
    assert want["summary"] == dict(cm.zero_summary(), errors=1, status=cm.ERR_INVALID)
    full = bodies.copy()                                            # a 16-byte command that fills the last vector
    out16 = out[: off + 16].copy()
    out16[off: off + 16] = np.frombuffer(b"/join 0000000011", np.uint8)
    full["length"][n - 1] = 16
    got, want = check(engine, full, out16, tag="16 bytes, the last vector")
    assert want["changes"]["room"][0] == 11
