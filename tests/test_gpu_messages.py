"""GPU checks of the message layer (gevws_messages_async): fragment assembly,
the RFC 6455 frame checks and the UTF-8 check of text messages, on hand-built
decoded batches and behind a real decode.  Every comparison is exact: against
bytes.decode where a verdict is all there is to compare, else against the
model of tests/_messages_model.py (pinned on the CPU by
tests/test_messages_model.py), every field of every table."""
import functools

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _messages_model as mm
from tests._helpers import gpu_decode, pack_streams

pytestmark = pytest.mark.gpu

T, B, C, PING, PONG, CLOSE = 1, 2, 0, 9, 10, 8
# where the UTF-8 pass changes hands inside a frame (gevws_message.hip): a
# 16-byte vector, a wave's load of 64 vectors, its step of four loads, and for
# frames of 256 KiB and more the 16 KiB tile and the threshold itself
VEC, WAVE_LOAD, WAVE_STEP, BIG_TILE, BIG_FRAME = 16, 1024, 4096, 16384, 256 * 1024


def py_valid(b: bytes) -> bool:
    try:
        b.decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def single_frame_batch(payloads: np.ndarray, lengths: np.ndarray, slot: int, opcode: int = T, pad: int = 0xBF):
    """N connections of one FIN frame each: payloads [N, slot] uint8 (slot a
    multiple of 16), the first lengths[i] bytes of row i the frame's; the rest
    of a row becomes pad."""
    n = payloads.shape[0]
    arena = payloads.copy()
    arena[np.arange(slot)[None, :] >= lengths[:, None]] = pad
    frames = np.zeros(n, mm.FRAME_DTYPE)
    frames["fin"], frames["opcode"], frames["length"] = 1, opcode, lengths
    frames["payload_off"] = np.arange(n, dtype=np.uint64) * slot
    co = np.zeros(n, mm.CONN_OUT_DTYPE)
    co["first_frame"], co["nframes"], co["payload_base"] = np.arange(n), 1, frames["payload_off"]
    return mm.Decoded.from_arrays(frames, co, arena.reshape(-1))


def check_verdicts(engine, d, valid: np.ndarray, tag=""):
    """One single-frame text message per connection: verdict == `valid`."""
    got = mm.run_device(engine, d)
    n = valid.size
    s = got["summary"]
    assert int(s["status"]) == 0 and int(s["frames"]) == n and int(s["errors"]) == int((~valid).sum()), tag
    assert int(s["payload_len"]) == int(d.frames["length"].sum()), tag
    cm = got["conn_msg"]
    wrong = np.flatnonzero(cm["error"] != np.where(valid, mm.OK, mm.ERR_UTF8))
    assert wrong.size == 0, (tag, wrong[:8], [bytes(d.arena[int(d.frames["payload_off"][i]):][: int(d.frames["length"][i])])
                                             for i in wrong[:8]])
    assert np.array_equal(cm["error_frame"], np.where(valid, mm.NO_FRAME, np.arange(n)).astype(np.uint64)), tag
    assert np.array_equal(cm["first_message"], np.arange(n)) and np.all(cm["nmessages"] == 1), tag
    m = got["messages"]
    assert np.array_equal(m["status"], np.where(valid, mm.OK, mm.ERR_UTF8)), tag
    assert np.array_equal(m["flags"], np.where(valid, mm.BEGIN | mm.END, mm.BEGIN)), tag
    assert np.array_equal(m["length"], d.frames["length"]) and np.array_equal(got["msg_of"], np.arange(n)), tag
    assert np.array_equal(got["state"]["failed"], np.where(valid, 0, mm.ERR_UTF8)), tag
    return got


# ---------------------------------------------------------------------------- 1. exhaustive short sequences
@functools.lru_cache(maxsize=None)
def short_sequences():
    """Every lead byte 0x80..0xFF x every second byte x a third and a fourth
    byte from {absent, 0x7F, 0x80, 0xBF, 0xC0}: (bytes [N, 4], lengths, valid)."""
    opt = np.array([-1, 0x7F, 0x80, 0xBF, 0xC0])
    lead, second, third, fourth = np.meshgrid(np.arange(0x80, 0x100), np.arange(256), opt, opt, indexing="ij")
    cols = np.stack([lead.ravel(), second.ravel(), third.ravel(), fourth.ravel()], 1)
    n = cols.shape[0]
    seq = np.zeros((n, 4), np.uint8)
    seq[:, 0], seq[:, 1] = cols[:, 0], cols[:, 1]
    length = np.full(n, 2, np.int64)
    for k in (2, 3):
        have = cols[:, k] >= 0
        seq[have, length[have]] = cols[have, k]
        length += have
    raw = seq.tobytes()
    valid = np.fromiter((py_valid(raw[4 * i: 4 * i + int(length[i])]) for i in range(n)), bool, n)
    assert n == 128 * 256 * 25 and 0 < valid.sum() < n
    return seq, length, valid


def test_exhaustive_short_sequences_bare(engine):
    seq, length, valid = short_sequences()
    rows = np.zeros((seq.shape[0], 16), np.uint8)
    rows[:, :4] = seq
    check_verdicts(engine, single_frame_batch(rows, length, 16), valid)


@pytest.mark.parametrize("offset", [13, 14, 15])
def test_exhaustive_short_sequences_across_a_vector_boundary(engine, offset):
    seq, length, valid = short_sequences()
    n = seq.shape[0]
    rows = np.full((n, 48), ord("a"), np.uint8)
    for k in range(4):
        have = length > k
        rows[have, offset + k] = seq[have, k]
    # (ASCII after a truncated sequence is as invalid as the end of the message)
    check_verdicts(engine, single_frame_batch(rows, np.full(n, 48, np.int64), 48), valid, f"offset {offset}")


# ---------------------------------------------------------------------------- 2. lengths and boundaries
def mixed_text(rng, nbytes: int) -> bytes:
    """Valid text of exactly nbytes bytes: 1-, 2-, 3- and 4-byte characters."""
    pools = [(0x20, 0x7F), (0xA0, 0x800), (0x800, 0xD800), (0xE000, 0xFFFE), (0x10000, 0x110000)]
    cps = np.concatenate([rng.integers(lo, hi, nbytes // 8 + 4) for lo, hi in pools])
    rng.shuffle(cps)
    b = "".join(map(chr, cps)).encode()
    while len(b) < nbytes:
        b += b
    cut = nbytes
    while cut and (b[cut] & 0xC0) == 0x80:
        cut -= 1
    return b[:cut] + b"." * (nbytes - cut)


def asciify(buf: bytearray, lo: int, hi: int) -> None:
    """Overwrite every character overlapping [lo, hi) with ASCII, whole."""
    lo, hi = max(lo, 0), min(hi, len(buf))
    while lo > 0 and (buf[lo] & 0xC0) == 0x80:
        lo -= 1
    while hi < len(buf) and (buf[hi] & 0xC0) == 0x80:
        hi += 1
    buf[lo:hi] = b"x" * (hi - lo)


LENGTHS = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 70000]


def test_frame_lengths_cut_on_and_inside_a_character(engine):
    rng = np.random.default_rng(0x6C656E)
    conns, want_err = [], []
    for L in LENGTHS:
        conns.append([(1, 0, T, mixed_text(rng, L))])
        want_err.append(mm.OK)
        if L:  # a 3-byte character laid over the cut: the frame ends inside it
            cutb = mixed_text(rng, L - 1) + "€".encode()[:1] if L < 2 else mixed_text(rng, L - 2) + "€".encode()[:2]
            conns.append([(1, 0, T, cutb)])
            want_err.append(mm.ERR_UTF8)
            conns.append([(0, 0, T, cutb)])  # not the FIN frame: pending, carried
            want_err.append(mm.OK)
    for pad in (0xBF, 0x00):  # pad bytes never count, whatever they hold
        d = mm.Decoded(conns, pad=pad)
        got = mm.run_device(engine, d)
        assert list(got["conn_msg"]["error"]) == want_err, pad
        mm.assert_tables_equal(got, d.model(), f"pad {pad:#x}")
        pending = got["state"]["utf8_n"][3::3]  # the frames that are not FIN (L = 1 first)
        assert np.all(pending[:1] == 1) and np.all(pending[1:] == 2)


def planted_frames(rng, size: int, boundaries):
    """Frames of `size` bytes of valid mixed text, one defect or one 4-byte
    character planted in each: (payload, valid) pairs."""
    base = mixed_text(rng, size)
    out = [(base, True)]
    spots = sorted({0, size - 1} | {p for b in boundaries for p in (b - 1, b) if 0 <= p < size})
    for pos in spots:
        b = bytearray(base)
        asciify(b, pos, pos + 1)
        b[pos] = 0xFF  # a byte that is never valid
        out.append((bytes(b), False))
        b = bytearray(base)
        asciify(b, pos - 1, pos + 2)
        if pos == 0:
            b[0:2] = b"\xe2\x82"  # a 3-byte sequence cut short by ASCII
        elif pos == size - 1:
            b[pos] = 0xE2         # ... by the end of the message
        else:
            b[pos - 1: pos + 1] = b"\xe2\x82"
        out.append((bytes(b), False))
    for bd in boundaries:
        for shift in (1, 2, 3):  # a 4-byte character with 1, 2 or 3 bytes before the boundary
            if bd - shift < 0 or bd - shift + 4 > size:
                continue
            b = bytearray(base)
            asciify(b, bd - shift, bd - shift + 4)
            b[bd - shift: bd - shift + 4] = "\U0001F600".encode()
            out.append((bytes(b), True))
    for payload, valid in out:
        assert py_valid(payload) == valid
    return out


@pytest.mark.parametrize("size,boundaries", [
    (70000, [VEC, 30000 // VEC * VEC, WAVE_LOAD, WAVE_STEP, 16 * WAVE_STEP, 70000 // VEC * VEC]),
    (BIG_FRAME + 40000, [VEC, WAVE_LOAD, WAVE_STEP, BIG_TILE, 5 * BIG_TILE, BIG_FRAME, BIG_FRAME + 40000 - 16]),
])
def test_one_defect_at_every_kind_of_boundary(engine, size, boundaries):
    rng = np.random.default_rng(size)
    cases = planted_frames(rng, size, boundaries)
    d = mm.Decoded([[(1, 0, T, p)] for p, _ in cases])
    check_verdicts(engine, d, np.array([v for _, v in cases]), f"size {size}")


def test_frame_at_the_big_frame_threshold(engine):
    rng = np.random.default_rng(0x626967)
    conns, valid = [], []
    for size in (BIG_FRAME - 1, BIG_FRAME, BIG_FRAME + 1):
        t = mixed_text(rng, size)
        for payload in (t, t[:-1] + b"\xc3", b"\x80" + t[1:]):
            conns.append([(1, 0, T, payload)])
            valid.append(py_valid(payload))
    assert valid == [True, False, False] * 3
    check_verdicts(engine, mm.Decoded(conns), np.array(valid))


# ---------------------------------------------------------------------------- 3. fragmentation
TEXT = "aé€\U0001F600z".encode()  # 1 + 2 + 3 + 4 + 1 bytes


def fragmentations(b: bytes):
    n = len(b)
    out = [[b[:i], b[i:]] for i in range(n + 1)]
    out += [[b[:i], b[i:j], b[j:]] for i in range(n + 1) for j in range(i, n + 1)]
    out.append([b[i:i + 1] for i in range(n)])  # a frame a byte: the 4-byte character spans 4 frames
    return out


def fragment_conn(frags, opcode=T, ping=False):
    conn = []
    for i, f in enumerate(frags):
        if ping and i:
            conn.append((1, 0, PING, b"\xff\xfe"))
        conn.append((i == len(frags) - 1, 0, opcode if i == 0 else C, f))
    return conn


INVALID_TEXTS = [b"a\xe2\x82z", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xc0\xaf", b"ab\xf0\x9f\x98", b"\xe2\x82\xac\xac",
                 b"\xf0\x9f\x98\x80\x80"]


def test_fragmented_text_every_split(engine):
    conns, fails = [], []
    for ping in (False, True):
        for text in [TEXT] + INVALID_TEXTS:
            for f in fragmentations(text):
                conns.append(fragment_conn(f, T, ping))
                fails.append(text is not TEXT)
    for bad in INVALID_TEXTS:  # binary: not validated
        for f in fragmentations(bad)[:8]:
            conns.append(fragment_conn(f, B))
            fails.append(False)
    d = mm.Decoded(conns)
    got = mm.run_device(engine, d)
    assert np.array_equal(got["conn_msg"]["error"], np.where(fails, mm.ERR_UTF8, mm.OK))
    mm.assert_tables_equal(got, d.model())


def test_fragmented_text_split_between_two_calls(engine):
    cases = []
    for text in [TEXT] + INVALID_TEXTS:
        for frags in fragmentations(text):
            for k in range(1, len(frags)):
                cases.append((fragment_conn(frags, T, ping=True), frags, k))
    cases = cases[::3]
    first, second = [], []
    for conn, frags, k in cases:
        cut = [i for i, fr in enumerate(conn) if fr[2] != PING][k]  # the k-th data frame opens the second call
        first.append(conn[:cut])
        second.append(conn[cut:])
    whole = mm.Decoded([c for c, _, _ in cases])
    d1, d2 = mm.Decoded(first), mm.Decoded(second)
    g1 = mm.run_device(engine, d1)
    w1 = d1.model()
    mm.assert_tables_equal(g1, w1, "first call")
    g2 = mm.run_device(engine, d2, state=g1["state"])
    mm.assert_tables_equal(g2, d2.model(w1["state"]), "second call")
    gw = mm.run_device(engine, whole)
    mm.assert_tables_equal(gw, whole.model(), "one call")
    assert gw["state"].tobytes() == g2["state"].tobytes()
    for c in range(len(cases)):
        one = gw["messages"][int(gw["conn_msg"]["first_message"][c])]
        e1, e2 = int(g1["conn_msg"]["error"][c]), int(g2["conn_msg"]["error"][c])
        assert (e1 or e2) == int(gw["conn_msg"]["error"][c]), c
        a = g1["messages"][int(g1["conn_msg"]["first_message"][c])]
        assert int(a["flags"]) == mm.BEGIN and int(a["opcode"]) == T
        if e1:  # failed in the first call: the second yields nothing and repeats the verdict
            assert int(g2["conn_msg"]["nmessages"][c]) == 0 and int(g2["conn_msg"]["error_frame"][c]) == mm.NO_FRAME
            assert [a[k] for k in ("length", "nframes", "flags", "status")] == \
                [one[k] for k in ("length", "nframes", "flags", "status")]
            continue
        b = g2["messages"][int(g2["conn_msg"]["first_message"][c])]
        assert int(b["opcode"]) == T and int(b["flags"]) == (0 if e2 else mm.END)
        assert int(a["length"]) + int(b["length"]) == int(one["length"])
        assert int(a["nframes"]) + int(b["nframes"]) == int(one["nframes"])
        assert int(b["status"]) == int(one["status"]) and int(a["status"]) == mm.OK


# ---------------------------------------------------------------------------- 4. protocol matrix
def healthy(i: int):
    return [[(1, 0, T, b"hi")], [(0, 0, B, b"\xff"), (1, 0, PING, b"p"), (1, 0, C, b"\xfe")],
            [(1, 0, PONG, b""), (1, 0, T, "é€".encode())]][i % 3]


OFFENDERS = {
    mm.ERR_RSV: (1, 2, T, b"a"),
    mm.ERR_OPCODE: (1, 0, 5, b"a"),
    mm.ERR_CONTROL: (0, 0, PING, b"a"),
    mm.ERR_CONTINUATION: (1, 0, C, b"a"),
    mm.ERR_INTERLEAVE: (1, 0, B, b"a"),
}


def test_protocol_errors_first_middle_last(engine):
    conns, state, expect = [], [], []
    for err, bad in OFFENDERS.items():
        inter = err == mm.ERR_INTERLEAVE
        opener = [(0, 0, T, b"\xe2")] if inter else [(1, 0, T, b"one")]
        after = [(1, 0, T, b"later"), (1, 0, PING, b"")]
        for where, conn, at, nmsg in (("first", [bad] + after, 0, 0),
                                      ("middle", opener + [(1, 0, PING, b"")] + [bad] + after, 2, 1),
                                      ("last", opener + [bad], 1, 1)):
            conns.append(healthy(len(conns)))
            state.append(0)
            expect.append((mm.OK, None, None))
            conns.append(conn)
            state.append(B if inter and where == "first" else 0)  # an open message carried in
            expect.append((err, at, nmsg))
    conns.append(healthy(0))
    state.append(0)
    expect.append((mm.OK, None, None))
    d = mm.Decoded(conns)
    st = np.zeros(len(conns), mm.MSG_STATE_DTYPE)
    st["opcode"] = state
    got = mm.run_device(engine, d, state=st)
    for c, (err, at, nmsg) in enumerate(expect):
        cm = got["conn_msg"][c]
        assert int(cm["error"]) == err, c
        if err:
            assert int(cm["error_frame"]) == int(d.conn_out["first_frame"][c]) + at and int(cm["nmessages"]) == nmsg, c
            first = int(d.conn_out["first_frame"][c])
            assert np.all(got["msg_of"][first + at: first + int(d.conn_out["nframes"][c])] == -1), c
            assert int(got["state"][c]["failed"]) == err and int(got["state"][c]["opcode"]) == 0
    mm.assert_tables_equal(got, d.model(st))
    # sticky: the same connections in a second call yield nothing and repeat their verdict
    d2 = mm.Decoded([healthy(c) for c in range(len(conns))])
    got2 = mm.run_device(engine, d2, state=got["state"])
    mm.assert_tables_equal(got2, d2.model(got["state"]), "second call")
    for c, (err, _, _) in enumerate(expect):
        cm = got2["conn_msg"][c]
        assert int(cm["error"]) == err and int(cm["error_frame"]) == mm.NO_FRAME, c
        assert (int(cm["nmessages"]) == 0) == bool(err), c
    assert int(got2["summary"]["errors"]) == 0  # none failed in this batch


def test_protocol_precedence_and_odd_connections(engine):
    conns = [
        [(0, 3, 0xB, b"a" * 126)],                  # rsv, reserved opcode, fragmented control, too long: RSV
        [(0, 0, 0xF, b"a" * 126)],                  # reserved control opcode, fragmented: OPCODE
        [(0, 0, CLOSE, b"")],                       # fragmented close
        [(1, 0, PING, b"a" * 126)],                 # control frame over 125 bytes
        [(1, 0, PING, b"a" * 125)],                 # ... of 125: fine
        [(1, 1, C, b"")],                           # rsv on a stray continuation: RSV
        [(0, 0, T, b"\xff"), (1, 4, T, b"")],       # a bad byte first: UTF8 at frame 0, not RSV at frame 1
        [(0, 0, T, b"ok"), (1, 0, T, b"\xff")],     # interleave, whatever the payload
        [(0, 0, B, b"\xff"), (0, 0, PING, b"")],    # fragmented ping inside a message; the message stays open
        (mm.ERR_LEN_MSB, [(1, 0, T, b"\xff"), (1, 0, C, b"")]),
        [],
        (mm.ERR_LEN_MSB, []),
        [(1, 0, T, b"")],
        [(0, 0, T, b""), (0, 0, C, b""), (1, 0, C, b"")],  # zero-length fragments
        [(1, 0, 0, b"x")],
    ]
    d = mm.Decoded(conns)
    want_err = [mm.ERR_RSV, mm.ERR_OPCODE, mm.ERR_CONTROL, mm.ERR_CONTROL, 0, mm.ERR_RSV, mm.ERR_UTF8, mm.ERR_INTERLEAVE,
                mm.ERR_CONTROL, 0, 0, 0, 0, 0, mm.ERR_CONTINUATION]
    for keep in (True, False):  # d_state == NULL: every connection fresh, nothing kept
        got = mm.run_device(engine, d, keep_state=keep)
        assert list(got["conn_msg"]["error"]) == want_err
        assert int(got["conn_msg"]["error_frame"][6]) == int(d.conn_out["first_frame"][6])
        mm.assert_tables_equal(got, d.model())
    # a poisoned stream and one without frames keep their state, whatever it holds
    st = np.zeros(len(conns), mm.MSG_STATE_DTYPE)
    st["opcode"][[9, 10]] = T
    st["utf8_n"][[9, 10]] = 1
    st["utf8"][[9, 10], 0] = 0xC3
    st["failed"][11] = mm.ERR_OPCODE
    got = mm.run_device(engine, d, state=st)
    mm.assert_tables_equal(got, d.model(st))
    assert got["state"][[9, 10, 11]].tobytes() == st[[9, 10, 11]].tobytes()
    assert int(got["conn_msg"]["error"][11]) == mm.ERR_OPCODE and int(got["conn_msg"]["error"][9]) == 0


def test_empty_and_failed_inputs(engine):
    got = mm.run_device(engine, mm.Decoded([]))  # n_conns == 0
    assert got["summary"].tobytes() == bytes(64)
    conns = [[(1, 0, T, b"\xff")], [(1, 0, T, b"ok")]]
    st = np.zeros(2, mm.MSG_STATE_DTYPE)
    st["opcode"], st["failed"][1] = B, mm.ERR_RSV
    for d in (mm.Decoded(conns, summary_status=gev_amd.ERR_CAPACITY), mm.Decoded([[], []])):  # a failed decode; no frames
        got = mm.run_device(engine, d, state=st)
        assert got["summary"].tobytes() == bytes(64)
        assert got["state"].tobytes() == st.tobytes() and np.all(got["msg_of"] == -1)
        mm.assert_tables_equal(got, d.model(st))


def test_capacity_then_retry(engine):
    conns = [[(1, 0, T, b"a"), (1, 0, B, b"b")], [(0, 0, T, b"\xe2")], [(1, 0, T, b"\xff")], [(1, 0, B, b"")]]
    d = mm.Decoded(conns)
    want = d.model()
    assert want["frames"] == 5
    got = mm.run_device(engine, d, max_messages=4)
    s = got["summary"]
    assert int(s["status"]) == gev_amd.ERR_CAPACITY and int(s["frames"]) == 5
    assert got["state"].tobytes() == bytes(8 * len(conns))  # untouched: the caller retries
    assert np.all(got["messages"].view(np.uint8) == 0xEE)   # nothing written
    mm.assert_tables_equal(mm.run_device(engine, d, max_messages=int(s["frames"])), want)


# ---------------------------------------------------------------------------- 5. scale of the bookkeeping
def client_conn(rng, n_frames: int):
    """A client's frames: messages of 1-4 fragments, control frames in
    between, mostly valid text, now and then an offence."""
    conn = []
    while len(conn) < n_frames:
        r = rng.random()
        if r < 0.2:
            conn.append((1, 0, int(rng.choice([PING, PONG])), bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8))))
            continue
        if r < 0.208:
            conn.append([(1, 1, T, b""), (1, 0, 6, b""), (0, 0, PING, b""), (1, 0, C, b"zz")][int(rng.integers(0, 4))])
            continue
        op = T if rng.random() < 0.7 else B
        if op == T:
            body = "".join(chr(int(rng.integers(*[(0x20, 0x7F), (0xA0, 0x800), (0x800, 0xD800), (0x10000, 0x110000)][
                int(rng.integers(0, 4))]))) for _ in range(int(rng.integers(0, 30)))).encode()
            if rng.random() < 0.02 and body:
                body = body[: int(rng.integers(0, len(body)))] + b"\xa0" + body
        else:
            body = bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8))
        k = int(rng.integers(1, 5))
        cuts = sorted(int(rng.integers(0, len(body) + 1)) for _ in range(k - 1))
        frags = [body[i:j] for i, j in zip([0] + cuts, cuts + [len(body)])]
        for i, f in enumerate(frags):
            conn.append((i == k - 1, 0, op if i == 0 else C, f))
            if rng.random() < 0.15:
                conn.append((1, 0, PING, b"?"))
    return conn[:n_frames]  # (may end inside a message: carried)


def test_random_batch_whole_table(engine):
    rng = np.random.default_rng(0x736361)
    n_conns = 900  # the per-connection passes run 256 connections a workgroup
    batches = [[], []]
    for _ in range(n_conns):  # each client's frames dealt to two calls, 0-60 frames a call
        n1, n2 = int(rng.integers(0, 61)), int(rng.integers(0, 61))
        conn = client_conn(rng, n1 + n2)
        batches[0].append(conn[:n1])
        batches[1].append(conn[n1:])
    state = None
    for i, conns in enumerate(batches):  # the second call carries the first one's state
        d = mm.Decoded(conns)
        assert d.frames.shape[0] > 3 * 256 * 16
        want = d.model(state)
        got = mm.run_device(engine, d, state=state)
        assert want["errors"] > 20 and ((want["messages"]["flags"] & mm.BEGIN) == 0).sum() >= (100 if i else 0)
        mm.assert_tables_equal(got, want, f"call {i}")
        state = got["state"]


# ---------------------------------------------------------------------------- 6. behind a real decode
def test_messages_behind_a_decode(engine):
    rng = np.random.default_rng(0x646563)
    streams, conns = [], []
    for _ in range(300):
        conn = client_conn(rng, int(rng.integers(0, 25)))
        if rng.random() < 0.3:  # longer frames: the 16- and 64-bit length forms
            conn.append((1, 0, T, mixed_text(rng, int(rng.integers(126, 70000)))))
        s = b""
        for fin, rsv, op, payload in conn:
            L = len(payload)
            forms = [f for f in (7, 16, 64) if (f != 7 or L <= 125) and (f != 16 or L <= 0xFFFF)]
            s += wo.encode_frame(payload, op, bool(fin), rsv, True, bytes(rng.integers(0, 256, 4, dtype=np.uint8)),
                                 int(rng.choice(forms)))
        if rng.random() < 0.3:
            s += wo.encode_frame(b"cut short", T, True, 0, True, b"\x01\x02\x03\x04")[:7]
        streams.append(s)
    arena, table = pack_streams(streams)
    out = gpu_decode(engine, arena, table)
    res = engine.messages(out)
    # the model over the oracle's frames of the same streams
    ref = [wo.decode_stream(s) for s in streams]
    d = mm.Decoded([(r.status, [(f.header.fin, f.header.rsv, f.header.opcode, f.payload) for f in r.frames])
                    for r in ref], pad=0)
    assert d.frames.shape[0] == int(out.summary_host()["frames"]) and len({f["length"] > 65535 for f in d.frames}) == 2
    assert np.array_equal(out.frames_host()["payload_off"], d.frames["payload_off"])  # the decode's own arena layout
    got = dict(summary=res.summary_host(), messages=res.messages_host(), msg_of=res.msg_of_host(),
               conn_msg=res.conn_msg_host(), state=None)
    want = d.model()
    assert want["errors"] > 5 and want["frames"] > 500
    mm.assert_tables_equal(got, want)
    # and a second pass of the same streams on the carried state, through Engine.messages(state=)
    import torch
    state = torch.zeros((len(streams), 8), dtype=torch.uint8, device=out.frames.device)
    engine.messages(out, state=state)
    res2 = engine.messages(out, state=state, max_messages=1)  # grows once on ERR_CAPACITY
    want2 = d.model(want["state"])
    got2 = dict(summary=res2.summary_host(), messages=res2.messages_host(), msg_of=res2.msg_of_host(),
                conn_msg=res2.conn_msg_host(), state=res2.state_host())
    mm.assert_tables_equal(got2, want2, "second pass")


# ---------------------------------------------------------------------------- 7. one large frame
def test_one_large_text_frame(engine):
    rng = np.random.default_rng(0x4D6942)
    text = mixed_text(rng, 3 * 1024 * 1024 + 5)
    broken = bytearray(text)
    asciify(broken, len(text) - 2, len(text) - 1)
    broken[-2] = 0xC3  # a lead byte followed by ASCII
    d = mm.Decoded([[(1, 0, T, text)], [(1, 0, T, bytes(broken))], [(1, 0, B, bytes(broken))]])
    got = mm.run_device(engine, d)
    assert list(got["conn_msg"]["error"]) == [mm.OK, mm.ERR_UTF8, mm.OK]
    assert list(got["conn_msg"]["error_frame"]) == [mm.NO_FRAME, 1, mm.NO_FRAME]
    assert list(got["messages"]["status"]) == [mm.OK, mm.ERR_UTF8, mm.OK]
    assert int(got["summary"]["payload_len"]) == 2 * len(text) and int(got["summary"]["errors"]) == 1
