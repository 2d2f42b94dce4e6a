"""CPU checks of the message layer: the host gevws_utf8_valid against
bytes.decode, the new structs' layouts, and the Python model the GPU tests
compare the device tables with (tests/_messages_model.py) pinned against
bytes.decode and codecs' incremental decoder.  No device work."""
import codecs
import ctypes

import numpy as np

import gev_amd
from gev_amd import _abi

from tests import _messages_model as mm

UTF8_CASES = [b"", b"bye", "héllo wörld ✓ 日本".encode(), b"\xf0\x9f\x98\x80ok", b"\xff", b"\xc0\xaf",
              b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xf4\x8f\xbf\xbf",
              b"\xf4\x90\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xc2", b"\xe2\x82", b"\xf0\x9f\x98",
              b"\x80", b"\xbf", b"a\x80", b"\xc2\xc2\xa0", b"\xe2\x82\xac\xac", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80",
              b"\xc1\xbf", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xe0\x9f\xbf", b"\xef\xbf\xbf", b"\x00", b"\x7f",
              b"ab\xe2\x82\xacd" * 9, "\U0010FFFFࠀ߿\x7f".encode()]


def py_valid(b: bytes) -> bool:
    try:
        b.decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def random_text(rng, n_chars: int) -> str:
    """A mix of 1-, 2-, 3- and 4-byte characters (no surrogates)."""
    ranges = [(0x20, 0x7F), (0x80, 0x800), (0x800, 0xD800), (0xE000, 0x10000), (0x10000, 0x110000)]
    return "".join(chr(int(rng.integers(*ranges[int(rng.integers(0, len(ranges)))]))) for _ in range(n_chars))


def mutated(rng, b: bytes) -> bytes:
    b = bytearray(b)
    for _ in range(int(rng.integers(0, 3))):
        if not b:
            break
        i, how = int(rng.integers(0, len(b))), int(rng.integers(0, 3))
        if how == 0:
            b[i] = int(rng.integers(0, 256))
        elif how == 1:
            del b[i]
        else:
            b.insert(i, int(rng.choice([0x80, 0xBF, 0xC0, 0xE0, 0xED, 0xF0, 0xF4, 0xF5, 0xFF])))
    return bytes(b)


# ---------------------------------------------------------------------------- the host entry point
def test_utf8_valid_edge_cases():
    for b in UTF8_CASES:
        assert gev_amd.utf8_valid(b) == py_valid(b), b
    assert gev_amd.lib.gevws_utf8_valid(None, 0) == 1


def test_utf8_valid_every_two_byte_string():
    for a in range(256):
        for b in range(256):
            s = bytes([a, b])
            assert gev_amd.utf8_valid(s) == py_valid(s), s
    for a in range(256):
        assert gev_amd.utf8_valid(bytes([a])) == py_valid(bytes([a])), a


def test_utf8_valid_three_and_four_byte_grid():
    tails = [0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xFF]
    for a in range(0xC0, 0x100):
        for b in tails:
            for c in tails:
                for s in (bytes([a, b, c]), bytes([a, b, c, 0x80]), bytes([a, b, c, 0xBF, 0x41])):
                    assert gev_amd.utf8_valid(s) == py_valid(s), s


def test_utf8_valid_random_strings():
    rng = np.random.default_rng(0x7574)
    for _ in range(3000):
        kind = rng.random()
        if kind < 0.3:
            s = bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8))
        else:
            s = mutated(rng, random_text(rng, int(rng.integers(0, 40))).encode())
        assert gev_amd.utf8_valid(s) == py_valid(s), s


def test_new_struct_layouts_match_dtypes():
    for struct, dtype, size in ((_abi.MsgState, gev_amd.MSG_STATE_DTYPE, 8), (_abi.Message, gev_amd.MESSAGE_DTYPE, 32),
                                (_abi.ConnMsg, gev_amd.CONN_MSG_DTYPE, 32)):
        assert ctypes.sizeof(struct) == dtype.itemsize == size
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
            assert getattr(struct, name).size == dtype.fields[name][0].itemsize, name
    for dt, mine in ((gev_amd.MSG_STATE_DTYPE, mm.MSG_STATE_DTYPE), (gev_amd.MESSAGE_DTYPE, mm.MESSAGE_DTYPE),
                     (gev_amd.CONN_MSG_DTYPE, mm.CONN_MSG_DTYPE), (gev_amd.FRAME_DTYPE, mm.FRAME_DTYPE),
                     (gev_amd.CONN_OUT_DTYPE, mm.CONN_OUT_DTYPE), (gev_amd.SUMMARY_DTYPE, mm.SUMMARY_DTYPE)):
        assert dt == mine
    assert (_abi.MSG_OK, _abi.MSG_ERR_RSV, _abi.MSG_ERR_OPCODE, _abi.MSG_ERR_CONTROL, _abi.MSG_ERR_CONTINUATION,
            _abi.MSG_ERR_INTERLEAVE, _abi.MSG_ERR_UTF8) == tuple(range(7))
    assert (_abi.MSG_BEGIN, _abi.MSG_END) == (mm.BEGIN, mm.END) == (1, 2)


# ---------------------------------------------------------------------------- the model itself
def incremental_failure(fragments):
    """The fragment at which codecs' incremental decoder raises (final= set on
    the last one), or None.  One correction: CPython holds back a truncated
    surrogate -- ED A0..BF at the very end of a non-final chunk -- as if it
    were incomplete (it exists for the surrogatepass handler) and raises at
    the next chunk; the byte after ED cannot continue a valid sequence, so the
    contract fails the frame that holds it."""
    dec = codecs.getincrementaldecoder("utf-8")("strict")
    for i, frag in enumerate(fragments):
        try:
            dec.decode(frag, final=i == len(fragments) - 1)
        except UnicodeDecodeError:
            return i
        held = dec.getstate()[0]
        if len(held) == 2 and held[0] == 0xED and held[1] >= 0xA0:
            return i
    return None


def random_split(rng, b: bytes):
    k = int(rng.integers(1, 6))
    cuts = sorted(int(rng.integers(0, len(b) + 1)) for _ in range(k - 1))
    return [b[i:j] for i, j in zip([0] + cuts, cuts + [len(b)])]


def test_model_utf8_machine_matches_python_decoders():
    rng = np.random.default_rng(0x6D6F64)
    cases = [[c] for c in UTF8_CASES]
    for c in UTF8_CASES:
        for i in range(len(c) + 1):
            cases.append([c[:i], c[i:]])
    for _ in range(1500):
        cases.append(random_split(rng, mutated(rng, random_text(rng, int(rng.integers(0, 12))).encode())))
    for frags in cases:
        ok, at = mm.text_message_verdict(frags)
        assert ok == py_valid(b"".join(frags)), frags
        assert at == incremental_failure(frags), frags


def test_model_tables_on_fragmented_streams():
    """The whole model on hand-built connections: a message per fragment list,
    verdict and failing frame as the incremental decoder's."""
    rng = np.random.default_rng(0x6D6F65)
    for _ in range(200):
        b = mutated(rng, random_text(rng, int(rng.integers(0, 10))).encode())
        frags = random_split(rng, b)
        conn = [(i == len(frags) - 1, 0, 1 if i == 0 else 0, f) for i, f in enumerate(frags)]
        ping = (True, 0, 9, b"\xff")  # a control frame somewhere after the first fragment: in no message
        conn.insert(int(rng.integers(1, len(conn) + 1)), ping)
        data = [i for i, fr in enumerate(conn) if fr[2] != 9]
        d = mm.Decoded([conn])
        want = d.model()
        at = incremental_failure(frags)
        cm = want["conn_msg"][0]
        if at is None:
            assert int(cm["error"]) == mm.OK and int(cm["error_frame"]) == mm.NO_FRAME
            m = want["messages"][0]
            assert (int(m["flags"]), int(m["status"]), int(m["nframes"]), int(m["length"])) == \
                (mm.BEGIN | mm.END, mm.OK, len(frags), len(b))
            assert want["frames"] == 1 and list(np.flatnonzero(want["msg_of"] == -1)) == [conn.index(ping)]
            assert want["state"][0].tobytes() == bytes(8)
        else:
            assert int(cm["error"]) == mm.ERR_UTF8 and int(cm["error_frame"]) == data[at]
            m = want["messages"][0]
            assert (int(m["flags"]), int(m["status"]), int(m["nframes"])) == (mm.BEGIN, mm.ERR_UTF8, at + 1)
            assert int(m["length"]) == sum(len(f) for f in frags[: at + 1])
            assert int(want["state"][0]["failed"]) == mm.ERR_UTF8 and want["errors"] == 1


def test_model_protocol_rules_and_carry():
    T, B, C, PING = 1, 2, 0, 9
    d = mm.Decoded([
        [(1, 0, T, b"a"), (0, 0, B, b"\xff"), (1, 0, PING, b""), (1, 0, C, b"\xfe")],   # ok: text, binary in 2
        [(1, 4, T, b"a")],                                                              # rsv
        [(1, 0, T, b"a"), (1, 0, 3, b"")],                                              # reserved opcode
        [(0, 0, T, b"a"), (0, 0, PING, b"")],                                           # fragmented ping
        [(1, 0, C, b"a")],                                                              # nothing to continue
        [(0, 0, T, b"a"), (1, 0, B, b"b")],                                             # interleave
        [(1, 1, 0xB, b"x" * 200)],                                                      # rsv before opcode
        (mm.ERR_LEN_MSB, [(1, 0, T, b"\xff")]),                                         # a poisoned stream
        [],
        [(0, 0, T, b"\xe2\x82")],                                                       # open, mid-sequence
    ])
    w = d.model()
    assert list(w["conn_msg"]["error"]) == [0, 1, 2, 3, 4, 5, 1, 0, 0, 0]
    assert list(w["conn_msg"]["nmessages"]) == [2, 0, 1, 1, 0, 1, 0, 0, 0, 1]
    assert w["errors"] == 6 and w["frames"] == 6
    last = w["state"][9]
    assert (int(last["opcode"]), int(last["utf8_n"]), bytes(last["utf8"][:2])) == (1, 2, b"\xe2\x82")
    # the carried message: finished by the next pass, no BEGIN flag
    d2 = mm.Decoded([[] for _ in range(9)] + [[(1, 0, C, b"\xac!")]])
    w2 = d2.model(w["state"])
    m = w2["messages"][0]
    assert (int(m["opcode"]), int(m["flags"]), int(m["status"]), int(m["conn"])) == (1, mm.END, 0, 9)
    assert w2["state"][9].tobytes() == bytes(8)
    assert int(w2["state"][1]["failed"]) == mm.ERR_RSV  # sticky; a connection without frames keeps its state
    d3 = mm.Decoded([[(1, 0, T, b"ok")] for _ in range(10)])
    w3 = d3.model(w["state"])
    assert int(w3["conn_msg"]["error"][1]) == mm.ERR_RSV and int(w3["conn_msg"]["error_frame"][1]) == mm.NO_FRAME
    assert int(w3["conn_msg"]["nmessages"][1]) == 0 and w3["errors"] == 1  # conn 9: text inside an open message
