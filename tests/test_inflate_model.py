"""The inflate verdict rules on the CPU: the Python model of
tests/_inflate_model.py pinned against zlib's raw inflate, and the host build
of the device's decode core (gevws_inflate_raw) pinned against both.

zlib is the authority.  Over intact, bit-flipped, truncated and random streams:
  (a) what zlib's compressor makes comes back OK and byte-equal;
  (b) wherever zlib raises, the model fails;
  (c) wherever the model says OK, zlib raised nothing and returned the same bytes;
  (d) where both stop short, their bytes agree on the common prefix.
"zlib raises exactly when the model says malformed" is not required: at the end
of the input zlib may still be waiting for bits where the model already knows
(truncation and malformation share one error code for that reason)."""
import functools
import zlib

import numpy as np
import pytest

import gev_amd
from tests import _inflate_corpus as ic
from tests import _inflate_model as im


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(0x696E666C)
    return ic.valid_streams(rng), ic.malformed_streams(rng, 4000)


def test_what_zlib_compresses_comes_back():
    valid, _ = corpus()
    assert len(valid) == len(ic.LEVELS) * len(ic.STRATEGIES) * 4
    for payload, data in valid:
        assert im.inflate(payload) == (im.OK, data)
        assert ic.zlib_inflate(payload) == (False, data)


def test_model_against_zlib_on_malformed_streams():
    _, bad = corpus()
    oks = fails = 0
    for p in bad:
        st, out = im.inflate(p)
        raised, z = ic.zlib_inflate(p)
        if raised:
            assert st == im.ERR_DEFLATE, p.hex()                       # (b)
        if st == im.OK:
            assert not raised and z == out, p.hex()                    # (c)
            oks += 1
        else:
            assert st == im.ERR_DEFLATE, p.hex()
            fails += 1
            if not raised:
                k = min(len(z), len(out))
                assert z[:k] == out[:k], p.hex()                       # (d)
    assert oks > 100 and fails > 1000  # the corpus exercises both


RFC7692_EXAMPLES = [  # section 7.2.3: payload hex -> message
    ("f248cdc9c90700", b"Hello"),                          # 7.2.3.1 one frame
    ("00050 0faff48656c6c6f00".replace(" ", ""), b"Hello"),  # 7.2.3.3 a stored block
    ("f348cdc9c9070000", b"Hello"),                        # 7.2.3.4 BFINAL set, then an empty block
    ("f248050000 00ffffcac9c90700".replace(" ", ""), b"Hello"),  # 7.2.3.5 two blocks in one message
]


@pytest.mark.parametrize("hexs,want", RFC7692_EXAMPLES)
def test_rfc7692_examples(hexs, want):
    p = bytes.fromhex(hexs)
    assert ic.zlib_inflate(p) == (False, want)  # the hex string itself, checked against zlib first
    assert im.inflate(p) == (im.OK, want)
    assert gev_amd.inflate_raw(p, 64) == (gev_amd.MSG_OK, want)


def test_rfc7692_fragmented_example_is_the_same_stream():
    # 7.2.3.1: the frames 41 03 f2 48 cd / 80 04 c9 c9 07 00 carry the one-frame payload in two parts
    assert bytes.fromhex("f248cd") + bytes.fromhex("c9c90700") == bytes.fromhex(RFC7692_EXAMPLES[0][0])


def test_rfc7692_context_takeover_example_is_refused():
    # 7.2.3.2: the second "Hello" points into the first message's window; with
    # no context takeover the window is empty and the distance is too far
    p = bytes.fromhex("f200110000")
    assert ic.zlib_inflate(p)[0]
    assert im.inflate(p)[0] == im.ERR_DEFLATE
    assert gev_amd.inflate_raw(p, 64)[0] == gev_amd.MSG_ERR_DEFLATE


def test_host_decoder_equals_the_model_and_zlib():
    valid, bad = corpus()
    for payload, data in valid:
        assert gev_amd.inflate_raw(payload, len(data) + 3) == (gev_amd.MSG_OK, data)
    for p in bad:
        st, out = im.inflate(p)
        for cap in (1 << 16, max(len(out) - 1, 1), 1):
            assert gev_amd.inflate_raw(p, cap) == im.inflate(p, cap), (p.hex(), cap)


def test_output_limit():
    rng = np.random.default_rng(5)
    for level in ic.LEVELS:
        data = ic.sample(rng, 3000, 0)
        p = ic.deflate(data, level)
        n = len(data)
        assert gev_amd.inflate_raw(p, n) == (gev_amd.MSG_OK, data)
        assert gev_amd.inflate_raw(p, n - 1) == (gev_amd.MSG_ERR_TOO_BIG, data[:n - 1])
        assert gev_amd.inflate_raw(p, 1) == (gev_amd.MSG_ERR_TOO_BIG, data[:1])
        assert im.inflate(p, n - 1) == (im.ERR_TOO_BIG, data[:n - 1]) and im.inflate(p, 1) == (im.ERR_TOO_BIG, data[:1])


def test_a_mebibyte_of_zeros():
    data = bytes(1 << 20)
    p = ic.deflate(data, 9)
    assert len(p) == 1033  # 1 MiB in 1 033 bytes of payload: the limit is what bounds the work
    assert gev_amd.inflate_raw(p, 1 << 20) == (gev_amd.MSG_OK, data)
    assert gev_amd.inflate_raw(p, (1 << 20) - 1)[0] == gev_amd.MSG_ERR_TOO_BIG
    st, out = gev_amd.inflate_raw(p, 1)
    assert (st, out) == (gev_amd.MSG_ERR_TOO_BIG, b"\0")


def test_the_empty_message():
    # RFC 7692 section 7.2.3.6: an empty message is the one byte 00 (with the tail, an empty stored block)
    assert ic.deflate(b"") == b"\x00"
    assert im.inflate(b"\x00") == (im.OK, b"") and gev_amd.inflate_raw(b"\x00", 8) == (gev_amd.MSG_OK, b"")
    assert zlib.decompressobj(-15).decompress(b"\x00" + im.TAIL) == b""
    # no payload at all: the tail alone is a stored block cut short
    assert im.inflate(b"")[0] == im.ERR_DEFLATE and gev_amd.inflate_raw(b"", 8)[0] == gev_amd.MSG_ERR_DEFLATE
