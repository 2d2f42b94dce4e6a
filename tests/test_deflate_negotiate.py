"""gevws_deflate_negotiate: the answer to a permessage-deflate offer (RFC 7692
section 7.1) from a server that inflates on the device without context
takeover and never compresses."""
import pytest

import gev_amd
from gev_amd import _abi

BASE = b"permessage-deflate; client_no_context_takeover; server_no_context_takeover"


@pytest.mark.parametrize("offer,answer", [
    (b"permessage-deflate", BASE),
    (b"permessage-deflate; client_max_window_bits", BASE),
    (b"permessage-deflate; client_max_window_bits=10", BASE),
    (b"permessage-deflate; client_max_window_bits=15", BASE),
    (b"permessage-deflate; server_no_context_takeover", BASE),
    (b"permessage-deflate; client_no_context_takeover", BASE),
    (b"permessage-deflate;server_no_context_takeover;client_no_context_takeover;client_max_window_bits", BASE),
    (b"permessage-deflate; server_max_window_bits=8", BASE + b"; server_max_window_bits=8"),
    (b"permessage-deflate; server_max_window_bits=15; client_max_window_bits",
     BASE + b"; server_max_window_bits=15"),
    (b'permessage-deflate; server_max_window_bits="12"', BASE + b"; server_max_window_bits=12"),  # quoted value
    (b'permessage-deflate; client_max_window_bits="9"', BASE),
    (b"  permessage-deflate ;\tclient_max_window_bits ", BASE),
])
def test_accepted_forms(offer, answer):
    assert gev_amd.deflate_negotiate(offer) == answer


@pytest.mark.parametrize("offer", [
    b"permessage-deflate; x-unknown",
    b"permessage-deflate; client_max_window_bits; client_max_window_bits",       # repeated
    b"permessage-deflate; server_no_context_takeover; server_no_context_takeover",
    b"permessage-deflate; server_max_window_bits",                                # needs a value
    b"permessage-deflate; server_max_window_bits=7",
    b"permessage-deflate; server_max_window_bits=16",
    b"permessage-deflate; client_max_window_bits=7",
    b"permessage-deflate; client_max_window_bits=16",
    b"permessage-deflate; server_max_window_bits=08",
    b"permessage-deflate; server_max_window_bits=1x",
    b'permessage-deflate; server_max_window_bits=""',
    b"permessage-deflate; server_no_context_takeover=1",
    b"permessage-deflate; client_no_context_takeover=yes",
    b"x-webkit-deflate-frame",
    b"permessage-deflateX",
    b"",
    b";bad",
    b'permessage-deflate; a="unclosed',
])
def test_refused_offers(offer):
    assert gev_amd.deflate_negotiate(offer) == b""


def test_first_usable_offer_wins():
    offer = (b"x-foo, permessage-deflate; server_max_window_bits=7, permessage-deflate; mystery, "
             b"permessage-deflate; server_max_window_bits=10, permessage-deflate")
    assert gev_amd.deflate_negotiate(offer) == BASE + b"; server_max_window_bits=10"
    assert gev_amd.deflate_negotiate(b"permessage-deflate; client_max_window_bits=16, permessage-deflate") == BASE


def test_small_output_buffer_is_a_capacity_error():
    import ctypes
    out, n = ctypes.create_string_buffer(8), ctypes.c_uint64(7)
    offer = b"permessage-deflate"
    assert gev_amd.lib.gevws_deflate_negotiate(offer, len(offer), out, 8, ctypes.byref(n)) == _abi.ERR_CAPACITY
    assert n.value == 0


REQ = (b"GET /chat HTTP/1.1\r\nHost: h\r\nUpgrade: websocket\r\nConnection: Upgrade\r\nSec-WebSocket-Version: 13\r\n"
       b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\n")


def _upgrade(extensions_line: bytes):
    def custom(conn, value, so_far):
        return so_far or gev_amd.deflate_negotiate(value), True
    u = gev_amd.Upgrader(extension_custom=custom)
    r = gev_amd.RingBuffer(1024)
    r.write(REQ + extensions_line + b"\r\n")
    return u.upgrade(gev_amd.Connection(upgraded=False), r)


def test_upgrader_round_trip_through_extension_custom():
    out, info, err = _upgrade(b"Sec-WebSocket-Extensions: permessage-deflate; client_max_window_bits\r\n")
    assert err is None and out.startswith(b"HTTP/1.1 101 ")
    assert info.extensions == BASE
    assert b"Sec-WebSocket-Extensions: " + BASE + b"\r\n" in out
    out, info, err = _upgrade(b"Sec-WebSocket-Extensions: x-foo, permessage-deflate; nope\r\n")
    assert err is None and out.startswith(b"HTTP/1.1 101 ") and info.extensions == b""
    assert b"Sec-WebSocket-Extensions" not in out
