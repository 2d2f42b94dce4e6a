"""gevws_deflate_negotiate_flags: the permessage-deflate answer of a server
whose inflate step keeps a window per connection (client context takeover),
and the conn_ext byte that goes with it.  Flags 0 is gevws_deflate_negotiate."""
import ctypes

import pytest

import gev_amd
from gev_amd import _abi
from tests import test_deflate_negotiate as base

KEEP = b"permessage-deflate; server_no_context_takeover"
NO = base.BASE
TAKE = gev_amd.NEGOTIATE_CLIENT_TAKEOVER
DEFLATE, BOTH = gev_amd.EXT_DEFLATE, gev_amd.EXT_DEFLATE | gev_amd.EXT_CLIENT_TAKEOVER


def offers_of(test):
    for mark in test.pytestmark:
        if mark.name == "parametrize":
            return [case[0] if isinstance(case, tuple) else case for case in mark.args[1]]
    raise AssertionError("no parametrize mark")


def test_flags_zero_is_deflate_negotiate():
    offers = offers_of(base.test_accepted_forms) + offers_of(base.test_refused_offers)
    assert len(offers) == 30
    for offer in offers:
        want = gev_amd.deflate_negotiate(offer)
        assert gev_amd.deflate_negotiate_ext(offer, 0) == (want, DEFLATE if want else 0), offer


@pytest.mark.parametrize("offer,answer,ext", [
    # plain offers: the client may keep its window
    (b"permessage-deflate", KEEP, BOTH),
    (b"permessage-deflate; server_no_context_takeover", KEEP, BOTH),
    (b"  permessage-deflate ;\tclient_max_window_bits ", KEEP, BOTH),
    # the offer carried client_no_context_takeover: echoed, the bit stays clear
    (b"permessage-deflate; client_no_context_takeover", NO, DEFLATE),
    (b"permessage-deflate;server_no_context_takeover;client_no_context_takeover;client_max_window_bits", NO, DEFLATE),
    (b"permessage-deflate; client_no_context_takeover; server_max_window_bits=9",
     NO + b"; server_max_window_bits=9", DEFLATE),
    # window bits: the server's echoed, the client's accepted and not echoed (the client then uses 15)
    (b"permessage-deflate; client_max_window_bits", KEEP, BOTH),
    (b"permessage-deflate; client_max_window_bits=10", KEEP, BOTH),
    (b"permessage-deflate; client_max_window_bits=15", KEEP, BOTH),
    (b'permessage-deflate; client_max_window_bits="9"', KEEP, BOTH),
    (b"permessage-deflate; server_max_window_bits=8", KEEP + b"; server_max_window_bits=8", BOTH),
    (b"permessage-deflate; server_max_window_bits=15; client_max_window_bits",
     KEEP + b"; server_max_window_bits=15", BOTH),
    (b'permessage-deflate; server_max_window_bits="12"', KEEP + b"; server_max_window_bits=12", BOTH),
    # unusable first offers: the first usable one is answered, and it decides the bit
    (b"x-foo, permessage-deflate; server_max_window_bits=7, permessage-deflate; mystery, "
     b"permessage-deflate; server_max_window_bits=10, permessage-deflate",
     KEEP + b"; server_max_window_bits=10", BOTH),
    (b"permessage-deflate; client_max_window_bits=16, permessage-deflate; client_no_context_takeover", NO, DEFLATE),
    (b"permessage-deflate; client_no_context_takeover; client_no_context_takeover, permessage-deflate", KEEP, BOTH),
    # malformed or unusable values: no answer, no extension
    (b"permessage-deflate; x-unknown", b"", 0),
    (b"permessage-deflate; client_no_context_takeover=yes", b"", 0),
    (b"permessage-deflate; server_max_window_bits=16", b"", 0),
    (b'permessage-deflate; a="unclosed', b"", 0),
    (b";bad", b"", 0),
    (b"", b"", 0),
])
def test_answers_with_the_takeover_flag(offer, answer, ext):
    assert gev_amd.deflate_negotiate_ext(offer, TAKE) == (answer, ext)
    assert b"server_no_context_takeover" in answer or not answer     # always sent
    assert b"client_max_window_bits" not in answer


def test_every_refused_offer_stays_refused():
    for offer in offers_of(base.test_refused_offers):
        assert gev_amd.deflate_negotiate_ext(offer, TAKE) == (b"", 0), offer


def call(offer, flags, cap, with_ext=True):
    out, n, ext = ctypes.create_string_buffer(max(cap, 1)), ctypes.c_uint64(7), ctypes.c_uint8(0xAA)
    st = gev_amd.lib.gevws_deflate_negotiate_flags(offer, len(offer), flags, out, cap, ctypes.byref(n),
                                                   ctypes.byref(ext) if with_ext else None)
    return st, out.raw[: n.value], ext.value


def test_a_bad_flag_bit_is_invalid():
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert call(b"permessage-deflate", flags, 256) == (_abi.ERR_INVALID, b"", 0)
        with pytest.raises(RuntimeError):
            gev_amd.deflate_negotiate_ext(b"permessage-deflate", flags)
    assert call(b"permessage-deflate", TAKE, 256) == (0, KEEP, BOTH)
    assert call(b"permessage-deflate", TAKE, 256, with_ext=False) == (0, KEEP, 0xAA)   # conn_ext may be NULL


def test_small_output_buffer_is_a_capacity_error():
    offer = b"permessage-deflate"
    assert call(offer, TAKE, len(KEEP) - 1) == (_abi.ERR_CAPACITY, b"", 0)
    assert call(offer, TAKE, len(KEEP)) == (0, KEEP, BOTH)
    assert call(offer, 0, len(NO) - 1) == (_abi.ERR_CAPACITY, b"", 0)
    assert call(offer, 0, len(NO)) == (0, NO, DEFLATE)
