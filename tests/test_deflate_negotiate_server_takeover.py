"""gevws_deflate_negotiate_takeover: the permessage-deflate answer of a server
whose deflate step may keep a window per connection too (server context
takeover), and the conn_ext byte that goes with it.  Flags 0 and 1 are
gevws_deflate_negotiate_flags byte for byte."""
import ctypes

import pytest

import gev_amd
from gev_amd import _abi
from tests import test_deflate_negotiate as base
from tests.test_deflate_negotiate_takeover import offers_of

PMD = b"permessage-deflate"
CNO, SNO = b"; client_no_context_takeover", b"; server_no_context_takeover"
CLIENT, SERVER = gev_amd.NEGOTIATE_CLIENT_TAKEOVER, gev_amd.NEGOTIATE_SERVER_TAKEOVER
D, C, S = gev_amd.EXT_DEFLATE, gev_amd.EXT_CLIENT_TAKEOVER, gev_amd.EXT_SERVER_TAKEOVER


def test_constants():
    assert (SERVER, S, gev_amd.DEF_CTX_BYTES) == (2, 4, 64 + 32768 + 8192)
    assert gev_amd.lib.gevws_abi_version() == 3


def test_flags_zero_and_one_are_negotiate_flags():
    offers = offers_of(base.test_accepted_forms) + offers_of(base.test_refused_offers)
    assert len(offers) == 30
    for offer in offers:
        for flags in (0, CLIENT):
            assert gev_amd.deflate_negotiate_takeover(offer, flags) == gev_amd.deflate_negotiate_ext(offer, flags), offer


@pytest.mark.parametrize("offer,flags,answer,ext", [
    # the server bit: server_no_context_takeover left out, the third bit set
    (PMD, SERVER, PMD + CNO, D | S),
    (b"  permessage-deflate ;\tclient_max_window_bits ", SERVER, PMD + CNO, D | S),
    (PMD + CNO, SERVER, PMD + CNO, D | S),
    # ... unless the chosen offer carried the parameter: echoed, the bit stays clear (RFC 7692 7.1.1.1)
    (PMD + SNO, SERVER, PMD + CNO + SNO, D),
    (PMD + b";client_no_context_takeover;server_no_context_takeover", SERVER, PMD + CNO + SNO, D),
    # both bits together, each decided by its own parameter
    (PMD, CLIENT | SERVER, PMD, D | C | S),
    (PMD + CNO, CLIENT | SERVER, PMD + CNO, D | S),
    (PMD + SNO, CLIENT | SERVER, PMD + SNO, D | C),
    (PMD + SNO + CNO, CLIENT | SERVER, PMD + CNO + SNO, D),
    # server_max_window_bits echoed: the window_bits of every message of the connection
    (PMD + b"; server_max_window_bits=9", SERVER, PMD + CNO + b"; server_max_window_bits=9", D | S),
    (PMD + b'; server_max_window_bits="12"; client_max_window_bits=10', CLIENT | SERVER,
     PMD + b"; server_max_window_bits=12", D | C | S),
    (PMD + SNO + b"; server_max_window_bits=15", SERVER, PMD + CNO + SNO + b"; server_max_window_bits=15", D),
    # the first usable offer decides
    (b"x-foo, permessage-deflate; mystery, permessage-deflate; server_no_context_takeover, permessage-deflate",
     CLIENT | SERVER, PMD + SNO, D | C),
    (b"permessage-deflate; server_max_window_bits=7, permessage-deflate", CLIENT | SERVER, PMD, D | C | S),
    # no usable offer: no answer, no extension
    (b"permessage-deflate; x-unknown", CLIENT | SERVER, b"", 0),
    (b"permessage-deflate; server_no_context_takeover=1", SERVER, b"", 0),
    (b"", SERVER, b"", 0),
])
def test_answers(offer, flags, answer, ext):
    assert gev_amd.deflate_negotiate_takeover(offer, flags) == (answer, ext)
    assert ext in (0, 1, 3, 5, 7)
    assert b"client_max_window_bits" not in answer


def test_every_conn_ext_value():
    seen = {gev_amd.deflate_negotiate_takeover(o, f)[1]
            for o, f in ((PMD, 0), (PMD, CLIENT), (PMD, SERVER), (PMD, CLIENT | SERVER), (b"nothing", 3))}
    assert seen == {1, 3, 5, 7, 0}


def test_every_refused_offer_stays_refused():
    for offer in offers_of(base.test_refused_offers):
        assert gev_amd.deflate_negotiate_takeover(offer, CLIENT | SERVER) == (b"", 0), offer


def call(offer, flags, cap, with_ext=True):
    out, n, ext = ctypes.create_string_buffer(max(cap, 1)), ctypes.c_uint64(7), ctypes.c_uint8(0xAA)
    st = gev_amd.lib.gevws_deflate_negotiate_takeover(offer, len(offer), flags, out, cap, ctypes.byref(n),
                                                      ctypes.byref(ext) if with_ext else None)
    return st, out.raw[: n.value], ext.value


def test_other_flag_bits_are_invalid():
    for flags in (4, 7, 8, 0x80000000, 0xFFFFFFFC):
        assert call(PMD, flags, 256) == (_abi.ERR_INVALID, b"", 0)
        with pytest.raises(RuntimeError):
            gev_amd.deflate_negotiate_takeover(PMD, flags)
    assert call(PMD, 3, 256) == (0, PMD, 7)
    assert call(PMD, 3, 256, with_ext=False) == (0, PMD, 0xAA)  # conn_ext may be NULL
    # gevws_deflate_negotiate_flags stays as it was
    with pytest.raises(RuntimeError):
        gev_amd.deflate_negotiate_ext(PMD, SERVER)


def test_small_output_buffer_is_a_capacity_error():
    want = PMD + CNO
    assert call(PMD, SERVER, len(want) - 1) == (_abi.ERR_CAPACITY, b"", 0)
    assert call(PMD, SERVER, len(want)) == (0, want, D | S)
    assert call(PMD, 3, len(PMD) - 1) == (_abi.ERR_CAPACITY, b"", 0)
    assert call(PMD, 3, len(PMD)) == (0, PMD, 7)
