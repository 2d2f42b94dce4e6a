"""CPU checks of the join / reply additions to the C ABI: libgevws.so exports
both entry points, gevws_body has the header's layout in ctypes and numpy, and
the constants are there.  No device compute is called here."""
import ctypes

import gev_amd
from gev_amd import _abi


def test_library_exports_join_and_reply():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("gevws_join_async", "gevws_reply_bodies_async"):
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES
    assert len(_abi.SIGNATURES["gevws_join_async"][1]) == 16
    assert len(_abi.SIGNATURES["gevws_reply_bodies_async"][1]) == 17


def test_body_layout():
    assert ctypes.sizeof(_abi.Body) == gev_amd.BODY_DTYPE.itemsize == 32
    want = dict(off=0, length=8, conn=16, opcode=20, flags=21, status=22, reserved=23)
    for f, o in want.items():
        assert getattr(_abi.Body, f).offset == o, f
        assert gev_amd.BODY_DTYPE.fields[f][1] == o, f


def test_constants():
    assert (gev_amd.JOIN_ALL, gev_amd.BODY_WHOLE, gev_amd.BODY_JOINED, gev_amd.BODY_INFLATED) == (1, 1, 2, 4)
    assert (_abi.JOIN_ALL, _abi.BODY_WHOLE, _abi.BODY_JOINED, _abi.BODY_INFLATED) == (1, 1, 2, 4)
    assert gev_amd.lib.gevws_abi_version() == 3
    for name in ("join_async", "join", "reply_bodies_async", "echo_messages"):
        assert callable(getattr(gev_amd.Engine, name)), name
