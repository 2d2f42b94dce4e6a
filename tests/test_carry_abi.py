"""CPU checks of the carry addition to the C ABI: libgevws.so exports
gevws_join_carry_async with its 26 arguments, gevws_carry has the header's
layout in ctypes and numpy, and the constants are there.  No device compute is
called here."""
import ctypes

import gev_amd
from gev_amd import _abi


def test_library_exports_join_carry():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "gevws_join_carry_async")
    restype, args = _abi.SIGNATURES["gevws_join_carry_async"]
    assert restype is ctypes.c_int and len(args) == 26
    # the 16 arguments of gevws_join_async, unchanged, in front
    assert args[:16] == _abi.SIGNATURES["gevws_join_async"][1]
    assert [args[i] for i in (17, 18, 21, 24)] == [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.c_uint64]


def test_carry_layout():
    assert ctypes.sizeof(_abi.Carry) == gev_amd.CARRY_DTYPE.itemsize == 32
    want = dict(off=0, length=8, opcode=16, flags=17, status=18, reserved=19)
    for f, o in want.items():
        assert getattr(_abi.Carry, f).offset == o, f
        assert gev_amd.CARRY_DTYPE.fields[f][1] == o, f


def test_constants():
    assert (gev_amd.CARRY_OPEN, gev_amd.CARRY_LOST) == (1, 2)
    assert (_abi.CARRY_OPEN, _abi.CARRY_LOST) == (1, 2)
    assert gev_amd.lib.gevws_abi_version() == 3
    for name in ("join_carry_async", "join"):
        assert callable(getattr(gev_amd.Engine, name)), name
    assert callable(gev_amd.Carry.records_host) and callable(gev_amd.Carry.carried_bytes)
