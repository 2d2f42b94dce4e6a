"""CPU checks of the compressed-carry addition to the C ABI: libgevws.so
exports gevws_inflate_carry_async and gevws_join_carry_ext_async, the two
constants have the header's values and gevws_carry's layout is unchanged.  No
device compute is called here."""
import ctypes
import inspect
import os
import re

import gev_amd
from gev_amd import _abi


def test_library_exports_the_two_entry_points():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "gevws_inflate_carry_async") and hasattr(lib, "gevws_join_carry_ext_async")
    restype, args = _abi.SIGNATURES["gevws_join_carry_ext_async"]
    assert restype is ctypes.c_int and len(args) == 27
    assert args[:26] == _abi.SIGNATURES["gevws_join_carry_async"][1] and args[26] is ctypes.c_uint32
    restype, args = _abi.SIGNATURES["gevws_inflate_carry_async"]
    assert restype is ctypes.c_int and len(args) == 21
    assert args[:18] == _abi.SIGNATURES["gevws_inflate_ctx_async"][1]
    assert args[18:] == [_abi.SIGNATURES["gevws_inflate_ctx_async"][1][0]] * 2 + [ctypes.c_uint64]


def test_constants_match_the_header():
    assert (gev_amd.CARRY_COMPRESSED, gev_amd.CARRY_KEEP_COMPRESSED) == (4, 1)
    assert (_abi.CARRY_COMPRESSED, _abi.CARRY_KEEP_COMPRESSED) == (4, 1)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
    with open(header) as f:
        text = f.read()
    assert re.search(r"#define GEVWS_CARRY_COMPRESSED 4u\b", text)
    assert re.search(r"#define GEVWS_CARRY_KEEP_COMPRESSED 1u\b", text)
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", text) and gev_amd.lib.gevws_abi_version() == 3
    assert (gev_amd.CARRY_OPEN, gev_amd.CARRY_LOST) == (1, 2)


def test_carry_layout_is_unchanged():
    assert ctypes.sizeof(_abi.Carry) == gev_amd.CARRY_DTYPE.itemsize == 32
    want = dict(off=0, length=8, opcode=16, flags=17, status=18, reserved=19)
    for f, o in want.items():
        assert getattr(_abi.Carry, f).offset == o, f
        assert gev_amd.CARRY_DTYPE.fields[f][1] == o, f


def test_python_surface():
    for name in ("inflate_carry_async", "join_carry_ext_async"):
        assert callable(getattr(gev_amd.Engine, name)), name
    p = inspect.signature(gev_amd.Carry.__init__).parameters
    assert p["compressed"].default is False and p["arena_bytes"].default == 0
    assert inspect.signature(gev_amd.Engine.inflate).parameters["carry"].default is None
