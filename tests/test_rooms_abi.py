"""CPU checks of the rooms' addition to the C ABI: libgevws.so exports
gevws_reply_rooms_async and gevws_room_plan_async with the header's argument
counts, the ABI version is unchanged, an invalid call fails before any device is
touched, and the Python layer has its entry points.  No device compute is
called here."""
import ctypes
import inspect
import os
import re

import gev_amd
from gev_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
REPLY, PLAN = "gevws_reply_rooms_async", "gevws_room_plan_async"
NARGS = {REPLY: 24, PLAN: 33}
FLAGS = {REPLY: 15, PLAN: 28}   # argument positions
MAX_SENDS = 30


def test_library_exports_both_calls():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(HEADER).read()
    for name in (REPLY, PLAN):
        assert hasattr(lib, name), name
        restype, args = _abi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(args) == NARGS[name], name
        assert args[FLAGS[name]] is ctypes.c_uint32, name
        assert args[FLAGS[name] - 1] is ctypes.c_uint32 and args[FLAGS[name] - 2] is ctypes.c_uint32, name
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1), flags=re.S)
        assert len(decl.split(",")) == NARGS[name], name
    assert _abi.SIGNATURES[PLAN][1][MAX_SENDS] is ctypes.c_uint64
    assert re.search(r"#define GEVWS_ROOM_NONE 0xFFFFFFFFu\b", text) and _abi.ROOM_NONE == 0xFFFFFFFF
    assert re.search(r"#define GEVWS_ROOMS_SKIP_SENDER 1u\b", text) and _abi.ROOMS_SKIP_SENDER == 1


def test_abi_version_is_still_3():
    assert gev_amd.lib.gevws_abi_version() == 3
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", open(HEADER).read())


def _args(name, fill):
    """The call's arguments: every pointer `fill(i)`, every integer 2."""
    _, types = _abi.SIGNATURES[name]
    return [fill(i) if t is ctypes.c_void_p else 2 for i, t in enumerate(types)]


def test_bad_flags_fail_the_call_without_a_device():
    """The flag check comes first: with every pointer NULL and with a buffer
    for each, any other bit is GEVWS_ERR_INVALID and nothing is written."""
    raw = (ctypes.c_uint8 * 8192)(*([0xEE] * 8192))
    base = ctypes.addressof(raw)
    for name in (REPLY, PLAN):
        fn = getattr(gev_amd.lib, name)
        for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
            for fill in (lambda i: None, lambda i: base + 128 * i):
                a = _args(name, fill)
                a[0] = None            # no context either way
                a[FLAGS[name]] = flags
                assert fn(*a) == _abi.ERR_INVALID, (name, flags)
        # a valid flag word with a NULL context is invalid too
        for flags in (0, _abi.ROOMS_SKIP_SENDER):
            a = _args(name, lambda i: None)
            a[FLAGS[name]] = flags
            assert fn(*a) == _abi.ERR_INVALID, (name, flags)
    assert bytes(raw) == b"\xee" * len(raw)


def test_max_sends_of_2_32_fails_the_call_without_a_device():
    raw = (ctypes.c_uint8 * 8192)(*([0xEE] * 8192))
    base = ctypes.addressof(raw)
    fn = gev_amd.lib.gevws_room_plan_async
    for max_sends in (1 << 32, (1 << 32) + 1, (1 << 64) - 1):
        for fill in (lambda i: None, lambda i: base + 128 * i):
            a = _args(PLAN, fill)
            a[0] = None
            a[FLAGS[PLAN]] = 0
            a[MAX_SENDS] = max_sends
            assert fn(*a) == _abi.ERR_INVALID, max_sends
    assert bytes(raw) == b"\xee" * len(raw)


def test_python_entry_points():
    assert callable(gev_amd.Engine.reply_rooms_async) and callable(gev_amd.Engine.room_plan_async)
    sig = inspect.signature(gev_amd.Engine.broadcast).parameters
    assert [sig[k].default for k in ("window_bits", "flags", "rooms_flags", "control_flags", "gather")] == [
        None, 0, 0, 0, False]
    assert list(sig)[:7] == ["self", "out", "msgs", "bodies", "policy", "conn_ext", "rooms"]
    assert set(gev_amd.Rooms.__dataclass_fields__) == {"conn_room", "room_first", "room_members", "n_rooms"}
    assert callable(gev_amd.Rooms.from_conn_room)
    assert gev_amd.ROOM_NONE == 0xFFFFFFFF and gev_amd.ROOMS_SKIP_SENDER == 1
    assert "Responses" in str(inspect.signature(gev_amd.Engine.broadcast).return_annotation)
