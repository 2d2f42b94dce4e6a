"""CPU checks of the room-command step's addition to the C ABI: libgevws.so
exports gevws_room_commands_async with the header's sixteen arguments and
gevws_room_command_parse, the ABI version is unchanged, GEVWS_MSG_COMMAND
continues the message enum, every invalid call fails before any device is
touched, and the Python layer has its entry points.  No device compute is
called here."""
import ctypes
import inspect
import os
import re

import gev_amd
from gev_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
NAME = "gevws_room_commands_async"
NARGS = 16
(CTX, STREAM, BODIES, MAX_MESSAGES, MSG_SUM, JOIN_SUM, CTL_SUM, OUT, SRC_BYTES, N_CONNS, N_ROOMS, FLAGS, CHANGES,
 MAX_CHANGES, CHANGE_OF, SUMMARY) = range(16)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, NAME) and hasattr(lib, "gevws_room_command_parse")
    restype, args = _abi.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(args) == NARGS
    text = open(HEADER).read()
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % NAME, text, re.S).group(1), flags=re.S)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == NARGS
    for i, p in enumerate(params):   # the binding's integer widths are the header's
        want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
        assert args[i] is want, (i, p)
    assert params[MAX_MESSAGES].endswith("max_messages") and params[MAX_CHANGES].endswith("max_changes")
    assert params[N_CONNS].endswith("n_conns") and params[N_ROOMS].endswith("n_rooms") and params[FLAGS].endswith("flags")
    assert params[BODIES].startswith("gevws_body *")          # written in place: not const
    assert _abi.SIGNATURES["gevws_room_command_parse"][0] is ctypes.c_int


def test_msg_command_continues_the_enum():
    text = open(HEADER).read()
    assert re.search(r"enum \{ GEVWS_MSG_COMMAND = 10 \};", text)
    assert re.search(r"enum \{ GEVWS_MSG_ERR_CLOSED = 9 \};", text)
    assert gev_amd.MSG_COMMAND == _abi.MSG_COMMAND == 10 == _abi.MSG_ERR_CLOSED + 1
    assert (gev_amd.CHANGE_NONE, gev_amd.CHANGE_REJECTED) == (-1, -2)


def test_abi_version_is_still_3():
    assert gev_amd.lib.gevws_abi_version() == 3
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", open(HEADER).read())


def _args(base):
    """A call that is valid but for its NULL context: every pointer a 16-aligned
    buffer of its own, two bodies, room for two changes."""
    _, types = _abi.SIGNATURES[NAME]
    a = [base + 128 * i if t is ctypes.c_void_p else 0 for i, t in enumerate(types)]
    a[CTX] = None
    a[MAX_MESSAGES], a[SRC_BYTES], a[N_CONNS], a[N_ROOMS], a[MAX_CHANGES] = 2, 64, 2, 2, 2
    return a


def test_invalid_calls_fail_without_a_device():
    raw = (ctypes.c_uint8 * 4096)(*([0xEE] * 4096))
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    fn = gev_amd.lib.gevws_room_commands_async
    assert fn(*_args(base)) == _abi.ERR_INVALID          # a NULL context, everything else in order
    cases = {}
    for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
        cases[f"flags {flags:#x}"] = {FLAGS: flags}
    for pos in (CHANGES, CHANGE_OF, SUMMARY):
        cases[f"a NULL output ({pos})"] = {pos: None}
    for n in (1 << 32, (1 << 32) + 1, (1 << 64) - 1):
        cases[f"max_messages {n:#x}"] = {MAX_MESSAGES: n}
        cases[f"max_changes {n:#x}"] = {MAX_CHANGES: n}
    for tag, edit in cases.items():
        for nulls in (False, True):   # with a buffer for every pointer, and with none at all
            a = _args(base)
            if nulls:
                a = [None if t is ctypes.c_void_p else v for v, t in zip(a, _abi.SIGNATURES[NAME][1])]
            for pos, v in edit.items():
                a[pos] = v
            assert fn(*a) == _abi.ERR_INVALID, (tag, nulls)
    assert bytes(raw) == b"\xee" * len(raw)


def test_python_entry_points():
    sig = inspect.signature(gev_amd.Engine.room_commands_async).parameters
    assert list(sig) == ["self", "bodies", "max_messages", "msg_summary", "join_summary", "ctl_summary", "out",
                         "src_bytes", "n_conns", "n_rooms", "flags", "changes", "max_changes", "change_of", "summary",
                         "stream"]
    b = inspect.signature(gev_amd.Engine.broadcast).parameters
    assert b["commands"].default is False and list(b)[-1] == "commands"
    assert gev_amd.Responses.__dataclass_fields__["room_changes"].default is None
    assert set(gev_amd.RoomChanges.__dataclass_fields__) == {"changes", "change_of", "summary", "max_changes",
                                                            "n_messages"}
    assert callable(gev_amd.RoomChanges.host) and callable(gev_amd.RoomChanges.change_of_host)
    assert callable(gev_amd.RoomChanges.summary_host)
    assert gev_amd.room_command_parse(b"/join 3", 4) == (1, 3)
    assert gev_amd.room_command_parse(b"/join 4", 4) == (2, gev_amd.ROOM_NONE)
    assert gev_amd.room_command_parse(b"/leave", 0) == (1, gev_amd.ROOM_NONE)
    assert gev_amd.room_command_parse(b"/leave ", 4) == (0, gev_amd.ROOM_NONE)
    for name in ("RoomChanges", "room_command_parse", "MSG_COMMAND"):
        assert name in gev_amd.__all__
