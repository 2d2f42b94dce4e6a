"""CPU checks of the membership update's addition to the C ABI: libgevws.so
exports gevws_rooms_update_async with the header's fifteen arguments, the ABI
version is unchanged, every invalid call fails before any device is touched,
and the Python layer has its entry points.  No device compute is called here."""
import ctypes
import inspect
import os
import re

import numpy as np

import gev_amd
from gev_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
NAME = "gevws_rooms_update_async"
NARGS = 15
# argument positions
(CTX, STREAM, IN, N_CONNS, N_ROOMS, CHANGES, MAX_CHANGES, PREV, CONN_SEND, PLAN, FLAGS, OUT, FIRST, MEMBERS,
 SUMMARY) = range(15)


def test_library_exports_the_call():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, NAME)
    restype, args = _abi.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(args) == NARGS
    text = open(HEADER).read()
    decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\((.*?)\);" % NAME, text, re.S).group(1), flags=re.S)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == NARGS
    for i, p in enumerate(params):   # the binding's integer widths are the header's
        want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
        assert args[i] is want, (i, p)
    assert args[MAX_CHANGES] is ctypes.c_uint64 and args[FLAGS] is ctypes.c_uint32
    assert params[N_CONNS].endswith("n_conns") and params[N_ROOMS].endswith("n_rooms")
    m = re.search(r"typedef struct gevws_room_change \{(.*?)\} gevws_room_change;", text, re.S)
    fields = re.findall(r"uint32_t (\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["conn", "room"]
    assert gev_amd.ROOM_CHANGE_DTYPE.itemsize == 8 and gev_amd.ROOM_CHANGE_DTYPE.names == ("conn", "room")
    assert [gev_amd.ROOM_CHANGE_DTYPE.fields[k][1] for k in ("conn", "room")] == [0, 4]


def test_abi_version_is_still_3():
    assert gev_amd.lib.gevws_abi_version() == 3
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", open(HEADER).read())


def _args(base):
    """A call that is valid but for its NULL context: every pointer a buffer of
    its own, two connections, two rooms, one change."""
    _, types = _abi.SIGNATURES[NAME]
    a = [base + 128 * i if t is ctypes.c_void_p else 0 for i, t in enumerate(types)]
    a[CTX] = None
    a[N_CONNS], a[N_ROOMS], a[MAX_CHANGES] = 2, 2, 1
    return a


def test_invalid_calls_fail_without_a_device():
    raw = (ctypes.c_uint8 * 4096)(*([0xEE] * 4096))
    base = ctypes.addressof(raw)
    fn = gev_amd.lib.gevws_rooms_update_async
    # a NULL context, everything else in order
    assert fn(*_args(base)) == _abi.ERR_INVALID
    cases = {}
    for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
        cases[f"flags {flags:#x}"] = {FLAGS: flags}
    for pos in (OUT, FIRST, MEMBERS, SUMMARY):
        cases[f"a NULL output ({pos})"] = {pos: None}
    cases["no input for two connections"] = {IN: None}
    cases["the output is the input"] = {OUT: base + 128 * IN}
    for n in (1 << 32, (1 << 32) + 1, (1 << 64) - 1):
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
    assert callable(gev_amd.Engine.rooms_update_async)
    sig = inspect.signature(gev_amd.Engine.rooms_update_async).parameters
    assert list(sig) == ["self", "conn_room_in", "n_conns", "n_rooms", "changes", "max_changes", "prev", "conn_send",
                         "plan_summary", "flags", "conn_room_out", "room_first_out", "room_members_out", "summary",
                         "stream"]
    b = inspect.signature(gev_amd.Rooms.build).parameters
    assert list(b) == ["engine", "conn_room", "n_rooms", "stream"] and b["stream"].default is None
    u = inspect.signature(gev_amd.Rooms.update).parameters
    assert list(u) == ["self", "engine", "changes", "closed", "n_rooms", "stream"]
    assert [u[k].default for k in ("changes", "closed", "n_rooms", "stream")] == [None] * 4
    assert "Rooms" in str(inspect.signature(gev_amd.Rooms.update).return_annotation)
    # methods only: the dataclass is what the room calls' wrappers read
    assert set(gev_amd.Rooms.__dataclass_fields__) == {"conn_room", "room_first", "room_members", "n_rooms"}
    assert callable(gev_amd.Rooms.from_conn_room) and callable(gev_amd.Rooms.csr)
    assert "ROOM_CHANGE_DTYPE" in gev_amd.__all__
    ch = np.zeros(2, gev_amd.ROOM_CHANGE_DTYPE)
    ch[1] = (3, gev_amd.ROOM_NONE)
    assert ch.view(np.uint32).tolist() == [0, 0, 3, 0xFFFFFFFF]
