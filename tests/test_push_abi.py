"""CPU checks of the push pass's addition to the C ABI: libgevws.so exports
gevws_push_lists_async, gevws_push_plan_async and gevws_push_check with the
header's argument counts, gevws_push has the header's layout, the ABI version is
unchanged, an invalid call fails before any device is touched, and the Python
layer has its entry points.  No device compute is called here."""
import ctypes
import inspect
import os
import re

import numpy as np

import gev_amd
from gev_amd import _abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
LISTS, PLAN, CHECK = "gevws_push_lists_async", "gevws_push_plan_async", "gevws_push_check"
NARGS = {LISTS: 22, PLAN: 27, CHECK: 5}
FLAGS = {LISTS: 15, PLAN: 22}   # argument positions
MAX_PUSHES, MAX_SENDS = 3, 24


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(HEADER).read()
    for name in (LISTS, PLAN, CHECK):
        assert hasattr(lib, name), name
        restype, args = _abi.SIGNATURES[name]
        assert restype is (ctypes.c_int64 if name == CHECK else ctypes.c_int) and len(args) == NARGS[name], name
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"int(?:64_t)? %s\((.*?)\);" % name, text, re.S).group(1),
                      flags=re.S)
        assert len(decl.split(",")) == NARGS[name], name
    for name in (LISTS, PLAN):
        args = _abi.SIGNATURES[name][1]
        assert args[FLAGS[name]] is ctypes.c_uint32 and args[MAX_PUSHES] is ctypes.c_uint64, name
        assert args[FLAGS[name] - 1] is ctypes.c_uint32 and args[FLAGS[name] - 2] is ctypes.c_uint32, name
    assert _abi.SIGNATURES[PLAN][1][MAX_SENDS] is ctypes.c_uint64
    for name, val in (("ALL", 0), ("ROOM", 1), ("CONN", 2)):
        assert re.search(r"#define GEVWS_PUSH_%s %du\b" % (name, val), text), name
        assert getattr(_abi, "PUSH_" + name) == val == getattr(gev_amd, "PUSH_" + name)


def test_the_record_is_32_bytes_with_the_headers_fields():
    text = open(HEADER).read()
    body = re.search(r"typedef struct gevws_push \{(.*?)\} gevws_push;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[.*\]", "", f.split()[-1]) for f in body.split(";") if f.strip()]
    assert fields == ["off", "length", "target", "kind", "opcode", "reserved"]
    assert ctypes.sizeof(_abi.Push) == 32 == gev_amd.PUSH_DTYPE.itemsize
    want = dict(off=0, length=8, target=16, kind=20, opcode=21, reserved=22)
    for f, o in want.items():
        assert getattr(_abi.Push, f).offset == o == gev_amd.PUSH_DTYPE.fields[f][1], f
    assert gev_amd.PUSH_DTYPE.fields["reserved"][0].shape == (10,)


def test_abi_version_is_still_3():
    assert gev_amd.lib.gevws_abi_version() == 3
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", open(HEADER).read())


def _args(name, fill):
    """The call's arguments: every pointer `fill(i)`, every integer 2."""
    _, types = _abi.SIGNATURES[name]
    return [fill(i) if t is ctypes.c_void_p else 2 for i, t in enumerate(types)]


def test_invalid_calls_fail_without_a_device():
    """Any flag bit, a max_pushes / max_sends of 2^32 and a NULL context are
    GEVWS_ERR_INVALID from the call, with every pointer NULL and with a buffer
    for each, and nothing is written."""
    raw = (ctypes.c_uint8 * 8192)(*([0xEE] * 8192))
    base = ctypes.addressof(raw)
    for name in (LISTS, PLAN):
        fn = getattr(gev_amd.lib, name)
        for fill in (lambda i: None, lambda i: base + 128 * i):
            for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
                a = _args(name, fill)
                a[0] = None            # no context either way
                a[FLAGS[name]] = flags
                assert fn(*a) == _abi.ERR_INVALID, (name, flags)
            for big in (1 << 32, (1 << 32) + 1, (1 << 64) - 1):
                for pos in [MAX_PUSHES] + ([MAX_SENDS] if name == PLAN else []):
                    a = _args(name, fill)
                    a[0] = None
                    a[FLAGS[name]] = 0
                    a[pos] = big
                    assert fn(*a) == _abi.ERR_INVALID, (name, pos, big)
            a = _args(name, fill)      # a valid flag word and valid counts, no context
            a[0] = None
            a[FLAGS[name]] = 0
            assert fn(*a) == _abi.ERR_INVALID, name
    assert bytes(raw) == b"\xee" * len(raw)


def test_push_check_invalid_calls():
    assert gev_amd.lib.gevws_push_check(None, 0, 1, 1, 0) == 0
    assert gev_amd.lib.gevws_push_check(None, 1, 1, 1, 0) == _abi.ERR_INVALID
    one = np.zeros(1, gev_amd.PUSH_DTYPE)
    one["opcode"] = 1
    assert gev_amd.lib.gevws_push_check(one.ctypes.data, 1 << 32, 1, 1, 0) == _abi.ERR_INVALID
    assert gev_amd.push_check(one, 1, 0, 0) == 0


def test_python_entry_points():
    assert callable(gev_amd.Engine.push_lists_async) and callable(gev_amd.Engine.push_plan_async)
    assert callable(gev_amd.push_records) and callable(gev_amd.push_check)
    sig = inspect.signature(gev_amd.Engine.push).parameters
    assert list(sig)[:11] == ["self", "pushes", "src", "conn_ext", "rooms", "window_bits", "live", "flags", "gather",
                              "max_fragment_bytes", "stream"]
    assert [sig[k].default for k in ("rooms", "window_bits", "live", "flags", "gather", "max_fragment_bytes",
                                     "stream")] == [None, None, None, 0, False, None, None]
    assert "Responses" in str(inspect.signature(gev_amd.Engine.push).return_annotation)
    recs, arena, perm = gev_amd.push_records([])
    assert recs.dtype == gev_amd.PUSH_DTYPE and recs.size == 0 and perm.size == 0 and arena.size == gev_amd.IN_PAD
