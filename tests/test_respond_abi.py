"""CPU checks of the control step's and the send plan's additions to the C ABI:
libgevws.so exports both entry points, the three records have the header's
layout in ctypes and numpy, the constants are there and agree with
include/gevws.h, and an unknown flag fails the call before any device is
touched.  No device compute is called here."""
import ctypes
import os
import re

import gev_amd
from gev_amd import _abi
from tests import _respond_model as rm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")


def test_library_exports_control_and_plan():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("gevws_control_async", "gevws_send_plan_async"):
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES
    assert len(_abi.SIGNATURES["gevws_control_async"][1]) == 24
    assert len(_abi.SIGNATURES["gevws_send_plan_async"][1]) == 26
    assert gev_amd.lib.gevws_abi_version() == 3


def test_record_layouts():
    for struct, dtype, model, want in (
            (_abi.ConnCtl, gev_amd.CONN_CTL_DTYPE, rm.CONN_CTL_DTYPE,
             dict(cut_frame=0, close_code=8, flags=12, reserved=16)),
            (_abi.Send, gev_amd.SEND_DTYPE, rm.SEND_DTYPE, dict(off=0, len=8, frame=16, conn=24, wire=28)),
            (_abi.ConnSend, gev_amd.CONN_SEND_DTYPE, rm.CONN_SEND_DTYPE,
             dict(first=0, count=8, bytes=16, flags=24, reserved=28))):
        assert ctypes.sizeof(struct) == dtype.itemsize == model.itemsize == 32, struct
        assert [n for n, _ in struct._fields_] == list(dtype.names) == list(model.names) == list(want)
        for f, o in want.items():
            assert getattr(struct, f).offset == o, (struct, f)
            assert dtype.fields[f][1] == o and model.fields[f][1] == o, (struct, f)
            assert getattr(struct, f).size == dtype.fields[f][0].itemsize, (struct, f)


def test_constants_agree_with_the_header():
    text = open(HEADER).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (GEVWS_\w+)\s+(\d+)u?\b", text)}
    assert defines["GEVWS_CONTROL_NO_PING_FOR_PONG"] == gev_amd.CONTROL_NO_PING_FOR_PONG == rm.NO_PING_FOR_PONG == 1
    assert defines["GEVWS_CTL_SHUTDOWN"] == gev_amd.CTL_SHUTDOWN == rm.SHUTDOWN == 1
    assert defines["GEVWS_CTL_FAILED"] == gev_amd.CTL_FAILED == rm.FAILED == 2
    assert defines["GEVWS_AUX_SLOT"] == _abi.AUX_SLOT == rm.AUX_SLOT == 128
    assert re.search(r"GEVWS_MSG_ERR_CLOSED = 9\b", text) and gev_amd.MSG_ERR_CLOSED == rm.ERR_CLOSED == 9
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", text)
    assert (gev_amd.WIRE_PLAIN, gev_amd.WIRE_DEFLATED, gev_amd.WIRE_CONTROL) == (0, 1, 2)
    for name in ("control_async", "send_plan_async", "respond", "echo_messages"):
        assert callable(getattr(gev_amd.Engine, name)), name
    for name in ("conn_bytes", "conn_send_host", "send_host"):
        assert callable(getattr(gev_amd.Responses, name)), name


def test_unknown_control_flags_fail_the_call_without_a_device():
    """The flag check comes first: with every pointer NULL, and with a buffer
    for each, any bit but NO_PING_FOR_PONG is GEVWS_ERR_INVALID and nothing is
    written (a valid flag word with a NULL context is invalid too)."""
    nulls = [None] * 24
    buf = (ctypes.c_uint8 * 256)(*([0xEE] * 256))
    p = ctypes.addressof(buf)
    ptrs = [None, None, p, 4, p, 2, p, p, 0, 256, p, p, 4, p, p, p, p, 0, p, p, p, p, p, p]
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
        for args in (nulls, ptrs):
            a = list(args)
            a[3] = a[3] or 0
            a[5], a[8], a[9], a[12] = a[5] or 0, a[8] or 0, a[9] or 0, a[12] or 0
            a[17] = flags
            assert gev_amd.lib.gevws_control_async(*a) == _abi.ERR_INVALID, flags
    a = list(ptrs)
    a[17] = gev_amd.CONTROL_NO_PING_FOR_PONG
    assert gev_amd.lib.gevws_control_async(*a) == _abi.ERR_INVALID  # no context
    assert bytes(buf) == b"\xee" * 256
