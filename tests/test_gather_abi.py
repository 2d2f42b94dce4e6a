"""CPU checks of the gather's addition to the C ABI: libgevws.so exports
gevws_send_gather_async, gevws_conn_buf has the header's layout in ctypes,
numpy and the model, the ABI version is unchanged, an invalid call fails before
any device is touched, and the Python layer has its entry points.  No device
compute is called here."""
import ctypes
import inspect
import os
import re

import gev_amd
from gev_amd import _abi
from tests import _gather_model as gm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
NARGS = 14
FLAGS, BUF = 9, 10  # argument positions


def test_library_exports_the_gather():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "gevws_send_gather_async")
    assert "gevws_send_gather_async" in _abi.SIGNATURES
    restype, args = _abi.SIGNATURES["gevws_send_gather_async"]
    assert restype is ctypes.c_int and len(args) == NARGS
    assert args[3] is ctypes.c_uint64 and args[5] is ctypes.c_uint32 and args[FLAGS] is ctypes.c_uint32
    assert args[11] is ctypes.c_uint64
    text = open(HEADER).read()
    decl = re.search(r"int gevws_send_gather_async\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == NARGS


def test_abi_version_is_still_3():
    assert gev_amd.lib.gevws_abi_version() == 3
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", open(HEADER).read())


def test_conn_buf_layout():
    want = dict(off=0, bytes=8, flags=16, reserved=20)
    struct, dtype, model = _abi.ConnBuf, gev_amd.CONN_BUF_DTYPE, gm.CONN_BUF_DTYPE
    assert ctypes.sizeof(struct) == dtype.itemsize == model.itemsize == 32
    assert [n for n, _ in struct._fields_] == list(dtype.names) == list(model.names) == list(want)
    for f, o in want.items():
        assert getattr(struct, f).offset == o, f
        assert dtype.fields[f][1] == o and model.fields[f][1] == o, f
        assert getattr(struct, f).size == dtype.fields[f][0].itemsize == model.fields[f][0].itemsize, f
    text = open(HEADER).read()
    body = re.search(r"typedef struct gevws_conn_buf \{(.*?)\} gevws_conn_buf;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+)(?:\[(\d)\])?;", body) == [("uint64_t", "off", ""), ("uint64_t", "bytes", ""),
                                                               ("uint32_t", "flags", ""), ("uint32_t", "reserved", "3")]


def _dummy():
    """A buffer for every pointer, 16-aligned, filled with 0xEE; the call's arguments over it."""
    raw = (ctypes.c_uint8 * (4096 + 16))(*([0xEE] * (4096 + 16)))
    p = (ctypes.addressof(raw) + 15) // 16 * 16
    bases = (ctypes.c_void_p * 3)(p + 1024, p + 1280, p + 1536)
    nbytes = (ctypes.c_uint64 * 3)(64, 64, 64)
    args = [None, None, p, 2, p + 256, 2, p + 512, ctypes.addressof(bases), ctypes.addressof(nbytes), 0, p + 2048, 512,
            p + 3072, p + 3584]
    return raw, (bases, nbytes), args


def test_nonzero_flags_fail_the_call_without_a_device():
    """The flag check comes first: with every pointer NULL and with a buffer
    for each, any bit is GEVWS_ERR_INVALID and nothing is written."""
    raw, keep, ptrs = _dummy()
    nulls = [None, None, None, 0, None, 0, None, None, None, 0, None, 0, None, None]
    for flags in (1, 2, 0x80000000, 0xFFFFFFFF):
        for args in (nulls, ptrs):
            a = list(args)
            a[FLAGS] = flags
            assert gev_amd.lib.gevws_send_gather_async(*a) == _abi.ERR_INVALID, flags
    assert bytes(raw) == b"\xee" * len(raw)


def test_misaligned_buffers_fail_the_call_without_a_device():
    raw, (bases, nbytes), ptrs = _dummy()
    nulls = [None, None, None, 0, None, 0, None, None, None, 0, None, 0, None, None]
    for mis in (1, 4, 8, 15):
        a = list(nulls)
        a[BUF] = 4096 + mis  # never dereferenced
        assert gev_amd.lib.gevws_send_gather_async(*a) == _abi.ERR_INVALID, mis
        a = list(ptrs)
        a[BUF] += mis
        assert gev_amd.lib.gevws_send_gather_async(*a) == _abi.ERR_INVALID, mis
        for w in range(3):
            b = (ctypes.c_void_p * 3)(*bases)
            b[w] = bases[w] + mis
            a = list(ptrs)
            a[7] = ctypes.addressof(b)
            assert gev_amd.lib.gevws_send_gather_async(*a) == _abi.ERR_INVALID, (mis, w)
    # a valid flag word and aligned buffers with a NULL context are invalid too
    assert gev_amd.lib.gevws_send_gather_async(*ptrs) == _abi.ERR_INVALID
    assert bytes(raw) == b"\xee" * len(raw)


def test_python_entry_points():
    assert callable(gev_amd.Engine.send_gather_async)
    assert callable(gev_amd.Responses.host_sends)
    p = inspect.signature(gev_amd.Engine.respond).parameters["gather"]
    assert p.default is False
    fields = gev_amd.Responses.__dataclass_fields__
    for name in ("send_buf", "conn_buf", "gather_summary"):
        assert fields[name].default is None, name
    assert callable(gev_amd.Responses.conn_bytes)
