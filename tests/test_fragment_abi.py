"""CPU checks of the fragment steps' addition to the C ABI: libgevws.so
exports the three calls with the header's argument counts, the ABI version is
unchanged, an invalid call fails before any device is touched, the Python layer
has its entry points, and the host twin (gev_amd.fragment_records) equals
tests/_fragment_model.py record for record.  No device compute is called
here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gev_amd
from gev_amd import _abi
from tests import _fragment_model as fm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gevws.h")
NARGS = {"gevws_fragment_async": 11, "gevws_fragment_offsets_async": 10, "gevws_fragment_records": 7}


def test_library_exports_the_fragment_calls():
    lib = ctypes.CDLL(_abi.LIB_PATH)
    text = open(HEADER).read()
    for name, nargs in NARGS.items():
        assert hasattr(lib, name), name
        restype, args = _abi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(args) == nargs, name
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == nargs, name
    a = _abi.SIGNATURES["gevws_fragment_async"][1]
    assert a[3] is ctypes.c_uint64 and a[5] is ctypes.c_uint64 and a[6] is ctypes.c_uint32 and a[8] is ctypes.c_uint64
    assert _abi.SIGNATURES["gevws_fragment_offsets_async"][1][3] is ctypes.c_uint64
    r = _abi.SIGNATURES["gevws_fragment_records"][1]
    assert r[1] is ctypes.c_uint64 and r[2] is ctypes.c_uint64 and r[4] is ctypes.c_uint64


def test_abi_version_is_still_3():
    assert gev_amd.lib.gevws_abi_version() == 3
    assert re.search(r"#define GEVWS_ABI_VERSION 3\b", open(HEADER).read())


def test_record_layout_of_the_model():
    assert fm.OUT_FRAME_DTYPE == gev_amd.OUT_FRAME_DTYPE and fm.SUMMARY_DTYPE == gev_amd.SUMMARY_DTYPE
    assert (fm.OK, fm.ERR_CAPACITY, fm.ERR_INVALID) == (_abi.OK, _abi.ERR_CAPACITY, _abi.ERR_INVALID)


def _dummy():
    """A buffer for every pointer, 16-aligned, filled with 0xEE."""
    raw = (ctypes.c_uint8 * (4096 + 16))(*([0xEE] * (4096 + 16)))
    return raw, (ctypes.addressof(raw) + 15) // 16 * 16


def test_invalid_fragment_calls_fail_without_a_device():
    """max_fragment_bytes == 0, any flag bit and counts >= 2^32 come first: with
    every pointer NULL and with a buffer for each the call is GEVWS_ERR_INVALID
    and nothing is written."""
    raw, p = _dummy()
    f = gev_amd.lib.gevws_fragment_async
    nulls = [None, None, None, 2, None, 16, 0, None, 8, None, None]
    ptrs = [None, None, p, 2, p + 256, 16, 0, p + 512, 8, p + 1024, p + 2048]
    for pos, values in ((5, (0,)), (6, (1, 2, 0x80000000, 0xFFFFFFFF)), (3, (1 << 32, (1 << 64) - 1)),
                        (8, (1 << 32, (1 << 64) - 1))):
        for v in values:
            for args in (nulls, ptrs):
                a = list(args)
                a[pos] = v
                assert f(*a) == _abi.ERR_INVALID, (pos, v)
    # fragments are stored as aligned vectors; and a valid call with a NULL context is invalid too
    for mis in (1, 4, 8, 15):
        a = list(ptrs)
        a[7] += mis
        assert f(*a) == _abi.ERR_INVALID, mis
    assert f(*ptrs) == _abi.ERR_INVALID
    assert bytes(raw) == b"\xee" * len(raw)


def test_invalid_offsets_calls_fail_without_a_device():
    raw, p = _dummy()
    f = gev_amd.lib.gevws_fragment_offsets_async
    ptrs = [None, None, p, 2, p + 256, p + 512, p + 1024, p + 1536, p + 2048, p + 3072]
    for n in (1 << 32, (1 << 64) - 1):
        a = list(ptrs)
        a[3] = n
        assert f(*a) == _abi.ERR_INVALID
        assert f(None, None, None, n, None, None, None, None, None, None) == _abi.ERR_INVALID
    assert f(*ptrs) == _abi.ERR_INVALID   # no context
    assert bytes(raw) == b"\xee" * len(raw)


def test_invalid_host_calls():
    raw, p = _dummy()
    f = gev_amd.lib.gevws_fragment_records
    assert f(p, 2, 0, p + 512, 8, p + 1024, p + 2048) == _abi.ERR_INVALID
    assert f(p, 1 << 32, 4, p + 512, 8, p + 1024, p + 2048) == _abi.ERR_INVALID
    assert f(p, 2, 4, p + 512, 1 << 32, p + 1024, p + 2048) == _abi.ERR_INVALID
    assert f(None, 2, 4, p + 512, 8, p + 1024, p + 2048) == _abi.ERR_INVALID
    assert f(p, 2, 4, None, 8, p + 1024, p + 2048) == _abi.ERR_INVALID
    assert f(p, 2, 4, p + 512, 8, None, p + 2048) == _abi.ERR_INVALID
    assert f(p, 2, 4, p + 512, 8, p + 1024, None) == _abi.ERR_INVALID
    assert bytes(raw) == b"\xee" * len(raw)
    with pytest.raises(RuntimeError):
        gev_amd.fragment_records(np.zeros(1, gev_amd.OUT_FRAME_DTYPE), 0)


def test_python_entry_points():
    assert callable(gev_amd.Engine.fragment_async) and callable(gev_amd.Engine.fragment_offsets_async)
    assert callable(gev_amd.fragment_records)
    for fn in (gev_amd.Engine.echo_messages, gev_amd.Engine.respond, gev_amd.Engine.broadcast):
        assert inspect.signature(fn).parameters["max_fragment_bytes"].default is None, fn
    fields = gev_amd.Echo.__dataclass_fields__
    assert fields["plain_first"].default is None and fields["def_first"].default is None


def host_raw(recs, F, max_frags):
    """gevws_fragment_records over 0xEE-filled outputs -> (frags, first, summary) as raw arrays."""
    n = len(recs)
    frags = np.full(max(max_frags, 1) * 32, 0xEE, np.uint8)
    first = np.full((n + 2) * 8, 0xEE, np.uint8)
    summary = np.full(64, 0xEE, np.uint8)
    recs = np.ascontiguousarray(recs)
    st = gev_amd.lib.gevws_fragment_records(recs.ctypes.data, n, F, frags.ctypes.data, max_frags, first.ctypes.data,
                                            summary.ctypes.data)
    assert st == _abi.OK
    return frags, first, summary.view(fm.SUMMARY_DTYPE)[0]


def check_host(recs, F, max_frags, tag):
    want_f, want_first, want_s = fm.fragment(recs, F, max_frags)
    frags, first, s = host_raw(recs, F, max_frags)
    assert s.tobytes() == want_s.tobytes(), (tag, s, want_s)
    if want_f is None:   # nothing but the summary is written
        assert (frags == 0xEE).all() and (first == 0xEE).all(), tag
        return s
    k = len(want_f) * 32
    assert frags[:k].tobytes() == want_f.tobytes() and (frags[k:] == 0xEE).all(), tag
    assert first[: (len(recs) + 1) * 8].tobytes() == want_first.tobytes() and (first[-8:] == 0xEE).all(), tag
    return s


@pytest.mark.parametrize("F", fm.LIMITS)
def test_host_twin_equals_the_model(F):
    rng = np.random.default_rng(0x66726100 + F)
    recs = fm.shape_records(F, rng)
    s = check_host(recs, F, 1 << 20, F)
    need = int(s["frames"])
    assert int(s["payload_bytes"]) > 0
    check_host(recs, F, need, (F, "exact"))
    c = check_host(recs, F, need - 1, (F, "capacity"))
    assert (int(c["status"]), int(c["frames"])) == (_abi.ERR_CAPACITY, need)
    if F <= 126:
        for n in (1, 255, 256, 257, 1025):
            check_host(fm.random_records(n, F, rng, max_len=3 * F + 7), F, 12 * n, (F, n))
    # the Python wrapper sizes the list itself
    frags, first, ws = gev_amd.fragment_records(recs, F)
    want_f, want_first, _ = fm.fragment(recs, F, 1 << 20)
    assert frags.tobytes() == want_f.tobytes() and first.tobytes() == want_first.tobytes()
    assert ws.tobytes() == s.tobytes()


def test_host_twin_long_record_and_malformed():
    mid = np.array([fm.record(5, off=0), fm.record(4097, opcode=2, rsv=4, off=16), fm.record(0, off=8192)],
                   fm.OUT_FRAME_DTYPE)
    s = check_host(mid, 1, 5000, "4097 fragments")
    assert (int(s["frames"]), int(s["payload_bytes"])) == (5 + 4097 + 1, 2)
    big = np.array([fm.record(3), fm.record(1 << 40), fm.record(2)], fm.OUT_FRAME_DTYPE)
    s = check_host(big, 1, 64, "malformed")
    assert (int(s["status"]), int(s["errors"]), int(s["frames"])) == (_abi.ERR_INVALID, 1, 0)
    frags, first, s = gev_amd.fragment_records(big, 1)
    assert len(frags) == 0 and not first.any() and int(s["status"]) == _abi.ERR_INVALID
    # an empty list: first[0] = 0 and a zero summary
    frags, first, s = gev_amd.fragment_records(np.zeros(0, gev_amd.OUT_FRAME_DTYPE), 7)
    assert len(frags) == 0 and first.tolist() == [0] and s.tobytes() == fm.summary().tobytes()
