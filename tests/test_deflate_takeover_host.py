"""Server context takeover on the host: gevws_deflate_raw_ctx, the device's
compressor over one connection's context slot (include/gevws.h).  A chain is
decoded two ways -- one zlib raw inflater with a window of 2^window_bits fed
payload + 00 00 ff ff message by message, and gevws_inflate_raw_ctx over one
inflate slot -- and the slot's bytes are checked against the stream."""
import ctypes
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import gev_amd
from gev_amd import _abi
from tests import _inflate_corpus as ic
from tests import _takeover_far as far
from tests import test_deflate_host as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
TAIL = b"\x00\x00\xff\xff"
DYN = gev_amd.DEFLATE_DYNAMIC
CTX = gev_amd.DEF_CTX_BYTES
LENGTHS = (0, 1, 3, 4, 17, 300, 4095, 4097, 9000)


def fresh() -> bytearray:
    return bytearray(CTX)


def total_of(ctx) -> int:
    return int.from_bytes(ctx[:8], "little")


def ring_of(ctx) -> bytes:
    return bytes(ctx[64:64 + 32768])


def check_slot(ctx, stream: bytes):
    """The head, the ring image of the last 32 768 stream bytes, zeros where nothing was written."""
    assert total_of(ctx) == len(stream) and not any(ctx[8:64])
    want = bytearray(32768)
    for i in range(max(0, len(stream) - 32768), len(stream)):
        want[i & 32767] = stream[i]
    assert ring_of(ctx) == bytes(want)


def chain_messages(rng, lengths=LENGTHS, rounds=2):
    """Every length with every kind; the starts fall at every residue mod 16."""
    msgs = [ic.sample(rng, n, kind) for _ in range(rounds) for kind in range(4) for n in lengths]
    order = rng.permutation(len(msgs))
    msgs = [msgs[i] for i in order]
    starts, at = set(), 0
    for k in range(16):  # ... made sure of with sixteen 17-byte messages
        msgs.append(ic.sample(rng, 17, k % 4))
    for m in msgs:
        if m:
            starts.add(at % 16)
        at += len(m)
    assert starts == set(range(16))
    return msgs


def test_zeroed_slot_is_deflate_raw():
    rng = np.random.default_rng(0x7A65726F)
    for n in base.SIZES:
        for kind in range(4) if n <= 4097 else (n % 4,):
            data = ic.sample(rng, n, kind)
            for flags in (0, DYN):
                for wb in (0, 9):
                    ctx = fresh()
                    assert gev_amd.deflate_raw_ctx(data, ctx, wb, flags) == gev_amd.deflate_raw(data, wb, flags), (n, kind)
                    check_slot(ctx, data)


@pytest.mark.parametrize("flags", [0, DYN])
def test_chains_decode_two_ways(flags):
    rng = np.random.default_rng(0x63686E73)
    msgs = chain_messages(rng)
    for wb in (8, 9, 10, 11, 12, 13, 14, 15, 0):
        ctx, ictx = fresh(), bytearray(gev_amd.INF_CTX_BYTES)
        d = zlib.decompressobj(-(wb or 15))
        stream = b""
        for i, m in enumerate(msgs):
            p = gev_amd.deflate_raw_ctx(m, ctx, wb, flags)
            assert len(p) <= gev_amd.deflate_bound(len(m))
            assert d.decompress(p + TAIL) == m, (wb, i, len(m))
            assert gev_amd.inflate_raw_ctx(p, len(m), ictx) == (0, m), (wb, i, len(m))
            if not m:
                assert p == b"\x00"
            stream += m
        check_slot(ctx, stream)
        assert ring_of(ctx) == bytes(ictx[64:])


def test_long_stream_wraps_the_ring_and_the_positions():
    rng = np.random.default_rng(0x6C6F6E67)
    text = ic.sample(rng, 9000, 0)
    for flags in (0, DYN):
        ctx, d, stream = fresh(), zlib.decompressobj(-15), b""
        sizes = []
        for k in range(16):  # 144 000 bytes: past 32 768, 65 536 and 131 072
            m = text[3 * k:] + text[:3 * k] if k % 3 else ic.sample(rng, 9000, k % 4)
            p = gev_amd.deflate_raw_ctx(m, ctx, 0, flags)
            assert d.decompress(p + TAIL) == m, k
            stream += m
            check_slot(ctx, stream)
            sizes.append(len(p))
        assert total_of(ctx) == 144000
        # a rotation of the text two messages back is in reach (18 000 < 30 720) and is found
        assert sizes[4] < sizes[1] and sizes[13] < sizes[1], sizes


def test_equal_messages():
    a = np.random.default_rng(0x657175).integers(0, 256, 300, dtype=np.uint8).tobytes()
    for flags in (0, DYN):
        ctx = fresh()
        first, second = gev_amd.deflate_raw_ctx(a, ctx, 0, flags), gev_amd.deflate_raw_ctx(a, ctx, 0, flags)
        print(f"equal 300-byte messages, flags {flags}: {len(first)} then {len(second)} bytes")
        assert 4 * len(second) < len(first)
        d = zlib.decompressobj(-15)
        assert d.decompress(first + TAIL) == a and d.decompress(second + TAIL) == a


def takeover_scripts():
    """The 64 connection scripts of the takeover shape tools/bench_deflate.py --takeover measures: 8 word-soup
    texts of about 512 B each, made by the tool's own generator."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_deflate
    finally:
        sys.path.pop(0)
    return bench_deflate.takeover_texts()


def test_wire_bytes_over_scripts():
    scripts = takeover_scripts()
    assert len(scripts) == 64 and all(len(s) == 8 and all(480 <= len(m) < 544 for m in s) for s in scripts)
    for flags in (0, DYN):
        with_ctx = without = 0
        for msgs in scripts:
            ctx, d = fresh(), zlib.decompressobj(-15)
            for m in msgs:
                p = gev_amd.deflate_raw_ctx(m, ctx, 0, flags)
                assert d.decompress(p + TAIL) == m
                with_ctx += len(p)
                without += len(gev_amd.deflate_raw(m, 0, flags))
        print(f"64 scripts x 8 messages, flags {flags}: {with_ctx} B with takeover, {without} B without, "
              f"ratio {with_ctx / without:.3f}")
        assert with_ctx < without


def raw_ctx(data, ctx, wb, flags, cap, pad=b""):
    """The C call on a source buffer with `pad` behind the message; (status, out buffer, out_len)."""
    src = ctypes.create_string_buffer(data + pad, len(data) + len(pad))
    out = ctypes.create_string_buffer(b"\xEE" * max(cap, 1), max(cap, 1))
    n = ctypes.c_uint64(77)
    slot = (ctypes.c_uint8 * CTX).from_buffer(ctx) if ctx is not None else None
    st = gev_amd.lib.gevws_deflate_raw_ctx(src, len(data), wb, flags, out, cap, ctypes.byref(n), slot)
    return st, out.raw[:max(cap, 1)], n.value


def test_slot_bytes_do_not_depend_on_the_pad():
    rng = np.random.default_rng(0x706164)
    msgs = [ic.sample(rng, n, k % 4) for k, n in enumerate((5, 17, 300, 1, 4097, 3, 9000, 31, 0, 20000, 16))]
    slots = []
    for pad in (b"\x00" * 64, b"\xff" * 64):
        ctx, stream, outs = fresh(), b"", []
        for m in msgs:
            st, out, n = raw_ctx(m, ctx, 0, 0, gev_amd.deflate_bound(len(m)), pad)
            assert st == 0
            outs.append(out[:n])
            stream += m
            check_slot(ctx, stream)
        slots.append((bytes(ctx), outs))
    assert slots[0] == slots[1]
    # the table too is the stream's alone: one message or the same bytes behind a history give other
    # tables, but the same cut gives the same
    again = fresh()
    for m in msgs:
        gev_amd.deflate_raw_ctx(m, again, 0, DYN)  # (the flag changes the coding, not the tokens)
    assert bytes(again) == slots[0][0]


def test_capacity_leaves_out_and_slot_untouched():
    rng = np.random.default_rng(0x636170)
    ctx = fresh()
    gev_amd.deflate_raw_ctx(ic.sample(rng, 700, 0), ctx)
    for flags in (0, DYN):
        for n in (0, 1, 300, 5000):
            m = ic.sample(rng, n, 0)
            before = bytes(ctx)
            want = gev_amd.deflate_raw_ctx(m, bytearray(before), 0, flags)
            st, out, need = raw_ctx(m, ctx, 0, flags, len(want) - 1)
            assert (st, need) == (_abi.ERR_CAPACITY, len(want)) and bytes(ctx) == before
            assert out == b"\xEE" * max(len(want) - 1, 1)
            st, out, need = raw_ctx(m, ctx, 0, flags, len(want))
            assert (st, out, need) == (0, want, len(want))
            assert (bytes(ctx) != before) == (n != 0)


def test_invalid_calls():
    for wb in (-1, 1, 7, 16, 31):
        ctx = fresh()
        assert raw_ctx(b"abc", ctx, wb, 0, 64)[0] == _abi.ERR_INVALID and bytes(ctx) == bytes(CTX)
    assert raw_ctx(b"abc", None, 0, 0, 64)[0] == _abi.ERR_INVALID
    assert raw_ctx(b"abc", fresh(), 0, 1, 64)[0] == _abi.ERR_INVALID  # PLAIN_IF_NOT_SMALLER is the caller's
    assert raw_ctx(b"abc", fresh(), 0, 4, 64)[0] == _abi.ERR_INVALID
    with pytest.raises(ValueError):
        gev_amd.deflate_raw_ctx(b"abc", bytearray(CTX - 1))
    with pytest.raises(RuntimeError):
        gev_amd.deflate_raw_ctx(b"abc", fresh(), 7)


def test_a_takeover_message_needs_its_window():
    """The twin of assert_chain_needs_its_window: a message that leans on history cannot be decoded with
    an empty window, or decodes differently."""
    rng = np.random.default_rng(0x6E656564)
    a = ic.sample(rng, 600, 0)
    for flags in (0, DYN):
        ctx = fresh()
        gev_amd.deflate_raw_ctx(a, ctx, 0, flags)
        second = gev_amd.deflate_raw_ctx(a, ctx, 0, flags)
        assert second != gev_amd.deflate_raw(a, 0, flags)
        raised, got = ic.zlib_inflate(second)
        assert raised or got != a
        st, got = gev_amd.inflate_raw(second, len(a))
        assert st != 0 or got != a


# ---------------------------------------------------------------------------- old connections: relocated slots
# A connection that has echoed 2 GiB, 4 GiB or far more: tests/_takeover_far.py.  Two references, neither of
# them the relocated run: zlib with the history as its dictionary, and the same call on the unrelocated slot.
@pytest.fixture(scope="module")
def old():
    """The two old slots per (flags, window_bits) -- `odd` at 70 001 bytes, `edge` at 131 055 -- and their
    plain history.  (The slot does not depend on the flags; it does on window_bits: the tokens differ.)"""
    rng = far.rng_of(0x6F6C64)
    hist = far.history_messages(rng)
    slots = {}
    for wb in (9, 12, 15):
        ctx, d = fresh(), zlib.decompressobj(-wb)
        for k, m in enumerate(hist):
            assert d.decompress(gev_amd.deflate_raw_ctx(m, ctx, wb, DYN if k % 2 else 0) + TAIL) == m
            if k == 2:
                slots["odd", wb] = bytes(ctx)
        slots["edge", wb] = bytes(ctx)
        check_slot(ctx, b"".join(hist))
    assert far.DefSlot(slots["odd", 15]).total == 70001 and far.DefSlot(slots["edge", 15]).total == 131055
    return dict(slots=slots, hist={"odd": b"".join(hist[:3]), "edge": b"".join(hist)})


def run_far_chain(slot0: bytes, history: bytes, msgs, shift: int, wb: int, flags: int, near=None, tag=""):
    """`msgs` one after the other on slot0 relocated by `shift`, each against both references; returns the
    unrelocated run [(payload, slot after)] for the next shift to share."""
    if near is None:
        ctx, near = bytearray(slot0), []
        for m in msgs:
            p = gev_amd.deflate_raw_ctx(m, ctx, wb, flags)
            near.append((p, bytes(ctx)))
    ctx, stream = far.DefSlot(slot0).relocated(shift), history
    for k, (m, (p_near, slot_near)) in enumerate(zip(msgs, near)):
        p = gev_amd.deflate_raw_ctx(m, ctx, wb, flags)
        # zlib, the history its dictionary (a window of 2^wb bytes reads no further back than the step's reach)
        d = zlib.decompressobj(-wb, zdict=stream[-(1 << wb):])
        assert d.decompress(p + TAIL) == m, (tag, k, "zlib with the history as dictionary")
        assert p == p_near, (tag, k, "payload differs from the unrelocated slot's")
        far.assert_def_translated(ctx, slot_near, shift, (tag, k))
        stream += m
    return near


@pytest.mark.parametrize("flags", [0, DYN])
@pytest.mark.parametrize("wb", [9, 12, 15])
def test_relocated_slots_cross_every_boundary(old, flags, wb):
    rng = far.rng_of(0x666172 + wb)
    slot0, history = old["slots"]["odd", wb], old["hist"]["odd"]
    cases = far.far_cases(far.DefSlot(slot0).total, far.U_DEF)
    helped = 0
    for kind in far.KINDS:
        # three messages: the second and third run on a slot the code itself wrote at the far position
        first = far.message(rng, history, kind)
        msgs = [first, far.message(rng, history + first, far.KINDS[(far.KINDS.index(kind) + 1) % 5], 5000),
                first[-300:]]
        assert all(len(m) for m in msgs)
        near = None
        for name, shift in cases:
            near = run_far_chain(slot0, history, msgs, shift, wb, flags, near, (name, kind, wb, flags))
        helped += kind != "random" and near[0][0] != gev_amd.deflate_raw(first, wb, flags)
    assert helped == 4                                      # the history was used: the window matters


@pytest.mark.parametrize("flags", [0, DYN])
def test_short_and_empty_messages_right_at_a_boundary(old, flags):
    rng = far.rng_of(0x65646765)
    slot0, history = old["slots"]["edge", 15], old["hist"]["edge"]
    short = history[-4000:-3983]
    msgs = [short, b"", far.message(rng, history + short, "text"), b"", far.message(rng, history, "runs", 17)]
    assert len(short) == 17
    near = None
    for name, shift in far.edge_cases(far.DefSlot(slot0).total, far.U_DEF):
        near = run_far_chain(slot0, history, msgs, shift, 15, flags, near, (name, flags))
    assert len(near[0][0]) < 12 and near[1][0] == b"\x00"   # a match into the history; an empty message


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_deflate_ctx_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "deflate_ctx_fuzz"
    r = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "deflate_ctx_fuzz.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_deflate_host.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "deflate_ctx_fuzz ok" in r.stdout, r.stdout + r.stderr
