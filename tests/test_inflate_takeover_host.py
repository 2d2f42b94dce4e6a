"""Client context takeover on the host: gevws_inflate_raw_ctx, the device's
decoder over one connection's context slot (include/gevws.h).  The oracle for
message k of a chain is "the window as stored blocks, then the payload" under
the no-takeover rules (tests/_inflate_takeover.py), through zlib for valid data
and through the Python model for verdicts.  Chains come from one persistent
zlib compressor with Z_SYNC_FLUSH per message; every chain whose compressor
can look back (level > 0, default or fixed strategy) is asserted to hold a
message that an empty window rejects or decodes differently."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import gev_amd
from tests import _inflate_corpus as ic
from tests import _inflate_gpu_model as gm
from tests import _inflate_model as im
from tests import _inflate_takeover as tk
from tests import _takeover_far as far

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
BIG = 1 << 20


def fresh() -> bytearray:
    return bytearray(tk.CTX_BYTES)


def run_chain(payloads, cap=BIG, ctx=None):
    ctx = fresh() if ctx is None else ctx
    return [gev_amd.inflate_raw_ctx(p, cap, ctx) for p in payloads], ctx


def test_constants():
    assert gev_amd.INF_CTX_BYTES == tk.CTX_BYTES == 32768 + 64
    assert gev_amd.EXT_CLIENT_TAKEOVER == 2 and gev_amd.NEGOTIATE_CLIENT_TAKEOVER == 1
    assert gev_amd.lib.gevws_abi_version() == 3


def test_chains_of_every_level_strategy_and_kind_against_zlib():
    rng = np.random.default_rng(0x63686E)
    differs = 0
    for level in ic.LEVELS:
        for strategy in ic.STRATEGIES:
            for kind in range(4):
                a, b, c = (ic.sample(rng, n, kind) for n in (300, 2000, 17))
                datas = [a, b, a, b"", c, a[:150] + b[:150], b, a]
                payloads = tk.chain(datas, level, strategy)
                got, ctx = run_chain(payloads)
                assert got == [(im.OK, d) for d in datas], (level, strategy, kind)
                model = tk.Slot()
                for p, d in zip(payloads, datas):       # zlib with the window as its dictionary agrees
                    assert tk.zlib_inflate_dict(model.window(), p) == (False, d)
                    model.append(d)
                assert bytes(ctx) == model.image()
                n = sum(tk.empty_window_differs(p, d) for p, d in zip(payloads[1:], datas[1:]))
                if level > 0 and strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED):
                    assert n >= 1, (level, strategy, kind)
                differs += n
    assert differs >= 100


def test_eleven_sample_messages_and_the_eight_byte_repeat():
    rng = np.random.default_rng(0x656C65)
    datas = [ic.sample(rng, 300, 0) for _ in range(11)]
    payloads = tk.chain(datas)
    assert sum(tk.zlib_inflate_dict(b"", p)[0] for p in payloads[1:]) >= 3  # an empty window rejects them
    got, _ = run_chain(payloads)
    assert got == [(im.OK, d) for d in datas]
    # each on a zeroed slot: the empty-window verdicts are inflate_raw's
    for p in payloads:
        assert gev_amd.inflate_raw_ctx(p, BIG, fresh()) == gev_amd.inflate_raw(p, BIG)
    text = ic.sample(rng, 300, 1)
    twice = tk.chain([text, text])
    assert len(twice[1]) <= 8 and tk.zlib_inflate_dict(b"", twice[1])[0]
    got, _ = run_chain(twice)
    assert got == [(im.OK, text), (im.OK, text)]


def test_zeroed_slot_is_inflate_raw():
    rng = np.random.default_rng(0x7A6572)
    streams = [p for p, _ in ic.valid_streams(rng)] + ic.malformed_streams(rng, 1500)
    seen = set()
    for cap in (BIG, 40):
        for p in streams:
            ctx = fresh()
            got = gev_amd.inflate_raw_ctx(p, cap, ctx)
            assert got == gev_amd.inflate_raw(p, cap)
            seen.add(got[0])
            slot = tk.Slot(bytes(ctx))
            if got[0] == im.OK:
                assert (slot.total, slot.broken, slot.window()) == (len(got[1]), 0, got[1][-tk.WIN:])
            else:
                assert (slot.total, slot.broken) == (0, got[0]) and not any(slot.ring)
    assert seen == {im.OK, im.ERR_DEFLATE, im.ERR_TOO_BIG}
    assert gev_amd.lib.gevws_inflate_raw_ctx(b"\0", 1, ctypes.create_string_buffer(8), 8, None, None) == \
        gev_amd.ERR_INVALID


def test_stream_longer_than_the_window_and_references_over_the_wrap():
    datas = tk.wrap_chain(np.random.default_rng(0x777270))
    for level in (1, 6, 9):
        payloads = tk.chain(datas, level)
        assert len(payloads[-1]) < 20 and len(payloads[1]) < 20         # back-references, not literals
        assert tk.empty_window_differs(payloads[-1], datas[-1]) and tk.empty_window_differs(payloads[7], datas[7])
        got, ctx = run_chain(payloads)
        assert got == [(im.OK, d) for d in datas], level
        model = tk.Slot()
        model.append(b"".join(datas))                                   # the slot is a function of the stream
        assert bytes(ctx) == model.image() and model.total == 119917


def test_distance_32768_needs_exactly_that_much_history():
    rng = np.random.default_rng(0x646973)
    m = tk.match3_at_32768()
    for n, status in ((32768, im.OK), (32767, im.ERR_DEFLATE), (40000, im.OK)):
        h = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        raised, z = tk.zlib_inflate_dict(h[-tk.WIN:], m)                # zlib agrees on both
        assert (raised, z) == (status != im.OK, h[-32768:][:3] if status == im.OK else b"")
        got, ctx = run_chain([ic.deflate(h, 0), m])
        assert got[0] == (im.OK, h) and got[1] == (status, z), n
        assert tk.Slot(bytes(ctx)).broken == (0 if status == im.OK else im.ERR_DEFLATE)


def test_mutated_streams_in_mid_chain_match_the_model():
    rng = np.random.default_rng(0x6D7574)
    seen = {}
    for kind, level in ((0, 6), (0, 9), (3, 6), (2, 1), (0, 1)):
        first, second = ic.sample(rng, int(rng.integers(60, 200)), kind), ic.sample(rng, 180, kind)
        second = first[:90] + second[:90]
        p1, p2 = tk.chain([first, second], level, zlib.Z_FIXED if level == 1 else zlib.Z_DEFAULT_STRATEGY)
        assert tk.empty_window_differs(p2, second)
        base = fresh()
        assert gev_amd.inflate_raw_ctx(p1, BIG, base) == (im.OK, first)
        assert len(tk.stored(first)) + len(p2) + 8 <= gm.MODEL_MAX
        for _ in range(400):
            mut = ic.mutate(rng, p2)[: gm.MODEL_MAX - len(tk.stored(first))]
            for cap in (1000, 40):
                ctx = bytearray(base)
                got = gev_amd.inflate_raw_ctx(mut, cap, ctx)
                want = tk.oracle(first, mut, cap)
                assert got == want, (kind, level, mut.hex(), cap)
                model = tk.Slot(bytes(base))
                assert model.feed(mut, cap) == want and bytes(ctx) == model.image()
                seen[got[0]] = seen.get(got[0], 0) + 1
    assert seen[im.OK] > 100 and seen[im.ERR_DEFLATE] > 500 and seen[im.ERR_TOO_BIG] > 100


def test_a_bfinal_ended_message_keeps_the_window():
    rng = np.random.default_rng(0x62666E)
    a = ic.sample(rng, 500, 0)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    final = c.compress(a) + c.flush(zlib.Z_FINISH)                      # ends with a BFINAL block, no sync tail
    c2 = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, a)
    again = (c2.compress(a) + c2.flush(zlib.Z_SYNC_FLUSH))[:-4]         # a reference into the dictionary
    assert len(again) < 20 and tk.zlib_inflate_dict(b"", again)[0]
    got, ctx = run_chain([final + b"garbage behind the final block", again])
    assert got == [(im.OK, a), (im.OK, a)]
    assert tk.Slot(bytes(ctx)).window() == a + a


def test_failures_mark_the_slot_broken_for_good():
    rng = np.random.default_rng(0x62726B)
    datas = [ic.sample(rng, 300, 0) for _ in range(4)]
    payloads = tk.chain(datas)
    for bad, cap, status in ((b"\x06garbage", BIG, im.ERR_DEFLATE), (payloads[1], 100, im.ERR_TOO_BIG)):
        ctx = fresh()
        assert gev_amd.inflate_raw_ctx(payloads[0], BIG, ctx) == (im.OK, datas[0])
        ring = bytes(ctx[64:])
        st, out = gev_amd.inflate_raw_ctx(bad, cap, ctx)
        assert st == status and (status != im.ERR_TOO_BIG or out == datas[1][:100])
        for p in payloads[1:] + [ic.deflate(b"on its own")]:            # sticky: nothing is decoded any more
            assert gev_amd.inflate_raw_ctx(p, BIG, ctx) == (status, b"")
        slot = tk.Slot(bytes(ctx))
        assert (slot.total, slot.broken, bytes(slot.ring)) == (300, status, ring)


def test_slot_is_a_function_of_the_stream_not_of_the_calls():
    rng = np.random.default_rng(0x637574)
    words = ic.sample(rng, 50000, 0)
    for cuts in ([50000], [1, 49999], [300] * 100 + [20000], [32768, 17232], [40000, 0, 10000]):
        datas, at = [], 0
        for n in cuts:
            datas.append(words[at:at + n])
            at += n
        got, ctx = run_chain(tk.chain(datas, 6))
        assert [g[0] for g in got] == [im.OK] * len(cuts) and b"".join(g[1] for g in got) == words[:at]
        model = tk.Slot()
        model.append(words[:at])
        assert bytes(ctx) == model.image(), cuts


# ---------------------------------------------------------------------------- old connections: relocated slots
# A connection that has inflated 2 GiB, 4 GiB or far more: tests/_takeover_far.py.  Two references, neither of
# them the relocated run: zlib, which made the payload with the history as its dictionary (the output must be
# the message), and the same call on the unrelocated slot.
@pytest.fixture(scope="module")
def old():
    """The old slots -- `odd` at 70 001 bytes, `edge` at 131 055 -- and their plain history."""
    rng = far.rng_of(0x6F6C64)
    hist = far.history_messages(rng)
    ctx, slots = fresh(), {}
    for k, (p, m) in enumerate(zip(tk.chain(hist, 6), hist)):
        assert gev_amd.inflate_raw_ctx(p, BIG, ctx) == (im.OK, m)
        if k == 2:
            slots["odd"] = bytes(ctx)
    slots["edge"] = bytes(ctx)
    model = tk.Slot()
    model.append(b"".join(hist))
    assert slots["edge"] == model.image() and tk.Slot(slots["odd"]).total == 70001 and model.total == 131055
    return dict(slots=slots, hist={"odd": b"".join(hist[:3]), "edge": b"".join(hist)})


peer_chain = far.peer_chain


def assert_inf_translated(ctx, near: bytes, shift: int, tag=""):
    """The slot is the unrelocated run's with `total` larger by exactly `shift`: the same ring image, the
    same `broken` byte, zeros elsewhere in the head (tk.Slot asserts those)."""
    a, b = tk.Slot(bytes(ctx)), tk.Slot(near)
    assert a.total == b.total + shift, (tag, a.total, b.total, shift)
    assert a.broken == b.broken and a.ring == b.ring, tag


def run_far_chain(slot0: bytes, payloads, shift: int, caps, near=None, tag=""):
    """The payloads one after the other on slot0 relocated by `shift`, against the unrelocated run
    [((status, bytes), slot after)], which is returned for the next shift to share."""
    if near is None:
        ctx, near = bytearray(slot0), []
        for p, cap in zip(payloads, caps):
            got = gev_amd.inflate_raw_ctx(p, cap, ctx)
            near.append((got, bytes(ctx)))
    ctx = bytearray(tk.Slot(slot0).relocated(shift).image())
    for k, (p, cap, (want, slot_near)) in enumerate(zip(payloads, caps, near)):
        got = gev_amd.inflate_raw_ctx(p, cap, ctx)
        assert got[0] == want[0] and len(got[1]) == len(want[1]) and got[1] == want[1], (tag, k, got[0], want[0])
        assert_inf_translated(ctx, slot_near, shift, (tag, k))
    return near


def test_relocated_slots_cross_every_boundary(old):
    rng = far.rng_of(0x666172)
    slot0, history = old["slots"]["odd"], old["hist"]["odd"]
    cases = far.far_cases(tk.Slot(slot0).total, far.U_INF)
    combos = [(6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
              (1, zlib.Z_DEFAULT_STRATEGY)]
    for kind, (level, strategy) in zip(far.KINDS, combos):
        # three messages: the second and third run on a slot the code itself wrote at the far position
        first = far.message(rng, history, kind)
        msgs = [first, far.message(rng, history + first, far.KINDS[(far.KINDS.index(kind) + 1) % 5], 5000),
                first[-300:]]
        payloads = peer_chain(history, msgs, level, strategy)
        assert tk.empty_window_differs(payloads[0], msgs[0]) and tk.empty_window_differs(payloads[2], msgs[2])
        near = None
        for name, shift in cases:
            near = run_far_chain(slot0, payloads, shift, [BIG] * 3, near, (name, kind))
        assert [g for g, _ in near] == [(im.OK, m) for m in msgs], kind      # zlib's dictionary run: the messages


def test_short_and_empty_messages_right_at_a_boundary(old):
    rng = far.rng_of(0x65646765)
    slot0, history = old["slots"]["edge"], old["hist"]["edge"]
    short = history[-4000:-3983]
    msgs = [short, b"", far.message(rng, history + short, "text"), b"", far.message(rng, history, "runs", 17)]
    payloads = peer_chain(history, msgs)
    assert len(short) == 17 and payloads[1] == b"\x00" and tk.empty_window_differs(payloads[0], short)
    near = None
    for name, shift in far.edge_cases(tk.Slot(slot0).total, far.U_INF):
        near = run_far_chain(slot0, payloads, shift, [BIG] * 5, near, name)
    assert [g for g, _ in near] == [(im.OK, m) for m in msgs]


def test_distances_on_relocated_slots(old):
    """An old slot holds 32 768 bytes of history wherever it stands, so every distance up to 32 768 is
    allowed -- also where the low 32 bits of `total` alone would say 4 465 bytes.  history + 1 is out of
    reach only on a young slot (32 769 is no DEFLATE distance), and stays GEVWS_MSG_ERR_DEFLATE there."""
    assert tk.match_at(32768) == tk.match3_at_32768()
    slot0, history = old["slots"]["odd"], old["hist"]["odd"]
    window = history[-tk.WIN:]
    cases = far.far_cases(tk.Slot(slot0).total, far.U_INF)
    on32 = tk.Slot(slot0).relocated(dict(cases)["on 2^32"])
    young_len = on32.total & 0xFFFFFFFF
    assert young_len == 4465
    for dist in (32768, young_len + 1, young_len, 1):
        want = (window[-dist:] * 3)[:3]
        assert tk.zlib_inflate_dict(window, tk.match_at(dist)) == (False, want)
        near = None
        for name, shift in cases:
            near = run_far_chain(slot0, [tk.match_at(dist)], shift, [BIG], near, (name, dist))
        assert near[0][0] == (im.OK, want), dist
    young = fresh()
    h = history[:young_len]
    assert gev_amd.inflate_raw_ctx(ic.deflate(h, 0), BIG, young) == (im.OK, h)
    assert gev_amd.inflate_raw_ctx(tk.match_at(young_len), BIG, bytearray(young)) == (im.OK, h[:3])
    assert gev_amd.inflate_raw_ctx(tk.match_at(young_len + 1), BIG, young) == (im.ERR_DEFLATE, b"")
    assert tk.zlib_inflate_dict(h, tk.match_at(young_len + 1))[0]


def test_relocated_failures(old):
    """A failure at a far position loses the context as it does near zero, and a relocated slot that is
    broken stays lost."""
    rng = far.rng_of(0x62726B)
    slot0, history = old["slots"]["odd"], old["hist"]["odd"]
    m = far.message(rng, history, "text")
    p, = peer_chain(history, [m])
    cases = far.far_cases(tk.Slot(slot0).total, far.U_INF)
    for bad, cap, status in ((b"\x06garbage", BIG, im.ERR_DEFLATE), (p, 70000, im.ERR_TOO_BIG)):
        near = None
        for name, shift in cases:
            near = run_far_chain(slot0, [bad, p, ic.deflate(b"on its own")], shift, [cap, BIG, BIG], near, (name, status))
        assert [g[0] for g, _ in near] == [status] * 3 and near[1][0][1] == near[2][0][1] == b""
        assert tk.Slot(near[2][1]).broken == status and tk.Slot(near[2][1]).total == 70001
        if status == im.ERR_TOO_BIG:
            assert near[0][0][1] == m[:70000]                                # the bytes up to the limit
        broken = near[0][1]                                                  # a broken slot, then relocated
        for name, shift in cases:
            ctx = bytearray(tk.Slot(broken).relocated(shift).image())
            before = bytes(ctx)
            assert gev_amd.inflate_raw_ctx(p, BIG, ctx) == (status, b"") and bytes(ctx) == before, name


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_inflate_ctx_fuzz_asan_ubsan(tmp_path):
    exe = tmp_path / "inflate_ctx_fuzz"
    r = subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "inflate_ctx_fuzz.cpp"),
                        os.path.join(ROOT, "gev_amd", "csrc", "gevws_inflate_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and "inflate_ctx_fuzz ok" in r.stdout, r.stdout + r.stderr
