"""GPU checks of the deflate step with GEVWS_DEFLATE_DYNAMIC: a run becomes a
stored, fixed or dynamic-Huffman block.  Every comparison is exact: a payload
is the bytes gevws_deflate_raw_flags (the host twin, pinned on the CPU in
tests/test_deflate_dynamic_host.py) gives for the same message and flag, zlib
inflates it to the input, and the records, the layout of d_out and the summary
are as include/gevws.h states them.  The helpers and the sentinels are those of
tests/test_gpu_deflate.py: 0xFF in every source pad, 0xEE in the outputs."""
import functools
import zlib

import numpy as np
import pytest

import gev_amd
from oracle import ws_oracle as wo
from tests import _inflate_corpus as ic
from tests.test_deflate_dynamic_host import btype, edge_messages
from tests.test_gpu_deflate import B, FILL, T, TAIL, build, check, r16, run, untouched

pytestmark = pytest.mark.gpu

DYN = gev_amd.DEFLATE_DYNAMIC
PLAIN = gev_amd.DEFLATE_PLAIN_IF_NOT_SMALLER
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 4095, 4096, 4097, 8191, 8193, 32769, 70000]


@functools.lru_cache(maxsize=None)
def host(data: bytes, wb: int = 0, flags: int = DYN) -> bytes:
    return gev_amd.deflate_raw(data, wb, flags)


@pytest.fixture(scope="module")
def corpus():
    """[(bytes, opcode, window_bits)] over SIZES: all four kinds up to 4 097, two (rotating) above."""
    rng = np.random.default_rng(0x64796E)
    msgs, k = [], 0
    for n in SIZES:
        kinds = range(4) if n <= 4097 else ((k % 4), (k + 1) % 4)
        for kind in kinds:
            msgs.append((ic.sample(rng, n, kind), T if kind in (2, 3) else B, 0))
        k += 1
    return msgs


def test_sizes_and_kinds(engine, corpus):
    arena, src_bytes, rec = build(corpus)
    want = [host(d, wb) for d, _, wb in corpus]
    for (d, _, _), w in zip(corpus, want):
        assert zlib.decompressobj(-15).decompress(w + TAIL) == d
        assert len(w) <= len(host(d, 0, 0)) <= gev_amd.deflate_bound(len(d))
    assert any(len(d) and btype(w) == 2 for (d, _, _), w in zip(corpus, want))  # dynamic blocks are in the batch
    need = sum(r16(len(w)) for w in want)
    got = run(engine, arena, src_bytes, rec, need + 4096, flags=DYN)
    check(got, corpus, want)
    assert sorted(set(int(x) for x in rec["length"])) == sorted(SIZES)


def test_edge_messages_in_one_batch(engine):
    msgs = [(d, B, wb) for _, d in edge_messages() for wb in (0, 9)]
    arena, src_bytes, rec = build(msgs)
    want = [host(d, wb) for d, _, wb in msgs]
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want), flags=DYN)
    check(got, msgs, want)


def test_alone_and_as_entry_37_of_64(engine):
    rng = np.random.default_rng(0x3337)
    sizes = [int(x) for x in rng.choice([0, 1, 5, 64, 100, 300, 1000, 4096, 5000, 9000, 20000], 64)]
    msgs = [(ic.sample(rng, n, int(rng.integers(0, 4))), B, int(rng.choice([0, 9, 10, 15]))) for n in sizes]
    mine = (ic.sample(rng, 13001, 0), T, 10)
    msgs[37] = mine
    arena, src_bytes, rec = build(msgs)
    want = [host(d, wb) for d, _, wb in msgs]
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want), flags=DYN)
    check(got, msgs, want)
    a1, n1, r1 = build([mine])
    a1[n1 - (r16(13001) - 13001):n1] = 0x00  # another pad behind it, too
    alone = run(engine, a1, n1, r1, r16(len(want[37])), flags=DYN)
    check(alone, [mine], [want[37]])
    f = got["frames"][37]
    assert alone["out"][:len(want[37])].tobytes() == \
        got["out"][int(f["payload_off"]):int(f["payload_off"]) + int(f["payload_len"])].tobytes()


def skewed(rng, n: int) -> bytes:
    """n random bytes over the 64 values 160..223: few matches, about 6 bits a
    byte with dynamic codes, 9 with the fixed code, 8 and a header stored."""
    return (rng.integers(0, 64, n, dtype=np.uint8) + 160).tobytes()


def test_combined_with_plain_if_not_smaller(engine):
    """The plain choice follows the dynamic-mode length.  `only` compresses
    with dynamic codes alone: 64 byte values of 9-bit fixed codes and few
    matches, which fixed and stored blocks both leave longer than the message."""
    rng = np.random.default_rng(0x706C64)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    only = skewed(rng, 3000)
    msgs = [(rnd(1000), B, 0), (b"", T, 0), (ic.sample(rng, 1000, 0), T, 0), (only, B, 0), (rnd(5000), B, 0),
            (b"abc", T, 0), (ic.sample(rng, 70000, 2), T, 12), (rnd(17), B, 9)]
    comp = [host(d, wb) for d, _, wb in msgs]
    fixed = [host(d, wb, 0) for d, _, wb in msgs]
    plain = [len(c) >= len(d) for (d, _, _), c in zip(msgs, comp)]
    assert plain == [True, True, False, False, True, True, False, True]
    assert len(fixed[3]) >= len(only) > len(comp[3])
    want = [d if p else c for (d, _, _), c, p in zip(msgs, comp, plain)]
    arena, src_bytes, rec = build(msgs)
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want), flags=DYN | PLAIN)
    check(got, msgs, want, plain)
    # with PLAIN alone the message that only dynamic codes compress goes out plain
    plain0 = [len(c) >= len(d) for (d, _, _), c in zip(msgs, fixed)]
    assert plain0[3] and not plain[3]
    want0 = [d if p else c for (d, _, _), c, p in zip(msgs, fixed, plain0)]
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want0), flags=PLAIN)
    check(got, msgs, want0, plain0)


def test_capacity_then_retry(engine):
    rng = np.random.default_rng(0x636170)
    msgs = [(ic.sample(rng, n, k), B, 0) for n, k in ((100, 0), (0, 0), (5000, 1), (5000, 0), (777, 2), (16, 1))]
    want = [host(d) for d, _, _ in msgs]
    need = sum(r16(len(w)) for w in want)
    arena, src_bytes, rec = build(msgs)
    short = run(engine, arena, src_bytes, rec, need - 1, flags=DYN)
    s = short["summary"]
    assert int(s["status"]) == gev_amd.ERR_CAPACITY and int(s["payload_bytes"]) == need and int(s["errors"]) == 0
    assert untouched(short)
    full = run(engine, arena, src_bytes, rec, need, flags=DYN)
    check(full, msgs, want)
    # Engine.deflate retries by itself
    import torch
    res = engine.deflate(rec, torch.from_numpy(arena).to(torch.device("cuda", engine.device)), src_bytes, flags=DYN,
                         out_cap=16)
    assert [res.payload(i) for i in range(len(msgs))] == want
    assert res.frames_host().tobytes() == full["frames"].tobytes()


def test_unknown_flag_bits(engine):
    msgs = [(b"abc", T, 0)]
    arena, src_bytes, rec = build(msgs)
    for flags in (4, 8 | DYN, 1 << 31):
        with pytest.raises(RuntimeError):
            run(engine, arena, src_bytes, rec, 64, flags=flags)


def test_flag_zero_is_unchanged(engine, corpus):
    msgs = [m for m in corpus if len(m[0]) <= 8193]
    arena, src_bytes, rec = build(msgs)
    want = [gev_amd.deflate_raw(d) for d, _, _ in msgs]
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want))
    check(got, msgs, want)


def test_closed_loop_on_the_device(engine):
    """deflate with dynamic blocks -> encode (unmasked, as a server sends) ->
    decode -> message pass with every connection EXT_DEFLATE -> inflate: the
    original messages."""
    import torch
    rng = np.random.default_rng(0x6C6F6F70)
    dev = torch.device("cuda", engine.device)
    utf8 = lambda b: b.decode("utf-8", "ignore").encode()  # noqa: E731
    groups = [  # one connection each; a frame needs six bytes at hand to be decoded, so each ends with a big one
        [(utf8(ic.sample(rng, 1000, 0)), T), (b"", T), (ic.sample(rng, 300, 1), B), (b"a", T),
         (utf8(ic.sample(rng, 70000, 0)), T)],
        [(ic.sample(rng, 5000, 1), B), (ic.sample(rng, 4096, 3), T), (ic.sample(rng, 33000, 2), T)],
        [(skewed(rng, 9000), B), (ic.sample(rng, 20000, 0), B)],
    ]
    flat = [(d, op, int(rng.choice([0, 10, 15]))) for g in groups for d, op in g]
    arena, src_bytes, rec = build(flat)
    want = [host(d, wb) for d, _, wb in flat]
    assert sum(btype(w) == 2 for w in want) >= 4
    got = run(engine, arena, src_bytes, rec, sum(r16(len(w)) for w in want), flags=DYN)
    check(got, flat, want)
    n = len(flat)
    # the records and d_out go to the encoder as they stand
    wire_cap = sum(len(w) + 10 for w in want)
    wire = torch.full((wire_cap + gev_amd._abi.OUT_PAD,), FILL, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(n, dtype=torch.int64, device=dev)
    esum = torch.zeros(64, dtype=torch.uint8, device=dev)
    engine.encode_async(got["dev"]["frames"], n, got["dev"]["out"], wire, wire_cap, out_off, esum)
    torch.cuda.synchronize(engine.device)
    es = esum.cpu().numpy().view(gev_amd.SUMMARY_DTYPE)[0]
    assert int(es["status"]) == gev_amd.OK
    total = int(es["payload_bytes"])
    wire_host = wire[:total].cpu().numpy().tobytes()
    offs = [int(x) for x in out_off.cpu().numpy()] + [total]
    res = wo.decode_stream(wire_host + b"\0" * 8)
    assert len(res.frames) >= n
    for i, (fr, (d, op, _), w) in enumerate(zip(res.frames, flat, want)):
        h = fr.header
        assert (h.fin, h.rsv, h.opcode, h.masked, h.length) == (True, 4, op, False, len(w)), i
        assert fr.stream_pos == offs[i] and fr.payload == w, i
    # back in: one connection per group
    table, k = [], 0
    for g in groups:
        table.append((offs[k], offs[k + len(g)] - offs[k]))
        k += len(g)
    from tests._helpers import gpu_decode
    out = gpu_decode(engine, np.frombuffer(wire_host, np.uint8).copy(), np.array(table, np.int64))
    assert int(out.summary_host()["frames"]) == n
    conn_ext = torch.full((len(groups),), gev_amd.EXT_DEFLATE, dtype=torch.uint8, device=dev)
    state = torch.zeros((len(groups), 8), dtype=torch.uint8, device=dev)
    msgs = engine.messages(out, state=state, conn_ext=conn_ext)
    m = msgs.messages_host()
    assert m.shape[0] == n and np.all(m["flags"] & gev_amd.MSG_COMPRESSED != 0)
    assert [int(x) for x in m["opcode"]] == [op for _, op, _ in flat]
    inf = engine.inflate(out, msgs, 1 << 20, state=state)
    s = inf.summary_host()
    assert int(s["frames"]) == n and int(s["errors"]) == 0
    for i, (d, _, _) in enumerate(flat):
        assert inf.message_bytes(i) == d, i
    assert not state.cpu().numpy().any()
