"""The synthetic-batch verifier (k_synth_verify behind gevws_synth_verify_async
and Engine.verify) pinned against a plain numpy restatement of its contract.

Every full-size claim rests on that kernel returning 0, so these tests make it
return something else: each mutation of a decoded batch's records or payload
must make the device count equal tests._helpers.verify_host's count on the
same data, exactly, and be non-zero.  The CPU test proves the reference itself:
0 on an oracle-decoded batch and the count derivable by hand for every
mutation that has one.  The layout is the one no workload config reaches:
masked and unmasked frames, non-minimal length forms, zero-length frames,
every opcode class, RSV bits, a frame of 64 KiB.

The mutations inject wrong data, never a wrong address: an out-of-range or
misaligned record is counted by the verifier and not dereferenced."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import gev_amd
from gev_amd import workloads as w
from oracle import ref
from tests._helpers import check_against_oracle, check_batch_structure, host_result, verify_host

BIG = 8192 + 5       # second trip of the verifier's 4 096-byte stride, 11 pad bytes
SEED = 0x67657607

# (payload length, FIN | RSV | opcode, masked, length form) per frame, per connection
_MIXED = [
    [(BIG, 0x82, 1, 16), (0, 0x81, 1, 7), (1, 0x81, 0, 7), (15, 0x89, 1, 7), (16, 0x82, 0, 16), (17, 0xC2, 1, 64)],
    [(1023, 0x82, 1, 16), (1024, 0x82, 0, 64), (1040, 0x01, 1, 16), (0, 0x00, 0, 16), (17, 0x9A, 0, 7),
     (0, 0x80, 1, 64), (0, 0x88, 1, 7)],
    [(4080, 0x82, 1, 16), (4095, 0x81, 0, 16), (4096, 0x02, 1, 64), (4097, 0x80, 0, 16), (BIG, 0x82, 0, 64)],
    [(65536, 0x82, 1, 64), (65536 + 5, 0x02, 0, 64), (1, 0xA0, 1, 16)],
    [(15, 0x8A, 0, 7), (16, 0x82, 1, 7), (125, 0x89, 1, 16), (126, 0x81, 0, 16), (BIG, 0x82, 1, 64)],
]
MID = sum(len(c) for c in _MIXED[:3]) - 1    # the unmasked BIG frame in the middle
K64 = MID + 1                                # the 64 KiB frame


def mixed_layout(n_conns: int = len(_MIXED)):
    cs = _MIXED[:n_conns]
    col = lambda k, t: [np.array([f[k] for f in c], t) for c in cs]
    return w.assemble("mixed forms", col(0, np.int64), col(1, np.uint8), col(2, np.uint8), SEED,
                      len_form_per_conn=col(3, np.uint8))


def grid_layout():
    """65 536 + 300 frames of 0..20 bytes: more frames than the verifier's grid has workgroups."""
    n = (1 << 16) + 300
    g = np.arange(n)
    L = ((g + 5) % 21).astype(np.int64)
    b0 = np.where(g % 5 == 0, 0x81, 0x82).astype(np.uint8)
    masked = (g % 3 != 0).astype(np.uint8)
    cuts = [0, 7, 1000, 1001, 40000, n]
    part = lambda a: [a[i:j] for i, j in zip(cuts[:-1], cuts[1:])]
    return w.assemble("grid stride", part(L), part(b0), part(masked), SEED + 1)


def _base_from_oracle(lay):
    arena = w.synth_host(lay)
    got = ref.decode_batch(arena, lay.conns[:, 0], lay.conns[:, 1], max_frames=lay.n_frames,
                           payload_cap=lay.payload_padded)
    assert got["frames"].shape[0] == lay.n_frames and got["total_payload"] == lay.payload_padded
    return SimpleNamespace(lay=lay, frames=got["frames"].view(gev_amd.FRAME_DTYPE), payload=got["payload"],
                           cap=lay.payload_padded)


# --------------------------------------------------------------------------- the mutation matrix
GROUPS = ["bytes", "fin", "rsv", "opcode", "masked", "key0", "key1", "key2", "key3", "length", "src_off",
          "unmasked_key", "payload_off_shift", "payload_off_misaligned", "payload_off_out_of_range",
          "truncated_cap", "additivity"]


def _flip(f, i):
    """Flip bits of byte i of frame f's slot in the arena (i may be a pad byte)."""
    def fn(fr, pay):
        pay[int(fr["payload_off"][f]) + i] ^= 0x5A
    return fn


def _field(f, name, delta):
    def fn(fr, pay):
        if name.startswith("key"):
            fr["mask"][f, int(name[3])] ^= delta
        elif name in ("fin", "rsv", "opcode", "masked"):
            fr[name][f] ^= delta
        else:
            fr[name][f] = int(fr[name][f]) + delta
    return fn


def _set_off(f, value):
    def fn(fr, pay):
        fr["payload_off"][f] = value(int(fr["payload_off"][f])) if callable(value) else value
    return fn


def _both(*fns):
    def fn(fr, pay):
        for x in fns:
            x(fr, pay)
    return fn


def mutations(base, group):
    """[(name, fn(frames, payload), payload_cap, count derivable by hand or None)]"""
    d = base.lay.desc
    n, cap = base.lay.n_frames, base.cap
    L = d["length"].astype(np.int64)
    pad = (L + 15) // 16 * 16
    first, last = 0, n - 1
    assert L[first] == BIG and L[MID] == BIG and L[last] == BIG and L[K64] == 65536
    assert d["masked"][first] and not d["masked"][MID]
    out = []
    if group == "bytes":
        for f in (first, MID, last):
            pos = [0, BIG - 1, 1023, 1024, 4095, 4096] + list(range(BIG, int(pad[f])))
            out += [(f"frame {f} byte {i}", _flip(f, i), cap, 1) for i in pos]
        out.append(("last byte of the 64 KiB frame", _flip(K64, 65535), cap, 1))
        for f in range(n):  # every other frame: its first and last byte and each pad byte
            if f in (first, MID, last) or L[f] == 0:
                continue
            pos = sorted({0, int(L[f]) - 1} | set(range(int(L[f]), int(pad[f]))))
            out += [(f"frame {f} (L={L[f]}) byte {i}", _flip(f, i), cap, 1) for i in pos]
    elif group in ("fin", "rsv", "opcode", "masked", "key0", "key1", "key2", "key3"):
        delta = {"fin": 1, "rsv": 2, "opcode": 8, "masked": 1}.get(group, 0x80)
        out += [(f"{group} of frame {f}", _field(f, group, delta), cap, 1) for f in (first, 1, MID, last)]
    elif group in ("length", "src_off"):
        out += [(f"{group} {s:+d} of frame {f}", _field(f, group, s), cap, 1)
                for f in (first, 1, MID, last) for s in (1, -1)]
    elif group == "unmasked_key":
        unm = [f for f in range(n) if not d["masked"][f]]
        out += [(f"key byte {k} of unmasked frame {f}", _field(f, f"key{k}", 7), cap, 1)
                for f in (unm[0], MID) for k in (0, 3)]
    elif group == "payload_off_shift":
        # still in range: the content at the new place mismatches, only the reference knows by how much
        out += [(f"payload_off +16 of frame {f}", _set_off(f, lambda o: o + 16), cap, None) for f in (first, MID, K64)]
        out.append(("payload_off -16 of the last frame", _set_off(last, lambda o: o - 16), cap, None))
    elif group == "payload_off_misaligned":
        # the alignment field alone: a misaligned record's bytes are not read
        out += [(f"payload_off +1 of frame {f}", _set_off(f, lambda o: o + 1), cap, 1) for f in (first, 1, MID)]
        out.append(("payload_off -15 of the last frame", _set_off(last, lambda o: o - 15), cap, 1))
        out.append(("payload_off +1 and fin of frame 0", _both(_set_off(first, lambda o: o + 1),
                                                              _field(first, "fin", 1)), cap, 2))
    elif group == "payload_off_out_of_range":
        for f in (first, 1, MID, last):
            for name, v in (("cap + 16", cap + 16), ("2**63", 1 << 63), ("2**64 - 16", (1 << 64) - 16)):
                out.append((f"payload_off = {name} of frame {f}", _set_off(f, v), cap, int(L[f]) + 1))
        out.append(("payload_off +16 of the last frame", _set_off(last, lambda o: o + 16), cap, BIG + 1))
        # a field mismatch of an out-of-range record is not counted on top
        out.append(("out of range and fin", _both(_set_off(MID, cap + 16), _field(MID, "fin", 1)), cap, BIG + 1))
    elif group == "truncated_cap":
        # the real buffer, a smaller number: the frames past it are out of range
        off = base.frames["payload_off"].astype(np.int64)
        for c in (cap - 16, int(off[last]) + 16, int(off[K64]) + 4096, 0):
            out.append((f"payload_cap = {c}", lambda fr, pay: None, c, None))
    elif group == "additivity":
        out.append(("two waves of one frame", _both(_flip(first, 0), _flip(first, 1024)), cap, 2))
        out.append(("both trips of one thread", _both(_flip(MID, 3), _flip(MID, 4096 + 3)), cap, 2))
        out.append(("three bytes of one vector", _both(_flip(last, 16), _flip(last, 17), _flip(last, 31)), cap, 3))
        out.append(("every wave of one frame", _both(*[_flip(K64, 1024 * k + 5) for k in range(64)]), cap, 64))
        out.append(("two frames", _both(_flip(first, 7), _flip(last, BIG - 1)), cap, 2))
        out.append(("field and byte", _both(_field(MID, "opcode", 1), _flip(MID, 100)), cap, 2))
        out.append(("every field of one record", _both(*[_field(3, k, 1) for k in
                                                         ("fin", "rsv", "opcode", "masked", "key1", "length",
                                                          "src_off")]), cap, 7))
    assert out
    return out


def _mutated(base, fn):
    fr, pay = base.frames.copy(), base.payload.copy()
    fn(fr, pay)
    return fr, pay


# --------------------------------------------------------------------------- CPU: the reference itself
@pytest.fixture(scope="module")
def oracle_base():
    return _base_from_oracle(mixed_layout())


def test_reference_verifier_accepts_an_oracle_decode(oracle_base):
    b = oracle_base
    assert verify_host(b.lay.desc, b.lay.seed, b.frames, b.payload, b.cap) == 0
    small = _base_from_oracle(mixed_layout(2))
    assert verify_host(small.lay.desc, small.lay.seed, small.frames, small.payload, small.cap) == 0


def test_mixed_layout_holds_what_the_configs_lack():
    d = mixed_layout().desc
    L = d["length"].astype(np.int64)
    assert set(d["masked"]) == {0, 1} and (L == 0).sum() >= 3 and (L >= 65536).sum() >= 1
    nonmin = d["len_form"] != w.min_len_form(L)
    assert set(d["len_form"][nonmin]) == {16, 64} and set(d["len_form"]) == {7, 16, 64}
    assert {0x0, 0x1, 0x2, 0x8, 0x9, 0xA} <= set(d["b0"] & 0x0F)
    assert (d["b0"] & 0x70).any() and set(d["b0"] >> 7) == {0, 1}
    assert (nonmin & (d["masked"] == 0)).any() and ((L == 0) & (d["masked"] == 0)).any()
    for x in (0, 1, 15, 16, 17, 1023, 1024, 1040, 4080, 4095, 4096, 4097, BIG, 65536):
        assert x in L


@pytest.mark.parametrize("group", GROUPS)
def test_reference_verifier_counts_each_mutation(oracle_base, group):
    b = oracle_base
    for name, fn, cap, hand in mutations(b, group):
        fr, pay = _mutated(b, fn)
        got = verify_host(b.lay.desc, b.lay.seed, fr, pay, cap)
        assert got > 0, name
        if hand is not None:
            assert got == hand, name
    if group == "truncated_cap":  # bounded by hand even where the exact count is the reference's
        L = b.lay.desc["length"].astype(np.int64)
        assert verify_host(b.lay.desc, b.lay.seed, b.frames, b.payload, b.cap - 16) == BIG + 1
        assert verify_host(b.lay.desc, b.lay.seed, b.frames, b.payload, 0) == int((L + 1).sum())


def test_reference_verifier_on_the_grid_stride_layout():
    """Its first two connections (1 000 frames, masked and not), oracle-decoded, count 0."""
    lay = grid_layout()
    assert lay.n_frames == 65536 + 300 and int(lay.desc["length"].max()) == 20
    n = 1000
    head = w.Layout(lay.name, lay.desc[:n], lay.conns[:2], int(lay.conns[1, 0] + lay.conns[1, 1]), 0, 0, lay.seed)
    got = ref.decode_batch(w.synth_host(head), head.conns[:, 0], head.conns[:, 1])
    assert got["frames"].shape[0] == n
    assert verify_host(head.desc, lay.seed, got["frames"], got["payload"], got["total_payload"]) == 0
    got["payload"][int(got["frames"]["payload_off"][n - 1])] ^= 1
    assert verify_host(head.desc, lay.seed, got["frames"], got["payload"], got["total_payload"]) == 1


# --------------------------------------------------------------------------- GPU
def _device_state(engine, lay):
    import torch
    dev = torch.device("cuda", engine.device)
    arena = torch.zeros(lay.arena_bytes + gev_amd.IN_PAD, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(lay.desc.view(np.uint8).copy()).to(dev)
    conns = torch.from_numpy(lay.conns.copy()).to(dev)
    engine.synth(arena, desc, lay.n_frames, lay.seed)
    out = engine.decode(arena, lay.arena_bytes, conns, lay.n_conns, max_frames=lay.n_frames,
                        payload_cap=lay.payload_padded)
    assert out.payload.numel() == lay.payload_padded + 16
    frames = out.frames[: lay.n_frames].cpu().numpy().reshape(-1).view(gev_amd.FRAME_DTYPE)
    return SimpleNamespace(lay=lay, frames=frames, payload=out.payload.cpu().numpy(), cap=lay.payload_padded,
                           arena=arena, desc_dev=desc, out=out, dev=dev)


def _device_count(engine, st, fr, pay, cap=None, calls: int = 1, start: int = 0) -> int:
    """The device verifier's counter after `calls` calls on clones of the records and the arena."""
    import torch
    lay = st.lay
    clone = gev_amd.Batch(frames=torch.from_numpy(fr.view(np.uint8).reshape(-1, 32).copy()).to(st.dev),
                          payload=torch.from_numpy(pay.copy()).to(st.dev), conn_out=st.out.conn_out,
                          summary=st.out.summary, n_conns=lay.n_conns)
    assert clone.payload.numel() == st.cap + 16
    mism = torch.full((1,), start, dtype=torch.int64, device=st.dev)
    for _ in range(calls):
        if cap is None or cap == st.cap:
            engine.verify(st.desc_dev, lay.n_frames, lay.seed, clone, mism)
        else:
            assert cap < st.cap  # the real buffer and only a smaller number
            rc = gev_amd.lib.gevws_synth_verify_async(
                engine._ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), st.desc_dev.data_ptr(),
                lay.n_frames, lay.seed, clone.frames.data_ptr(), clone.payload.data_ptr(), cap, mism.data_ptr())
            assert rc == gev_amd.OK
    torch.cuda.synchronize()
    return int(mism.item())


@pytest.fixture(scope="module")
def mixed(engine):
    return _device_state(engine, mixed_layout())


@pytest.mark.gpu
@pytest.mark.parametrize("n_conns", [len(_MIXED), 2])
def test_mixed_layout_three_ways(engine, n_conns):
    """Generator == host generator, decode == oracle, verifier == reference (both 0),
    on the whole mixed layout and on a part small enough for the one-launch decode."""
    import torch
    from gev_amd import _abi
    lay = mixed_layout(n_conns)
    assert (lay.arena_bytes <= _abi.ONE_LAUNCH_MAX_BYTES) == (n_conns == 2)
    st = _device_state(engine, lay)
    host_in = w.synth_host(lay)
    assert np.array_equal(st.arena[: lay.arena_bytes].cpu().numpy(), host_in)
    assert not st.arena[lay.arena_bytes:].any()
    check_against_oracle(host_result(st.out), host_in, lay.conns, lay.name)
    check_batch_structure(st.out, lay, st.desc_dev)
    mism = torch.zeros(1, dtype=torch.int64, device=st.dev)
    engine.verify(st.desc_dev, lay.n_frames, lay.seed, st.out, mism)
    torch.cuda.synchronize()
    assert int(mism.item()) == 0
    assert verify_host(lay.desc, lay.seed, st.frames, st.payload, st.cap) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_device_verifier_counts_each_mutation(engine, mixed, group):
    st = mixed
    for name, fn, cap, hand in mutations(st, group):
        fr, pay = _mutated(st, fn)
        want = verify_host(st.lay.desc, st.lay.seed, fr, pay, cap)
        got = _device_count(engine, st, fr, pay, cap)
        print(f"{group}: {name}: device {got}, reference {want}, by hand {hand}")
        assert got == want, name
        assert got > 0, name
        if hand is not None:
            assert got == hand, name


@pytest.mark.gpu
def test_device_verifier_accumulates(engine, mixed):
    st = mixed
    fr, pay = _mutated(st, _both(_flip(0, 0), _flip(MID, 4096), _field(K64, "rsv", 1)))
    want = verify_host(st.lay.desc, st.lay.seed, fr, pay, st.cap)
    assert want == 3
    assert _device_count(engine, st, fr, pay) == want
    assert _device_count(engine, st, fr, pay, calls=2) == 2 * want
    assert _device_count(engine, st, fr, pay, calls=1, start=1000) == 1000 + want
    assert _device_count(engine, st, st.frames, st.payload, calls=2, start=5) == 5


@pytest.mark.gpu
def test_device_verifier_past_its_grid_cap(engine):
    """Frames 65 536 and up are reached only by the grid-stride loop."""
    lay = grid_layout()
    st = _device_state(engine, lay)
    check_batch_structure(st.out, lay, st.desc_dev)
    assert _device_count(engine, st, st.frames, st.payload) == 0
    n = lay.n_frames
    f, last = (1 << 16) + 7, n - 1
    L = lay.desc["length"].astype(np.int64)
    assert L[f] == 7 and L[last] == 5
    fr, pay = _mutated(st, _both(_flip(f, 0), _flip(last, 4), _flip(last, 15), _field(last, "fin", 1)))
    got = _device_count(engine, st, fr, pay)
    assert got == 4
    assert got == verify_host(lay.desc, lay.seed, fr, pay, st.cap)
    # one mutation at a time, frames on both sides of the cap
    for g in (0, (1 << 16) - 1, 1 << 16, f, last):
        fr, pay = _mutated(st, _field(g, "src_off", 1))
        assert _device_count(engine, st, fr, pay) == 1, g


@pytest.mark.gpu
def test_verify_argument_contract(engine, mixed):
    import torch
    st = mixed
    lay = st.lay
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = gev_amd.lib.gevws_synth_verify_async
    mism = torch.full((1,), 5, dtype=torch.int64, device=st.dev)
    args = (st.desc_dev.data_ptr(), lay.n_frames, lay.seed, st.out.frames.data_ptr(), st.out.payload.data_ptr(),
            st.cap)
    assert call(engine._ctx, stream, None, 0, lay.seed, None, None, 0, mism.data_ptr()) == gev_amd.OK
    assert call(engine._ctx, stream, args[0], 0, *args[2:], mism.data_ptr()) == gev_amd.OK
    assert call(engine._ctx, stream, *args, None) == gev_amd.ERR_INVALID
    assert call(engine._ctx, stream, args[0], lay.n_frames, lay.seed, None, args[4], st.cap,
                mism.data_ptr()) == gev_amd.ERR_INVALID
    assert call(engine._ctx, stream, None, lay.n_frames, lay.seed, args[3], args[4], st.cap,
                mism.data_ptr()) == gev_amd.ERR_INVALID
    assert call(None, stream, *args, mism.data_ptr()) == gev_amd.ERR_INVALID
    torch.cuda.synchronize()
    assert int(mism.item()) == 5
    with pytest.raises(ValueError):
        engine.verify(st.desc_dev, lay.n_frames + 1, lay.seed, st.out, mism)
