"""Compressed messages that span passes (gevws_inflate_carry_async,
gevws_join_carry_ext_async; include/gevws.h) restated in plain Python on top of
tests/_carry_model.py, tests/_inflate_gpu_model.py and
tests/_inflate_takeover.py, which this module imports and does not change.

  model_inflate_carry   it.model_inflate_ctx with the carry's `in` side: a
                        continued message over an OPEN | COMPRESSED record is
                        whole behind its carried bytes
  carry_model_ext       cm.carry_model with carry_flags
  chain_model / chain_device
                        messages -> inflate(carry) -> join(carry, compressed)
                        over a list of passes, state, slots and carry handed on

Expected bytes come from zlib and the verdicts of small streams from the Python
inflate model, as in the modules underneath."""
from __future__ import annotations

import zlib

import numpy as np

from tests import _carry_model as cm
from tests import _inflate_gpu_model as gm
from tests import _inflate_model as im
from tests import _inflate_takeover as it
from tests import _join_model as jm
from tests import _messages_model as mm

OPEN, LOST, COMPRESSED = cm.OPEN, cm.LOST, 4
KEEP_COMPRESSED = 1
RSV1 = 4
FILL, GUARD = jm.FILL, jm.GUARD


def _bad_open(r, src_bytes: int) -> bool:
    return bool(int(r["flags"]) & OPEN and (int(r["off"]) % 16 or int(r["off"]) + int(r["length"]) > src_bytes))


# ---------------------------------------------------------------------------- the inflate
def model_inflate_carry(d: mm.Decoded, tables: dict, limit: int, state, ext, slots, n_conns: int, carry_in,
                        carry_src, carry_src_bytes=None):
    """What gevws_inflate_carry_async must produce: it.model_inflate_ctx's dict,
    or dict(invalid=count) for malformed input.  ext None: no takeover; slots
    (a list of it.Slot, or None without contexts) is updated in place."""
    msgs, msg_of = tables["messages"], tables["msg_of"]
    ext = np.zeros(n_conns, np.uint8) if ext is None else ext
    src_bytes = carry_src.size if carry_src_bytes is None else carry_src_bytes
    bad = int(np.count_nonzero(msgs["conn"] >= n_conns))
    bad += sum(1 for c in sorted({int(c) for c in msgs["conn"] if int(c) < n_conns})
               if _bad_open(carry_in[c], src_bytes))
    if bad:
        return dict(invalid=bad)
    rec = np.zeros(msgs.shape[0], gm.INFLATED_DTYPE)
    data = [b""] * msgs.shape[0]
    st_out = None if state is None else state.copy()
    off = ok = total = errors = 0
    failed_conns, stopped = set(), set()
    for m in range(msgs.shape[0]):
        flags, c = int(msgs["flags"][m]), int(msgs["conn"][m])
        if not flags & gm.COMPRESSED:
            continue
        take = bool(slots is not None and int(ext[c]) & it.EXT_TAKEOVER)
        ci = carry_in[c]
        cf = int(ci["flags"])
        kind, prefix = "pending", b""
        if flags & (mm.BEGIN | mm.END) == (mm.BEGIN | mm.END):
            kind = "whole"
        elif not flags & mm.BEGIN and flags & mm.END and int(msgs["status"][m]) == mm.OK:
            if cf & (OPEN | COMPRESSED) == OPEN | COMPRESSED:
                kind = "whole"
                prefix = carry_src[int(ci["off"]): int(ci["off"]) + int(ci["length"])].tobytes()
            elif not cf & OPEN and cf & LOST and int(ci["status"]):
                kind = "lost"
        if take and slots[c].broken:
            st, out = slots[c].broken, b""
        elif kind == "pending" or (take and c in stopped):
            rec[m]["flags"] = gm.INF_PENDING
            stopped.add(c)
            continue
        elif kind == "lost":
            st, out = int(ci["status"]), b""
            if take:
                slots[c].broken = st
        else:
            fs = np.flatnonzero(msg_of == m)
            payload = prefix + b"".join(
                d.arena[int(d.frames["payload_off"][f]):][: int(d.frames["length"][f])].tobytes() for f in fs)
            st, out = slots[c].feed(payload, limit) if take else gm.expect_stream(payload, limit)
        if st == im.OK and int(msgs["opcode"][m]) == 1 and not gm.py_valid(out):
            st = mm.ERR_UTF8
        keep = st in (im.OK, mm.ERR_UTF8)
        rec[m]["flags"], rec[m]["status"], rec[m]["out_off"] = gm.INF_DONE, st, off
        if keep:
            rec[m]["length"], data[m] = len(out), out
            off += (len(out) + 15) // 16 * 16
            total += len(out)
        if st == im.OK:
            ok += 1
        else:
            errors += 1
            if c not in failed_conns and st_out is not None and int(st_out[c]["failed"]) == 0:
                st_out[c]["failed"] = st
            failed_conns.add(c)
    return dict(inflated=rec, bytes=data, state=st_out, frames=ok, payload_bytes=off, payload_len=total,
                errors=errors)


def inflate_image(want: dict, cap: int) -> np.ndarray:
    """d_out[0, cap) behind the inflate `want`, over FILL."""
    img = np.full(cap, FILL, np.uint8)
    wi = want["inflated"]
    for m in np.flatnonzero(wi["length"] > 0):
        o, n = int(wi["out_off"][m]), int(wi["length"][m])
        img[o: o + n] = np.frombuffer(want["bytes"][m], np.uint8)
        img[o + n: o + jm.round16(n)] = 0
    return img


# ---------------------------------------------------------------------------- the join
def carry_model_ext(frames, arena, tables, n_conns, max_message_bytes, carry_in=None, carry_src=None, flags=0,
                    out_cap=None, carry_cap=None, inflated=None, inflate_summary=None, msg_status=0, out_image=None,
                    carry_src_bytes=None, carry_flags=0):
    """cm.carry_model with carry_flags.  With KEEP_COMPRESSED the rules are
    cm.carry_model's over rewritten inputs: an open compressed message is kept
    like a plain one, a continued compressed message that ends is delivered
    like a whole one (from its inflate record), and a record and a message that
    disagree in COMPRESSED meet like a message and a zero record; the kept
    records get the bit and the rewritten messages' body status is put back."""
    args = (flags, out_cap, carry_cap, inflated, inflate_summary, msg_status, out_image, carry_src_bytes)
    if not carry_flags & KEEP_COMPRESSED:
        return cm.carry_model(frames, arena, tables, n_conns, max_message_bytes, carry_in, carry_src, *args)
    messages, conn_msg = tables["messages"].copy(), tables["conn_msg"]
    orig = tables["messages"]
    cin = (np.zeros(n_conns, cm.CARRY_DTYPE) if carry_in is None else carry_in).copy()
    src_bytes = (0 if carry_src is None else carry_src.size) if carry_src_bytes is None else carry_src_bytes
    n = messages.shape[0]
    kept = np.zeros(n_conns, bool)      # an OPEN output record of c holds compressed bytes
    as_plain = []                       # open compressed messages shown to the model as plain
    sane = not np.any(messages["conn"] >= n_conns) and all(
        int(conn_msg["first_message"][c]) + int(conn_msg["nmessages"][c]) <= n for c in range(n_conns))
    for c in range(n_conns if sane else 0):
        nm = int(conn_msg["nmessages"][c])
        ci_comp = bool(int(cin["flags"][c]) & COMPRESSED)
        if _bad_open(cin[c], src_bytes):
            continue  # (the call is INVALID)
        if nm == 0:
            kept[c] = ci_comp
            continue
        first, last = int(conn_msg["first_message"][c]), int(conn_msg["first_message"][c]) + nm - 1
        ff = int(orig["flags"][first])
        if not ff & mm.BEGIN and int(cin["flags"][c]) & OPEN and bool(ff & gm.COMPRESSED) != ci_comp:
            cin[c] = np.zeros((), cm.CARRY_DTYPE)  # the caller mixed up its states
        if ff & gm.COMPRESSED and not ff & mm.BEGIN and ff & mm.END:
            messages["flags"][first] |= mm.BEGIN   # delivered from its inflate record, like a whole one
        lf = int(orig["flags"][last])
        if lf & gm.COMPRESSED and not lf & mm.END:
            messages["flags"][last] &= ~np.uint8(gm.COMPRESSED)
            as_plain.append(last)
            kept[c] = True
    t2 = dict(tables, messages=messages)
    w = cm.carry_model(frames, arena, t2, n_conns, max_message_bytes, cin, carry_src, *args)
    if w["carry"] is not None:
        for c in np.flatnonzero(kept):
            if int(w["carry"]["flags"][c]) & OPEN:
                w["carry"]["flags"][c] |= COMPRESSED
    if w["bodies"] is not None:
        for m in as_plain:
            w["bodies"]["status"][m] = orig["status"][m] if inflated is None else inflated["status"][m]
    return w


# ---------------------------------------------------------------------------- device runs
def run_inflate_carry(engine, got: dict, limit: int, out_cap: int, ext, ctx, n_conns: int, carry_in, carry_src,
                      carry_src_bytes=None, use_state=True):
    """gevws_inflate_carry_async behind cm.run_messages' tables, as
    it.run_inflate_ctx; carry_in / carry_src: numpy records and arena or None."""
    import torch
    t = got["dev"]
    dev = t["frames"].device
    nm = t["n_messages"]
    inf = torch.full((max(nm, 1) * 32,), FILL, dtype=torch.uint8, device=dev)
    out = torch.full((out_cap + 64,), FILL, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    st = t["state"] if use_state else None
    d_ext = None if ext is None else mm._dev(np.asarray(ext, np.uint8), dev, 1)
    d_cin = None if carry_in is None else mm._dev(carry_in, dev, 32)
    d_src = None
    if carry_src is not None:
        d_src = mm._dev(np.concatenate([carry_src, np.full(16, 0xBF, np.uint8)]), dev)
    nbytes = (0 if carry_src is None else carry_src.size) if carry_src_bytes is None else carry_src_bytes
    engine.inflate_carry_async(t["frames"], t["n_frames"], t["messages"], nm, t["msg_of"], t["summary"], t["payload"],
                               limit, st, inf, out, out_cap, summ, d_ext, ctx, n_conns, d_cin, d_src, nbytes)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0], inflated_raw=inf.cpu().numpy(),
                inflated=inf[: nm * 32].cpu().numpy().view(gm.INFLATED_DTYPE), out=out.cpu().numpy(),
                state=None if st is None else st.cpu().numpy()[: got["conn_msg"].shape[0] * 8].view(mm.MSG_STATE_DTYPE),
                dev=dict(inflated=inf, summary=summ, out=out))


def run_join_carry_ext(engine, t: dict, n_conns: int, max_message_bytes: int, flags: int, out_cap: int,
                       carry_cap: int, carry_in=None, carry_src=None, carry_src_bytes=None, inflated=None,
                       inflate_summary=None, out=None, carry_flags=KEEP_COMPRESSED):
    """cm.run_join_carry through gevws_join_carry_ext_async."""
    import torch
    dev = t["frames"].device
    nm = t["n_messages"]
    f = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    bodies, summ, csumm = f(max(nm, 1) * 32), f(64), f(64)
    if out is None:
        out = f(out_cap + GUARD)
    crec, cdst = f(max(n_conns, 1) * 32), f(carry_cap + GUARD)
    d_cin = None if carry_in is None else mm._dev(carry_in, dev, 32)
    src = np.zeros(0, np.uint8) if carry_src is None else carry_src
    d_src = mm._dev(np.concatenate([src, np.full(16, 0xBF, np.uint8)]), dev)  # (whole vectors are loaded)
    engine.join_carry_ext_async(t["frames"], t["n_frames"], t["messages"], nm, t["msg_of"], t["summary"],
                                t["payload"], inflated, inflate_summary, flags, bodies, out, out_cap, summ,
                                t["conn_msg"], n_conns, max_message_bytes, d_cin, d_src,
                                src.size if carry_src_bytes is None else carry_src_bytes, crec, cdst, carry_cap,
                                csumm, carry_flags)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0], bodies_raw=bodies.cpu().numpy(),
                bodies=bodies[: nm * 32].cpu().numpy().view(jm.BODY_DTYPE), out=out.cpu().numpy(),
                carry_summary=csumm.cpu().numpy().view(mm.SUMMARY_DTYPE)[0], carry_raw=crec.cpu().numpy(),
                carry=crec[: n_conns * 32].cpu().numpy().view(cm.CARRY_DTYPE), carry_dst=cdst.cpu().numpy())


def assert_invalid(inf: dict, count: int, tag="") -> None:
    """The call ended GEVWS_ERR_INVALID with `count`; nothing else written."""
    s = inf["summary"]
    assert (int(s["status"]), int(s["errors"])) == (jm.ERR_INVALID, count), (tag, s)
    assert (int(s["frames"]), int(s["payload_bytes"]), int(s["payload_len"])) == (0, 0, 0), tag
    assert np.all(inf["inflated_raw"] == FILL) and np.all(inf["out"] == FILL), (tag, "written by a call that failed")


# ---------------------------------------------------------------------------- the chain
def z(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    """One message's payload without context takeover."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]


def chain_model(passes, ext, limit, max_message_bytes, flags=jm.JOIN_ALL, carry_flags=KEEP_COMPRESSED, slots=None,
                start=None):
    """messages -> inflate(carry) -> join(carry) over `passes` (lists of
    connections): per pass dict(d, tables, inf, join, cin, csrc, state_in).
    slots: the takeover connections' it.Slot list (updated in place), or None.
    start: (state, carry records, carry arena) in front of the first pass."""
    n_conns = len(passes[0])
    state, cin, csrc = (None, np.zeros(n_conns, cm.CARRY_DTYPE), np.zeros(0, np.uint8)) if start is None else start
    res = []
    for conns in passes:
        d = mm.Decoded(conns, pad=0xFF)
        t = gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, state, ext)
        inf = model_inflate_carry(d, t, limit, t["state"], ext, slots, n_conns, cin, csrc)
        base = jm.round16(inf["payload_bytes"])
        isum = dict(payload_bytes=inf["payload_bytes"], status=0)
        need = carry_model_ext(d.frames, d.arena, t, n_conns, max_message_bytes, cin, csrc, flags, None, None,
                               inf["inflated"], isum, carry_flags=carry_flags)
        oc = int(need["summary"]["payload_bytes"])
        img = np.concatenate([inflate_image(inf, base), np.full(oc - base, FILL, np.uint8)])
        w = carry_model_ext(d.frames, d.arena, t, n_conns, max_message_bytes, cin, csrc, flags, oc, None,
                            inf["inflated"], isum, out_image=img, carry_flags=carry_flags)
        res.append(dict(d=d, tables=t, inf=inf, join=w, cin=cin, csrc=csrc, state_in=state))
        state, cin, csrc = inf["state"], w["carry"], w["carry_dst"]
    return res


def chain_device(engine, passes, ext, limit, max_message_bytes, flags=jm.JOIN_ALL, carry_flags=KEEP_COMPRESSED,
                 slots=None, tag="", start=None):
    """chain_model on the device, every pass compared with the models bit for
    bit; capacities are exactly the needs.  -> [(inflate, join, model entry)],
    and the device's slots (a tensor) when slots were given."""
    import torch
    n_conns = len(passes[0])
    ctx = None if slots is None else it.slots_to_device(slots, torch.device("cuda", engine.device))
    out = []
    state = None if start is None else start[0]
    for p, e in enumerate(chain_model(passes, ext, limit, max_message_bytes, flags, carry_flags, slots, start)):
        d, t, wi, w = e["d"], e["tables"], e["inf"], e["join"]
        got = cm.run_messages(engine, d, state, ext)
        mm.assert_tables_equal(got, t, f"{tag} pass {p}")
        ic = wi["payload_bytes"]
        inf = run_inflate_carry(engine, got, limit, ic, ext if slots is not None else None, ctx, n_conns, e["cin"],
                                e["csrc"])
        gm.assert_inflated(inf, wi, ic, f"{tag} pass {p}")
        dev = got["dev"]["frames"].device
        oc, cc = w["out"].size, w["carry_dst"].size
        base = jm.round16(ic)
        before = np.concatenate([inf["out"][:base], np.full(oc - base + GUARD, FILL, np.uint8)])
        g = run_join_carry_ext(engine, got["dev"], n_conns, max_message_bytes, flags, oc, cc, e["cin"], e["csrc"],
                               None, inf["dev"]["inflated"], inf["dev"]["summary"],
                               torch.from_numpy(before.copy()).to(dev), carry_flags)
        cm.assert_join_carry(g, w, oc, cc, f"{tag} pass {p}")
        out.append((inf, g, e))
        state = inf["state"]
    return (out, ctx) if slots is not None else out


# ---------------------------------------------------------------------------- random streams
def random_streams(rng, n_conns: int, takeover_every: int = 3):
    """(conns, ext, want): per connection a frame list of 1..4 whole messages,
    compressed (RSV1 on the first frame) and plain, fragmented, control frames in
    between; ext: EXT_DEFLATE everywhere, EXT_CLIENT_TAKEOVER on every
    takeover_every-th connection (its compressed messages come from one
    compressor); want: per connection the [(opcode, bytes)] sent."""
    words = [b"carry ", b"window ", b"pass ", b"fragment ", b"\xe2\x82\xac ", b"0123456789", b"\n"]
    conns, want = [], []
    ext = np.full(n_conns, it.EXT_DEFLATE, np.uint8)
    for c in range(n_conns):
        take = takeover_every and c % takeover_every == 0
        if take:
            ext[c] |= it.EXT_TAKEOVER
        co = zlib.compressobj(6, zlib.DEFLATED, -15) if take else None
        frs, sent = [], []
        for _ in range(int(rng.integers(1, 5))):
            kind = rng.random()
            n = int(rng.integers(0, 3000)) if rng.random() < 0.6 else int(rng.integers(0, 30))
            if kind < 0.3:      # incompressible: stored blocks
                data, op = bytes(rng.integers(0, 256, n, dtype=np.uint8)), 2
            else:               # text: fixed and dynamic blocks
                data = b"".join(words[int(i)] for i in rng.integers(0, len(words), n // 6))
                op = 1 if kind < 0.8 else 2
            compressed = rng.random() < 0.7
            if not compressed:
                wire = data
            elif take:
                wire = (co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH))[:-4]
            else:
                wire = z(data, int(rng.integers(0, 10)))
            k = int(rng.integers(1, 6))
            cuts = sorted(int(x) for x in rng.integers(0, len(wire) + 1, k - 1))
            edges = [0, *cuts, len(wire)]
            for i in range(k):
                frs.append((1 if i == k - 1 else 0, RSV1 if compressed and i == 0 else 0, op if i == 0 else 0,
                            wire[edges[i]: edges[i + 1]]))
                if i < k - 1 and rng.random() < 0.25:
                    frs.append((1, 0, 9 if rng.random() < 0.5 else 10,
                                bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8))))
            sent.append((op, data))
        conns.append(frs)
        want.append(sent)
    return conns, ext, want


def wire_len(frame) -> int:
    """A masked client frame's bytes on the wire."""
    n = len(frame[3])
    return 2 + (0 if n < 126 else 2 if n < 65536 else 8) + 4 + n


def byte_cuts(rng, conns, npass: int):
    """Per connection npass - 1 sorted frame indices from cuts at random BYTE
    positions of its wire stream: a pass holds the frames that are complete at
    its cut (a frame the cut falls into waits for the next pass)."""
    cuts = []
    for frs in conns:
        ends = np.cumsum([wire_len(f) for f in frs]) if frs else np.zeros(0, np.int64)
        total = int(ends[-1]) if len(frs) else 0
        pos = sorted(int(x) for x in rng.integers(0, total + 1, npass - 1))
        cuts.append([int(np.searchsorted(ends, p, side="right")) for p in pos])
    return cuts


def sequences(n_conns: int, results):
    """Per connection the (opcode, bytes) of every delivered body of the
    carry_model_ext results `results`, pass after pass."""
    return cm.sequences(n_conns, results)
