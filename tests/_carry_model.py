"""The carry half of the join step (gevws_join_carry_async, include/gevws.h)
restated in plain Python over the tables of tests/_messages_model.py: the
bodies and d_out as tests/_join_model.py has them, plus a continued message's
carried prefix, the per-connection carry records and the d_carry_dst image.

The model is pinned on the CPU by hand-derived cases and by the cut-invariance
property (tests/test_carry_model.py); the GPU tests compare every output of
the device with it, byte for byte."""
from __future__ import annotations

import numpy as np

from tests import _join_model as jm
from tests import _messages_model as mm

OPEN, LOST = 1, 2
ERR_TOO_BIG = 8
FILL, GUARD = jm.FILL, jm.GUARD
CARRY_DTYPE = np.dtype([("off", "<u8"), ("length", "<u8"), ("opcode", "u1"), ("flags", "u1"), ("status", "u1"),
                        ("reserved", "u1", (13,))])
_KEYS = ("frames", "payload_bytes", "payload_len", "errors", "status")


def _status_only(st):
    return dict(jm.zero_summary(), status=st)


def carry_model(frames, arena, tables, n_conns, max_message_bytes, carry_in=None, carry_src=None, flags=0,
                out_cap=None, carry_cap=None, inflated=None, inflate_summary=None, msg_status=0, out_image=None,
                carry_src_bytes=None):
    """What gevws_join_carry_async must produce: dict(bodies, out, summary,
    base, carry, carry_dst, carry_summary).  tables: the message pass's
    (messages, msg_of, conn_msg); carry_in / carry_src: the previous pass's
    records (CARRY_DTYPE) and arena, or None.  bodies / carry are None where
    the call may write neither; `out` / `carry_dst` are whole images over FILL.
    out_cap / carry_cap None: exactly the need."""
    messages, msg_of, conn_msg = tables["messages"], tables["msg_of"], tables["conn_msg"]
    cin = np.zeros(n_conns, CARRY_DTYPE) if carry_in is None else carry_in
    src = np.zeros(0, np.uint8) if carry_src is None else carry_src
    src_bytes = src.size if carry_src_bytes is None else carry_src_bytes

    def image(cap, img=None):
        return np.full(cap, FILL, np.uint8) if img is None else img[:cap].copy()

    def nothing(s_body, s_carry):
        return dict(bodies=None, out=image(out_cap or 0, out_image), summary=s_body, base=0, carry=None,
                    carry_dst=image(carry_cap or 0), carry_summary=s_carry)

    if n_conns == 0:
        return nothing(jm.zero_summary(), jm.zero_summary())
    if msg_status != 0:
        return nothing(_status_only(msg_status), _status_only(msg_status))
    if inflate_summary is not None and inflate_summary["status"] != 0:
        return nothing(_status_only(inflate_summary["status"]), _status_only(inflate_summary["status"]))
    n = messages.shape[0]
    # malformed input, before anything is indexed by it
    bad = int(np.count_nonzero(messages["conn"] >= n_conns))
    for c in range(n_conns):
        r = cin[c]
        if int(r["flags"]) & OPEN and (int(r["off"]) % 16 or int(r["off"]) + int(r["length"]) > src_bytes):
            bad += 1
        elif int(conn_msg["first_message"][c]) + int(conn_msg["nmessages"][c]) > n:
            bad += 1
    if bad:
        s = dict(jm.zero_summary(), errors=bad, status=jm.ERR_INVALID)
        return nothing(s, dict(s))

    by_msg = {}
    for f in np.flatnonzero(msg_of >= 0):
        by_msg.setdefault(int(msg_of[f]), []).append(int(f))

    def data_of(m):
        return b"".join(arena[int(frames["payload_off"][f]):][: int(frames["length"][f])].tobytes()
                        for f in by_msg.get(m, []))

    def carried(c):
        return src[int(cin["off"][c]): int(cin["off"][c]) + int(cin["length"][c])].tobytes()

    # ---- the body side
    bodies = np.zeros(n, jm.BODY_DTYPE)
    base = jm.round16(int(inflate_summary["payload_bytes"])) if n and inflate_summary is not None else 0
    cur, delivered, total, too_big = base, 0, 0, 0
    copies = []
    for m in range(n):
        r, b = messages[m], bodies[m]
        b["conn"], b["opcode"], b["status"] = r["conn"], r["opcode"], r["status"]
        mflags, c = int(r["flags"]), int(r["conn"])
        ok_end = mflags & mm.END and int(r["status"]) == mm.OK
        if mflags & jm.COMPRESSED:
            if inflated is None:
                continue
            b["status"] = inflated["status"][m]
            if mflags & mm.BEGIN and ok_end and int(inflated["flags"][m]) & jm.INF_DONE and \
                    int(inflated["status"][m]) == mm.OK:
                b["flags"], b["off"], b["length"] = jm.WHOLE | jm.INFLATED, inflated["out_off"][m], inflated["length"][m]
                delivered, total = delivered + 1, total + int(inflated["length"][m])
            continue
        data = None
        if mflags & mm.BEGIN:
            if ok_end and (int(r["nframes"]) >= 2 or flags & jm.JOIN_ALL):
                data = data_of(m)
            elif ok_end:
                delivered, total = delivered + 1, total + int(r["length"])
                b["flags"], b["length"] = jm.WHOLE, r["length"]
                b["off"] = frames["payload_off"][int(r["first_frame"])]
        elif int(cin["flags"][c]) & OPEN:
            if ok_end and int(cin["length"][c]) + int(r["length"]) <= max_message_bytes:
                data = carried(c) + data_of(m)
            elif ok_end:
                b["status"] = ERR_TOO_BIG
                too_big += 1
        elif int(cin["flags"][c]) & LOST and int(cin["status"][c]):
            b["status"] = cin["status"][c]
        if data is not None:
            delivered, total = delivered + 1, total + len(data)
            b["flags"], b["off"], b["length"] = jm.WHOLE | jm.JOINED, cur, len(data)
            copies.append((cur, data))
            cur += jm.round16(len(data))
    summary = dict(frames=delivered, payload_bytes=cur, payload_len=total, errors=0, status=0) if n else \
        jm.zero_summary()

    # ---- the carry side
    carry = np.zeros(n_conns, CARRY_DTYPE)
    ccur, nopen, clen = 0, 0, 0
    ccopies = []
    for c in range(n_conns):
        cm, ci, o = conn_msg[c], cin[c], carry[c]
        if int(cm["error"]) != 0:
            continue
        nm = int(cm["nmessages"])
        data, lost = None, None   # lost: the status of a LOST record
        if nm == 0:
            op = int(ci["opcode"])
            if int(ci["flags"]) & OPEN:
                data = carried(c)
            elif int(ci["flags"]) & LOST:
                lost = int(ci["status"])
        else:
            last = int(cm["first_message"]) + nm - 1
            r = messages[last]
            mflags, op = int(r["flags"]), int(r["opcode"])
            if mflags & mm.END:
                continue
            if mflags & jm.COMPRESSED:
                lost = int(ci["status"]) if not mflags & mm.BEGIN and int(ci["flags"]) & LOST else 0
            elif mflags & mm.BEGIN:
                data = data_of(last)
            elif int(ci["flags"]) & OPEN:
                data = carried(c) + data_of(last)
            else:
                lost = int(ci["status"]) if int(ci["flags"]) & LOST else 0
        if data is not None and len(data) > max_message_bytes:
            data, lost = None, ERR_TOO_BIG
            too_big += 1
        if data is not None:
            o["off"], o["length"], o["opcode"], o["flags"] = ccur, len(data), op, OPEN
            ccopies.append((ccur, data))
            ccur += jm.round16(len(data))
            nopen, clen = nopen + 1, clen + len(data)
        elif lost is not None:
            o["opcode"], o["flags"], o["status"] = op, LOST, lost
    carry_summary = dict(frames=nopen, payload_bytes=ccur, payload_len=clen, errors=too_big, status=0)

    out_cap = cur if out_cap is None else out_cap
    carry_cap = ccur if carry_cap is None else carry_cap
    out, dst = image(out_cap, out_image), image(carry_cap)
    if cur > out_cap or ccur > carry_cap:
        if cur > out_cap:
            summary["status"] = jm.ERR_CAPACITY
        if ccur > carry_cap:
            carry_summary["status"] = jm.ERR_CAPACITY
        return dict(bodies=None, out=out, summary=summary, base=base, carry=None, carry_dst=dst,
                    carry_summary=carry_summary)
    for img, cs in ((out, copies), (dst, ccopies)):
        for off, data in cs:
            img[off: off + len(data)] = np.frombuffer(data, np.uint8)
            img[off + len(data): off + jm.round16(len(data))] = 0
    return dict(bodies=bodies, out=out, summary=summary, base=base, carry=carry, carry_dst=dst,
                carry_summary=carry_summary)


def delivered(res, conn_payload=None):
    """[(conn, opcode, bytes)] of the delivered bodies of one carry_model result
    (every delivered plain body JOINED: a call with JOIN_ALL)."""
    out = []
    for b in res["bodies"]:
        if int(b["flags"]) & jm.WHOLE:
            assert int(b["flags"]) & (jm.JOINED | jm.INFLATED)
            off, n = int(b["off"]), int(b["length"])
            out.append((int(b["conn"]), int(b["opcode"]), res["out"][off: off + n].tobytes()))
    return out


def split_passes(conns, cuts):
    """conns: per connection a frame list; cuts: per connection the sorted frame
    indices at which a new pass starts.  -> a list of passes, each a list of
    connections (frame lists, possibly empty)."""
    npass = max(len(c) for c in cuts) + 1
    passes = []
    for p in range(npass):
        batch = []
        for frs, cs in zip(conns, cuts):
            edges = [0, *cs, len(frs)] + [len(frs)] * (npass - len(cs) - 1)
            batch.append(frs[edges[p]: edges[p + 1]])
        passes.append(batch)
    return passes


def chain_model(passes, max_message_bytes, flags=jm.JOIN_ALL, model=None):
    """The message model and the carry model chained over `passes` (lists of
    connections): [(Decoded, tables, carry_model result)] per pass.  model: the
    message pass's model as f(Decoded, state) (default: the plain one)."""
    n_conns = len(passes[0])
    state, cin, csrc = None, None, None
    res = []
    for conns in passes:
        d = mm.Decoded(conns)
        t = d.model(state) if model is None else model(d, state)
        w = carry_model(d.frames, d.arena, t, n_conns, max_message_bytes, cin, csrc, flags)
        res.append((d, t, w, cin, csrc))
        state, cin, csrc = t["state"], w["carry"], w["carry_dst"]
    return res


def random_streams(rng, n_conns, budget, text=False):
    """Per connection a stream of whole messages as frames (fin, rsv, opcode,
    payload), `budget` payload bytes in all at the most; control frames between
    fragments.  text: opcode 1, multi-byte characters cut across frames."""
    alphabet = "aZ09 éßЖ中€\U0001f600\U00010348"
    conns = []
    per = budget // n_conns
    for c in range(n_conns):
        left, frs = per, []
        for _ in range(int(rng.integers(1, 5))):
            total = int(rng.integers(0, min(left, 6000) + 1)) if rng.random() < 0.7 else int(rng.integers(0, 40))
            total = min(total, left)
            if text:
                data = b""
                for i in rng.integers(0, len(alphabet), total):
                    e = alphabet[int(i)].encode()
                    if len(data) + len(e) > total:
                        break
                    data += e
            else:
                data = bytes(rng.integers(0, 256, total, dtype=np.uint8))
            left -= len(data)
            k = int(rng.integers(1, 7))
            cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, k - 1))
            edges = [0, *cuts, len(data)]
            for i in range(k):
                frs.append((1 if i == k - 1 else 0, 0, (1 if text else 2) if i == 0 else 0,
                            data[edges[i]: edges[i + 1]]))
                if i < k - 1 and rng.random() < 0.2:
                    frs.append((1, 0, 9 if rng.random() < 0.5 else 10, bytes(rng.integers(0, 256, int(rng.integers(0, 20)),
                                                                                          dtype=np.uint8))))
        conns.append(frs)
    return conns


def random_cuts(rng, conns, npass):
    """Per connection npass - 1 sorted frame indices (duplicates: an idle pass)."""
    return [sorted(int(x) for x in rng.integers(0, len(frs) + 1, npass - 1)) for frs in conns]


def sequences(n_conns, results):
    """Per connection the (opcode, bytes) of every delivered body, pass after pass."""
    seq = [[] for _ in range(n_conns)]
    for res in results:
        for c, op, data in delivered(res):
            seq[c].append((op, data))
    return seq


# ---------------------------------------------------------------------------- device runs
def run_messages(engine, d: mm.Decoded, state=None, conn_ext=None):
    """gevws_messages_ext_async on a hand-built batch, every table kept on the
    device (conn_msg too): dict(summary, messages, msg_of, conn_msg, state, dev)."""
    import torch
    dev = torch.device("cuda", engine.device)
    n_frames, n_conns = d.frames.shape[0], d.conn_out.shape[0]
    fr, co, sm = mm._dev(d.frames, dev, 32), mm._dev(d.conn_out, dev, 32), mm._dev(d.summary, dev, 64)
    pay = mm._dev(d.arena, dev)
    st = mm._dev(np.zeros(n_conns, mm.MSG_STATE_DTYPE) if state is None else state, dev, 8)
    ext = None if conn_ext is None else mm._dev(np.asarray(conn_ext, np.uint8), dev, 1)
    msgs = torch.full((max(n_frames, 1) * 32,), FILL, dtype=torch.uint8, device=dev)
    msg_of = torch.full((max(n_frames, 1),), 7777, dtype=torch.int64, device=dev)
    cm = torch.full((max(n_conns, 1) * 32,), FILL, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    engine.messages_ext_async(fr, n_frames, co, n_conns, sm, pay, st, msgs, n_frames, msg_of, cm, summ, ext)
    torch.cuda.synchronize(engine.device)
    s = summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0]
    nm = min(int(s["frames"]), n_frames) if int(s["status"]) == 0 else 0
    return dict(summary=s, messages=msgs[: nm * 32].cpu().numpy().view(mm.MESSAGE_DTYPE),
                msg_of=msg_of[:n_frames].cpu().numpy(),
                conn_msg=cm[: n_conns * 32].cpu().numpy().view(mm.CONN_MSG_DTYPE),
                state=st[: n_conns * 8].cpu().numpy().view(mm.MSG_STATE_DTYPE),
                dev=dict(frames=fr, payload=pay, messages=msgs, msg_of=msg_of, summary=summ, state=st, conn_msg=cm,
                         n_frames=n_frames, n_messages=nm, n_conns=n_conns))


def run_join_carry(engine, t: dict, n_conns: int, max_message_bytes: int, flags: int, out_cap: int, carry_cap: int,
                   carry_in=None, carry_src=None, carry_src_bytes=None, inflated=None, inflate_summary=None, out=None):
    """gevws_join_carry_async behind a message pass's device tensors (the "dev"
    entry of run_messages).  carry_in / carry_src: numpy records and arena of
    the previous pass, or None.  Host copies of all four outputs (each prefilled
    FILL, GUARD bytes behind each capacity) and both summaries."""
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
    engine.join_carry_async(t["frames"], t["n_frames"], t["messages"], nm, t["msg_of"], t["summary"], t["payload"],
                            inflated, inflate_summary, flags, bodies, out, out_cap, summ, t["conn_msg"], n_conns,
                            max_message_bytes, d_cin, d_src, src.size if carry_src_bytes is None else carry_src_bytes,
                            crec, cdst, carry_cap, csumm)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0], bodies_raw=bodies.cpu().numpy(),
                bodies=bodies[: nm * 32].cpu().numpy().view(jm.BODY_DTYPE), out=out.cpu().numpy(),
                carry_summary=csumm.cpu().numpy().view(mm.SUMMARY_DTYPE)[0], carry_raw=crec.cpu().numpy(),
                carry=crec[: n_conns * 32].cpu().numpy().view(CARRY_DTYPE), carry_dst=cdst.cpu().numpy(),
                dev=dict(bodies=bodies, out=out, summary=summ, n_messages=nm, carry=crec, carry_dst=cdst,
                         carry_summary=csumm))


def assert_join_carry(got: dict, want: dict, out_cap: int, carry_cap: int, tag="") -> None:
    """Every output of the device == the model's: the body half through
    jm.assert_join, then the carry records, the whole of d_carry_dst and the
    carry summary."""
    jm.assert_join(got, want, out_cap, tag)
    s = got["carry_summary"]
    assert jm.summary_tuple(s) == tuple(want["carry_summary"][k] for k in _KEYS), \
        (tag, "carry summary", jm.summary_tuple(s), want["carry_summary"])
    assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), tag
    dst = got["carry_dst"]
    assert np.all(dst[carry_cap:] == FILL), (tag, "written past carry_cap")
    bad = np.flatnonzero(dst[:carry_cap] != want["carry_dst"])
    assert bad.size == 0, (tag, "d_carry_dst differs at", bad[:8], dst[bad[:8]], want["carry_dst"][bad[:8]])
    if want["carry"] is None:
        assert np.all(got["carry_raw"] == FILL), (tag, "d_carry_out written by a call that failed")
        return
    gc, wc = got["carry"], want["carry"]
    assert gc.shape == wc.shape, tag
    for k in CARRY_DTYPE.names:
        bad = np.flatnonzero((gc[k] != wc[k]).reshape(gc.shape[0], -1).any(axis=1))
        assert bad.size == 0, (tag, "carry", k, bad[:8], gc[k][bad[:8]], wc[k][bad[:8]])
    assert np.all(got["carry_raw"][gc.shape[0] * 32:] == FILL), tag


def chain_device(engine, passes, max_message_bytes, flags=jm.JOIN_ALL, conn_ext=None, model=None, tag=""):
    """Every pass of `passes` through the device message pass and
    gevws_join_carry_async, state and carry handed from pass to pass, each pass
    compared with the models; capacities are exactly the needs.  -> the list of
    (device result, model result)."""
    res = []
    state = None
    for p, (d, t, w, cin, csrc) in enumerate(chain_model(passes, max_message_bytes, flags, model)):
        got = run_messages(engine, d, state, conn_ext)
        mm.assert_tables_equal(got, t, f"{tag} pass {p}")
        oc, cc = w["out"].size, w["carry_dst"].size
        g = run_join_carry(engine, got["dev"], len(passes[0]), max_message_bytes, flags, oc, cc, cin, csrc)
        assert_join_carry(g, w, oc, cc, f"{tag} pass {p}")
        res.append((g, w))
        state = got["state"]
    return res
