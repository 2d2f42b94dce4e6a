"""The permessage-deflate contract (gevws_messages_ext_async,
gevws_inflate_async; include/gevws.h) restated in plain Python on top of
tests/_messages_model.py, and the helpers that run both device steps on a
hand-built decoded batch.

Expected bytes of well-formed streams come from zlib; the Python model of
tests/_inflate_model.py gives the verdicts of small (malformed) streams."""
from __future__ import annotations

import zlib

import numpy as np

from tests import _inflate_model as im
from tests import _messages_model as mm

COMPRESSED = 4
EXT_DEFLATE = 1
INF_DONE, INF_PENDING = 1, 2
ERR_DEFLATE, ERR_TOO_BIG = 7, 8
INFLATED_DTYPE = np.dtype([("out_off", "<u8"), ("length", "<u8"), ("status", "u1"), ("flags", "u1"),
                           ("reserved", "u1", (14,))])
MODEL_MAX = 400  # streams up to this many bytes get their verdict from the Python model


def model_ext(frames, conn_out, n_decoded, arena, state=None, conn_ext=None):
    """mm.model with the RSV1 rules of a deflate connection: the tables
    gevws_messages_ext_async must produce."""
    n_conns = conn_out.shape[0]
    ext = np.zeros(n_conns, np.uint8) if conn_ext is None else conn_ext
    st_in = np.zeros(n_conns, mm.MSG_STATE_DTYPE) if state is None else state.copy()
    st_out = st_in.copy()
    msgs = []
    msg_of = np.full(max(n_decoded, 0), -1, np.int64)
    conn_msg = np.zeros(n_conns, mm.CONN_MSG_DTYPE)
    text_bytes = errors = 0
    for c in range(n_conns):
        first, nfr, status = int(conn_out["first_frame"][c]), int(conn_out["nframes"][c]), int(conn_out["status"][c])
        s = st_in[c]
        deflate = bool(int(ext[c]) & EXT_DEFLATE)
        conn_msg[c]["first_message"] = len(msgs)
        conn_msg[c]["error_frame"] = mm.NO_FRAME
        end = min(first + nfr, n_decoded)
        if n_decoded == 0 or status != 0 or end <= first or int(s["failed"]):
            conn_msg[c]["error"] = int(s["failed"]) if n_decoded else 0
            continue
        open_op = int(s["opcode"])
        comp = bool(deflate and open_op and int(s["reserved"][0]))
        utf = mm.Utf8(bytes(s["utf8"][: int(s["utf8_n"])])) if open_op == 1 and not comp else mm.Utf8()
        cur = None
        err, err_frame = mm.OK, mm.NO_FRAME
        for f in range(first, end):
            fin, rsv, op, L = (int(frames[k][f]) for k in ("fin", "rsv", "opcode", "length"))
            if (rsv & 3 or (rsv & 4 and (op & 8 or op == 0))) if deflate else rsv:
                err = mm.ERR_RSV
            elif 3 <= op <= 7 or op >= 0xB:
                err = mm.ERR_OPCODE
            elif op & 8 and (not fin or L > 125):
                err = mm.ERR_CONTROL
            elif op == 0 and not open_op:
                err = mm.ERR_CONTINUATION
            elif op in (1, 2) and open_op:
                err = mm.ERR_INTERLEAVE
            if err:
                err_frame = f
                break
            if op & 8:
                continue
            if op:
                open_op, comp = op, bool(rsv & 4)
                utf = mm.Utf8()
            if op or cur is None:
                cur = dict(first_frame=f, length=0, conn=c, nframes=0, opcode=open_op,
                           flags=(mm.BEGIN if op else 0) | (COMPRESSED if comp else 0), status=mm.OK)
            cur["length"] += L
            cur["nframes"] += 1
            msg_of[f] = len(msgs)
            if open_op == 1 and not comp:
                off = int(frames["payload_off"][f])
                text_bytes += L
                if not utf.feed(arena[off:off + L].tobytes()) or (fin and utf.need):
                    err, err_frame = mm.ERR_UTF8, f
                    cur["status"] = mm.ERR_UTF8
                    break
            if fin:
                cur["flags"] |= mm.END
                msgs.append(cur)
                cur, open_op = None, 0
        if cur is not None:
            msgs.append(cur)
        conn_msg[c]["nmessages"] = len(msgs) - int(conn_msg[c]["first_message"])
        conn_msg[c]["error"] = err
        conn_msg[c]["error_frame"] = err_frame
        st_out[c] = np.zeros((), mm.MSG_STATE_DTYPE)
        if err:
            errors += 1
            st_out[c]["failed"] = err
        else:
            st_out[c]["opcode"] = open_op
            if open_op and comp:
                st_out[c]["reserved"][0] = 1
            elif open_op == 1:
                st_out[c]["utf8_n"] = len(utf.pend)
                st_out[c]["utf8"][: len(utf.pend)] = list(utf.pend)
    out = np.zeros(len(msgs), mm.MESSAGE_DTYPE)
    for i, m in enumerate(msgs):
        for k, v in m.items():
            out[i][k] = v
    return dict(messages=out, msg_of=msg_of, conn_msg=conn_msg, state=st_out, frames=len(msgs),
                payload_len=text_bytes, errors=errors)


def expect_stream(payload: bytes, limit: int):
    """(status, bytes) of one compressed payload: zlib's bytes for a stream it
    inflates whole, the Python model's verdict for a small one."""
    if len(payload) <= MODEL_MAX:
        st, out = im.inflate(payload, limit)
        if st == im.OK:  # well-formed: zlib's bytes are the expectation
            z = zlib.decompressobj(-15).decompress(payload + im.TAIL)
            assert z == out
        return st, out
    d = zlib.decompressobj(-15)
    out = d.decompress(payload + im.TAIL, limit + 1)  # a larger stream here is one zlib's compressor made
    return (ERR_TOO_BIG, out[:limit]) if len(out) > limit else (im.OK, out)


def py_valid(b: bytes) -> bool:
    try:
        b.decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def model_inflate(d: mm.Decoded, tables: dict, limit: int, state=None):
    """What gevws_inflate_async must produce behind the message tables
    `tables` (model_ext's): dict(inflated, bytes (per message), state, frames,
    payload_bytes, payload_len, errors)."""
    msgs, msg_of = tables["messages"], tables["msg_of"]
    rec = np.zeros(msgs.shape[0], INFLATED_DTYPE)
    data = [b""] * msgs.shape[0]
    st_out = None if state is None else state.copy()
    off = ok = total = errors = 0
    failed_conns = set()
    for m in range(msgs.shape[0]):
        flags = int(msgs["flags"][m])
        if not flags & COMPRESSED:
            continue
        if flags & (mm.BEGIN | mm.END) != (mm.BEGIN | mm.END):
            rec[m]["flags"] = INF_PENDING
            continue
        fs = np.flatnonzero(msg_of == m)
        payload = b"".join(d.arena[int(d.frames["payload_off"][f]):][: int(d.frames["length"][f])].tobytes() for f in fs)
        st, out = expect_stream(payload, limit)
        if st == im.OK and int(msgs["opcode"][m]) == 1 and not py_valid(out):
            st = mm.ERR_UTF8
        keep = st in (im.OK, mm.ERR_UTF8)
        rec[m]["flags"], rec[m]["status"], rec[m]["out_off"] = INF_DONE, st, off
        if keep:
            rec[m]["length"], data[m] = len(out), out
            off += (len(out) + 15) // 16 * 16
            total += len(out)
        if st == im.OK:
            ok += 1
        else:
            errors += 1
            c = int(msgs["conn"][m])
            if c not in failed_conns and st_out is not None and int(st_out[c]["failed"]) == 0:
                st_out[c]["failed"] = st
            failed_conns.add(c)
    return dict(inflated=rec, bytes=data, state=st_out, frames=ok, payload_bytes=off, payload_len=total,
                errors=errors)


# ---------------------------------------------------------------------------- device runs
def run_messages_ext(engine, d: mm.Decoded, conn_ext=None, state=None, keep_state=True):
    """gevws_messages_ext_async on a hand-built batch: the host copies of its
    tables (as mm.run_device) plus the device tensors under "dev"."""
    import torch
    dev = torch.device("cuda", engine.device)
    n_frames, n_conns = d.frames.shape[0], d.conn_out.shape[0]
    fr, co, sm = mm._dev(d.frames, dev, 32), mm._dev(d.conn_out, dev, 32), mm._dev(d.summary, dev, 64)
    pay = mm._dev(d.arena, dev)
    st = None
    if keep_state:
        st = mm._dev(np.zeros(n_conns, mm.MSG_STATE_DTYPE) if state is None else state, dev, 8)
    ext = None if conn_ext is None else mm._dev(np.asarray(conn_ext, np.uint8), dev, 1)
    msgs = torch.full((max(n_frames, 1) * 32,), 0xEE, dtype=torch.uint8, device=dev)
    msg_of = torch.full((max(n_frames, 1),), 7777, dtype=torch.int64, device=dev)
    cm = torch.full((max(n_conns, 1) * 32,), 0xEE, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    engine.messages_ext_async(fr, n_frames, co, n_conns, sm, pay, st, msgs, n_frames, msg_of, cm, summ, ext)
    torch.cuda.synchronize(engine.device)
    s = summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0]
    nm = min(int(s["frames"]), n_frames)
    return dict(summary=s, messages=msgs[: nm * 32].cpu().numpy().view(mm.MESSAGE_DTYPE),
                msg_of=msg_of[:n_frames].cpu().numpy(),
                conn_msg=cm[: n_conns * 32].cpu().numpy().view(mm.CONN_MSG_DTYPE),
                state=st[: n_conns * 8].cpu().numpy().view(mm.MSG_STATE_DTYPE) if st is not None else None,
                dev=dict(frames=fr, payload=pay, messages=msgs, msg_of=msg_of, summary=summ, state=st,
                         n_frames=n_frames, n_messages=nm))


def run_inflate(engine, got: dict, limit: int, out_cap: int, use_state=True):
    """gevws_inflate_async behind run_messages_ext's tables: host copies of
    d_inflated, the whole of d_out (prefilled 0xEE, 64 guard bytes behind
    out_cap), the summary and the state."""
    import torch
    t = got["dev"]
    dev = t["frames"].device
    nm = t["n_messages"]
    inf = torch.full((max(nm, 1) * 32,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.full((out_cap + 64,), 0xEE, dtype=torch.uint8, device=dev)
    summ = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    st = t["state"] if use_state else None
    engine.inflate_async(t["frames"], t["n_frames"], t["messages"], nm, t["msg_of"], t["summary"], t["payload"],
                         limit, st, inf, out, out_cap, summ)
    torch.cuda.synchronize(engine.device)
    return dict(summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0],
                inflated=inf[: nm * 32].cpu().numpy().view(INFLATED_DTYPE), out=out.cpu().numpy(),
                state=None if st is None else st.cpu().numpy()[: got["conn_msg"].shape[0] * 8].view(mm.MSG_STATE_DTYPE))


def assert_inflated(got: dict, want: dict, out_cap: int, tag="") -> None:
    """The device's records, bytes, summary and state == the model's; d_out
    untouched outside the messages' 16-byte-rounded ranges."""
    s = got["summary"]
    assert int(s["status"]) == 0, tag
    assert (int(s["frames"]), int(s["payload_bytes"]), int(s["payload_len"]), int(s["errors"])) == \
        (want["frames"], want["payload_bytes"], want["payload_len"], want["errors"]), tag
    gi, wi = got["inflated"], want["inflated"]
    for k in ("flags", "status", "length"):
        bad = np.flatnonzero(gi[k] != wi[k])
        assert bad.size == 0, (tag, k, bad[:8], gi[k][bad[:8]], wi[k][bad[:8]])
    assert not gi["reserved"].any(), tag
    done = wi["flags"] == INF_DONE
    assert np.array_equal(gi["out_off"][done], wi["out_off"][done]), tag
    assert np.all(gi["out_off"][~done] == 0), tag
    out = got["out"]
    used = np.zeros(out.size, bool)
    for m in np.flatnonzero(wi["length"] > 0):
        off, n = int(wi["out_off"][m]), int(wi["length"][m])
        assert out[off:off + n].tobytes() == want["bytes"][m], (tag, m)
        pad = (n + 15) // 16 * 16
        assert not out[off + n: off + pad].any(), (tag, m, "pad not zeroed")
        used[off: off + pad] = True
    assert used.sum() == want["payload_bytes"] <= out_cap, tag
    assert np.all(out[~used] == 0xEE), (tag, "d_out written outside the messages' ranges")
    if want["state"] is not None and got["state"] is not None:
        assert got["state"].tobytes() == want["state"].tobytes(), tag
