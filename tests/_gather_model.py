"""The gather's contract (gevws_send_gather_async; include/gevws.h) restated in
plain numpy, and the helpers that run the device step on hand-built send lists.

The model is pinned on the CPU (tests/test_gather_model.py) by hand-derived
cases and against the concatenation rule of gev_amd.Responses.conn_bytes; the
GPU tests compare every output of the device with it, byte for byte, the bytes
behind the used part of the buffer included."""
from __future__ import annotations

import numpy as np

from tests import _join_model as jm
from tests import _messages_model as mm
from tests import _respond_model as rm

FILL = jm.FILL
ERR_CAPACITY, ERR_INVALID = rm.ERR_CAPACITY, rm.ERR_INVALID
SEND_DTYPE, CONN_SEND_DTYPE = rm.SEND_DTYPE, rm.CONN_SEND_DTYPE
CONN_BUF_DTYPE = np.dtype([("off", "<u8"), ("bytes", "<u8"), ("flags", "<u4"), ("reserved", "<u4", (3,))])
U64 = 1 << 64
GUARD_BYTES = 256  # FILL bytes behind buf_cap that must stay FILL


def round16(x: int) -> int:
    return (x + 15) // 16 * 16


def gather_model(send, conn_send, wires, wire_bytes, buf_cap, plan_status=0, plan_frames=None):
    """What gevws_send_gather_async must produce: dict(buf, conn_buf, summary).
    send: SEND_DTYPE [max_sends], conn_send: CONN_SEND_DTYPE [n_conns], wires:
    three uint8 arrays, wire_bytes: their readable bytes, plan_frames: the
    plan summary's `frames` (None: every record of `send`).  buf is the image
    of d_buf[0, payload_bytes), pads included; buf and conn_buf are None where
    nothing may be written."""
    max_sends, n_conns = send.shape[0], conn_send.shape[0]
    n = min(max_sends if plan_frames is None else plan_frames, max_sends) if plan_status == 0 else 0
    nothing = dict(buf=None, conn_buf=None, summary=rm.zero_summary())
    if n == 0 or n_conns == 0:
        return nothing
    first = [int(x) for x in conn_send["first"]]
    count = [int(x) for x in conn_send["count"]]
    nbytes = [int(x) for x in conn_send["bytes"]]
    bad = 0
    acc = [0] * n_conns
    ok = [False] * n
    for k in range(n):
        e = send[k]
        off, ln, c, w = int(e["off"]), int(e["len"]), int(e["conn"]), int(e["wire"])
        if w > 2 or c >= n_conns or off > int(wire_bytes[w]) or ln > int(wire_bytes[w]) - off:
            bad += 1
        elif k < first[c] or k - first[c] >= count[c]:
            bad += 1
        else:
            ok[k] = True
            acc[c] += ln
    for c in range(n_conns):
        wrong = first[c] > n or count[c] > n - first[c]
        if c:
            wrong |= first[c] < min(first[c - 1] + count[c - 1], U64 - 1)
        wrong |= nbytes[c] != acc[c]
        bad += bool(wrong)
    if bad:
        return dict(nothing, summary=dict(rm.zero_summary(), errors=bad, status=ERR_INVALID))
    total = sum(round16(b) for b in nbytes)
    summary = dict(frames=n, payload_bytes=total, payload_len=sum(nbytes), errors=0, status=0)
    if total > buf_cap:
        return dict(nothing, summary=dict(summary, status=ERR_CAPACITY))
    buf = np.zeros(total, np.uint8)
    conn_buf = np.zeros(n_conns, CONN_BUF_DTYPE)
    at = 0
    for c in range(n_conns):
        conn_buf[c]["off"], conn_buf[c]["bytes"], conn_buf[c]["flags"] = at, nbytes[c], conn_send["flags"][c]
        p = at
        for e in send[first[c]: first[c] + count[c]]:
            off, ln = int(e["off"]), int(e["len"])
            buf[p: p + ln] = wires[int(e["wire"])][off: off + ln]
            p += ln
        assert p == at + nbytes[c]
        at += round16(nbytes[c])
    return dict(buf=buf, conn_buf=conn_buf, summary=summary)


def make_lists(conns, n_conns=None, flags=None):
    """(send, conn_send) from [[(wire, off, len), ..] per connection], the way
    the plan writes them: entries in connection order, `frame` the entry's index."""
    n_conns = len(conns) if n_conns is None else n_conns
    send = np.zeros(sum(len(c) for c in conns), SEND_DTYPE)
    conn_send = np.zeros(n_conns, CONN_SEND_DTYPE)
    k = 0
    for c, ents in enumerate(conns):
        conn_send[c] = (k, len(ents), sum(e[2] for e in ents), 0 if flags is None else flags[c], 0)
        for w, off, ln in ents:
            send[k] = (off, ln, k, c, w)
            k += 1
    for c in range(len(conns), n_conns):
        conn_send[c]["first"] = k
    return send, conn_send


def run_gather(engine, send, conn_send, wires, wire_bytes, buf_cap, plan_status=0, plan_frames=None, pinned=None):
    """gevws_send_gather_async on host tables: host copies of everything it may
    write, prefilled with FILL -- the buffer with GUARD_BYTES more behind
    buf_cap.  Every wire gets the encodes' 16 bytes of slack behind its
    (16-rounded) bytes.  pinned: a gev_amd.PinnedArena to gather into."""
    import torch
    dev = torch.device("cuda", engine.device)
    max_sends, n_conns = send.shape[0], conn_send.shape[0]
    f = lambda nbytes: torch.full((max(nbytes, 16),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    dw = []
    for w, nb in zip(wires, wire_bytes):
        t = torch.full((round16(max(int(nb), w.size)) + 16,), 0xA5, dtype=torch.uint8, device=dev)
        if w.size:
            t[: w.size] = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
        dw.append(t)
    plan = rm.summary_np(frames=max_sends if plan_frames is None else plan_frames, status=plan_status)
    cb, summ = f(n_conns * 32), f(64)
    if pinned is None:
        buf = f(buf_cap + GUARD_BYTES)
    else:
        assert pinned.nbytes >= buf_cap + GUARD_BYTES
        pinned.host[:] = FILL
        buf = pinned.at(0)
    engine.send_gather_async(mm._dev(send, dev, 32), max_sends, mm._dev(conn_send, dev, 32), n_conns,
                             mm._dev(plan, dev, 64), dw, [int(x) for x in wire_bytes], buf, buf_cap, cb, summ)
    torch.cuda.synchronize(engine.device)
    host = buf.cpu().numpy() if pinned is None else pinned.host[: buf_cap + GUARD_BYTES].copy()
    return dict(buf=host, conn_buf=cb.cpu().numpy(), summary=summ.cpu().numpy().view(mm.SUMMARY_DTYPE)[0])


def assert_gather(got: dict, want: dict, tag="") -> None:
    """Every output of the device == the model's, untouched bytes included."""
    s = got["summary"]
    assert jm.summary_tuple(s) == tuple(want["summary"][k] for k in ("frames", "payload_bytes", "payload_len", "errors",
                                                                     "status")), (tag, jm.summary_tuple(s), want["summary"])
    assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), tag
    if want["buf"] is None:
        assert np.all(got["buf"] == FILL) and np.all(got["conn_buf"] == FILL), (tag, "written by a call that failed")
        return
    used = want["buf"].size
    diff = np.flatnonzero(got["buf"][:used] != want["buf"])
    assert diff.size == 0, (tag, "send buffer differs from the model at", diff[:8], "of", used)
    past = np.flatnonzero(got["buf"][used:] != FILL)
    assert past.size == 0, (tag, "written past payload_bytes at", past[:8] + used)
    w = np.ascontiguousarray(want["conn_buf"]).view(np.uint8).reshape(-1)
    assert got["conn_buf"][: w.size].tobytes() == w.tobytes(), (tag, "conn_buf differs",
                                                                got["conn_buf"][: w.size].view(CONN_BUF_DTYPE),
                                                                want["conn_buf"])
    assert np.all(got["conn_buf"][w.size:] == FILL), (tag, "conn_buf written past the table")
