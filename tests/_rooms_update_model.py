"""gevws_rooms_update_async's contract (include/gevws.h) restated in plain
Python: the changes applied in list order, the closes, then Rooms.csr of the
result -- and the helper that runs the device call on host arrays with every
output prefilled with 0xEE.

The model is pinned on the CPU (tests/test_rooms_update_model.py); the GPU tests
compare the three outputs and the summary of the device with it, bit for bit."""
from __future__ import annotations

import numpy as np

import gev_amd
from tests import _messages_model as mm
from tests import _rooms_model as ro

ROOM_NONE = ro.ROOM_NONE
ERR_INVALID = ro.ERR_INVALID
FILL = ro.FILL
CTL_SHUTDOWN, CTL_FAILED = 1, 2
CHANGE_DTYPE = np.dtype([("conn", "<u4"), ("room", "<u4")])


def changes_np(pairs) -> np.ndarray:
    """(conn, room) pairs as gevws_room_change records."""
    a = np.zeros(len(pairs), CHANGE_DTYPE)
    for k, (c, g) in enumerate(pairs):
        a[k] = (c, g)
    return a


def count_of(changes, max_changes=None, prev=None) -> int:
    """The changes a call reads: max_changes (None: all of them), cut to the
    gate's frames."""
    if changes is None:
        return 0
    n = len(changes) if max_changes is None else max_changes
    if prev is not None:
        n = min(n, int(prev["frames"]))
    return n


def update_model(conn_room, n_rooms, changes=None, max_changes=None, prev=None, conn_flags=None, plan=None):
    """What the call must produce: dict(conn_room, first, members, summary);
    the tables are None where nothing may be written.  prev / plan: the gates'
    summaries as dicts with `status` (and `frames` for prev), or None;
    conn_flags: d_conn_send's flags per connection, or None."""
    cr = np.asarray(conn_room, np.uint32).reshape(-1)
    nothing = dict(conn_room=None, first=None, members=None)
    for gate in (prev, plan):
        if gate is not None and int(gate["status"]) != 0:
            return dict(nothing, summary=dict(ro.zero_summary(), status=int(gate["status"])))
    n = count_of(changes, max_changes, prev)
    ok_room = lambda g: g < n_rooms or g == ROOM_NONE  # noqa: E731
    bad = sum(1 for g in cr.tolist() if not ok_room(g))
    new = cr.copy()
    for k in range(n):
        c, g = int(changes[k]["conn"]), int(changes[k]["room"])
        if c >= cr.size or not ok_room(g):
            bad += 1
            continue
        new[c] = g
    if conn_flags is not None:
        new[(np.asarray(conn_flags, np.uint32)[: cr.size] & CTL_SHUTDOWN) != 0] = ROOM_NONE
    if bad:
        return dict(nothing, summary=dict(ro.zero_summary(), errors=bad, status=ERR_INVALID))
    first, members, _ = gev_amd.Rooms.csr(new, n_rooms)
    summary = dict(ro.zero_summary(), frames=int(members.size), payload_len=int(np.count_nonzero(new != cr)),
                   payload_bytes=n)
    return dict(conn_room=new, first=first, members=members, summary=summary)


# ---------------------------------------------------------------------------- device runs
def conn_send_np(conn_flags) -> np.ndarray:
    cs = np.zeros(len(conn_flags), gev_amd.CONN_SEND_DTYPE)
    cs["flags"] = conn_flags
    cs["first"], cs["count"], cs["bytes"] = 7, 3, 99   # (the call reads the flags alone)
    return cs


def summary_np(frames=0, status=0) -> np.ndarray:
    s = np.zeros(1, mm.SUMMARY_DTYPE)
    s["frames"], s["status"] = frames, status
    return s


def run_update(engine, conn_room, n_rooms, changes=None, max_changes=None, prev=None, conn_flags=None, plan=None,
               conn_room_dev=None):
    """gevws_rooms_update_async on host arrays: host copies of everything it
    may write, each prefilled with FILL, and of d_conn_room_in after the call.
    conn_room_dev: the input as a device tensor (a previous call's output)."""
    import torch
    dev = torch.device("cuda", engine.device)
    cr = np.ascontiguousarray(np.asarray(conn_room, np.uint32).reshape(-1))
    nc = cr.size
    d_in = conn_room_dev if conn_room_dev is not None else mm._dev(cr, dev, 4)
    d_ch = None if changes is None else mm._dev(np.ascontiguousarray(changes), dev, 8)
    nch = 0 if changes is None else (len(changes) if max_changes is None else max_changes)
    d_prev = None if prev is None else mm._dev(summary_np(int(prev.get("frames", 0)), int(prev["status"])), dev, 64)
    d_plan = None if plan is None else mm._dev(summary_np(int(plan.get("frames", 0)), int(plan["status"])), dev, 64)
    d_cs = None if conn_flags is None else mm._dev(conn_send_np(conn_flags), dev, 32)
    f = lambda nbytes: torch.full((max(nbytes, 8),), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    out, first, members, summ = f(nc * 4), f((n_rooms + 1) * 4), f(nc * 4), f(64)
    engine.rooms_update_async(d_in if nc else None, nc, n_rooms, d_ch, nch, d_prev, d_cs, d_plan, 0, out, first,
                              members, summ)
    torch.cuda.synchronize(engine.device)
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(conn_room=h(out), first=h(first), members=h(members), summary=h(summ).view(mm.SUMMARY_DTYPE)[0],
                conn_room_in=h(d_in)[: nc * 4].view(np.uint32) if nc else np.zeros(0, np.uint32), dev_out=out)


def assert_update(got: dict, want: dict, conn_room, tag="") -> None:
    """Device == model on the summary and the three outputs; what is not an
    output entry is still FILL; the input is unchanged."""
    s, w = got["summary"], want["summary"]
    have = tuple(int(s[k]) for k in ("frames", "payload_bytes", "payload_len", "errors", "status"))
    assert have == tuple(int(w[k]) for k in ("frames", "payload_bytes", "payload_len", "errors", "status")), (
        tag, "summary", have, w)
    assert int(s["flags"]) == 0 and int(s["run_frames"]) == 0 and not s["reserved"].any(), (tag, "summary tail")
    assert np.array_equal(got["conn_room_in"], np.asarray(conn_room, np.uint32).reshape(-1)), (tag, "input written")
    if want["conn_room"] is None:
        for k in ("conn_room", "first", "members"):
            assert np.all(got[k] == FILL), (tag, k, "written by a call that wrote nothing")
        return
    for k in ("conn_room", "first", "members"):
        w8 = np.ascontiguousarray(want[k], dtype=np.uint32).view(np.uint8)
        g8 = got[k]
        assert np.array_equal(g8[: w8.size], w8), (tag, k, g8[: w8.size].view(np.uint32)[:16],
                                                    np.asarray(want[k])[:16])
        assert np.all(g8[w8.size:] == FILL), (tag, k, "written behind its end")
