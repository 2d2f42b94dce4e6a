"""GPU checks of the push pass (gevws_push_lists_async, gevws_push_plan_async)
through the C ABI, bit-exact against tests/_push_model.py -- both lists,
d_plain_of / d_def_of, d_send, d_conn_send, the summaries, everything else still
the 0xEE it was prefilled with -- and of the whole chain as the clients see it
(Engine.push)."""
import zlib

import numpy as np
import pytest

import gev_amd
from tests import _join_model as jm
from tests import _push_model as pm
from tests import _respond_model as rm
from tests import _rooms_model as ro
from tests import _session as se

pytestmark = pytest.mark.gpu

SHAPE = pm.base_shape()
NC = SHAPE["n_conns"]
INVALID, CAPACITY = gev_amd.ERR_INVALID, gev_amd.ERR_CAPACITY


def records(seed, n, n_conns=NC, **kw):
    recs, arena, _ = gev_amd.push_records(pm.random_items(np.random.default_rng(seed), n, n_conns, **kw))
    return recs, arena, arena.size - gev_amd.IN_PAD


def both(engine, recs, src_bytes, shape=SHAPE, max_sends=None, prev=None, max_pushes=None, good=None, statuses=None,
         plan_tables=None, tag=""):
    """The list step and the plan on synthetic wires: device == model for both
    calls.  prev: d_prev as dict(frames, status); good: (recs, shape) whose
    lists the plan is given when the call's own input is malformed; statuses:
    the plan's gate summaries' statuses; plan_tables: a function that edits the
    plan's (plain_of, def_of, model wires, device wires)."""
    nc, ext, wb, live, rooms = shape["n_conns"], shape.get("ext"), shape.get("wb"), shape.get("live"), shape.get("rooms")
    prev_np = None if prev is None else rm.summary_np(**prev)
    want_l = pm.lists_model(recs, src_bytes, ext, wb, live, nc, rooms, prev, max_pushes)
    got_l = pm.run_lists(engine, recs, src_bytes, ext, wb, live, nc, rooms, prev_np, max_pushes)
    pm.assert_lists(got_l, want_l, (tag, "lists"))
    lists = want_l
    if good is not None or want_l["plain"] is None:
        grecs, gshape = good if good is not None else (recs, shape)
        lists = pm.lists_model(grecs, src_bytes, gshape.get("ext"), None, gshape.get("live"), gshape["n_conns"],
                               gshape.get("rooms"))
    if lists["plain"] is None:   # no records at all: tables of one unused entry
        lists = dict(lists, plain_of=np.full(1, -1, np.int64), def_of=np.full(1, -1, np.int64))
    model_w, dev_w = pm.synthetic_wires(lists)
    plain_of, def_of = lists["plain_of"], lists["def_of"]
    assert plain_of.size == def_of.size >= min(len(recs), max_pushes if max_pushes is not None else len(recs),
                                               prev["frames"] if prev is not None else len(recs))
    if plan_tables is not None:
        plain_of, def_of, model_w, dev_w = plan_tables(plain_of.copy(), def_of.copy(), model_w, dev_w)
    st = dict(plain=0, deflate=0, enc=(0, 0))
    st.update(statuses or {})
    for (tab, s), e in zip(dev_w, st["enc"]):
        s["status"] = e
    gate_ok = not (st["plain"] or st["deflate"] or any(st["enc"]))
    want_p = pm.plan_model(recs, src_bytes, plain_of, def_of, model_w, ext, live, nc, rooms, max_sends, gate_ok, prev,
                           max_pushes)
    cap = max_sends if max_sends is not None else max(int(want_p["summary"]["frames"]), 1)
    got_p = pm.run_plan(engine, recs, src_bytes, rm.summary_np(frames=len(model_w[0][0]), status=st["plain"]),
                        rm.summary_np(frames=len(model_w[1][0]), status=st["deflate"]), plain_of, def_of, dev_w, ext,
                        live, nc, rooms, cap, prev_np, max_pushes)
    pm.assert_plan(got_p, want_p, (tag, "plan"))
    return dict(lists=got_l, lists_model=want_l, plan=got_p, plan_model=want_p)


# ---------------------------------------------------------------------------- 1. both calls against the model
@pytest.mark.parametrize("n", [0, 1, 3, 600])
def test_both_calls_against_the_model(engine, n):
    recs, arena, src_bytes = records(0x7075 + n, n)
    r = both(engine, recs, src_bytes, tag=f"{n} pushes")
    if n < 600:
        return
    send = r["plan_model"]["send"]
    assert {int(x) for x in recs["kind"]} == {0, 1, 2} and {int(x) for x in recs["opcode"]} == {1, 2, 9, 10}
    assert {int(x) for x in recs["length"]} == set(pm.LENGTHS)
    assert int(r["lists"]["plain_summary"]["frames"]) > 256 and int(r["lists"]["def_summary"]["frames"]) > 256
    assert send.size > 20000 and set(send["wire"].tolist()) == {0, 1}
    dead = np.flatnonzero(SHAPE["live"] == 0)
    for kind, targets in ((pm.CONN, set(dead.tolist())), (pm.ROOM, {pm.EMPTY_ROOM}), (pm.ROOM, {pm.DEAD_ROOM})):
        hit = [p for p in range(n) if int(recs["kind"][p]) == kind and int(recs["target"][p]) in targets]
        assert hit and all(r["lists_model"]["plain_of"][p] < 0 and r["lists_model"]["def_of"][p] < 0 for p in hit)
    assert set(r["lists_model"]["def_msgs"]["window_bits"].tolist()) <= {9, 15}
    # the count from d_prev and from max_pushes
    both(engine, recs, src_bytes, prev=dict(frames=450, status=0), tag="450 of 600 by d_prev")
    both(engine, recs, src_bytes, prev=dict(frames=700, status=0), tag="d_prev above max_pushes")
    both(engine, recs, src_bytes, max_pushes=300, tag="300 of 600 by max_pushes")
    both(engine, recs, src_bytes, prev=dict(frames=257, status=0), max_pushes=300, tag="257 by d_prev under 300")


# ---------------------------------------------------------------------------- 2. the client's view
def messages_of(wire: bytes, F):
    """[(opcode, rsv of the first frame, payload)] of what a socket was sent,
    fragments joined (and their pattern under the limit F checked)."""
    out, cur = [], None
    for f in se.parse_wire(wire):
        h = f.header
        assert not h.masked
        if h.opcode & 8:
            assert cur is None and h.fin and h.rsv == 0 and h.length <= 125
            out.append((h.opcode, 0, f.payload))
            continue
        if cur is None:
            assert h.opcode in (1, 2)
            cur = [h.opcode, h.rsv, []]
        else:
            assert h.opcode == 0 and h.rsv == 0
        cur[2].append(f.payload)
        if h.fin:
            parts = cur[2]
            if F is None:
                assert len(parts) == 1
            else:
                assert all(len(p) == F for p in parts[:-1]) and len(parts[-1]) <= F
                assert len(parts) == max(1, -(-sum(len(p) for p in parts) // F))
            out.append((cur[0], cur[1], b"".join(parts)))
            cur = None
    assert cur is None
    return out


@pytest.fixture(scope="module")
def view_case():
    rng = np.random.default_rng(0x76696577)
    items = pm.random_items(rng, 48, NC, all_max=126)
    takers = [c for c in range(NC) if SHAPE["live"][c] and pm.takes_deflate(SHAPE["ext"], c)]
    takeover = [c for c in range(NC) if SHAPE["live"][c] and SHAPE["ext"][c] & pm.EXT_SERVER_TAKEOVER]
    room = int(SHAPE["conn_room"][takeover[0]])
    # a repeat 1500 bytes back: a match inside a window of 15 bits, outside one of 9
    blk = bytes(rng.integers(0x20, 0x7F, 1500, dtype=np.uint8))
    items += [(pm.CONN, takers[0], pm.PING, b"ping to a deflate-taker"), (pm.CONN, takeover[0], pm.TEXT, b"takeover " * 9),
              (pm.ALL, 0, pm.TEXT, b"publish message"), (pm.ALL, 0, pm.PONG, b""),
              (pm.ALL, 0, pm.TEXT, blk + blk[:1100])]
    if room != pm.ROOM_NONE:
        items.append((pm.ROOM, room, pm.TEXT, b"to the takeover member's room " * 5))
    recs, arena, perm = gev_amd.push_records(items)
    want = pm.client_view(recs, arena, SHAPE["ext"], SHAPE["live"], NC, SHAPE["rooms"])
    return dict(recs=recs, arena=arena, want=want, taker=takers[0], takeover=takeover[0])


@pytest.mark.parametrize("F", [None, 1000])
def test_the_clients_view(engine, view_case, F):
    import torch
    dev = torch.device("cuda", engine.device)
    recs, arena, want = view_case["recs"], view_case["arena"], view_case["want"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rooms = gev_amd.Rooms.from_conn_room(SHAPE["conn_room"], dev, n_rooms=pm.N_ROOMS)
    res = engine.push(recs, arena, up(SHAPE["ext"]), rooms, window_bits=up(SHAPE["wb"]), live=up(SHAPE["live"]),
                      gather=True, max_fragment_bytes=F)
    lists = pm.lists_model(recs, arena.size - gev_amd.IN_PAD, SHAPE["ext"], SHAPE["wb"], SHAPE["live"], NC,
                           SHAPE["rooms"])
    assert np.array_equal(res.plain_of, lists["plain_of"]) and np.array_equal(res.def_of, lists["def_of"])
    dm = res.echo.deflated
    sends, cs = res.host_sends(), res.conn_send_host()
    assert int(res.summary_host()["frames"]) == sum(len(w) for w in want) == int(cs["count"].sum())
    assert int(res.summary_host()["errors"]) == 0 and not cs["flags"].any()
    seen = dict(plain=0, deflated=0, ctl=0)
    for c in range(NC):
        wire = bytes(sends[c])
        assert len(wire) == int(cs["bytes"][c]), c
        got = messages_of(wire, F)
        assert len(got) == len(want[c]), (c, len(got), len(want[c]))
        if not SHAPE["live"][c]:
            assert wire == b"", c
        for (op, rsv, payload), (wop, body, compressed) in zip(got, want[c]):
            assert op == wop, c
            if rsv:
                assert rsv == 4 and compressed, c
                payload = zlib.decompressobj(-15).decompress(payload + b"\x00\x00\xff\xff")
                seen["deflated"] += 1
            else:
                seen["ctl" if op & 8 else "plain"] += 1
                # (PLAIN_IF_NOT_SMALLER is off: a deflate-taker's data message is always compressed)
                assert not compressed, (c, op)
            assert payload == body, (c, op, len(body))
    assert min(seen.values()) > 50
    for c in (0, 17, view_case["taker"], view_case["takeover"], NC - 1):
        assert res.conn_bytes(c) == bytes(sends[c]), c
    # a ping to a deflate-taker arrives uncompressed; a takeover member's text arrives with RSV1 clear
    t = messages_of(bytes(sends[view_case["taker"]]), F)
    assert (pm.PING, 0, b"ping to a deflate-taker") in t and any(rsv == 4 for _, rsv, _ in t)
    k = messages_of(bytes(sends[view_case["takeover"]]), F)
    assert (pm.TEXT, 0, b"takeover " * 9) in k and all(rsv == 0 for _, rsv, _ in k)
    # each deflate-list entry's window is the model's minimum, and the payload is compressed within it
    nd = int(lists["def_summary"]["frames"])
    assert nd > 10 and set(lists["def_msgs"]["window_bits"].tolist()) == {9, 15}
    for i in range(nd):
        d = lists["def_msgs"][i]
        body = bytes(arena[int(d["payload_off"]): int(d["payload_off"]) + int(d["length"])])
        assert dm.payload(i) == gev_amd.deflate_raw(body, int(d["window_bits"])), i
    far = [i for i in range(nd) if int(lists["def_msgs"][i]["length"]) == 2600]   # the repeat 1500 bytes back
    assert len(far) == 1 and int(lists["def_msgs"][far[0]]["window_bits"]) == 9
    body = bytes(arena[int(lists["def_msgs"][far[0]]["payload_off"]):][:2600])
    assert dm.payload(far[0]) != gev_amd.deflate_raw(body, 15)


# ---------------------------------------------------------------------------- 3. degenerate shapes
def test_degenerate_shapes(engine):
    recs, arena, src_bytes = records(0x6465, 40)
    only_all = recs[recs["kind"] == pm.ALL]
    assert only_all.size > 5
    r = both(engine, only_all, src_bytes, dict(SHAPE, live=np.zeros(NC, np.uint8)), tag="nobody is live")
    assert jm.summary_tuple(r["plan"]["summary"]) == (0, 0, 0, 0, 0)
    assert int(r["lists"]["plain_summary"]["frames"]) == 0 and int(r["lists"]["def_summary"]["frames"]) == 0
    no_room = recs[recs["kind"] != pm.ROOM]
    r = both(engine, no_room, src_bytes, dict(SHAPE, rooms=None), tag="rooms=None")
    assert int(r["plan"]["summary"]["frames"]) > NC
    r = both(engine, recs, src_bytes, dict(SHAPE, rooms=None), good=(recs, SHAPE), tag="a ROOM push without tables")
    n_room = int(np.count_nonzero(recs["kind"] == pm.ROOM))
    assert jm.summary_tuple(r["lists"]["def_summary"]) == (0, 0, 0, n_room, INVALID)
    r = both(engine, recs, src_bytes, dict(SHAPE, ext=None), tag="conn_ext=None")
    assert int(r["lists"]["def_summary"]["frames"]) == 0 and int(r["lists"]["plain_summary"]["frames"]) > 10
    both(engine, recs, src_bytes, dict(SHAPE, live=None), tag="live=None")
    both(engine, recs, src_bytes, dict(SHAPE, wb=None), tag="window_bits=None")
    # one connection
    one, arena1, sb1 = records(0x6F6E, 12, n_conns=1)
    for ext in (0, pm.EXT_DEFLATE):
        shape = dict(n_conns=1, rooms=ro.csr_of([0], n_rooms=2), ext=np.array([ext], np.uint8),
                     wb=np.array([10], np.uint8), live=None)
        one_r = one.copy()
        one_r["target"][one_r["kind"] == pm.ROOM] %= 2
        one_r = one_r[np.argsort(pm.keys(one_r), kind="stable")]
        r = both(engine, one_r, sb1, shape, tag=f"one connection, ext {ext}")
        assert int(r["plan"]["summary"]["frames"]) > 4
    # 257 connections, all in one room
    n = 257
    shape = dict(n_conns=n, rooms=ro.csr_of(np.zeros(n, np.uint32)), ext=(np.arange(n) % 2).astype(np.uint8),
                 wb=None, live=None)
    recs257, _, sb257 = records(0x3235, 9, n_conns=n, n_rooms=1, lengths=(0, 5, 126))
    r = both(engine, recs257, sb257, shape, tag="257 in one room")
    want = sum(n if int(k) != pm.CONN else 1 for k in recs257["kind"])
    assert int(r["plan"]["summary"]["frames"]) == want > 2 * n


# ---------------------------------------------------------------------------- 4. capacity
def test_capacity(engine):
    recs, arena, src_bytes = records(0x6361, 20)
    r = both(engine, recs, src_bytes, tag="enough")
    need = int(r["plan"]["summary"]["frames"])
    assert need > NC
    both(engine, recs, src_bytes, max_sends=need, tag="exactly the need")
    g = both(engine, recs, src_bytes, max_sends=need - 1, tag="one entry short")
    assert jm.summary_tuple(g["plan"]["summary"]) == (need, int(r["plan"]["summary"]["payload_bytes"]), 0, 0, CAPACITY)
    assert np.all(g["plan"]["send"] == pm.FILL) and np.all(g["plan"]["conn_send"] == pm.FILL)
    again = both(engine, recs, src_bytes, max_sends=need, tag="the retry")
    assert again["plan"]["send"].tobytes() == r["plan"]["send"].tobytes()


# ---------------------------------------------------------------------------- 5. malformed input, gates
def test_malformed_records(engine):
    recs, arena, src_bytes = records(0x6D61, 300, lengths=(0, 1, 16, 125, 126, 300))
    last_all = int(np.flatnonzero(recs["kind"] == pm.ALL)[-1])     # (the last of its kind: the next key stays above)
    last_room = int(np.flatnonzero(recs["kind"] == pm.ROOM)[-1])
    ctl = int(np.flatnonzero(recs["opcode"] >= 9)[0])
    j = int(np.flatnonzero(pm.keys(recs)[1:] > pm.keys(recs)[:-1])[2])
    first_conn = int(np.flatnonzero(recs["kind"] == pm.CONN)[0])
    causes = {
        "a kind above 2": (299, "kind", 3),
        "a room out of range": (last_room, "target", pm.N_ROOMS),
        "a connection out of range": (299, "target", NC),
        "a nonzero target for ALL": (last_all, "target", 1),
        "a close frame": (5, "opcode", 8),
        "opcode 0": (256, "opcode", 0),
        "an offset off the alignment": (257, "off", 8),
        "a range past the arena": (1, "length", src_bytes + 1),
        "a sum that overflows": (2, "off", (1 << 64) - 16),
        "a length of 2^32": (3, "length", 1 << 32),
        "a ping of 126 bytes": (ctl, "length", 126),
    }
    for tag, (i, field, v) in causes.items():
        m = recs.copy()
        m[i][field] = v
        assert gev_amd.push_check(m, NC, pm.N_ROOMS, src_bytes) == 1, tag
        g = both(engine, m, src_bytes, good=(recs, SHAPE), tag=tag)
        for s in (g["lists"]["def_summary"], g["lists"]["plain_summary"], g["plan"]["summary"]):
            assert jm.summary_tuple(s) == (0, 0, 0, 1, INVALID), tag
    m = recs.copy()
    m[first_conn]["reserved"][9] = 1
    g = both(engine, m, src_bytes, good=(recs, SHAPE), tag="a reserved byte")
    assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 1, INVALID)
    m = recs.copy()
    m[[j, j + 1]] = m[[j + 1, j]]
    g = both(engine, m, src_bytes, good=(recs, SHAPE), tag="a key below the previous record's")
    assert jm.summary_tuple(g["lists"]["def_summary"]) == (0, 0, 0, 1, INVALID)
    # two causes in two records count twice, two in one record once
    m = recs.copy()
    m[4]["opcode"], m[4]["off"], m[299]["kind"] = 8, 8, 9
    g = both(engine, m, src_bytes, good=(recs, SHAPE), tag="two records")
    assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 2, INVALID)


def test_malformed_tables(engine):
    recs, arena, src_bytes = records(0x7461, 30)
    cr, first, members = SHAPE["rooms"]

    def edit(which, idx, val):
        tabs = [cr.copy(), first.copy(), members.copy()]
        tabs[which][idx] = val
        return tuple(tabs)

    roomed = int(np.flatnonzero(cr != pm.ROOM_NONE)[5])
    unroomed = int(np.flatnonzero(cr == pm.ROOM_NONE)[0])
    swapped = members.copy()
    a = int(first[0])
    swapped[[a, a + 1]] = swapped[[a + 1, a]]
    cases = {
        "a member >= n_conns": edit(2, 1, NC),
        "an out-of-order pair": (cr, first, swapped),
        "conn_room disagrees with the CSR": edit(0, roomed, (int(cr[roomed]) + 1) % 7),
        "a roomed connection missing from the CSR": edit(0, unroomed, 0),
        "a room id >= n_rooms": edit(0, roomed, pm.N_ROOMS),
        "a decreasing first": edit(1, 1, int(first[2]) + 1),
    }
    for tag, bad in cases.items():
        count = ro.check_tables(bad, NC)
        assert count >= 1, tag
        g = both(engine, recs, src_bytes, dict(SHAPE, rooms=bad), good=(recs, SHAPE), tag=tag)
        for s in (g["lists"]["def_summary"], g["lists"]["plain_summary"], g["plan"]["summary"]):
            assert jm.summary_tuple(s) == (0, 0, 0, count, INVALID), tag
    # a window byte of 7: on a live deflate-taker it is a bad record of the list step (the plan reads no windows)
    takers = [c for c in range(NC) if pm.takes_deflate(SHAPE["ext"], c)]
    live_t = [c for c in takers if SHAPE["live"][c]][:2]
    dead_t = [c for c in takers if not SHAPE["live"][c]][0]
    plain_c = [c for c in range(NC) if not pm.takes_deflate(SHAPE["ext"], c)][0]
    wb = SHAPE["wb"].copy()
    wb[live_t + [dead_t, plain_c]] = 7
    g = both(engine, recs, src_bytes, dict(SHAPE, wb=wb), good=(recs, SHAPE), tag="window bytes of 7")
    assert jm.summary_tuple(g["lists"]["def_summary"]) == (0, 0, 0, 2, INVALID)
    assert int(g["plan"]["summary"]["status"]) == 0
    wb = SHAPE["wb"].copy()
    wb[live_t[0]] = 16
    g = both(engine, recs, src_bytes, dict(SHAPE, wb=wb), good=(recs, SHAPE), tag="a window byte of 16")
    assert jm.summary_tuple(g["lists"]["plain_summary"]) == (0, 0, 0, 1, INVALID)


def test_malformed_plan_tables_and_gates(engine):
    recs, arena, src_bytes = records(0x706C, 30)
    base = both(engine, recs, src_bytes, tag="well formed")
    po, do = base["lists_model"]["plain_of"], base["lists_model"]["def_of"]
    in_both = int(np.flatnonzero((po >= 0) & (do >= 0))[0])
    plain_only = int(np.flatnonzero((po >= 0) & (do < 0))[0])
    npl, nd = int(base["lists"]["plain_summary"]["frames"]), int(base["lists"]["def_summary"]["frames"])

    def setter(which, p, v):
        def f(plain_of, def_of, mw, dw):
            (plain_of, def_of)[which][p] = v
            return plain_of, def_of, mw, dw
        return f

    def decreasing(plain_of, def_of, mw, dw):
        tab = mw[0][0].copy()
        k = int(np.flatnonzero(np.diff(tab.astype(np.int64)) > 2)[0])
        tab[k] = tab[k + 1] + 1   # entry k now starts behind entry k + 1
        return plain_of, def_of, [(tab, mw[0][1], mw[0][2]), mw[1]], [(tab, dw[0][1]), dw[1]]

    cases = {
        "a plain index outside its list": setter(0, in_both, npl),
        "a deflate index outside its list": setter(1, in_both, nd),
        "a push a plain-taker needs from the plain list": setter(0, plain_only, -1),
        "an offset table that decreases": decreasing,
    }
    for tag, f in cases.items():
        g = both(engine, recs, src_bytes, plan_tables=f, tag=tag)
        s = jm.summary_tuple(g["plan"]["summary"])
        assert s[:3] == (0, 0, 0) and s[3] >= 1 and s[4] == INVALID, (tag, s)
    # a deflate-taker's push missing from the deflate list alone comes from the plain wire: well formed
    g = both(engine, recs, src_bytes, plan_tables=setter(1, in_both, -1), tag="deflate index cleared")
    assert int(g["plan"]["summary"]["status"]) == 0
    # gates: a failed summary gives zero summaries, whatever else is wrong
    g = both(engine, recs, src_bytes, prev=dict(frames=30, status=CAPACITY), tag="a failed d_prev")
    for s in (g["lists"]["def_summary"], g["lists"]["plain_summary"], g["plan"]["summary"]):
        assert jm.summary_tuple(s) == (0, 0, 0, 0, 0)
    for st in (dict(plain=INVALID), dict(deflate=CAPACITY), dict(enc=(CAPACITY, 0)), dict(enc=(0, INVALID))):
        g = both(engine, recs, src_bytes, statuses=st, tag=f"failed gate {st}")
        assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 0, 0)
    m = recs.copy()
    m[0]["opcode"] = 8
    g = both(engine, m, src_bytes, prev=dict(frames=30, status=INVALID), good=(recs, SHAPE), tag="gate first")
    assert jm.summary_tuple(g["plan"]["summary"]) == (0, 0, 0, 0, 0)


# ---------------------------------------------------------------------------- 6. determinism
def test_the_same_call_twice(engine):
    recs, arena, src_bytes = records(0x6474, 600, lengths=(0, 1, 16, 125, 126, 300))
    a = both(engine, recs, src_bytes, tag="first")
    b = both(engine, recs, src_bytes, tag="second")
    for step in ("lists", "plan"):
        for k, v in a[step].items():
            assert np.asarray(v).tobytes() == np.asarray(b[step][k]).tobytes(), (step, k)
