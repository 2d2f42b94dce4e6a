"""CPU checks of the push pass's model (tests/_push_model.py): its own
properties over seeded cases -- every entry's recipient is a recipient of its
push, a connection is sent its pushes in list order, a push is in a list exactly
when some recipient takes it that way -- gev_amd.push_records against its
permutation, and gevws_push_check against the model's record rule on mutated
records.  No device is used."""
import numpy as np
import pytest

import gev_amd
from tests import _push_model as pm
from tests import _rooms_model as ro

SHAPE = pm.base_shape()


def case(seed, n, shape=SHAPE, **kw):
    rng = np.random.default_rng(seed)
    recs, arena, perm = gev_amd.push_records(pm.random_items(rng, n, shape["n_conns"], **kw))
    return recs, arena, perm, arena.size - gev_amd.IN_PAD


def both_models(recs, src_bytes, shape=SHAPE, ext="ext", live="live", rooms="rooms"):
    e, lv, r = shape.get(ext), shape.get(live), shape.get(rooms)
    nc = shape["n_conns"]
    lists = pm.lists_model(recs, src_bytes, e, shape["wb"], lv, nc, r)
    model_w, _ = pm.synthetic_wires(lists)
    plan = pm.plan_model(recs, src_bytes, lists["plain_of"], lists["def_of"], model_w, e, lv, nc, r)
    return lists, plan, model_w


@pytest.mark.parametrize("seed,n", [(1, 0), (2, 1), (3, 3), (4, 60), (5, 600)])
def test_properties_of_the_model(seed, n):
    recs, arena, perm, src_bytes = case(seed, n)
    nc, rooms, ext, live = SHAPE["n_conns"], SHAPE["rooms"], SHAPE["ext"], SHAPE["live"]
    lists, plan, wires = both_models(recs, src_bytes)
    if n == 0:
        assert lists["plain"] is None and plan["send"] is None and plan["summary"] == pm.zero_summary()
        return
    assert lists["def_summary"]["status"] == 0 and plan["summary"]["status"] == 0
    R = [pm.recipients(r, nc, rooms, live) for r in recs]
    # list membership is exactly "some recipient takes it"
    for p, r in enumerate(recs):
        ctl = int(r["opcode"]) in (pm.PING, pm.PONG)
        takes_plain = [c for c in R[p] if ctl or not pm.takes_deflate(ext, c)]
        takes_def = [c for c in R[p] if not ctl and pm.takes_deflate(ext, c)]
        assert (lists["plain_of"][p] >= 0) == bool(takes_plain), p
        assert (lists["def_of"][p] >= 0) == bool(takes_def), p
        if takes_def:
            d = lists["def_msgs"][int(lists["def_of"][p])]
            assert int(d["window_bits"]) == min(int(SHAPE["wb"][c]) or 15 for c in takes_def), p
            assert (int(d["payload_off"]), int(d["length"]), int(d["opcode"])) == (int(r["off"]), int(r["length"]),
                                                                                   int(r["opcode"]))
    # both lists keep the push order
    for k in ("plain_of", "def_of"):
        idx = lists[k][lists[k] >= 0]
        assert idx.tolist() == list(range(idx.size)), k
    # every entry's recipient is a recipient of its push; a connection's entries are in list order and complete
    send, cs = plan["send"], plan["conn_send"]
    assert int(cs["count"].sum()) == send.size == plan["summary"]["frames"] == sum(len(x) for x in R)
    for c in range(nc):
        mine = send[int(cs["first"][c]): int(cs["first"][c]) + int(cs["count"][c])]
        assert np.all(mine["conn"] == c)
        frames = [int(x) for x in mine["frame"]]
        assert frames == sorted(frames) and frames == [p for p in range(n) if c in R[p]], c
        assert int(cs["bytes"][c]) == int(mine["len"].sum()) and int(cs["flags"][c]) == 0
        if not live[c]:
            assert mine.size == 0
        for e in mine:
            p, wire = int(e["frame"]), int(e["wire"])
            assert wire == (1 if pm.takes_deflate(ext, c) and lists["def_of"][p] >= 0 else 0)
            tab, cnt, total = wires[wire]
            i = int((lists["def_of"] if wire else lists["plain_of"])[p])
            assert int(e["off"]) == int(tab[i]) and int(e["len"]) == (int(tab[i + 1]) if i + 1 < cnt else total) - int(
                tab[i])
    if n >= 60:   # the shape's corners are exercised
        assert any(not R[p] for p in range(n)) and set(send["wire"].tolist()) == {0, 1}
        assert any(int(r["kind"]) == pm.ROOM and int(r["target"]) == pm.DEAD_ROOM for r in recs)
        assert {int(x) for x in recs["length"]} >= set(pm.LENGTHS)


def test_degenerate_tables():
    recs, arena, perm, src_bytes = case(7, 40)
    nc = SHAPE["n_conns"]
    # nobody is live: no entry, both lists empty
    dead = dict(SHAPE, live=np.zeros(nc, np.uint8))
    lists, plan, _ = both_models(recs, src_bytes, dead)
    assert lists["plain_summary"]["frames"] == lists["def_summary"]["frames"] == 0 and plan["summary"]["frames"] == 0
    assert np.all(plan["conn_send"]["count"] == 0)
    # no extension table: the deflate list is empty, everything goes out plain
    lists, plan, _ = both_models(recs, src_bytes, SHAPE, ext="none")
    assert lists["def_summary"]["frames"] == 0 and set(plan["send"]["wire"].tolist()) == {0}
    # no room tables: a ROOM push is malformed
    lists, _, _ = both_models(recs, src_bytes, SHAPE, rooms="none")
    n_room = int(np.count_nonzero(recs["kind"] == pm.ROOM))
    assert n_room > 3 and lists["def_summary"] == dict(pm.zero_summary(), errors=n_room, status=pm.ERR_INVALID)
    # a bad window byte counts on a live deflate-taker only, once
    wb = SHAPE["wb"].copy()
    takers = [c for c in range(nc) if pm.takes_deflate(SHAPE["ext"], c)]
    live_t, dead_t = [c for c in takers if SHAPE["live"][c]][0], [c for c in takers if not SHAPE["live"][c]][0]
    plain_c = [c for c in range(nc) if not pm.takes_deflate(SHAPE["ext"], c)][0]
    wb[[live_t, dead_t, plain_c]] = 7
    assert pm.table_bad(SHAPE["rooms"], nc, SHAPE["ext"], wb, SHAPE["live"]) == 1
    assert pm.table_bad(SHAPE["rooms"], nc, SHAPE["ext"], wb, None) == 2


def test_capacity_and_gates_of_the_model():
    recs, arena, perm, src_bytes = case(8, 20)
    nc = SHAPE["n_conns"]
    lists, plan, wires = both_models(recs, src_bytes)
    need = plan["summary"]["frames"]
    args = (recs, src_bytes, lists["plain_of"], lists["def_of"], wires, SHAPE["ext"], SHAPE["live"], nc,
            SHAPE["rooms"])
    short = pm.plan_model(*args, max_sends=need - 1)
    assert short["send"] is None and short["summary"] == dict(plan["summary"], status=pm.ERR_CAPACITY)
    assert pm.plan_model(*args, max_sends=need)["summary"]["status"] == 0
    assert pm.plan_model(*args, gate_ok=False)["summary"] == pm.zero_summary()
    assert pm.plan_model(*args, prev=dict(frames=20, status=pm.ERR_CAPACITY))["summary"] == pm.zero_summary()
    # the count from d_prev: a shorter list is a prefix
    part = pm.lists_model(recs, src_bytes, SHAPE["ext"], SHAPE["wb"], SHAPE["live"], nc, SHAPE["rooms"],
                          prev=dict(frames=5, status=0))
    assert part["plain_of"].size == 5 and np.array_equal(part["plain_of"], lists["plain_of"][:5])
    # a push a recipient needs from a list it is not in
    po = lists["plain_of"].copy()
    p = int(np.flatnonzero(po >= 0)[0])
    po[p] = -1
    bad = pm.plan_model(recs, src_bytes, po, lists["def_of"], wires, SHAPE["ext"], SHAPE["live"], nc, SHAPE["rooms"])
    assert bad["summary"] == dict(pm.zero_summary(), errors=1, status=pm.ERR_INVALID)


def test_push_records_round_trips_through_its_permutation():
    rng = np.random.default_rng(9)
    items = pm.random_items(rng, 200, 50, lengths=(0, 1, 15, 16, 17, 125, 126, 1000))
    recs, arena, perm = gev_amd.push_records(items)
    assert recs.dtype == gev_amd.PUSH_DTYPE and sorted(perm.tolist()) == list(range(200))
    k = pm.keys(recs)
    assert np.all(k[1:] >= k[:-1])
    for j, i in enumerate(perm):
        kind, target, op, body = items[int(i)]
        r = recs[j]
        assert (int(r["kind"]), int(r["target"]), int(r["opcode"]), int(r["length"])) == (kind, target, op, len(body))
        assert int(r["off"]) % gev_amd.PAYLOAD_ALIGN == 0 and not r["reserved"].any()
        assert bytes(arena[int(r["off"]): int(r["off"]) + len(body)]) == body
    # stable: pushes of one key keep their order; bodies do not overlap; the slack is there and zero
    for a, b in zip(range(199), range(1, 200)):
        if k[a] == k[b]:
            assert perm[a] < perm[b]
    spans = sorted((int(r["off"]), int(r["length"])) for r in recs)
    assert all(o + ln <= o2 for (o, ln), (o2, _) in zip(spans, spans[1:]))
    src_bytes = arena.size - gev_amd.IN_PAD
    assert src_bytes % 16 == 0 and max(o + ln for o, ln in spans) <= src_bytes and not arena[src_bytes:].any()
    assert gev_amd.push_check(recs, 50, pm.N_ROOMS, src_bytes) == 0


def test_push_check_agrees_with_the_model_on_mutated_records():
    rng = np.random.default_rng(10)
    recs, arena, perm = gev_amd.push_records(pm.random_items(rng, 64, 40, lengths=(0, 1, 16, 125, 126, 300)))
    src_bytes = arena.size - gev_amd.IN_PAD
    nc, nr = 40, pm.N_ROOMS
    assert not pm.records_bad(recs, nc, nr, src_bytes).any()
    mutations = {
        "kind": (3, 255), "target": (nr, 40, 0xFFFFFFFF, 1), "opcode": (0, 3, 8, 11, 255),
        "off": (8, 1, src_bytes, src_bytes + 16, (1 << 64) - 16),
        "length": (src_bytes + 1, 1 << 32, (1 << 64) - 1, 126),
    }
    seen_bad = seen_good = 0
    for field, values in mutations.items():
        for v in values:
            for i in (0, 1, 31, 63):
                m = recs.copy()
                m[i][field] = v
                want = int(pm.records_bad(m, nc, nr, src_bytes).sum())
                assert gev_amd.push_check(m, nc, nr, src_bytes) == want, (field, v, i)
                seen_bad += want > 0
                seen_good += want == 0
    for i in (0, 40):
        for b in range(10):
            m = recs.copy()
            m[i]["reserved"][b] = 1 + b
            assert gev_amd.push_check(m, nc, nr, src_bytes) == 1 == int(pm.records_bad(m, nc, nr, src_bytes).sum())
    # the order: a swap of two records with different keys is one bad record (the second)
    m = recs.copy()
    j = int(np.flatnonzero(pm.keys(recs)[1:] > pm.keys(recs)[:-1])[0])
    m[[j, j + 1]] = m[[j + 1, j]]
    assert gev_amd.push_check(m, nc, nr, src_bytes) == int(pm.records_bad(m, nc, nr, src_bytes).sum()) >= 1
    # random bytes
    for it in range(200):
        m = recs[:8].copy()
        raw = m.view(np.uint8).reshape(-1)
        for _ in range(int(rng.integers(1, 4))):
            raw[int(rng.integers(0, raw.size))] = int(rng.integers(0, 256))
        assert gev_amd.push_check(m, nc, nr, src_bytes) == int(pm.records_bad(m, nc, nr, src_bytes).sum()), it
    assert seen_bad > 20 and seen_good > 0
    assert ro.ROOM_NONE == gev_amd.ROOM_NONE
