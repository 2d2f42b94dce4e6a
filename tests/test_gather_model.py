"""CPU checks that pin tests/_gather_model.gather_model, the reference of the
GPU tests: hand-derived buffers, offsets and summaries for every rule of
gevws_send_gather_async's contract, and the spans against the concatenation
rule of gev_amd.Responses.conn_bytes on random send lists."""
import numpy as np

import gev_amd
from tests import _gather_model as gm

ZERO = dict(frames=0, payload_bytes=0, payload_len=0, errors=0, status=0)


def wires3(seed=1, sizes=(40, 33, 20)):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, n, dtype=np.uint8) for n in sizes]


def test_two_spans_by_hand():
    w = wires3()
    send, cs = gm.make_lists([[(0, 3, 5), (2, 0, 2)], [(1, 1, 16)]], flags=[0, 3])
    m = gm.gather_model(send, cs, w, [40, 33, 20], 64)
    want = bytes(w[0][3:8]) + bytes(w[2][0:2]) + bytes(9) + bytes(w[1][1:17])
    assert m["buf"].tobytes() == want and len(want) == 32
    assert m["summary"] == dict(frames=3, payload_bytes=32, payload_len=23, errors=0, status=0)
    assert [tuple(int(x) for x in (b["off"], b["bytes"], b["flags"])) for b in m["conn_buf"]] == [(0, 7, 0), (16, 16, 3)]
    assert not m["conn_buf"]["reserved"].any()


def test_empty_connections_point_at_the_next_span():
    w = wires3()
    send, cs = gm.make_lists([[], [(0, 0, 17)], [], [], [(2, 19, 1)], []])
    m = gm.gather_model(send, cs, w, [40, 33, 20], 1 << 20)
    assert [int(x) for x in m["conn_buf"]["off"]] == [0, 0, 32, 32, 32, 48]
    assert [int(x) for x in m["conn_buf"]["bytes"]] == [0, 17, 0, 0, 1, 0]
    assert m["summary"] == dict(frames=2, payload_bytes=48, payload_len=18, errors=0, status=0)
    assert m["buf"][:17].tobytes() == bytes(w[0][:17]) and not m["buf"][17:32].any()
    assert m["buf"][32] == w[2][19] and not m["buf"][33:].any()


def test_zero_length_entries_and_an_exact_multiple_of_16():
    w = wires3()
    send, cs = gm.make_lists([[(0, 0, 0), (1, 0, 16), (2, 5, 0)], [(0, 40, 0)], [(2, 4, 16)]])
    m = gm.gather_model(send, cs, w, [40, 33, 20], 32)
    assert m["buf"].tobytes() == bytes(w[1][:16]) + bytes(w[2][4:20])
    assert [int(x) for x in m["conn_buf"]["off"]] == [0, 16, 16]
    assert m["summary"] == dict(frames=5, payload_bytes=32, payload_len=32, errors=0, status=0)


def test_gates_give_a_zero_summary_and_no_tables():
    w = wires3()
    send, cs = gm.make_lists([[(0, 0, 4)]])
    for kw in (dict(plan_status=gm.ERR_CAPACITY), dict(plan_status=gm.ERR_INVALID), dict(plan_frames=0)):
        m = gm.gather_model(send, cs, w, [40, 33, 20], 64, **kw)
        assert m["buf"] is None and m["conn_buf"] is None and m["summary"] == ZERO, kw
    m = gm.gather_model(send, cs[:0], w, [40, 33, 20], 64)
    assert m["buf"] is None and m["summary"] == ZERO
    m = gm.gather_model(send[:0], cs, w, [40, 33, 20], 64)
    assert m["buf"] is None and m["summary"] == ZERO


def test_the_entries_are_the_plan_count_capped_by_the_table():
    w = wires3()
    send, cs = gm.make_lists([[(0, 0, 4), (0, 4, 4)]])
    m = gm.gather_model(send, cs, w, [40, 33, 20], 64, plan_frames=7)  # more than max_sends: the table's two
    assert m["summary"]["frames"] == 2 and m["buf"][:8].tobytes() == bytes(w[0][:8])
    m = gm.gather_model(send, cs, w, [40, 33, 20], 64, plan_frames=1)  # the range now ends behind the entries
    assert m["buf"] is None and m["summary"] == dict(ZERO, errors=1, status=gm.ERR_INVALID)


def test_capacity_reports_the_need():
    w = wires3()
    send, cs = gm.make_lists([[(0, 0, 17)], [(1, 0, 1)]])
    m = gm.gather_model(send, cs, w, [40, 33, 20], 32)
    assert m["buf"] is None and m["conn_buf"] is None
    assert m["summary"] == dict(frames=2, payload_bytes=48, payload_len=18, errors=0, status=gm.ERR_CAPACITY)
    assert gm.gather_model(send, cs, w, [40, 33, 20], 48)["summary"]["status"] == 0


def malformed(edit, wire_bytes=(40, 33, 20)):
    w = wires3()
    send, cs = gm.make_lists([[(0, 0, 4), (2, 1, 3)], [(1, 2, 9)], [(0, 8, 8), (0, 16, 8)]])
    edit(send, cs)
    m = gm.gather_model(send, cs, w, list(wire_bytes), 1 << 20)
    assert m["buf"] is None and m["conn_buf"] is None
    assert m["summary"]["status"] == gm.ERR_INVALID and m["summary"]["frames"] == 0
    assert m["summary"]["payload_bytes"] == 0 and m["summary"]["payload_len"] == 0
    return m["summary"]["errors"]


def put(table, i, field, v):
    def edit(send, cs):
        (send if table == "send" else cs)[i][field] = v
    return edit


def test_malformed_records_are_counted():
    # a bad entry leaves its connection's sum short: the entry and the connection count
    assert malformed(put("send", 1, "wire", 3)) == 2
    assert malformed(put("send", 2, "off", 25)) == 2          # 25 + 9 > 33
    assert malformed(put("send", 2, "off", (1 << 64) - 4)) == 2   # off + len overflows
    assert malformed(put("send", 2, "len", (1 << 64) - 1)) == 2
    assert malformed(put("send", 0, "conn", 3)) == 2          # conn >= n_conns
    assert malformed(put("send", 0, "conn", 1)) == 2          # outside connection 1's range, and connection 0's sum is short
    assert malformed(put("send", 4, "len", 0)) == 1           # a zero-length entry is fine: only the sum is off
    assert malformed(put("conn_send", 1, "bytes", 8)) == 1
    assert malformed(put("conn_send", 2, "count", 3)) == 1    # beyond the entry count
    assert malformed(put("conn_send", 2, "first", 6)) == 3    # beyond it, and both of its entries outside
    assert malformed(put("conn_send", 1, "first", 1)) == 2    # overlaps connection 0, and its own entry 2 lies outside

    def two(send, cs):  # two at once
        send[1]["wire"] = 7
        cs[1]["bytes"] = 1
    assert malformed(two) == 3


def test_a_segment_may_end_on_its_wires_last_byte():
    w = wires3()
    send, cs = gm.make_lists([[(0, 30, 10)], [(2, 0, 20)]])
    assert gm.gather_model(send, cs, w, [40, 33, 20], 64)["summary"]["status"] == 0
    m = gm.gather_model(send, cs, w, [39, 33, 20], 64)
    assert m["summary"]["status"] == gm.ERR_INVALID and m["summary"]["errors"] == 2


def test_spans_follow_conn_bytes_concatenation():
    """For random valid lists, every span of the model's buffer is what
    Responses.conn_bytes (the host's three-wire join) gives for that
    connection, the pads are zero and the spans lie in order on 16."""
    import torch
    rng = np.random.default_rng(77)
    for trial in range(20):
        sizes = [int(rng.integers(1, 5000)) for _ in range(3)]
        w = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
        conns = []
        for _ in range(int(rng.integers(1, 9))):
            ents = []
            for _ in range(int(rng.integers(0, 6))):
                wi = int(rng.integers(0, 3))
                ln = int(rng.integers(0, min(sizes[wi], 300) + 1))
                ents.append((wi, int(rng.integers(0, sizes[wi] - ln + 1)), ln))
            conns.append(ents)
        send, cs = gm.make_lists(conns, flags=[int(rng.integers(0, 4)) for _ in conns])
        m = gm.gather_model(send, cs, w, sizes, 1 << 30)
        if send.shape[0] == 0:
            assert m["buf"] is None
            continue
        assert m["summary"]["status"] == 0 and m["summary"]["frames"] == send.shape[0]
        plan = np.zeros(1, gev_amd.SUMMARY_DTYPE)
        plan["frames"] = send.shape[0]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy())  # noqa: E731
        echo = gev_amd.Echo(def_wire=t(w[1]), def_conn=None, def_off=None, plain_wire=t(w[0]), plain_conn=None,
                            plain_off=None, reply_of=None)
        res = gev_amd.Responses(echo=echo, ctl_wire=t(w[2]), ctl_conn=None, ctl_of=None, msg_end=None, conn_ctl=None,
                                ctl_summary=None, send=t(send).reshape(-1, 32), conn_send=t(cs).reshape(-1, 32),
                                summary=t(plan), n_conns=len(conns))
        end = 0
        for c, b in enumerate(m["conn_buf"]):
            off, nb = int(b["off"]), int(b["bytes"])
            assert off % 16 == 0 and off == end and int(b["flags"]) == int(cs["flags"][c])
            assert m["buf"][off: off + nb].tobytes() == res.conn_bytes(c), (trial, c)
            end = off + gm.round16(nb)
            assert not m["buf"][off + nb: end].any()
        assert end == m["summary"]["payload_bytes"] == m["buf"].size
        assert m["summary"]["payload_len"] == sum(int(x) for x in cs["bytes"])
