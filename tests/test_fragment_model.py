"""tests/_fragment_model.py pinned by the properties of the fragment rule
(include/gevws.h, RFC 6455 section 5.4, RFC 7692 section 6.1) on random record
lists: the model is what the library's host twin and the device step are
compared with, so it is checked by what fragments must be, not by another
implementation."""
import numpy as np
import pytest

from tests import _fragment_model as fm


def lists():
    rng = np.random.default_rng(0x66726167)
    for F in (1, 2, 7, 16, 125, 126, 1000):
        yield F, fm.random_records(60, F, rng)
        yield F, fm.shape_records(F, rng)


@pytest.mark.parametrize("case", range(14))
def test_properties_of_the_fragments(case):
    F, recs = list(lists())[case]
    frags, first, s = fm.fragment(recs, F, 1 << 32)
    n = len(recs)
    assert int(s["status"]) == fm.OK and int(s["errors"]) == 0
    assert first[0] == 0 and int(first[n]) == len(frags) == int(s["frames"])
    assert int(s["payload_len"]) == int(recs["payload_len"].sum()) == int(frags["payload_len"].sum())
    split = 0
    for k, r in enumerate(recs):
        fs = frags[int(first[k]): int(first[k + 1])]
        assert len(fs) >= 1
        if not fm.splittable(r, F):
            assert len(fs) == 1 and fs[0].tobytes() == r.tobytes(), k   # byte-identical
            continue
        split += 1
        L = int(r["payload_len"])
        assert len(fs) == -(-L // F) >= 2
        # the payload ranges concatenate to the record's
        at = int(r["payload_off"])
        for f in fs:
            assert int(f["payload_off"]) == at and int(f["length"]) == int(f["payload_len"])
            at += int(f["payload_len"])
        assert at == int(r["payload_off"]) + L
        # exactly one FIN, on the last fragment
        assert [int(f["fin"]) for f in fs] == [0] * (len(fs) - 1) + [1]
        # opcode and rsv on the first fragment only
        assert int(fs[0]["opcode"]) == int(r["opcode"]) and int(fs[0]["rsv"]) == int(r["rsv"])
        assert not fs[1:]["opcode"].any() and not fs[1:]["rsv"].any()
        # every fragment at most F, all but the last exactly F
        assert all(int(f["payload_len"]) == F for f in fs[:-1]) and 1 <= int(fs[-1]["payload_len"]) <= F
        # the mask travels with every fragment
        assert all(int(f["masked"]) == int(r["masked"]) and f["mask"].tobytes() == r["mask"].tobytes() for f in fs)
    assert int(s["payload_bytes"]) == split
    assert split > 0


def test_a_limit_at_or_above_the_longest_record_is_the_identity():
    rng = np.random.default_rng(0x66726168)
    recs = fm.random_records(80, 50, rng)
    longest = int(recs["payload_len"].max())
    for F in (longest, longest + 1, 1 << 40):
        frags, first, s = fm.fragment(recs, F, len(recs))
        assert frags.tobytes() == recs.tobytes()
        assert first.tolist() == list(range(len(recs) + 1))
        assert (int(s["frames"]), int(s["payload_bytes"]), int(s["status"])) == (len(recs), 0, fm.OK)
    # one byte below the longest record that may split, exactly that record splits
    data = max(int(r["payload_len"]) for r in recs if fm.splittable(r, 0))
    frags, _, s = fm.fragment(recs, data - 1, 1 << 20)
    assert len(frags) > len(recs) and int(s["payload_bytes"]) >= 1
    assert fm.fragment(recs, data, 1 << 20)[0].tobytes() == recs.tobytes()


def test_capacity_gate_and_malformed():
    rng = np.random.default_rng(0x66726169)
    recs = fm.random_records(40, 9, rng)
    _, _, s = fm.fragment(recs, 9, 1 << 20)
    need = int(s["frames"])
    frags, first, c = fm.fragment(recs, 9, need - 1)
    assert frags is None and first is None
    assert (int(c["frames"]), int(c["status"])) == (need, fm.ERR_CAPACITY)
    frags, first, c = fm.fragment(recs, 9, need)
    assert len(frags) == need and int(c["status"]) == fm.OK
    # the gate: a count below the list, and a failed step before
    frags, first, c = fm.fragment(recs, 9, 1 << 20, prev=fm.summary(frames=7))
    want = fm.fragment(recs[:7], 9, 1 << 20)
    assert frags.tobytes() == want[0].tobytes() and first.tolist() == want[1].tolist() and len(first) == 8
    frags, first, c = fm.fragment(recs, 9, 1 << 20, prev=fm.summary(frames=7, status=fm.ERR_CAPACITY))
    assert frags is None and first is None and c.tobytes() == fm.summary().tobytes()
    # malformed: more than 2^31 - 1 fragments of one record, and nothing else
    big = np.array([fm.record(3), fm.record(1 << 40), fm.record((1 << 31) - 1), fm.record(1 << 31, opcode=2)],
                   fm.OUT_FRAME_DTYPE)
    frags, first, c = fm.fragment(big, 1, 1 << 62)
    assert frags is None and first is None
    assert (int(c["frames"]), int(c["payload_len"]), int(c["errors"]), int(c["status"])) == (0, 0, 2, fm.ERR_INVALID)
    _, _, c = fm.fragment(big[[0, 2]], 1, 10)
    assert (int(c["frames"]), int(c["status"])) == (3 + (1 << 31) - 1, fm.ERR_CAPACITY)
    _, _, c = fm.fragment(big, 2, 10)   # at F = 2 only the 2^40 record is malformed
    assert (int(c["errors"]), int(c["status"])) == (1, fm.ERR_INVALID)


def test_offsets_model():
    rng = np.random.default_rng(0x6672616A)
    recs = fm.random_records(30, 5, rng)
    frags, first, s = fm.fragment(recs, 5, 1 << 20)
    sizes = [2 + int(x) for x in frags["payload_len"]]
    frag_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    enc = fm.summary(len(frags), sum(sizes), int(frags["payload_len"].sum()))
    off, r = fm.offsets(first, len(recs), None, s, frag_off, enc)
    assert (int(r["frames"]), int(r["payload_bytes"]), int(r["payload_len"]), int(r["status"])) == \
        (len(recs), sum(sizes), int(enc["payload_len"]), fm.OK)
    # reply k's bytes run to the next reply's first fragment or the wire total: its fragments' sizes
    ends = list(off[1:]) + [sum(sizes)]
    for k in range(len(recs)):
        assert int(ends[k]) - int(off[k]) == sum(sizes[int(first[k]): int(first[k + 1])])
    # gates, first failing status first; the encode's CAPACITY hands its need through
    cap = fm.summary(len(frags), 12345, status=fm.ERR_CAPACITY)
    assert fm.offsets(first, len(recs), None, s, frag_off, cap)[1].tobytes() == \
        fm.summary(payload_bytes=12345, status=fm.ERR_CAPACITY).tobytes()
    bad_prev = fm.summary(3, 777, status=fm.ERR_CAPACITY)
    assert fm.offsets(first, len(recs), bad_prev, s, frag_off, cap)[1].tobytes() == \
        fm.summary(status=fm.ERR_CAPACITY).tobytes()
    inv = fm.summary(errors=2, status=fm.ERR_INVALID)
    assert fm.offsets(first, len(recs), None, inv, frag_off, cap)[1].tobytes() == \
        fm.summary(status=fm.ERR_INVALID).tobytes()
    # misfits
    dec = first.copy()
    dec[4], dec[5] = dec[5], dec[4]
    o, r = fm.offsets(dec, len(recs), None, s, frag_off, enc)
    assert o is None and int(r["status"]) == fm.ERR_INVALID and int(r["errors"]) >= 1 and int(r["frames"]) == 0
    o, r = fm.offsets(first, len(recs), None, fm.summary(len(frags) + 1), frag_off, enc)
    assert o is None and (int(r["errors"]), int(r["status"])) == (1, fm.ERR_INVALID)
    nz = first.copy()
    nz[0] = 1
    assert int(fm.offsets(nz, len(recs), None, s, frag_off, enc)[1]["errors"]) == 1
