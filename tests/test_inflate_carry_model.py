"""CPU checks of tests/_inflate_carry_model.py, the model the GPU tests of
gevws_inflate_carry_async and gevws_join_carry_ext_async compare with.

Cut invariance against zlib: random connections of compressed and plain
messages, fragmented, control frames in between, with and without client context
takeover, cut at random byte positions of the wire stream into 1 to 4 passes.
Whatever the cut, the chained models deliver every message once, in order, with
the bytes that went into zlib's compressor; the takeover slots end as the
one-pass run leaves them."""
import numpy as np
import pytest

from tests import _carry_model as cm
from tests import _inflate_carry_model as icm
from tests import _inflate_takeover as it

BIG = 1 << 22


@pytest.mark.parametrize("seed", range(6))
def test_cut_invariance_against_zlib(seed):
    rng = np.random.default_rng(0x1C0000 + seed)
    n_conns = 24
    conns, ext, want = icm.random_streams(rng, n_conns)
    images = []
    for npass in (1, 2, 3, 4):
        cuts = icm.byte_cuts(rng, conns, npass)
        slots = [it.Slot() for _ in range(n_conns)]
        res = icm.chain_model(cm.split_passes(conns, cuts) if npass > 1 else [conns], ext, BIG, BIG, slots=slots)
        seq = icm.sequences(n_conns, [e["join"] for e in res])
        for c in range(n_conns):
            assert seq[c] == want[c], (npass, c, cuts[c])
        last = res[-1]["join"]
        assert not last["carry"].view(np.uint8).any(), "every message ended: no carry left"
        assert all(int(e["join"]["carry_summary"]["errors"]) == 0 and e["inf"]["errors"] == 0 for e in res)
        images.append([s.image() for s in slots])
    assert all(im == images[0] for im in images[1:]), "a slot is a function of the stream, not of the cuts"


def test_open_compressed_record_between_passes():
    """The record between the passes: OPEN | COMPRESSED, the running compressed
    length, the bytes; an idle pass moves it on; without the flag it is LOST."""
    data = b"a compressed message that spans three passes " * 5
    wire = icm.z(data)
    a, b = 7, len(wire) - 9
    passes = [[[(0, icm.RSV1, 1, wire[:a])]], [[(0, 0, 0, wire[a:b])]], [[]], [[(1, 0, 9, b"ping")]],
              [[(1, 0, 0, wire[b:])]]]
    ext = np.array([it.EXT_DEFLATE], np.uint8)
    res = icm.chain_model(passes, ext, BIG, BIG)
    for p, n in ((0, a), (1, b), (2, b), (3, b)):
        r = res[p]["join"]["carry"][0]
        assert (int(r["flags"]), int(r["length"]), int(r["opcode"]), int(r["status"])) == \
            (icm.OPEN | icm.COMPRESSED, n, 1, 0), p
        assert res[p]["join"]["carry_dst"][:n].tobytes() == wire[:n]
        assert cm.delivered(res[p]["join"]) == []
    assert [int(x) for x in res[1]["inf"]["inflated"]["flags"]] == [2]  # PENDING while it is open
    assert cm.delivered(res[4]["join"]) == [(0, 1, data)]
    assert not res[4]["join"]["carry"].view(np.uint8).any()
    lost = icm.chain_model(passes, ext, BIG, BIG, carry_flags=0)
    assert [int(e["join"]["carry"]["flags"][0]) for e in lost] == [icm.LOST] * 4 + [0]
    assert all(cm.delivered(e["join"]) == [] for e in lost)


def test_mismatched_records_end_lost():
    wire = icm.z(b"mixed up " * 20)
    ext = np.array([it.EXT_DEFLATE] * 2, np.uint8)
    # pass 1 without the flag semantics of pass 2's messages: the records are swapped by hand
    res = icm.chain_model([[[(0, icm.RSV1, 2, wire[:5])], [(0, 0, 2, b"plain, open")]]], ext, BIG, BIG)
    cin, csrc = res[0]["join"]["carry"][::-1].copy(), res[0]["join"]["carry_dst"]
    d = icm.mm.Decoded([[(0, 0, 0, wire[5:9])], [(0, 0, 0, b" goes on")]], pad=0xFF)
    t = icm.gm.model_ext(d.frames, d.conn_out, d.n_decoded, d.arena, res[0]["inf"]["state"], ext)
    w = icm.carry_model_ext(d.frames, d.arena, t, 2, BIG, cin, csrc, 1, carry_flags=icm.KEEP_COMPRESSED)
    assert [(int(r["flags"]), int(r["status"]), int(r["length"])) for r in w["carry"]] == [(icm.LOST, 0, 0)] * 2
