"""A plain numpy / Python restatement of the fragment steps' contracts in
include/gevws.h (gevws_fragment_async, gevws_fragment_offsets_async,
gevws_fragment_records): the rule that splits a record, the fragment list with
its d_first table and summary, and the per-reply offsets behind the encode.
Written from the contract, one record at a time; it shares no code with the
library."""
import numpy as np

OK, ERR_CAPACITY, ERR_INVALID = 0, -2, -3
M64 = (1 << 64) - 1
MAX_FRAGMENTS = (1 << 31) - 1

OUT_FRAME_DTYPE = np.dtype([("fin", "u1"), ("rsv", "u1"), ("opcode", "u1"), ("masked", "u1"),
                            ("mask", "u1", (4,)), ("length", "<i8"),
                            ("payload_off", "<u8"), ("payload_len", "<u8")])
SUMMARY_DTYPE = np.dtype([("frames", "<u8"), ("payload_bytes", "<u8"), ("payload_len", "<u8"),
                          ("errors", "<u8"), ("status", "<i4"), ("flags", "<u4"), ("run_frames", "<u8"),
                          ("reserved", "<u8", (2,))])
assert OUT_FRAME_DTYPE.itemsize == 32 and SUMMARY_DTYPE.itemsize == 64


def summary(frames=0, payload_bytes=0, payload_len=0, errors=0, status=OK):
    s = np.zeros(1, SUMMARY_DTYPE)[0]
    s["frames"], s["payload_bytes"], s["payload_len"] = frames, payload_bytes, payload_len & M64
    s["errors"], s["status"] = errors, status
    return s


def record(length, opcode=1, fin=1, rsv=0, off=0, masked=0, mask=(0, 0, 0, 0), hdr_length=None):
    """One gevws_out_frame; hdr_length differs from payload_len when given."""
    r = np.zeros(1, OUT_FRAME_DTYPE)[0]
    r["fin"], r["rsv"], r["opcode"], r["masked"], r["mask"] = fin, rsv, opcode, masked, mask
    r["length"] = length if hdr_length is None else hdr_length
    r["payload_off"], r["payload_len"] = off, length
    return r


def splittable(r, F):
    L = int(r["payload_len"])
    return (int(r["fin"]) == 1 and int(r["opcode"]) in (1, 2) and int(r["length"]) >= 0
            and int(r["length"]) == L and L > F)


def count(r, F):
    """(fragments, malformed)."""
    if not splittable(r, F):
        return 1, False
    c = -(-int(r["payload_len"]) // F)
    return (0, True) if c > MAX_FRAGMENTS else (c, False)


def fragments_of(r, F):
    c, bad = count(r, F)
    assert not bad
    if c == 1:
        return [r.copy()]
    L, out = int(r["payload_len"]), []
    for i in range(c):
        o = r.copy()
        n = min(F, L - i * F)
        o["fin"] = 1 if i == c - 1 else 0
        o["rsv"] = r["rsv"] if i == 0 else 0
        o["opcode"] = r["opcode"] if i == 0 else 0
        o["length"], o["payload_len"] = n, n
        o["payload_off"] = (int(r["payload_off"]) + i * F) & M64
        out.append(o)
    return out


def gated(max_records, prev):
    """The records looked at, or None when the gate failed."""
    if prev is None:
        return max_records
    if int(prev["status"]) != OK:
        return None
    return min(int(prev["frames"]), max_records)


def fragment(records, F, max_frags, prev=None, max_records=None):
    """-> (frags or None, first or None, summary): None = not written."""
    assert F >= 1
    records = np.asarray(records, OUT_FRAME_DTYPE).reshape(-1)
    n = gated(len(records) if max_records is None else max_records, prev)
    if n is None:
        return None, None, summary()
    counts = [count(r, F) for r in records[:n]]
    bad = sum(1 for _, b in counts if b)
    if bad:
        return None, None, summary(errors=bad, status=ERR_INVALID)
    total = sum(c for c, _ in counts)
    s = summary(total, sum(1 for c, _ in counts if c > 1), sum(int(r["payload_len"]) for r in records[:n]))
    if total > max_frags:
        s["status"] = ERR_CAPACITY
        return None, None, s
    frags = np.zeros(total, OUT_FRAME_DTYPE)
    first = np.zeros(n + 1, np.uint64)
    at = 0
    for k, r in enumerate(records[:n]):
        first[k] = at
        for o in fragments_of(r, F):
            frags[at] = o
            at += 1
    first[n] = at
    return frags, first, s


def offsets(first, max_records, prev, fragged, frag_off, frag_encoded):
    """-> (reply_off or None, summary)."""
    for g in (prev, fragged, frag_encoded):
        if g is not None and int(g["status"]) != OK:
            need = int(g["payload_bytes"]) if g is frag_encoded and int(g["status"]) == ERR_CAPACITY else 0
            return None, summary(payload_bytes=need, status=int(g["status"]))
    n = gated(max_records, prev)
    first = [int(x) for x in first[: n + 1]]
    frames, enc_frames = int(fragged["frames"]), int(frag_encoded["frames"])
    bad = 0
    for k in range(n + 1):
        wrong = (k == 0 and first[0] != 0) or (k < n and first[k] > first[k + 1]) or \
                (k == n and (first[n] != frames or first[n] != enc_frames))
        bad += bool(wrong)
    if bad:
        return None, summary(errors=bad, status=ERR_INVALID)
    total = int(frag_encoded["payload_bytes"])
    reply_off = np.array([int(frag_off[f]) if f < enc_frames else total for f in first[:n]], np.uint64)
    return reply_off, summary(n, total, int(frag_encoded["payload_len"]))


# The shapes of the step's tests: for each limit the lengths around it, every
# kind of record that must pass through, and the kinds that split.
LIMITS = (1, 2, 16, 17, 125, 126, 65535, 65536)


def lengths_for(F):
    return sorted({0, 1, max(F - 1, 0), F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1, 3 * F + 7})


def shape_records(F, rng):
    """Every record kind of the contract at every length around F, payloads laid out 16-aligned."""
    recs, off = [], 0

    def add(length, **kw):
        nonlocal off
        recs.append(record(length, off=off, **kw))
        off += (length + 15) // 16 * 16

    for L in lengths_for(F):
        add(L, opcode=1)
        add(L, opcode=2)
        add(L, opcode=2, rsv=4)
        add(L, opcode=1, rsv=4, masked=1, mask=tuple(int(x) for x in rng.integers(0, 256, 4)))
        add(L, opcode=9)             # a control record, longer than F for most L: inconsistent, passed through
        add(L, opcode=8, rsv=4)
        add(L, opcode=1, fin=0)      # a fragment already
        add(L, opcode=0)             # a continuation
        add(L, opcode=0, fin=0)
        add(L, opcode=2, hdr_length=L + 1)    # hdr.length != payload_len
        add(L, opcode=1, hdr_length=-1)
    return np.array(recs, OUT_FRAME_DTYPE)


def random_records(n, F, rng, max_len=None):
    """n records, mostly splittable data messages, lengths around multiples of F."""
    max_len = 6 * F if max_len is None else max_len
    recs, off = [], 0
    for _ in range(n):
        kind = int(rng.integers(0, 10))
        L = int(rng.integers(0, max_len + 1))
        if kind < 6:
            r = record(L, opcode=int(rng.integers(1, 3)), rsv=int(rng.choice([0, 4])), off=off)
        elif kind == 6:
            r = record(L, opcode=int(rng.choice([8, 9, 10])), off=off)
        elif kind == 7:
            r = record(L, opcode=int(rng.integers(0, 3)), fin=0, off=off)
        elif kind == 8:
            r = record(L, opcode=1, hdr_length=L + int(rng.integers(1, 5)), off=off)
        else:
            r = record(L, opcode=2, masked=1, mask=tuple(int(x) for x in rng.integers(0, 256, 4)), off=off)
        recs.append(r)
        off += (L + 15) // 16 * 16
    return np.array(recs, OUT_FRAME_DTYPE)
