// gevws_rooms.hip -- the room broadcast (gevws_reply_rooms_async,
// gevws_room_plan_async; include/gevws.h): the room twins of the reply step
// (gevws_join.hip) and of the send plan (gevws_respond.hip).  A delivered body
// goes to every member of its sender's room: it enters the plain list and the
// deflate list once each, whatever the room's size, and the plan names the one
// encoded frame once per recipient.  The reference fans out on the host
// (example/websocket/main.go loops over serv.sessions and sends the same packed
// message to each); it has no room table and no compression.
//
// Both calls check the caller's room tables first (rooms_check, one lane per
// record) and index nothing by them that the check has not bounded.
//
// The reply step, two memsets and five launches, no host round trip:
//   k_rooms_check<true>  the tables; per room the plain-takers, the
//                        deflate-takers and the smallest window (integer
//                        atomics into zeroed scratch: order-independent)
//   k_rr_count / k_scan_blocks / k_rr_verdict / k_rr_emit
//                        the reply step's compaction, into two lists at once
//
// The plan, two memsets and twelve launches:
//   k_rooms_check<false> the tables, slot -> room and connection -> slot
//   k_rp_walk<false>     one lane per connection walks its frames (as
//                        k_ctl_classify does): publications and control
//                        replies, counts and bytes per wire
//   k_rp_orphans         one lane per frame: a frame of no connection that
//                        would send something is malformed
//   k_rp_slots           one lane per member slot of the CSR: its publications
//                        per wire, block partials; the room totals by atomics
//   k_scan_blocks / k_rp_slot_bases
//                        where each slot's publications start in the two
//                        publication lists: the CSR is room-major, so a room's
//                        publications are one contiguous slice
//   k_rp_conns / k_scan_blocks / k_rp_verdict / k_rp_conn_emit
//                        entries per connection (the room's slice, less its own
//                        part when the sender is skipped, plus its control
//                        replies), the summary, CAPACITY, d_conn_send
//   k_rp_walk<true>      the publications and the control replies into their lists
//   k_rp_emit            the hot loop, one lane per output entry: the recipient
//                        by bisection of the connections' first entries, the
//                        rank into the room's slice, 32 bytes read, 32 written
// Nothing but the summary is written before the verdict.  No payload byte is touched.
#include "gevws_internal.hpp"
#include "gevws_roomtabs.hpp"

namespace {

static_assert(sizeof(gevws_send) == 32 && offsetof(gevws_send, frame) == 16 && offsetof(gevws_send, conn) == 24 &&
                  offsetof(gevws_send, wire) == 28, "gevws_send layout");
static_assert(sizeof(gevws_conn_send) == 32 && offsetof(gevws_conn_send, bytes) == 16 &&
                  offsetof(gevws_conn_send, flags) == 24, "gevws_conn_send layout");
static_assert(sizeof(gevws_deflate_msg) == 24 && sizeof(gevws_out_frame) == 32 && sizeof(gevws_body) == 32,
              "list record layouts");

// ctl[]: the call's counters
constexpr int kCtlBadTable = 0;  // malformed table records
constexpr int kCtlRoomed = 1;    // connections with a room
constexpr int kCtlShut = 2;      // (plan) connections with GEVWS_CTL_SHUTDOWN
constexpr int kCtlBadFrame = 3;  // (plan) frames with a malformed index

// KINDS (the reply step): per room the members that take plain, those that
// take deflate, and the smallest effective window of the latter.
template <bool KINDS>
__global__ __launch_bounds__(kWalkBlock) void k_rooms_check(RoomTabs T, Gates G, int skip_all,
                                                            const uint8_t* __restrict__ ext,
                                                            const uint8_t* __restrict__ wbits,
                                                            uint32_t* __restrict__ slot_room,
                                                            uint32_t* __restrict__ conn_slot,
                                                            uint32_t* __restrict__ room_kind,
                                                            uint32_t* __restrict__ room_wb,
                                                            uint64_t* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t bad = 0, roomed = 0;
  if (!skip_all && gate_count(G)) {  // (a call without records reads none of its tables)
    RoomRec r = rooms_check(T, i);
    if (i < T.n_members && r.room != kNoRoom) {
      slot_room[i] = r.room;
      if (r.member != kNoSlot) {
        conn_slot[r.member] = (uint32_t)i;
        if constexpr (KINDS) {
          if (takes_deflate(ext, r.member)) {
            const uint32_t wb = wbits ? wbits[r.member] : 0u;
            if (wb != 0 && (wb < 8 || wb > 15)) {
              bad += !r.member_bad;  // (the slot's record counts once, whatever is wrong with it)
            } else {
              atomicAdd(room_kind + 2 * (uint64_t)r.room + 1, 1u);
              atomicMin(room_wb + r.room, wb ? wb : 15u);
            }
          } else {
            atomicAdd(room_kind + 2 * (uint64_t)r.room, 1u);
          }
        }
      }
    }
    bad += r.bad;
    roomed = r.roomed;
  }
  count_up(ctl + kCtlBadTable, bad);
  count_up(ctl + kCtlRoomed, roomed);
}

// ------------------------------------------------------------------ the reply step
struct RoomDec {
  bool plain, deflate, bad;
  uint32_t room;
};
__device__ __forceinline__ RoomDec rr_decide(const gevws_body& b, int policy, const uint8_t* __restrict__ ext,
                                             const RoomTabs& T, uint32_t flags,
                                             const uint32_t* __restrict__ room_kind) {
  RoomDec r{false, false, false, kNoRoom};
  if (policy == GEVWS_HANDLER_NONE || !(b.flags & GEVWS_BODY_WHOLE)) return r;
  // both lists address one arena: a body left in its frame's slot has no place in them
  if (!(b.flags & (GEVWS_BODY_JOINED | GEVWS_BODY_INFLATED)) || b.conn >= T.n_conns) {
    r.bad = true;
    return r;
  }
  const uint32_t g = T.conn_room[b.conn];
  if (g >= T.n_rooms) return r;  // no room: it publishes nothing (a bad id is the table check's)
  uint32_t np = room_kind[2 * (uint64_t)g], nd = room_kind[2 * (uint64_t)g + 1];
  if (flags & GEVWS_ROOMS_SKIP_SENDER) {
    if (takes_deflate(ext, b.conn)) nd -= nd > 0;
    else np -= np > 0;
  }
  r.plain = np > 0, r.deflate = nd > 0, r.room = g;
  return r;
}

__global__ __launch_bounds__(kWalkBlock) void k_rr_count(const gevws_body* __restrict__ bodies, Gates G, int policy,
                                                         const uint8_t* __restrict__ ext, RoomTabs T, uint32_t flags,
                                                         const uint32_t* __restrict__ room_kind,
                                                         uint64_t* __restrict__ blk) {
  const uint64_t n = gate_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[3] = {0, 0, 0};  // deflate-list entries, plain-list entries, malformed records
  if (m < n) {
    const RoomDec r = rr_decide(bodies[m], policy, ext, T, flags, room_kind);
    vals[0] = r.deflate, vals[1] = r.plain, vals[2] = r.bad;
  }
  block_partial<3>(vals, blk, blockIdx.x);
}

// The scan left {deflate entries, plain entries, malformed bodies} in
// *def_sum's frames / payload_bytes / payload_len: the two summaries from them
// and from the table check's counters.
__global__ void k_rr_verdict(Gates G, int policy, uint32_t n_members, const uint64_t* __restrict__ ctl,
                             gevws_summary* __restrict__ def_sum, gevws_summary* __restrict__ plain_sum) {
  const gevws_summary s = *def_sum;
  gevws_summary a, b;
  memset(&a, 0, sizeof(a));
  memset(&b, 0, sizeof(b));
  if (gate_count(G) && policy != GEVWS_HANDLER_NONE) {
    const uint64_t bad = s.payload_len + ctl[kCtlBadTable] + (ctl[kCtlRoomed] != n_members ? 1u : 0u);
    if (bad) {
      a.errors = b.errors = bad;
      a.status = b.status = GEVWS_ERR_INVALID;
    } else {
      a.frames = s.frames;
      b.frames = s.payload_bytes;
    }
  }
  *def_sum = a;
  *plain_sum = b;
}

__global__ __launch_bounds__(kWalkBlock) void k_rr_emit(
    const gevws_body* __restrict__ bodies, Gates G, int policy, const uint8_t* __restrict__ ext, RoomTabs T,
    uint32_t flags, const uint32_t* __restrict__ room_kind, const uint32_t* __restrict__ room_wb,
    const uint64_t* __restrict__ blk, const gevws_summary* __restrict__ def_sum,
    gevws_deflate_msg* __restrict__ def_msgs, uint32_t* __restrict__ def_conn, gevws_out_frame* __restrict__ plain,
    uint32_t* __restrict__ plain_conn, int64_t* __restrict__ plain_of, int64_t* __restrict__ def_of) {
  if (def_sum->status != GEVWS_OK) return;  // a malformed record: nothing written
  const uint64_t n = gate_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  gevws_body b;
  memset(&b, 0, sizeof(b));
  RoomDec r{false, false, false, kNoRoom};
  if (m < n) {
    b = bodies[m];
    r = rr_decide(b, policy, ext, T, flags, room_kind);
  }
  const uint64_t v[2] = {(uint64_t)r.deflate, (uint64_t)r.plain};
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (m >= n) return;
  const uint8_t op = policy == GEVWS_HANDLER_ECHO_TEXT ? 1 : 2;
  int64_t pi = -1, di = -1;
  if (r.deflate) {
    const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
    const uint32_t wb = room_wb[r.room];
    gevws_deflate_msg d;
    memset(&d, 0, sizeof(d));
    d.payload_off = b.off;
    d.length = b.length;
    d.opcode = op;
    d.window_bits = (uint8_t)(wb <= 15 ? wb : 15u);
    def_msgs[k] = d;
    def_conn[k] = b.conn;
    di = (int64_t)k;
  }
  if (r.plain) {
    const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
    gevws_out_frame o;
    memset(&o, 0, sizeof(o));
    o.hdr.fin = 1;
    o.hdr.opcode = op;
    o.hdr.length = (int64_t)b.length;
    o.payload_off = b.off;
    o.payload_len = b.length;
    plain[k] = o;
    plain_conn[k] = b.conn;
    pi = (int64_t)k;
  }
  plain_of[m] = pi;
  def_of[m] = di;
}

struct RrScratch {
  uint64_t* ctl;
  uint64_t* blk;        // [nblk][kBlkFields]
  uint32_t* room_kind;  // [g][2]: plain-takers, deflate-takers
  uint32_t* room_wb;    // [g] the deflate-takers' smallest window (all ones: none)
  uint32_t* slot_room;  // [k]
  uint32_t* conn_slot;  // [c]
  size_t zero_bytes, ones_off, ones_bytes, total;
};
inline RrScratch rr_scratch(void* base, uint32_t nblk, uint32_t n_rooms, uint32_t n_members, uint32_t n_conns) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  RrScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t));
  s.room_kind = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_rooms * 8 + 8);
  s.zero_bytes = o;
  s.ones_off = o;
  s.room_wb = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_rooms * 4 + 4);
  s.slot_room = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_members * 4 + 4);
  s.conn_slot = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_conns * 4 + 4);
  s.ones_bytes = o - s.ones_off;
  s.total = o;
  return s;
}

// ------------------------------------------------------------------ the plan
struct RpIn {
  uint64_t max_frames, max_messages;
  const gevws_summary* __restrict__ msg_sum;
  const gevws_summary* __restrict__ enc0;  // the plain wire's encode summary, its table below
  const gevws_summary* __restrict__ enc1;  // the deflated wire's
  const gevws_summary* __restrict__ enc2;  // the control wire's
  const uint64_t* __restrict__ off0;
  const uint64_t* __restrict__ off1;
  const uint64_t* __restrict__ off2;
  const int64_t* __restrict__ msg_of;
  const uint64_t* __restrict__ msg_end;
  const int64_t* __restrict__ plain_of;
  const int64_t* __restrict__ def_of;
  const int64_t* __restrict__ ctl_of;
  const uint8_t* __restrict__ conn_ext;  // may be null
  uint32_t flags;
};

// Reply idx of wire w as a byte range of that wire, as the send plan takes it;
// false: an index outside its list, or a table that decreases.
__device__ __forceinline__ bool rp_range(const RpIn& p, uint32_t w, uint64_t idx, uint64_t& off, uint64_t& len) {
  const gevws_summary* __restrict__ enc = w == 0 ? p.enc0 : (w == 1 ? p.enc1 : p.enc2);
  const uint64_t* __restrict__ tab = w == 0 ? p.off0 : (w == 1 ? p.off1 : p.off2);
  const uint64_t cnt = enc->frames, total = enc->payload_bytes;
  if (idx >= cnt) return false;
  off = tab[idx];
  const uint64_t next = idx + 1 < cnt ? tab[idx + 1] : total;
  if (next < off) return false;
  len = next - off;
  return true;
}

struct RpConn {  // what a connection's frames yield, per wire (2: its control replies)
  uint64_t n[3], b[3];
};

struct RpScratch {
  uint64_t* ctl;
  uint64_t* blk_s;      // [nblks][kBlkFields]: a slot's publications in wire 0, in wire 1
  uint64_t* blk_c;      // [nblkc][kBlkFields]: a connection's entries, control replies, bytes
  uint64_t* room_tot;   // [g][4]: the room's publications in wire 0 / 1, their bytes
  gevws_summary* sum_s; // the slot scan's summary (not used)
  uint32_t* slot_room;  // [k]
  uint32_t* conn_slot;  // [c]
  uint32_t* fconn;      // [f] the connection whose walk passed frame f (kNoSlot: none)
  RpConn* cc;           // [c]
  uint64_t* sbase0;     // [k] where slot k's wire-0 publications start; [n_members] all of them
  uint64_t* sbase1;
  uint64_t* cfirst;     // [c] the connection's first entry; [n_conns] all of them
  uint64_t* cbase2;     // [c] where its control replies start in the control list
  gevws_send* pub0;     // [max_frames] the publications, room-major
  gevws_send* pub1;
  gevws_send* ctl_list; // [max_frames] the control replies, by connection
  size_t zero_bytes, ones_off, ones_bytes, total;
};
inline RpScratch rp_scratch(void* base, uint64_t max_frames, uint32_t nblks, uint32_t nblkc, uint32_t n_rooms,
                            uint32_t n_members, uint32_t n_conns) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  RpScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk_s = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblks * kBlkFields * sizeof(uint64_t) + 8);
  s.blk_c = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblkc * kBlkFields * sizeof(uint64_t) + 8);
  s.room_tot = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)n_rooms * 32 + 8);
  s.sum_s = reinterpret_cast<gevws_summary*>(p + o), o += 256;
  s.zero_bytes = o;
  s.ones_off = o;
  s.slot_room = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_members * 4 + 4);
  s.conn_slot = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_conns * 4 + 4);
  s.fconn = reinterpret_cast<uint32_t*>(p + o), o += up(max_frames * 4);
  s.ones_bytes = o - s.ones_off;
  s.cc =reinterpret_cast<RpConn*>(p + o), o += up((size_t)n_conns * sizeof(RpConn));
  s.sbase0 = reinterpret_cast<uint64_t*>(p + o), o += up(((size_t)n_members + 1) * 8);
  s.sbase1 = reinterpret_cast<uint64_t*>(p + o), o += up(((size_t)n_members + 1) * 8);
  s.cfirst = reinterpret_cast<uint64_t*>(p + o), o += up(((size_t)n_conns + 1) * 8);
  s.cbase2 = reinterpret_cast<uint64_t*>(p + o), o += up(((size_t)n_conns + 1) * 8);
  s.pub0 = reinterpret_cast<gevws_send*>(p + o), o += up(max_frames * sizeof(gevws_send));
  s.pub1 = reinterpret_cast<gevws_send*>(p + o), o += up(max_frames * sizeof(gevws_send));
  s.ctl_list = reinterpret_cast<gevws_send*>(p + o), o += up(max_frames * sizeof(gevws_send));
  s.total = o;
  return s;
}

// One lane per connection walks its frames in stream order.  A frame yields
// its control reply, else -- when it ends a message and its connection has a
// room -- a publication in each wire whose list holds the message.  EMIT false:
// the counts into cc[c], the malformed frames and the shutdowns counted;
// EMIT true (behind the verdict): the records into the three lists.
template <bool EMIT>
__global__ __launch_bounds__(kWalkBlock) void k_rp_walk(
    RpIn p, Gates G, RoomTabs T, const gevws_conn_out* __restrict__ cout, const gevws_conn_ctl* __restrict__ conn_ctl,
    const uint32_t* __restrict__ conn_slot, uint32_t* __restrict__ fconn, RpConn* __restrict__ cc,
    const uint64_t* __restrict__ sbase0, const uint64_t* __restrict__ sbase1, const uint64_t* __restrict__ cbase2,
    gevws_send* __restrict__ pub0,
    gevws_send* __restrict__ pub1, gevws_send* __restrict__ ctl_list, const gevws_summary* __restrict__ sum,
    uint64_t* __restrict__ ctl) {
  if (EMIT && sum->status != GEVWS_OK) return;
  const uint64_t n = gate_count(G);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t shut = 0, bad = 0;
  if (n && c < T.n_conns) {
    const uint64_t nm = gated_count(p.max_messages, p.msg_sum);
    const gevws_conn_out co = cout[c];
    const uint64_t lo = co.first_frame < n ? co.first_frame : n;
    const uint64_t hi = co.nframes < n - lo ? lo + co.nframes : n;
    const bool roomed = T.conn_room[c] < T.n_rooms;
    RpConn w;
    memset(&w, 0, sizeof(w));
    uint64_t at[3] = {0, 0, 0};  // EMIT: where this connection's next record of each list goes
    if constexpr (EMIT) {
      const uint32_t k = roomed ? conn_slot[c] : kNoSlot;
      at[0] = k < T.n_members ? sbase0[k] : p.max_frames;  // (past the lists: never written)
      at[1] = k < T.n_members ? sbase1[k] : p.max_frames;
      at[2] = cbase2[c];
    }
    auto take = [&](uint32_t wire, uint64_t idx, uint64_t f) -> bool {
      uint64_t off, len;
      if (!rp_range(p, wire, idx, off, len)) return false;
      if constexpr (EMIT) {
        gevws_send* __restrict__ list = wire == 0 ? pub0 : (wire == 1 ? pub1 : ctl_list);
        const uint64_t i = at[wire] + w.n[wire];
        if (i < p.max_frames) {
          gevws_send o;
          o.off = off, o.len = len, o.frame = f, o.conn = c, o.wire = wire;
          list[i] = o;
        }
      }
      w.n[wire] += 1, w.b[wire] += len;
      return true;
    };
    for (uint64_t f = lo; f < hi; ++f) {  // (bounded by the decode's count)
      if constexpr (!EMIT) fconn[f] = c;
      const int64_t k = p.ctl_of[f];
      if (k >= 0) {
        if (!take(2, (uint64_t)k, f)) ++bad;
        continue;
      }
      const int64_t m = p.msg_of[f];
      if (m < 0) continue;
      if ((uint64_t)m >= nm) {
        ++bad;
        continue;
      }
      if (p.msg_end[m] != f || !roomed) continue;
      const int64_t p0 = p.plain_of[m], p1 = p.def_of[m];
      bool ok = true;
      if (p0 >= 0) ok &= take(0, (uint64_t)p0, f);
      if (p1 >= 0) ok &= take(1, (uint64_t)p1, f);
      if (!ok) ++bad;
    }
    if constexpr (!EMIT) {
      cc[c] = w;
      shut = (conn_ctl[c].flags & GEVWS_CTL_SHUTDOWN) ? 1 : 0;
    }
  }
  if constexpr (!EMIT) {
    count_up(ctl + kCtlShut, shut);
    count_up(ctl + kCtlBadFrame, bad);
  }
}

// One lane per frame: a frame that no connection's walk passed and that would
// send something -- a control reply, or the end of a message that is in a list
// -- belongs to no connection: malformed, as in the send plan.
__global__ __launch_bounds__(kWalkBlock) void k_rp_orphans(RpIn p, Gates G, const uint32_t* __restrict__ fconn,
                                                           uint64_t* __restrict__ ctl) {
  const uint64_t n = gate_count(G);
  const uint64_t f = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t bad = 0;
  if (f < n && fconn[f] == kNoSlot) {
    if (p.ctl_of[f] >= 0) {
      bad = 1;
    } else {
      const int64_t m = p.msg_of[f];
      if (m >= 0) {
        if ((uint64_t)m >= gated_count(p.max_messages, p.msg_sum)) bad = 1;
        else if (p.msg_end[m] == f && (p.plain_of[m] >= 0 || p.def_of[m] >= 0)) bad = 1;
      }
    }
  }
  count_up(ctl + kCtlBadFrame, bad);
}

// Member slot k's publications per wire: {n0, n1} (none for a slot whose
// record the check refused: the verdict is INVALID then).
__device__ __forceinline__ void rp_slot(const RoomTabs& T, const RpConn* __restrict__ cc, uint64_t k, uint64_t (&v)[2],
                                        uint64_t (&b)[2]) {
  v[0] = v[1] = b[0] = b[1] = 0;
  if (k >= T.n_members) return;
  const uint32_t m = T.members[k];
  if (m >= T.n_conns) return;
  const RpConn w = cc[m];
  v[0] = w.n[0], v[1] = w.n[1], b[0] = w.b[0], b[1] = w.b[1];
}

__global__ __launch_bounds__(kWalkBlock) void k_rp_slots(Gates G, RoomTabs T, const RpConn* __restrict__ cc,
                                                         const uint32_t* __restrict__ slot_room,
                                                         uint64_t* __restrict__ room_tot, uint64_t* __restrict__ blk) {
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t v[2] = {0, 0}, b[2] = {0, 0};
  if (gate_count(G) && k < T.n_members) {
    rp_slot(T, cc, k, v, b);
    const uint32_t g = slot_room[k];
    if (g < T.n_rooms) {
      unsigned long long* t = reinterpret_cast<unsigned long long*>(room_tot + 4 * (uint64_t)g);
      if (v[0]) atomicAdd(t + 0, (unsigned long long)v[0]), atomicAdd(t + 2, (unsigned long long)b[0]);
      if (v[1]) atomicAdd(t + 1, (unsigned long long)v[1]), atomicAdd(t + 3, (unsigned long long)b[1]);
    }
  }
  block_partial<2>(v, blk, blockIdx.x);
}

__global__ __launch_bounds__(kWalkBlock) void k_rp_slot_bases(Gates G, RoomTabs T, const RpConn* __restrict__ cc,
                                                              const uint64_t* __restrict__ blk,
                                                              uint64_t* __restrict__ sbase0,
                                                              uint64_t* __restrict__ sbase1) {
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t v[2] = {0, 0}, b[2];
  const bool live = gate_count(G) != 0;
  if (live) rp_slot(T, cc, k, v, b);
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (!live || k >= T.n_members) return;
  const uint64_t b0 = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
  const uint64_t b1 = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
  sbase0[k] = b0, sbase1[k] = b1;
  if (k == (uint64_t)T.n_members - 1) sbase0[T.n_members] = b0 + v[0], sbase1[T.n_members] = b1 + v[1];
}

// Connection c's entries: its room's publications in the wire it takes, less
// its own when the sender is skipped, plus its control replies.
struct RpEntries {
  uint64_t count, ctl, bytes;
};
__device__ __forceinline__ RpEntries rp_entries(const RpIn& p, const RoomTabs& T, const RpConn* __restrict__ cc,
                                                const uint64_t* __restrict__ room_tot, uint32_t c) {
  const RpConn w = cc[c];
  RpEntries e{w.n[2], w.n[2], w.b[2]};
  const uint32_t g = T.conn_room[c];
  if (g < T.n_rooms) {
    const uint32_t wire = takes_deflate(p.conn_ext, c) ? 1u : 0u;
    uint64_t cnt = room_tot[4 * (uint64_t)g + wire], bytes = room_tot[4 * (uint64_t)g + 2 + wire];
    if (p.flags & GEVWS_ROOMS_SKIP_SENDER) {  // (its own are part of the room's: never below zero on checked tables)
      cnt -= w.n[wire] < cnt ? w.n[wire] : cnt;
      bytes -= w.b[wire] < bytes ? w.b[wire] : bytes;
    }
    e.count += cnt, e.bytes += bytes;
  }
  return e;
}

__global__ __launch_bounds__(kWalkBlock) void k_rp_conns(RpIn p, Gates G, RoomTabs T, const RpConn* __restrict__ cc,
                                                         const uint64_t* __restrict__ room_tot,
                                                         uint64_t* __restrict__ blk) {
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[3] = {0, 0, 0};  // entries, control replies, bytes
  if (gate_count(G) && c < T.n_conns) {
    const RpEntries e = rp_entries(p, T, cc, room_tot, c);
    vals[0] = e.count, vals[1] = e.ctl, vals[2] = e.bytes;
  }
  block_partial<3>(vals, blk, blockIdx.x);
}

// The scan left {entries, control replies, bytes} in *sum's frames /
// payload_bytes / payload_len, and CAPACITY against max_sends: the summary from
// them and from the counters.
__global__ void k_rp_verdict(Gates G, uint32_t n_members, const uint64_t* __restrict__ ctl,
                             gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  if (gate_count(G)) {
    const uint64_t bad = ctl[kCtlBadTable] + (ctl[kCtlRoomed] != n_members ? 1u : 0u) + ctl[kCtlBadFrame];
    if (bad) {
      o.errors = bad;
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = s.frames;
      o.payload_bytes = s.payload_len;
      o.errors = ctl[kCtlShut];
      o.status = s.status;
    }
  }
  *sum = o;
}

__global__ __launch_bounds__(kWalkBlock) void k_rp_conn_emit(RpIn p, Gates G, RoomTabs T,
                                                             const RpConn* __restrict__ cc,
                                                             const uint64_t* __restrict__ room_tot,
                                                             const gevws_conn_ctl* __restrict__ conn_ctl,
                                                             const uint64_t* __restrict__ blk,
                                                             const gevws_summary* __restrict__ sum,
                                                             uint64_t* __restrict__ cfirst,
                                                             uint64_t* __restrict__ cbase2,
                                                             gevws_conn_send* __restrict__ conn_send) {
  if (sum->status != GEVWS_OK) return;  // more entries than max_sends, or a malformed record: nothing written
  const bool live = gate_count(G) != 0;
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  RpEntries e{0, 0, 0};
  if (live && c < T.n_conns) e = rp_entries(p, T, cc, room_tot, c);
  const uint64_t v[2] = {e.count, e.ctl};
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (!live || c >= T.n_conns) return;
  const uint64_t first = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
  cfirst[c] = first;
  cbase2[c] = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
  if (c == T.n_conns - 1) cfirst[T.n_conns] = first + e.count;
  gevws_conn_send o;
  memset(&o, 0, sizeof(o));
  o.first = first;
  o.count = e.count;
  o.bytes = e.bytes;
  o.flags = conn_ctl[c].flags;
  conn_send[c] = o;
}

// The hot loop, one lane per output entry: 32 bytes read, 32 written.
__global__ __launch_bounds__(kWalkBlock) void k_rp_emit(RpIn p, Gates G, RoomTabs T, uint64_t max_sends,
                                                        const uint32_t* __restrict__ conn_slot,
                                                        const uint64_t* __restrict__ sbase0,
                                                        const uint64_t* __restrict__ sbase1,
                                                        const uint64_t* __restrict__ cfirst,
                                                        const uint64_t* __restrict__ cbase2,
                                                        const gevws_send* __restrict__ pub0,
                                                        const gevws_send* __restrict__ pub1,
                                                        const gevws_send* __restrict__ ctl_list,
                                                        const gevws_summary* __restrict__ sum,
                                                        gevws_send* __restrict__ send) {
  if (sum->status != GEVWS_OK || !gate_count(G)) return;
  const uint64_t total = sum->frames < max_sends ? sum->frames : max_sends;
  const uint64_t e = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (e >= total) return;
  // the recipient: the last connection whose first entry is at or before e (those before it there are empty)
  uint32_t lo = 0, hi = T.n_conns - 1;
  while (lo < hi) {  // (at most 32 rounds)
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (cfirst[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t c = lo;
  const uint64_t rank = e - cfirst[c];
  const uint32_t g = T.conn_room[c];
  uint64_t npub = 0;
  if (g < T.n_rooms) {
    const uint32_t wire = takes_deflate(p.conn_ext, c) ? 1u : 0u;
    const uint64_t* __restrict__ sb = wire ? sbase1 : sbase0;
    const uint64_t a = sb[T.first[g]], b = sb[T.first[g + 1]];
    uint64_t oa = b, own = 0;
    if (p.flags & GEVWS_ROOMS_SKIP_SENDER) {
      const uint32_t k = conn_slot[c];
      if (k < T.n_members) oa = sb[k], own = sb[k + 1] - oa;
    }
    npub = (b - a) - own;
    if (rank < npub) {
      uint64_t idx = a + rank;
      if (idx >= oa) idx += own;  // past the recipient's own publications
      if (idx >= p.max_frames) return;
      gevws_send o = (wire ? pub1 : pub0)[idx];
      o.conn = c;
      send[e] = o;
      return;
    }
  }
  const uint64_t idx = cbase2[c] + (rank - npub);
  if (idx >= p.max_frames) return;
  send[e] = ctl_list[idx];
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_reply_rooms_async(gevws_ctx* ctx, void* stream, const gevws_body* d_bodies,
                                       uint64_t max_messages, const gevws_summary* d_msg_summary,
                                       const gevws_summary* d_join_summary, int policy, const uint8_t* d_conn_ext,
                                       const uint8_t* d_conn_window_bits, uint32_t n_conns,
                                       const uint32_t* d_conn_room, const uint32_t* d_room_first,
                                       const uint32_t* d_room_members, uint32_t n_rooms, uint32_t n_members,
                                       uint32_t flags, gevws_deflate_msg* d_def_msgs, uint32_t* d_def_conn,
                                       gevws_summary* d_def_summary, gevws_out_frame* d_plain,
                                       uint32_t* d_plain_conn, gevws_summary* d_plain_summary, int64_t* d_plain_of,
                                       int64_t* d_def_of) {
  if (flags & ~GEVWS_ROOMS_SKIP_SENDER) return GEVWS_ERR_INVALID;
  if (!ctx || !d_def_summary || !d_plain_summary || max_messages > 0x7FFFFFFFull * kWalkBlock ||
      (policy != GEVWS_HANDLER_NONE && policy != GEVWS_HANDLER_ECHO_BINARY && policy != GEVWS_HANDLER_ECHO_TEXT))
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (max_messages == 0) {
    GEVWS_HIP(hipMemsetAsync(d_def_summary, 0, sizeof(gevws_summary), st));
    GEVWS_HIP(hipMemsetAsync(d_plain_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_bodies || !d_msg_summary || !d_join_summary || !d_def_msgs || !d_def_conn || !d_plain || !d_plain_conn ||
      !d_plain_of || !d_def_of || !d_room_first || (n_conns && !d_conn_room) || (n_members && !d_room_members))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_messages + kWalkBlock - 1) / kWalkBlock);
  uint64_t recs = (uint64_t)n_rooms + 1;
  if (n_members > recs) recs = n_members;
  if (n_conns > recs) recs = n_conns;
  const uint32_t nblkt = (uint32_t)((recs + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, rr_scratch(nullptr, nblk, n_rooms, n_members, n_conns).total);
  if (r != GEVWS_OK) return r;
  const RrScratch s = rr_scratch(ctx->scratch, nblk, n_rooms, n_members, n_conns);
  const RoomTabs T{d_conn_room, d_room_first, d_room_members, n_rooms, n_members, n_conns};
  const Gates G{{d_join_summary, nullptr, nullptr, nullptr, nullptr, nullptr}, d_msg_summary, max_messages};
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  GEVWS_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(ctx->scratch) + s.ones_off, 0xFF, s.ones_bytes, st));
  k_rooms_check<true><<<nblkt, kWalkBlock, 0, st>>>(T, G, policy == GEVWS_HANDLER_NONE, d_conn_ext,
                                                    d_conn_window_bits, s.slot_room, s.conn_slot, s.room_kind,
                                                    s.room_wb, s.ctl);
  k_rr_count<<<nblk, kWalkBlock, 0, st>>>(d_bodies, G, policy, d_conn_ext, T, flags, s.room_kind, s.blk);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk, UINT64_MAX, UINT64_MAX, d_def_summary);
  k_rr_verdict<<<1, 1, 0, st>>>(G, policy, n_members, s.ctl, d_def_summary, d_plain_summary);
  k_rr_emit<<<nblk, kWalkBlock, 0, st>>>(d_bodies, G, policy, d_conn_ext, T, flags, s.room_kind, s.room_wb, s.blk,
                                         d_def_summary, d_def_msgs, d_def_conn, d_plain, d_plain_conn, d_plain_of,
                                         d_def_of);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_room_plan_async(gevws_ctx* ctx, void* stream, uint64_t max_frames,
                                     const gevws_summary* d_decoded, const gevws_conn_out* d_conn_out,
                                     uint32_t n_conns, const int64_t* d_msg_of, const uint64_t* d_msg_end,
                                     const int64_t* d_plain_of, const int64_t* d_def_of, uint64_t max_messages,
                                     const gevws_summary* d_msg_summary, const gevws_summary* d_join_summary,
                                     const uint8_t* d_conn_ext, const int64_t* d_ctl_of,
                                     const gevws_conn_ctl* d_conn_ctl, const gevws_summary* d_ctl_summary,
                                     const uint64_t* d_plain_off, const gevws_summary* d_plain_encoded,
                                     const uint64_t* d_def_off, const gevws_summary* d_def_encoded,
                                     const uint64_t* d_ctl_off, const gevws_summary* d_ctl_encoded,
                                     const uint32_t* d_conn_room, const uint32_t* d_room_first,
                                     const uint32_t* d_room_members, uint32_t n_rooms, uint32_t n_members,
                                     uint32_t flags, gevws_send* d_send, uint64_t max_sends,
                                     gevws_conn_send* d_conn_send, gevws_summary* d_summary) {
  if ((flags & ~GEVWS_ROOMS_SKIP_SENDER) || max_sends > 0xFFFFFFFFull) return GEVWS_ERR_INVALID;
  if (!ctx || !d_summary || max_frames > 0xFFFFFFFFull || max_messages > 0xFFFFFFFFull) return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (n_conns == 0 || max_frames == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_decoded || !d_conn_out || !d_msg_of || !d_msg_summary || !d_join_summary || !d_ctl_of || !d_conn_ctl ||
      !d_ctl_summary || !d_plain_off || !d_plain_encoded || !d_def_off || !d_def_encoded || !d_ctl_off ||
      !d_ctl_encoded || !d_conn_send || (max_sends && !d_send) ||
      (max_messages && (!d_msg_end || !d_plain_of || !d_def_of)) || !d_conn_room || !d_room_first ||
      (n_members && !d_room_members))
    return GEVWS_ERR_INVALID;
  uint64_t recs = (uint64_t)n_rooms + 1;
  if (n_members > recs) recs = n_members;
  if (n_conns > recs) recs = n_conns;
  const uint32_t nblkt = (uint32_t)((recs + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkc = (n_conns + kWalkBlock - 1) / kWalkBlock;
  const uint32_t nblks = (uint32_t)(((uint64_t)n_members + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblke = (uint32_t)((max_sends + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkf = (uint32_t)((max_frames + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, rp_scratch(nullptr, max_frames, nblks, nblkc, n_rooms, n_members, n_conns).total);
  if (r != GEVWS_OK) return r;
  const RpScratch s = rp_scratch(ctx->scratch, max_frames, nblks, nblkc, n_rooms, n_members, n_conns);
  const RoomTabs T{d_conn_room, d_room_first, d_room_members, n_rooms, n_members, n_conns};
  const Gates G{{d_msg_summary, d_join_summary, d_ctl_summary, d_plain_encoded, d_def_encoded, d_ctl_encoded},
                d_decoded,
                max_frames};
  const RpIn p{max_frames,  max_messages, d_msg_summary, d_plain_encoded, d_def_encoded, d_ctl_encoded,
               d_plain_off, d_def_off,    d_ctl_off,     d_msg_of,        d_msg_end,     d_plain_of,
               d_def_of,    d_ctl_of,     d_conn_ext,    flags};
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  GEVWS_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(ctx->scratch) + s.ones_off, 0xFF, s.ones_bytes, st));
  k_rooms_check<false><<<nblkt, kWalkBlock, 0, st>>>(T, G, 0, d_conn_ext, nullptr, s.slot_room, s.conn_slot, nullptr,
                                                     nullptr, s.ctl);
  k_rp_walk<false><<<nblkc, kWalkBlock, 0, st>>>(p, G, T, d_conn_out, d_conn_ctl, s.conn_slot, s.fconn, s.cc,
                                                 s.sbase0, s.sbase1, s.cbase2, s.pub0, s.pub1, s.ctl_list, d_summary,
                                                 s.ctl);
  k_rp_orphans<<<nblkf, kWalkBlock, 0, st>>>(p, G, s.fconn, s.ctl);
  if (nblks) {
    k_rp_slots<<<nblks, kWalkBlock, 0, st>>>(G, T, s.cc, s.slot_room, s.room_tot, s.blk_s);
    k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk_s, nblks, UINT64_MAX, UINT64_MAX, s.sum_s);
    k_rp_slot_bases<<<nblks, kWalkBlock, 0, st>>>(G, T, s.cc, s.blk_s, s.sbase0, s.sbase1);
  }
  k_rp_conns<<<nblkc, kWalkBlock, 0, st>>>(p, G, T, s.cc, s.room_tot, s.blk_c);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk_c, nblkc, max_sends, UINT64_MAX, d_summary);
  k_rp_verdict<<<1, 1, 0, st>>>(G, n_members, s.ctl, d_summary);
  k_rp_conn_emit<<<nblkc, kWalkBlock, 0, st>>>(p, G, T, s.cc, s.room_tot, d_conn_ctl, s.blk_c, d_summary, s.cfirst,
                                               s.cbase2, d_conn_send);
  k_rp_walk<true><<<nblkc, kWalkBlock, 0, st>>>(p, G, T, d_conn_out, d_conn_ctl, s.conn_slot, s.fconn, s.cc,
                                                s.sbase0, s.sbase1, s.cbase2, s.pub0, s.pub1, s.ctl_list, d_summary,
                                                s.ctl);
  if (nblke)
    k_rp_emit<<<nblke, kWalkBlock, 0, st>>>(p, G, T, max_sends, s.conn_slot, s.sbase0, s.sbase1, s.cfirst, s.cbase2,
                                            s.pub0, s.pub1, s.ctl_list, d_summary, d_send);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
