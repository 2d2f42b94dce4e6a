// gevws_respond.hip -- the last two steps of the message chain
// (gevws_control_async, gevws_send_plan_async; include/gevws.h): the control
// replies and the close of a failed connection, and the order in which a
// connection's reply bytes leave.  The reference answers control frames frame
// by frame (HandlerWrap.OnMessage, plugins/websocket/wrap.go:38-90; the reply
// itself is gevws_dispatch.hpp's, shared with the frame-level dispatch) and
// has no code for a failed connection: it knows nothing of messages.
//
// The control step, behind the join and before the reply step: two memsets,
// six launches, no host round trip:
//   k_ctl_classify  one lane per connection walks its frames, four requests
//                   at a time (d_msg_of and the record's header): the cut, the
//                   close code, one class byte per frame, each message's last
//                   data frame; malformed tables and shutdowns are counted
//   k_ctl_count     one lane per frame: replies and aux slots, block partials
//   k_scan_blocks   block bases, the summary, CAPACITY
//   k_ctl_verdict   one lane: the gates, INVALID, the shutdown count
//   k_ctl_emit      one lane per frame: d_ctl, d_ctl_conn, d_ctl_of, the close
//                   bodies in their aux slots
//   k_ctl_tables    one lane per connection and per message: d_conn_ctl,
//                   d_msg_end, and the bodies behind the cut stripped in place
// Nothing but the summary is written before the verdict.
//
// The send plan, behind the three encodes: an order-preserving compaction of
// the frames that trigger a reply (records are ordered by connection, then
// stream order, so that is the send order):
//   k_plan_conns    one lane per connection: the frame -> connection map,
//                   connections shut down
//   k_plan_count / k_scan_blocks / k_plan_verdict / k_plan_emit
//                   entries and bytes, the summary, d_send and every frame's
//                   exclusive prefix
//   k_plan_conn_emit  one lane per connection: d_conn_send from the prefixes
// No payload byte is touched but a close frame's body (<= 125 bytes).
#include "gevws_internal.hpp"
#include "gevws_dispatch.hpp"

namespace {

static_assert(sizeof(gevws_conn_ctl) == 32 && offsetof(gevws_conn_ctl, close_code) == 8 &&
                  offsetof(gevws_conn_ctl, flags) == 12, "gevws_conn_ctl layout");
static_assert(sizeof(gevws_send) == 32 && offsetof(gevws_send, frame) == 16 && offsetof(gevws_send, conn) == 24 &&
                  offsetof(gevws_send, wire) == 28, "gevws_send layout");
static_assert(sizeof(gevws_conn_send) == 32 && offsetof(gevws_conn_send, bytes) == 16 &&
                  offsetof(gevws_conn_send, flags) == 24, "gevws_conn_send layout");
static_assert(GEVWS_AUX_SLOT == kAuxSlot, "one close body per aux slot");

// cls[f]: disp_kind's kinds, and the close this side sends for a failed connection
constexpr uint8_t kCtlNone = 0, kCtlPayload = 1, kCtlCloseBody = 2, kCtlCloseBare = 3, kCtlFail = 4;
constexpr int kCtlWalkBatch = 4;  // frames a connection's lane requests at once (as k_msg_classify)
constexpr uint32_t kNoConn = 0xFFFFFFFFu;

struct CtlConn {  // per-connection hand-off between the passes
  uint64_t cut;
  uint32_t code, flags;
};

struct CtlScratch {
  uint64_t* ctl;     // [0] connections shut down, [1] malformed tables
  uint64_t* blk;     // [nblk][kBlkFields]: replies, aux slots
  uint8_t* cls;      // [f]
  uint64_t* mend;    // [m] the message's last data frame in this batch (UINT64_MAX: none seen)
  uint32_t* mconn;   // [m] the connection whose walk saw it (kNoConn: none)
  uint32_t* fconn;   // [f] the connection of a frame with cls != 0
  CtlConn* work;     // [c]
  size_t zero_bytes, ones_off, ones_bytes, total;
};
inline CtlScratch ctl_scratch(void* base, uint64_t max_frames, uint64_t max_messages, uint32_t n_conns, uint32_t nblk) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  CtlScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t));
  s.cls = p + o, o += up(max_frames);
  s.zero_bytes = o;
  s.ones_off = o;
  s.mend = reinterpret_cast<uint64_t*>(p + o), o += up(max_messages * 8);
  s.mconn = reinterpret_cast<uint32_t*>(p + o), o += up(max_messages * 4);
  s.ones_bytes = o - s.ones_off;
  s.fconn = reinterpret_cast<uint32_t*>(p + o), o += up(max_frames * 4);
  s.work = reinterpret_cast<CtlConn*>(p + o), o += up((size_t)n_conns * sizeof(CtlConn));
  s.total = o;
  return s;
}

// The wave's sum of a per-connection count -> one atomic on the call's counter.
__device__ __forceinline__ void count_up(uint64_t* __restrict__ counter, uint64_t v) {
  const uint64_t sm = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && sm) atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)sm);
}

// ------------------------------------------------------------------ the control step
// The frames of the call: the decode's count, none when the message pass or the join failed.
__device__ __forceinline__ uint64_t ctl_frames(uint64_t max_frames, const gevws_summary* __restrict__ dec,
                                               const gevws_summary* __restrict__ msg_sum,
                                               const gevws_summary* __restrict__ join_sum) {
  if (msg_sum->status != GEVWS_OK || join_sum->status != GEVWS_OK) return 0;
  return gated_count(max_frames, dec);
}

__device__ __forceinline__ uint32_t close_code_of(uint32_t status) {
  if (status == GEVWS_MSG_ERR_UTF8 || status == GEVWS_MSG_ERR_DEFLATE) return 1007;  // invalid payload data
  if (status == GEVWS_MSG_ERR_TOO_BIG) return 1009;                                   // message too big
  return 1002;                                                                        // protocol error
}

__global__ __launch_bounds__(kWalkBlock) void k_ctl_classify(
    const gevws_frame* __restrict__ fr, uint64_t max_frames, const gevws_conn_out* __restrict__ cout, uint32_t n_conns,
    const gevws_summary* __restrict__ dec, const int64_t* __restrict__ msg_of, uint64_t max_messages,
    const gevws_conn_msg* __restrict__ conn_msg, const gevws_summary* __restrict__ msg_sum,
    const gevws_body* __restrict__ bodies, const gevws_summary* __restrict__ join_sum, uint32_t flags,
    uint8_t* __restrict__ cls, uint32_t* __restrict__ fconn, uint64_t* __restrict__ mend, uint32_t* __restrict__ mconn,
    CtlConn* __restrict__ work, uint64_t* __restrict__ ctl) {
  const uint64_t n = ctl_frames(max_frames, dec, msg_sum, join_sum);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t shut = 0, bad = 0;
  if (n && c < n_conns) {  // (a call without frames reads none of its inputs)
    const uint64_t nm = gated_count(max_messages, msg_sum);
    CtlConn w{UINT64_MAX, 0u, 0u};
    const gevws_conn_out co = cout[c];
    const gevws_conn_msg cm = conn_msg[c];
    const uint64_t first = co.first_frame;
    const uint64_t end = first < n ? (co.nframes < n - first ? first + co.nframes : n) : first;
    const bool came_failed = cm.error != 0 && cm.error_frame == UINT64_MAX;
    if (co.status == GEVWS_OK && end > first && !came_failed) {
      uint64_t errf = UINT64_MAX;  // cut (b)
      if (cm.error >= GEVWS_MSG_ERR_RSV && cm.error <= GEVWS_MSG_ERR_UTF8) {
        if (cm.error_frame < first || cm.error_frame >= end) bad = 1;  // never an index (k_ctl_verdict)
        else errf = cm.error_frame;
      }
      if (!bad) {
        // frames behind the failing frame belong to no message and lie behind the cut
        const uint64_t stop = errf != UINT64_MAX ? errf + 1 : end;
        uint64_t close_f = UINT64_MAX, fail_f = UINT64_MAX;  // cuts (a) and (c)
        uint32_t fail_st = 0;
        int64_t cur = -1;  // the message whose data frames are being passed
        uint64_t cur_last = 0;
        uint32_t cur_st = 0;
        auto finish = [&]() {
          if (cur < 0) return;
          mend[cur] = cur_last;
          if (cur_st != GEVWS_MSG_OK && fail_f == UINT64_MAX) fail_f = cur_last, fail_st = cur_st;
        };
        for (uint64_t f0 = first; f0 < stop && !bad; f0 += kCtlWalkBatch) {
          gevws_header hb[kCtlWalkBatch];
          int64_t mo[kCtlWalkBatch];
#pragma unroll
          for (int u = 0; u < kCtlWalkBatch; ++u)
            if (f0 + u < stop) hb[u] = fr[f0 + u].hdr, mo[u] = msg_of[f0 + u];
#pragma unroll
          for (int u = 0; u < kCtlWalkBatch; ++u) {
            const uint64_t f = f0 + u;
            if (f >= stop) break;
            const int64_t m = mo[u];
            if (m < -1 || (m >= 0 && (uint64_t)m >= nm)) {  // outside the message table: never an index
              bad = 1;
              break;
            }
            if (m >= 0) {
              if (m != cur) {
                finish();
                cur = m;
                cur_st = bodies[m].status;
                mconn[m] = c;
              }
              cur_last = f;
            }
            const uint32_t op = hb[u].opcode;
            uint8_t k = kCtlNone;
            if (op == 0x8) {
              k = hb[u].length == 0 ? kCtlCloseBare : kCtlCloseBody;
              if (close_f == UINT64_MAX) close_f = f;
            } else if (op == 0x9) {
              k = kCtlPayload;
            } else if (op == 0xA) {
              k = (flags & GEVWS_CONTROL_NO_PING_FOR_PONG) ? kCtlNone : kCtlPayload;
            }
            if (k) cls[f] = k, fconn[f] = c;
          }
        }
        if (!bad) {
          finish();
          uint64_t cut = close_f < errf ? close_f : errf;
          if (fail_f < cut) cut = fail_f;
          if (cut != UINT64_MAX) {
            w.cut = cut;
            w.flags = GEVWS_CTL_SHUTDOWN;
            if (cut == errf) {  // (a close frame that is itself the failing frame counts as (b))
              w.flags |= GEVWS_CTL_FAILED;
              w.code = close_code_of((uint32_t)cm.error);
            } else if (cut == fail_f) {
              w.flags |= GEVWS_CTL_FAILED;
              w.code = close_code_of(fail_st);
            }
            if (w.flags & GEVWS_CTL_FAILED) cls[cut] = kCtlFail, fconn[cut] = c;
            for (uint64_t f = cut + 1; f < stop; ++f) cls[f] = kCtlNone;  // behind the cut: ignored
            shut = 1;
          }
        }
      }
    }
    work[c] = w;
  }
  count_up(ctl + 0, shut);
  count_up(ctl + 1, bad);
}

__device__ __forceinline__ bool ctl_takes_slot(uint32_t k) { return k == kCtlCloseBody || k == kCtlFail; }

__global__ __launch_bounds__(kWalkBlock) void k_ctl_count(uint64_t max_frames, const gevws_summary* __restrict__ dec,
                                                          const gevws_summary* __restrict__ msg_sum,
                                                          const gevws_summary* __restrict__ join_sum,
                                                          const uint8_t* __restrict__ cls, uint64_t* __restrict__ blk) {
  const uint64_t n = ctl_frames(max_frames, dec, msg_sum, join_sum);
  const uint64_t f = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[2] = {0, 0};  // replies, aux slots
  if (f < n) {
    const uint32_t k = cls[f];
    vals[0] = k != kCtlNone, vals[1] = ctl_takes_slot(k);
  }
  block_partial<2>(vals, blk, blockIdx.x);
}

// The scan left {replies, aux slots} and CAPACITY in *sum: the gates, the
// malformed tables and the shutdown count on top.
__global__ void k_ctl_verdict(uint64_t max_frames, const gevws_summary* __restrict__ dec,
                              const gevws_summary* __restrict__ msg_sum, const gevws_summary* __restrict__ join_sum,
                              const uint64_t* __restrict__ ctl, gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  if (ctl_frames(max_frames, dec, msg_sum, join_sum)) {
    if (ctl[1]) {
      o.errors = ctl[1];
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = s.frames;
      o.payload_bytes = s.payload_bytes;
      o.errors = ctl[0];
      o.status = s.status;
    }
  }
  *sum = o;
}

__global__ __launch_bounds__(kWalkBlock) void k_ctl_emit(
    const gevws_frame* __restrict__ fr, uint64_t max_frames, const gevws_summary* __restrict__ dec,
    const gevws_summary* __restrict__ msg_sum, const gevws_summary* __restrict__ join_sum,
    const uint8_t* __restrict__ payload, uint64_t aux_off, const uint8_t* __restrict__ cls,
    const uint32_t* __restrict__ fconn, const CtlConn* __restrict__ work, const uint64_t* __restrict__ blk,
    const gevws_summary* __restrict__ sum, gevws_out_frame* __restrict__ rep, uint32_t* __restrict__ rep_conn,
    int64_t* __restrict__ reply_of, uint8_t* __restrict__ aux_base) {
  if (sum->status != GEVWS_OK) return;  // capacity or a malformed table: nothing written
  const uint64_t n = ctl_frames(max_frames, dec, msg_sum, join_sum);
  const uint64_t f = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  const uint32_t k = f < n ? cls[f] : kCtlNone;
  const uint64_t v[2] = {(uint64_t)(k != kCtlNone), (uint64_t)ctl_takes_slot(k)};
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (f >= n) return;
  if (k == kCtlNone) {
    reply_of[f] = -1;
    return;
  }
  const uint64_t r = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
  const uint64_t slot = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
  const uint32_t c = fconn[f];
  if (k == kCtlFail) {
    // the close of a failed connection: the code alone, no reason
    const uint32_t code = work[c].code;
    uint8_t* body = aux_base + slot * kAuxSlot;
    body[0] = (uint8_t)(code >> 8);
    body[1] = (uint8_t)code;
    gevws_out_frame o;
    memset(&o, 0, sizeof(o));
    o.hdr.fin = 1;
    o.hdr.opcode = 0x8;
    o.hdr.length = 2;
    o.payload_off = aux_off + slot * kAuxSlot;
    o.payload_len = 2;
    reply_of[f] = (int64_t)r;
    rep[r] = o;
  } else {
    const gevws_frame in = fr[f];
    const uint32_t op = in.hdr.opcode == 0x9 ? 0xAu : 0x9u;  // (a payload reply: ping -> pong, pong -> ping)
    disp_reply(in, (int)k, op, f, r, slot, payload, aux_off, rep, reply_of, aux_base);
  }
  rep_conn[r] = c;
}

__global__ __launch_bounds__(kWalkBlock) void k_ctl_tables(
    uint64_t max_frames, const gevws_summary* __restrict__ dec, const gevws_summary* __restrict__ msg_sum,
    const gevws_summary* __restrict__ join_sum, const gevws_message* __restrict__ msgs, uint64_t max_messages,
    uint32_t n_conns, const uint64_t* __restrict__ mend, const uint32_t* __restrict__ mconn,
    const CtlConn* __restrict__ work, const gevws_summary* __restrict__ sum, gevws_conn_ctl* __restrict__ conn_ctl,
    uint64_t* __restrict__ msg_end, gevws_body* __restrict__ bodies) {
  if (sum->status != GEVWS_OK) return;
  if (!ctl_frames(max_frames, dec, msg_sum, join_sum)) return;
  const uint64_t i = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (i < n_conns) {
    const CtlConn w = work[i];
    gevws_conn_ctl o;
    memset(&o, 0, sizeof(o));
    o.cut_frame = w.cut;
    o.close_code = w.code;
    o.flags = w.flags;
    conn_ctl[i] = o;
  }
  if (i < gated_count(max_messages, msg_sum)) {
    const uint64_t e = mend[i];
    const uint32_t c = mconn[i];
    msg_end[i] = (e != UINT64_MAX && (msgs[i].flags & GEVWS_MSG_END)) ? e : UINT64_MAX;
    if (e != UINT64_MAX && c < n_conns) {
      const uint64_t cut = work[c].cut;
      if (cut != UINT64_MAX && e > cut) {  // its last data frame lies behind the cut: not delivered
        gevws_body b = bodies[i];
        b.off = 0;
        b.length = 0;
        b.flags = 0;
        b.status = GEVWS_MSG_ERR_CLOSED;
        bodies[i] = b;
      }
    }
  }
}

// ------------------------------------------------------------------ the send plan
struct PlanIn {
  uint64_t max_frames, max_messages;
  const gevws_summary* __restrict__ dec;
  const gevws_summary* __restrict__ msg_sum;
  const gevws_summary* __restrict__ join_sum;
  const gevws_summary* __restrict__ ctl_sum;
  const gevws_summary* __restrict__ enc0;  // the plain wire's encode summary, its table below
  const gevws_summary* __restrict__ enc1;  // the deflated wire's
  const gevws_summary* __restrict__ enc2;  // the control wire's
  const uint64_t* __restrict__ off0;
  const uint64_t* __restrict__ off1;
  const uint64_t* __restrict__ off2;
  const int64_t* __restrict__ msg_of;
  const uint64_t* __restrict__ msg_end;
  const int64_t* __restrict__ reply_of;
  const int64_t* __restrict__ ctl_of;
  const uint8_t* __restrict__ conn_ext;  // may be null
  uint32_t n_conns;
};

// The frames of the call: the decode's count, none when any step before failed.
__device__ __forceinline__ uint64_t plan_frames(const PlanIn& p) {
  if (p.msg_sum->status != GEVWS_OK || p.join_sum->status != GEVWS_OK || p.ctl_sum->status != GEVWS_OK ||
      p.enc0->status != GEVWS_OK || p.enc1->status != GEVWS_OK || p.enc2->status != GEVWS_OK)
    return 0;
  return gated_count(p.max_frames, p.dec);
}

struct PlanDec {
  uint64_t off, len;
  uint32_t wire;
  bool send, bad;
};
// What frame f of connection c triggers: its control reply, else the reply to
// the message it ends.  Every index is checked against its list before it is used.
__device__ __forceinline__ PlanDec plan_decide(const PlanIn& p, uint64_t f, uint32_t c, uint64_t nm) {
  PlanDec d{0, 0, 0u, false, false};
  uint64_t idx;
  const int64_t k = p.ctl_of[f];
  if (k >= 0) {
    d.wire = 2, idx = (uint64_t)k;
  } else {
    const int64_t m = p.msg_of[f];
    if (m < 0) return d;
    if ((uint64_t)m >= nm) {
      d.bad = true;
      return d;
    }
    if (p.msg_end[m] != f) return d;
    const int64_t r = p.reply_of[m];
    if (r < 0) return d;
    if (c >= p.n_conns) {
      d.bad = true;
      return d;
    }
    d.wire = (p.conn_ext && (p.conn_ext[c] & GEVWS_EXT_DEFLATE)) ? 1u : 0u;
    idx = (uint64_t)r;
  }
  const gevws_summary* __restrict__ enc = d.wire == 0 ? p.enc0 : (d.wire == 1 ? p.enc1 : p.enc2);
  const uint64_t* __restrict__ tab = d.wire == 0 ? p.off0 : (d.wire == 1 ? p.off1 : p.off2);
  const uint64_t cnt = enc->frames, total = enc->payload_bytes;
  if (c >= p.n_conns || idx >= cnt) {  // a frame of no connection, or a reply outside its list
    d.bad = true;
    return d;
  }
  d.off = tab[idx];
  const uint64_t next = idx + 1 < cnt ? tab[idx + 1] : total;
  if (next < d.off) {
    d.bad = true;
    return d;
  }
  d.len = next - d.off;
  d.send = true;
  return d;
}

struct PlanScratch {
  uint64_t* ctl;     // [0] connections with SHUTDOWN
  uint64_t* blk;     // [nblk][kBlkFields]: entries, bytes, malformed
  uint32_t* fconn;   // [f] the frame's connection (kNoConn: none)
  uint64_t* pre_n;   // [f] entries before frame f; [n] all of them
  uint64_t* pre_b;   // [f] their bytes
  size_t zero_bytes, ones_off, ones_bytes, total;
};
inline PlanScratch plan_scratch(void* base, uint64_t max_frames, uint32_t nblk) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  PlanScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t));
  s.zero_bytes = o;
  s.ones_off = o;
  s.fconn = reinterpret_cast<uint32_t*>(p + o), o += up(max_frames * 4);
  s.ones_bytes = o - s.ones_off;
  s.pre_n = reinterpret_cast<uint64_t*>(p + o), o += up((max_frames + 1) * 8);
  s.pre_b = reinterpret_cast<uint64_t*>(p + o), o += up((max_frames + 1) * 8);
  s.total = o;
  return s;
}

__global__ __launch_bounds__(kWalkBlock) void k_plan_conns(PlanIn p, const gevws_conn_out* __restrict__ cout,
                                                           const gevws_conn_ctl* __restrict__ conn_ctl,
                                                           uint32_t* __restrict__ fconn, uint64_t* __restrict__ ctl) {
  const uint64_t n = plan_frames(p);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t shut = 0;
  if (n && c < p.n_conns) {
    const gevws_conn_out co = cout[c];
    const uint64_t lo = co.first_frame < n ? co.first_frame : n;
    const uint64_t hi = co.nframes < n - lo ? lo + co.nframes : n;
    for (uint64_t f = lo; f < hi; ++f) fconn[f] = c;
    shut = (conn_ctl[c].flags & GEVWS_CTL_SHUTDOWN) ? 1 : 0;
  }
  count_up(ctl, shut);
}

__global__ __launch_bounds__(kWalkBlock) void k_plan_count(PlanIn p, const uint32_t* __restrict__ fconn,
                                                           uint64_t* __restrict__ blk) {
  const uint64_t n = plan_frames(p);
  const uint64_t f = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[3] = {0, 0, 0};  // entries, their bytes, malformed indices
  if (f < n) {
    const PlanDec d = plan_decide(p, f, fconn[f], gated_count(p.max_messages, p.msg_sum));
    vals[0] = d.send, vals[1] = d.len, vals[2] = d.bad;
  }
  block_partial<3>(vals, blk, blockIdx.x);
}

// The scan left {entries, bytes, malformed} in *sum's frames / payload_bytes /
// payload_len, and CAPACITY against max_sends: the summary from them, and the
// prefixes' last entry.
__global__ void k_plan_verdict(PlanIn p, const uint64_t* __restrict__ ctl, uint64_t* __restrict__ pre_n,
                               uint64_t* __restrict__ pre_b, gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  const uint64_t n = plan_frames(p);
  if (n) {
    if (s.payload_len) {
      o.errors = s.payload_len;
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = s.frames;
      o.payload_bytes = s.payload_bytes;
      o.errors = ctl[0];
      o.status = s.status;
      if (s.status == GEVWS_OK) pre_n[n] = s.frames, pre_b[n] = s.payload_bytes;
    }
  }
  *sum = o;
}

__global__ __launch_bounds__(kWalkBlock) void k_plan_emit(PlanIn p, const uint32_t* __restrict__ fconn,
                                                          const uint64_t* __restrict__ blk,
                                                          const gevws_summary* __restrict__ sum,
                                                          uint64_t* __restrict__ pre_n, uint64_t* __restrict__ pre_b,
                                                          gevws_send* __restrict__ send) {
  if (sum->status != GEVWS_OK) return;  // more entries than max_sends, or a malformed index: nothing written
  const uint64_t n = plan_frames(p);
  const uint64_t f = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  PlanDec d{0, 0, 0u, false, false};
  uint32_t c = kNoConn;
  if (f < n) {
    c = fconn[f];
    d = plan_decide(p, f, c, gated_count(p.max_messages, p.msg_sum));
  }
  const uint64_t v[2] = {(uint64_t)d.send, d.len};
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (f >= n) return;
  const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
  const uint64_t b = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
  pre_n[f] = k;
  pre_b[f] = b;
  if (!d.send) return;
  gevws_send o;
  o.off = d.off;
  o.len = d.len;
  o.frame = f;
  o.conn = c;
  o.wire = d.wire;
  send[k] = o;
}

__global__ __launch_bounds__(kWalkBlock) void k_plan_conn_emit(PlanIn p, const gevws_conn_out* __restrict__ cout,
                                                               const gevws_conn_ctl* __restrict__ conn_ctl,
                                                               const uint64_t* __restrict__ pre_n,
                                                               const uint64_t* __restrict__ pre_b,
                                                               const gevws_summary* __restrict__ sum,
                                                               gevws_conn_send* __restrict__ conn_send) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t n = plan_frames(p);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  if (!n || c >= p.n_conns) return;
  const gevws_conn_out co = cout[c];
  const uint64_t lo = co.first_frame < n ? co.first_frame : n;
  const uint64_t hi = co.nframes < n - lo ? lo + co.nframes : n;
  gevws_conn_send o;
  memset(&o, 0, sizeof(o));
  o.first = pre_n[lo];
  o.count = pre_n[hi] - pre_n[lo];
  o.bytes = pre_b[hi] - pre_b[lo];
  o.flags = conn_ctl[c].flags;
  conn_send[c] = o;
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_control_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames, uint64_t max_frames,
                                   const gevws_conn_out* d_conn_out, uint32_t n_conns, const gevws_summary* d_decoded,
                                   uint8_t* d_payload, uint64_t aux_off, uint64_t aux_cap, const int64_t* d_msg_of,
                                   const gevws_message* d_messages, uint64_t max_messages,
                                   const gevws_conn_msg* d_conn_msg, const gevws_summary* d_msg_summary,
                                   gevws_body* d_bodies, const gevws_summary* d_join_summary, uint32_t flags,
                                   gevws_out_frame* d_ctl, uint32_t* d_ctl_conn, int64_t* d_ctl_of,
                                   uint64_t* d_msg_end, gevws_conn_ctl* d_conn_ctl, gevws_summary* d_summary) {
  if ((flags & ~GEVWS_CONTROL_NO_PING_FOR_PONG) || !ctx || !d_summary || max_frames > 0xFFFFFFFFull ||
      max_messages > 0xFFFFFFFFull)
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (n_conns == 0 || max_frames == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_frames || !d_conn_out || !d_decoded || !d_payload || !d_msg_of || !d_conn_msg || !d_msg_summary ||
      !d_join_summary || !d_ctl || !d_ctl_conn || !d_ctl_of || !d_conn_ctl ||
      (max_messages && (!d_messages || !d_bodies || !d_msg_end)))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_frames + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkc = (n_conns + kWalkBlock - 1) / kWalkBlock;
  const uint32_t nblkm = (uint32_t)((max_messages + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, ctl_scratch(nullptr, max_frames, max_messages, n_conns, nblk).total);
  if (r != GEVWS_OK) return r;
  const CtlScratch s = ctl_scratch(ctx->scratch, max_frames, max_messages, n_conns, nblk);
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  if (s.ones_bytes) GEVWS_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(ctx->scratch) + s.ones_off, 0xFF, s.ones_bytes, st));
  k_ctl_classify<<<nblkc, kWalkBlock, 0, st>>>(d_frames, max_frames, d_conn_out, n_conns, d_decoded, d_msg_of,
                                               max_messages, d_conn_msg, d_msg_summary, d_bodies, d_join_summary,
                                               flags, s.cls, s.fconn, s.mend, s.mconn, s.work, s.ctl);
  k_ctl_count<<<nblk, kWalkBlock, 0, st>>>(max_frames, d_decoded, d_msg_summary, d_join_summary, s.cls, s.blk);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk, max_frames, aux_cap / kAuxSlot, d_summary);
  k_ctl_verdict<<<1, 1, 0, st>>>(max_frames, d_decoded, d_msg_summary, d_join_summary, s.ctl, d_summary);
  k_ctl_emit<<<nblk, kWalkBlock, 0, st>>>(d_frames, max_frames, d_decoded, d_msg_summary, d_join_summary, d_payload,
                                          aux_off, s.cls, s.fconn, s.work, s.blk, d_summary, d_ctl, d_ctl_conn,
                                          d_ctl_of, d_payload + aux_off);
  k_ctl_tables<<<nblkc > nblkm ? nblkc : nblkm, kWalkBlock, 0, st>>>(
      max_frames, d_decoded, d_msg_summary, d_join_summary, d_messages, max_messages, n_conns, s.mend, s.mconn,
      s.work, d_summary, d_conn_ctl, d_msg_end, d_bodies);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_send_plan_async(gevws_ctx* ctx, void* stream, uint64_t max_frames,
                                     const gevws_summary* d_decoded, const gevws_conn_out* d_conn_out,
                                     uint32_t n_conns, const int64_t* d_msg_of, const uint64_t* d_msg_end,
                                     const int64_t* d_reply_of, uint64_t max_messages,
                                     const gevws_summary* d_msg_summary, const gevws_summary* d_join_summary,
                                     const uint8_t* d_conn_ext, const int64_t* d_ctl_of,
                                     const gevws_conn_ctl* d_conn_ctl, const gevws_summary* d_ctl_summary,
                                     const uint64_t* d_plain_off, const gevws_summary* d_plain_encoded,
                                     const uint64_t* d_def_off, const gevws_summary* d_def_encoded,
                                     const uint64_t* d_ctl_off, const gevws_summary* d_ctl_encoded,
                                     gevws_send* d_send, uint64_t max_sends, gevws_conn_send* d_conn_send,
                                     gevws_summary* d_summary) {
  if (!ctx || !d_summary || max_frames > 0xFFFFFFFFull || max_messages > 0xFFFFFFFFull) return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (n_conns == 0 || max_frames == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_decoded || !d_conn_out || !d_msg_of || !d_msg_summary || !d_join_summary || !d_ctl_of || !d_conn_ctl ||
      !d_ctl_summary || !d_plain_off || !d_plain_encoded || !d_def_off || !d_def_encoded || !d_ctl_off ||
      !d_ctl_encoded || !d_conn_send || (max_sends && !d_send) || (max_messages && (!d_msg_end || !d_reply_of)))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_frames + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkc = (n_conns + kWalkBlock - 1) / kWalkBlock;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, plan_scratch(nullptr, max_frames, nblk).total);
  if (r != GEVWS_OK) return r;
  const PlanScratch s = plan_scratch(ctx->scratch, max_frames, nblk);
  const PlanIn p{max_frames,   max_messages, d_decoded,   d_msg_summary, d_join_summary, d_ctl_summary,
                 d_plain_encoded, d_def_encoded, d_ctl_encoded, d_plain_off, d_def_off, d_ctl_off,
                 d_msg_of,     d_msg_end,    d_reply_of,  d_ctl_of,      d_conn_ext,     n_conns};
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  GEVWS_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(ctx->scratch) + s.ones_off, 0xFF, s.ones_bytes, st));
  k_plan_conns<<<nblkc, kWalkBlock, 0, st>>>(p, d_conn_out, d_conn_ctl, s.fconn, s.ctl);
  k_plan_count<<<nblk, kWalkBlock, 0, st>>>(p, s.fconn, s.blk);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk, max_sends, UINT64_MAX, d_summary);
  k_plan_verdict<<<1, 1, 0, st>>>(p, s.ctl, s.pre_n, s.pre_b, d_summary);
  k_plan_emit<<<nblk, kWalkBlock, 0, st>>>(p, s.fconn, s.blk, d_summary, s.pre_n, s.pre_b, d_send);
  k_plan_conn_emit<<<nblkc, kWalkBlock, 0, st>>>(p, d_conn_out, d_conn_ctl, s.pre_n, s.pre_b, d_summary, d_conn_send);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
