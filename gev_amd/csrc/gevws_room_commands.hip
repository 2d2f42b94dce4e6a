// gevws_room_commands.hip -- room commands out of message bodies
// (gevws_room_commands_async; include/gevws.h): "/join N" and "/leave" in
// delivered text messages become the {conn, room} change records of
// gevws_rooms_update_async, in message order, and leave the broadcast.  The
// step stands behind the control step and in front of gevws_reply_rooms_async;
// its summary is the update's d_prev, so neither the records nor their count
// visit the host.  The reference has no rooms and no commands
// (example/websocket/main.go sends every message to every session).
//
// One memset and four launches, no host round trip:
//   k_cmd_count    one lane per body: the 32-byte record, and for a looked-at
//                  body (delivered, text, 6..16 bytes) one aligned 16-byte load
//                  of its bytes; the rule of gevws_room_command.hpp; a class
//                  byte per body and the room of a change into scratch; block
//                  partials {changes, rejected, stripped, malformed}
//   k_scan_blocks  the partials' scan, CAPACITY against max_changes
//   k_cmd_verdict  one lane: the summary from the scan and the gates
//   k_cmd_emit     one lane per body, from the class bytes alone: a block scan
//                  of the changes places the record (message order kept, no
//                  atomic), d_change_of, and the strip of the body's record
// Nothing but the summary is written before the verdict, every writer of an
// output returns unless the summary is GEVWS_OK, and a record's off / conn are
// bounded before anything is loaded or indexed by them.  The body bytes in
// d_out are read only.
#include "gevws_internal.hpp"
#include "gevws_room_command.hpp"

namespace {

static_assert(sizeof(gevws_body) == 32 && offsetof(gevws_body, conn) == 16 && offsetof(gevws_body, status) == 22,
              "gevws_body layout");
static_assert(sizeof(gevws_room_change) == 8 && offsetof(gevws_room_change, room) == 4, "gevws_room_change layout");
static_assert(GEVWS_MSG_COMMAND == 10, "continues the GEVWS_MSG_* enum behind GEVWS_MSG_ERR_CLOSED");

namespace rc = gevws_room_command;
constexpr uint8_t kCmdBad = 3;  // a class byte beside rc::kNone / kChange / kRejected: a malformed record

struct CmdGates {
  const gevws_summary* __restrict__ msg;   // also the body count's gate
  const gevws_summary* __restrict__ join;
  const gevws_summary* __restrict__ ctl;   // may be null
  uint64_t max_messages;
};
// The bodies of the call: none unless every gate is GEVWS_OK.
__device__ __forceinline__ uint64_t cmd_count(const CmdGates& g) {
  if (g.join->status != GEVWS_OK || (g.ctl && g.ctl->status != GEVWS_OK)) return 0;
  return gated_count(g.max_messages, g.msg);
}

__global__ __launch_bounds__(kWalkBlock) void k_cmd_count(const gevws_body* __restrict__ bodies, CmdGates G,
                                                          const uint8_t* __restrict__ out, uint64_t src_bytes,
                                                          uint32_t n_conns, uint32_t n_rooms,
                                                          uint8_t* __restrict__ cls, uint32_t* __restrict__ room,
                                                          uint64_t* __restrict__ blk) {
  const uint64_t n = cmd_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[kBlkFields] = {0, 0, 0, 0};  // changes, rejected, stripped, malformed
  if (m < n) {
    const gevws_body b = bodies[m];
    uint8_t c = rc::kNone;
    if (b.flags & GEVWS_BODY_WHOLE) {
      if (!(b.flags & (GEVWS_BODY_JOINED | GEVWS_BODY_INFLATED)) || b.conn >= n_conns) {
        c = kCmdBad;  // (as the reply step: a delivered body must lie in d_out and name a connection)
      } else if (b.opcode == 1 && b.length >= rc::kMinLength && b.length <= rc::kMaxLength) {
        if ((b.off & 15) || b.off > src_bytes || b.length > src_bytes - b.off) {
          c = kCmdBad;
        } else {
          // the whole aligned vector that holds the body's first byte (the join's rule for d_out)
          const u32x4 v = *reinterpret_cast<const u32x4*>(out + b.off);
          uint32_t r;
          c = (uint8_t)rc::classify((uint64_t)v[0] | ((uint64_t)v[1] << 32), (uint64_t)v[2] | ((uint64_t)v[3] << 32),
                                    b.length, n_rooms, r);
          if (c == rc::kChange) room[m] = r;
        }
      }
    }
    cls[m] = c;
    vals[0] = c == rc::kChange, vals[1] = c == rc::kRejected;
    vals[2] = vals[0] + vals[1], vals[3] = c == kCmdBad;
  }
  block_partial<kBlkFields>(vals, blk, blockIdx.x);
}

// The scan left {changes, rejected, stripped, malformed} in *sum's frames /
// payload_bytes / payload_len / errors, and CAPACITY against max_changes: the
// summary from them and from the gates.
__global__ void k_cmd_verdict(CmdGates G, gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  if (cmd_count(G)) {
    if (s.errors) {
      o.errors = s.errors;
      o.status = GEVWS_ERR_INVALID;
    } else if (s.status != GEVWS_OK) {
      o.frames = s.frames;  // the need
      o.status = s.status;
    } else {
      o.frames = s.frames;
      o.payload_bytes = s.payload_bytes;
      o.payload_len = s.payload_len;
    }
  }
  *sum = o;
}

__global__ __launch_bounds__(kWalkBlock) void k_cmd_emit(gevws_body* __restrict__ bodies, CmdGates G,
                                                         const uint8_t* __restrict__ cls,
                                                         const uint32_t* __restrict__ room,
                                                         const uint64_t* __restrict__ blk, uint64_t max_changes,
                                                         const gevws_summary* __restrict__ sum,
                                                         gevws_room_change* __restrict__ changes,
                                                         int64_t* __restrict__ change_of) {
  if (sum->status != GEVWS_OK) return;  // more changes than max_changes, or a malformed record: nothing written
  const uint64_t n = cmd_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  const uint8_t c = m < n ? cls[m] : (uint8_t)rc::kNone;
  const uint64_t v[1] = {(uint64_t)(c == rc::kChange)};
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (m >= n) return;
  int64_t at = c == rc::kRejected ? -2 : -1;
  if (c != rc::kNone) {
    gevws_body b = bodies[m];  // (this lane's record: nobody else reads or writes it in this launch)
    if (c == rc::kChange) {
      const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields] + ex[0];
      if (k < max_changes) {  // (always: the verdict found the count within max_changes)
        gevws_room_change ch;
        ch.conn = b.conn, ch.room = room[m];
        changes[k] = ch;
      }
      at = (int64_t)k;
    }
    b.off = 0;
    b.length = 0;
    b.flags = 0;
    b.status = GEVWS_MSG_COMMAND;
    bodies[m] = b;
  }
  change_of[m] = at;
}

struct CmdScratch {
  uint64_t* blk;   // [nblk][kBlkFields]
  uint8_t* cls;    // [m] the body's class
  uint32_t* room;  // [m] a change's room (written for changes only)
  size_t zero_bytes, total;
};
inline CmdScratch cmd_scratch(void* base, uint32_t nblk, uint64_t max_messages) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  CmdScratch s{};
  size_t o = 0;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t));
  s.cls = p + o, o += up((size_t)max_messages);
  s.zero_bytes = o;
  s.room = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)max_messages * 4);
  s.total = o;
  return s;
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_room_commands_async(gevws_ctx* ctx, void* stream, gevws_body* d_bodies, uint64_t max_messages,
                                         const gevws_summary* d_msg_summary, const gevws_summary* d_join_summary,
                                         const gevws_summary* d_ctl_summary, const uint8_t* d_out,
                                         uint64_t src_bytes, uint32_t n_conns, uint32_t n_rooms, uint32_t flags,
                                         gevws_room_change* d_changes, uint64_t max_changes, int64_t* d_change_of,
                                         gevws_summary* d_summary) {
  if (!ctx || flags != 0 || !d_changes || !d_change_of || !d_summary || max_messages > 0xFFFFFFFFull ||
      max_changes > 0xFFFFFFFFull)
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (max_messages == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_bodies || !d_msg_summary || !d_join_summary || (src_bytes && !d_out) ||
      (reinterpret_cast<uintptr_t>(d_out) & 15))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_messages + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, cmd_scratch(nullptr, nblk, max_messages).total);
  if (r != GEVWS_OK) return r;
  const CmdScratch s = cmd_scratch(ctx->scratch, nblk, max_messages);
  const CmdGates G{d_msg_summary, d_join_summary, d_ctl_summary, max_messages};
  GEVWS_HIP(hipMemsetAsync(s.blk, 0, s.zero_bytes, st));
  k_cmd_count<<<nblk, kWalkBlock, 0, st>>>(d_bodies, G, d_out, src_bytes, n_conns, n_rooms, s.cls, s.room, s.blk);
  // the 256-lane shape of the scan: the 1 024-lane one spills to scratch memory in this file
  k_scan_blocks<false, kBlkFields, kWalkBlock><<<1, kWalkBlock, 0, st>>>(s.blk, nblk, max_changes, UINT64_MAX,
                                                                         d_summary);
  k_cmd_verdict<<<1, 1, 0, st>>>(G, d_summary);
  k_cmd_emit<<<nblk, kWalkBlock, 0, st>>>(d_bodies, G, s.cls, s.room, s.blk, max_changes, d_summary, d_changes,
                                          d_change_of);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
