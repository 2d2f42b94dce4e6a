// gevws_message.hip -- the message layer behind a decode (gevws_messages_async,
// include/gevws.h): RFC 6455 fragment assembly (section 5.4), the frame-level
// checks of sections 5.2 and 5.5, and the UTF-8 check of text messages
// (section 8.1).  The reference has no code for it: HandlerWrap.OnMessage
// (plugins/websocket/wrap.go:71) hands every data frame to the user.
//
// Six launches behind two memsets, no host round trip:
//   k_msg_classify     one lane per connection: checks 1-5, which frames are
//                      data frames of which kind of message (cls[f])
//   k_msg_utf8_frames  one wave per text-message data frame: its part summary
//                      (lead / bad / tail); frames of kMsgBigFrame bytes and
//                      more are only listed
//   k_msg_utf8_big     the listed frames in tiles of kMsgBigTile bytes dealt
//                      round robin over the waves of a CU-filling grid
//   k_msg_stitch       one lane per connection: parts stitched onto the carry
//                      state, the verdict, the message count
//   k_scan_blocks      message bases, the summary
//   k_msg_emit         one lane per connection: d_messages, d_msg_of,
//                      d_conn_msg, d_state
// Only the UTF-8 pass touches payload bytes (every byte of every text frame,
// once); the other passes read records and one byte / word per frame.
// gevws_messages_ext_async adds one extension byte per connection: on a
// permessage-deflate connection RSV1 on an opcode-1 / 2 frame opens a
// compressed message, whose frames get the class bit kClsComp and skip the
// UTF-8 pass (gevws_inflate.hip inflates them and checks the text afterwards).
#include "gevws_internal.hpp"
#include "gevws_utf8.hpp"

namespace {

// ------------------------------------------------------------------ scratch
// cls[f]: what frame f is to the message layer (0: control frame, or past its
// connection's frame-level error, or not looked at)
constexpr uint32_t kClsData = 1, kClsText = 2, kClsBegin = 4, kClsEnd = 8;
// a data frame of a compressed message (permessage-deflate): its bytes are DEFLATE, not text
constexpr uint32_t kClsComp = 16;
// part[f] of a text-message data frame: bits 0-2 `lead`, its leading
// continuation bytes (4 = four or more); bits 3-4 `tail`, the bytes of the
// unfinished sequence at its end; bit 5 `bad`, a wrong byte in [lead, L)
// read from a clean start
constexpr uint32_t kPartBad = 32;
// One wave takes a frame in steps of kMsgStepVecs vectors a lane ...
constexpr int kMsgStepVecs = 4;
// ... up to this size; larger frames are spread over the grid in tiles
constexpr uint64_t kMsgBigFrame = 256 * 1024;
constexpr uint64_t kMsgBigTile = 16 * 1024;  // one wave, four steps
constexpr int kMsgWgPerCU = 4;
// The per-connection walks request this many frames' records / class bytes at
// once: one lane walks a connection, and a load per frame, each waited for,
// is what such a walk costs.
constexpr int kMsgWalkBatch = 4;
static_assert(kMsgBigTile % (64 * 16 * kMsgStepVecs) == 0, "a tile = whole wave steps");

struct MsgConn {  // per-connection hand-off between the passes (32 bytes)
  uint64_t err_frame;
  int32_t err;
  uint32_t nmsg;
  gevws_msg_state st;  // classify: the state the connection came in with; stitch: the one it leaves with
  uint32_t active;     // its frames are walked (status OK, has frames, not failed before)
  uint32_t ext;        // its GEVWS_EXT_* bits (d_conn_ext)
};
static_assert(sizeof(MsgConn) == 32 && sizeof(gevws_msg_state) == 8 && sizeof(gevws_message) == 32 &&
                  sizeof(gevws_conn_msg) == 32, "message-layer layouts");

struct MsgScratch {
  unsigned long long* ctl;  // [0]: listed big frames (low 32 bits) | their tiles (high 32)
  uint8_t* cls;
  uint32_t* part;
  uint4* big;  // (frame, its first tile's number in the pass, its tiles, -)
  MsgConn* conn;
  uint64_t* blk;
  size_t zero_bytes, total;
};
inline MsgScratch msg_scratch(void* base, uint64_t max_frames, uint32_t n_conns, uint32_t nblk) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  MsgScratch s;
  size_t o = 0;
  s.ctl = reinterpret_cast<unsigned long long*>(p + o), o += 256;
  s.cls = p + o, o += up(max_frames);
  s.part = reinterpret_cast<uint32_t*>(p + o), o += up(max_frames * 4);
  s.zero_bytes = o;
  s.big = reinterpret_cast<uint4*>(p + o), o += up(max_frames * 16);
  s.conn = reinterpret_cast<MsgConn*>(p + o), o += up((size_t)n_conns * sizeof(MsgConn));
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t));
  s.total = o;
  return s;
}

// ------------------------------------------------------------------ 1. classify (checks 1-5)
__global__ __launch_bounds__(kWalkBlock) void k_msg_classify(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                                             const gevws_conn_out* __restrict__ cout, uint32_t n_conns,
                                                             const gevws_summary* __restrict__ gate,
                                                             const gevws_msg_state* __restrict__ state,
                                                             const uint8_t* __restrict__ conn_ext,
                                                             uint8_t* __restrict__ cls, MsgConn* __restrict__ work) {
  const uint64_t n = gated_count(max_frames, gate);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  if (c >= n_conns) return;
  MsgConn w;
  memset(&w, 0, sizeof(w));
  w.err_frame = UINT64_MAX;
  if (n) {  // (a pass without frames reads none of its inputs)
    const gevws_conn_out co = cout[c];
    if (state) w.st = state[c];
    if (conn_ext) w.ext = conn_ext[c] & GEVWS_EXT_DEFLATE;
    w.err = w.st.failed;
    const uint64_t first = co.first_frame;
    const uint64_t end = first < n ? (co.nframes < n - first ? first + co.nframes : n) : first;
    if (co.status == GEVWS_OK && end > first && !w.st.failed) {
      w.active = 1;
      uint32_t open = w.st.opcode == 1 || w.st.opcode == 2 ? w.st.opcode : 0u;
      const bool deflate = w.ext != 0;
      bool comp = deflate && open && w.st.reserved[0];  // the open message is compressed
      bool done = false;
      for (uint64_t f0 = first; f0 < end && !done; f0 += kMsgWalkBatch) {
        gevws_header hb[kMsgWalkBatch];
#pragma unroll
        for (int u = 0; u < kMsgWalkBatch; ++u)
          if (f0 + u < end) hb[u] = fr[f0 + u].hdr;
#pragma unroll
        for (int u = 0; u < kMsgWalkBatch; ++u) {
          const uint64_t f = f0 + u;
          if (f >= end) break;
          const gevws_header h = hb[u];
          const uint32_t op = h.opcode;
          int e = GEVWS_MSG_OK;
          // RSV1 belongs to a deflate connection's first data frames only (RFC 7692 section 6)
          if (deflate ? ((h.rsv & 3) || ((h.rsv & 4) && ((op & 8) || op == 0))) : h.rsv != 0) e = GEVWS_MSG_ERR_RSV;
          else if (op > 0xA || (op > 2 && op < 8)) e = GEVWS_MSG_ERR_OPCODE;
          else if ((op & 8) && (!h.fin || (uint64_t)h.length > 125)) e = GEVWS_MSG_ERR_CONTROL;
          else if (op == 0 && !open) e = GEVWS_MSG_ERR_CONTINUATION;
          else if ((op == 1 || op == 2) && open) e = GEVWS_MSG_ERR_INTERLEAVE;
          if (e) {
            w.err = e;
            w.err_frame = f;
            done = true;
            break;
          }
          if (op & 8) continue;
          if (op) open = op, comp = (h.rsv & 4) != 0;
          cls[f] = (uint8_t)(kClsData | (open == 1 ? kClsText : 0u) | (op ? kClsBegin : 0u) | (h.fin ? kClsEnd : 0u) |
                             (comp ? kClsComp : 0u));
          if (h.fin) open = 0;
        }
      }
    }
  }
  work[c] = w;
}

// ------------------------------------------------------------------ 2. the UTF-8 pass
// The first four and the last three bytes of the L > 0 bytes at p (any
// alignment; indices clamped into the frame), loaded at once: a small frame's
// cost is its chain of dependent loads, and these seven depend on nothing but
// the record.
struct Utf8Edges {
  uint32_t head[4], last[3];  // last[i] = byte L - 1 - i
};
__device__ __forceinline__ Utf8Edges utf8_edges(const uint8_t* __restrict__ p, uint64_t L) {
  Utf8Edges e;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) e.head[i] = p[i < L ? i : L - 1];
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i) e.last[i] = p[i < L ? L - 1 - i : 0];
  return e;
}
// lead | tail << 3 (part[f]'s low bits) from them.
__device__ __forceinline__ uint32_t utf8_lead_tail(const Utf8Edges& e, uint64_t L) {
  uint32_t lead = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) lead += (uint32_t)(lead == i && i < L && (e.head[i] & 0xC0) == 0x80);
  const uint64_t body = L - lead;  // (lead = 4 fails the frame whatever follows)
  uint32_t tail = 0;
  if (body >= 1 && e.last[0] >= 0xC0) tail = 1;
  else if (body >= 2 && e.last[1] >= 0xE0) tail = 2;
  else if (body >= 3 && e.last[2] >= 0xF0) tail = 3;
  return lead | (tail << 3);
}

__global__ __launch_bounds__(kWalkBlock) void k_msg_utf8_frames(const gevws_frame* __restrict__ fr,
                                                                uint64_t max_frames,
                                                                const gevws_summary* __restrict__ gate,
                                                                const uint8_t* __restrict__ payload,
                                                                const uint8_t* __restrict__ cls,
                                                                uint32_t* __restrict__ part,
                                                                unsigned long long* __restrict__ ctl,
                                                                uint4* __restrict__ big) {
  const uint64_t n = gated_count(max_frames, gate);
  const uint64_t f = (uint64_t)blockIdx.x * (kWalkBlock / 64) + (threadIdx.x >> 6);  // one wave per frame
  if (f >= n) return;
  const uint32_t k = cls[f];
  const gevws_frame rec = fr[f];  // (requested beside cls[f], not behind it)
  if (!(k & kClsText) || (k & kClsComp)) return;
  const uint64_t L = (uint64_t)rec.hdr.length;
  if (L == 0) return;  // part 0
  const uint8_t* __restrict__ p = payload + rec.payload_off;
  const uint32_t lane = threadIdx.x & 63;
  const Utf8Edges edges = utf8_edges(p, L);
  uint32_t bad = 0, lt;
  if (rec.payload_off & (GEVWS_PAYLOAD_ALIGN - 1)) {
    // not a decode's arena layout: byte by byte on one lane
    lt = utf8_lead_tail(edges, L);
    if (lane == 0) {
      uint32_t p1 = 0, p2 = 0, p3 = 0;
      for (uint64_t i = lt & 7; i < L; ++i) {
        const uint32_t c = p[i];
        bad |= utf8_byte_bad(c, p1, p2, p3);
        p3 = p2, p2 = p1, p1 = c;
      }
    }
  } else if (L >= kMsgBigFrame) {
    if (lane == 0) {
      const uint64_t tiles = (L + kMsgBigTile - 1) / kMsgBigTile;
      const unsigned long long old = atomicAdd(ctl, (unsigned long long)((tiles << 32) | 1u));
      big[(uint32_t)old] = make_uint4((uint32_t)f, (uint32_t)(old >> 32), (uint32_t)tiles, 0u);
      atomicOr(part + f, utf8_lead_tail(edges, L));
    }
    return;
  } else {
    const uint64_t nvec = (L + 15) >> 4;
    u32x4 v[kMsgStepVecs];
    uint32_t pw[kMsgStepVecs];
    auto load_step = [&](uint64_t j0) {
#pragma unroll
      for (int u = 0; u < kMsgStepVecs; ++u) {
        const uint64_t j = j0 + (uint64_t)u * 64 + lane;
        if (j < nvec) {
          v[u] = *reinterpret_cast<const u32x4*>(p + 16 * j);
          pw[u] = j ? *reinterpret_cast<const uint32_t*>(p + 16 * j - 4) : 0u;
        }
      }
    };
    auto check_step = [&](uint64_t j0) {
#pragma unroll
      for (int u = 0; u < kMsgStepVecs; ++u) {
        const uint64_t j = j0 + (uint64_t)u * 64 + lane;
        if (j < nvec) bad |= utf8_vec_bad(v[u], pw[u], j, L, lt & 7);
      }
    };
    load_step(0);  // the first step's vectors are on their way before the edge bytes are looked at
    lt = utf8_lead_tail(edges, L);
    check_step(0);
    for (uint64_t j0 = 64 * kMsgStepVecs; j0 < nvec; j0 += 64 * kMsgStepVecs) {
      load_step(j0);
      check_step(j0);
    }
  }
  const bool any = __ballot(bad != 0) != 0;
  if (lane == 0) part[f] = lt | (any ? kPartBad : 0u);
}

// The listed frames' tiles dealt round robin over the grid's waves: tile k of
// an entry is tile first + k of the pass, and wave (first + k) mod nw takes it.
// Each lane looks at one entry of 64 at a time; the wave then works through
// those that hold a tile of its own.
__global__ __launch_bounds__(kWalkBlock) void k_msg_utf8_big(const gevws_frame* __restrict__ fr,
                                                             const uint8_t* __restrict__ payload,
                                                             uint32_t* __restrict__ part,
                                                             const unsigned long long* __restrict__ ctl,
                                                             const uint4* __restrict__ big) {
  const uint32_t nbig = (uint32_t)*ctl;
  const uint32_t nw = gridDim.x * (kWalkBlock / 64), wid = blockIdx.x * (kWalkBlock / 64) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t e0 = 0; e0 < nbig; e0 += 64) {
    uint4 ent = make_uint4(0, 0, 0, 0);  // (frame, first tile, tiles, -)
    if (e0 + lane < nbig) ent = big[e0 + lane];
    const uint32_t k0 = (wid + nw - ent.y % nw) % nw;
    uint64_t todo = __ballot(k0 < ent.z);
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t f = (uint32_t)__shfl((int)ent.x, src, 64), tiles = (uint32_t)__shfl((int)ent.z, src, 64);
      const gevws_frame rec = fr[f];
      const uint64_t L = (uint64_t)rec.hdr.length, nvec = (L + 15) >> 4;
      const uint8_t* __restrict__ p = payload + rec.payload_off;
      const uint32_t lead = part[f] & 7;
      uint32_t bad = 0;
      for (uint64_t k = (uint32_t)__shfl((int)k0, src, 64); k < tiles; k += nw) {
        for (uint64_t j0 = k * (kMsgBigTile / 16); j0 < (k + 1) * (kMsgBigTile / 16) && j0 < nvec;
             j0 += 64 * kMsgStepVecs) {
          u32x4 v[kMsgStepVecs];
          uint32_t pw[kMsgStepVecs];
#pragma unroll
          for (int u = 0; u < kMsgStepVecs; ++u) {
            const uint64_t j = j0 + (uint64_t)u * 64 + lane;
            if (j < nvec) {
              v[u] = *reinterpret_cast<const u32x4*>(p + 16 * j);
              pw[u] = j ? *reinterpret_cast<const uint32_t*>(p + 16 * j - 4) : 0u;
            }
          }
#pragma unroll
          for (int u = 0; u < kMsgStepVecs; ++u) {
            const uint64_t j = j0 + (uint64_t)u * 64 + lane;
            if (j < nvec) bad |= utf8_vec_bad(v[u], pw[u], j, L, lead);
          }
        }
      }
      if (__ballot(bad != 0) != 0 && lane == 0) atomicOr(part + f, kPartBad);
    }
  }
}

// ------------------------------------------------------------------ 3. stitch: parts onto the carry state
// One text fragment (L > 0 bytes at p, part summary pt) after the n pending
// bytes pend[]: false = a wrong byte in this frame; else pend / n are the
// unfinished sequence at its end.  Reads at most 3 + 3 payload bytes.
__device__ bool utf8_stitch(const uint8_t* __restrict__ p, uint64_t L, uint32_t pt, uint8_t (&pend)[3], uint32_t& n) {
  const uint32_t lead = pt & 7, tail = (pt >> 3) & 3;
  if (n) {
    const uint32_t need = utf8_need(pend[0]);
    if (n > need) return false;  // (not a state this layer writes)
    const uint32_t r = need - (n - 1);
    uint32_t p1 = pend[n - 1], p2 = n > 1 ? pend[n - 2] : 0u, p3 = n > 2 ? pend[n - 3] : 0u;
    const uint32_t m = L < r ? (uint32_t)L : r;
    for (uint32_t i = 0; i < m; ++i) {
      const uint32_t c = p[i];
      if (utf8_byte_bad(c, p1, p2, p3)) return false;
      p3 = p2, p2 = p1, p1 = c;
      if (n < 3) pend[n] = (uint8_t)c;
      ++n;
    }
    if (L < r) return true;  // still inside the sequence
    if (lead != r) return false;  // a continuation byte too many
  } else if (lead) {
    return false;
  }
  if (pt & kPartBad) return false;
  n = tail;
  for (uint32_t i = 0; i < tail; ++i) pend[i] = p[L - tail + i];
  return true;
}

__global__ __launch_bounds__(kWalkBlock) void k_msg_stitch(const gevws_frame* __restrict__ fr,
                                                           const gevws_conn_out* __restrict__ cout, uint32_t n_conns,
                                                           uint64_t max_frames, const gevws_summary* __restrict__ gate,
                                                           const uint8_t* __restrict__ payload,
                                                           const uint8_t* __restrict__ cls,
                                                           const uint32_t* __restrict__ part,
                                                           MsgConn* __restrict__ work, uint64_t* __restrict__ blk) {
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t nmsg = 0, text_bytes = 0, failed = 0;
  if (c < n_conns && work[c].active) {
    const uint64_t n = gated_count(max_frames, gate);
    MsgConn w = work[c];
    const gevws_conn_out co = cout[c];
    const uint64_t first = co.first_frame, end = co.nframes < n - first ? first + co.nframes : n;
    uint32_t open = w.st.opcode == 1 || w.st.opcode == 2 ? w.st.opcode : 0u;
    bool comp = w.ext && open && w.st.reserved[0];
    uint32_t pn = open == 1 && !comp && w.st.utf8_n <= 3 ? w.st.utf8_n : 0u;
    uint8_t pend[3] = {w.st.utf8[0], w.st.utf8[1], w.st.utf8[2]};
    bool in_batch = false;  // the open message has a data frame in this batch
    const uint64_t stop = w.err_frame < end ? w.err_frame : end;  // the frame-level error, if any
    bool done = false;
    for (uint64_t f0 = first; f0 < stop && !done; f0 += kMsgWalkBatch) {
      uint32_t kb[kMsgWalkBatch], ptb[kMsgWalkBatch];
      gevws_frame recb[kMsgWalkBatch];  // (a control or binary frame's is not used)
#pragma unroll
      for (int u = 0; u < kMsgWalkBatch; ++u)
        if (f0 + u < stop) kb[u] = cls[f0 + u], ptb[u] = part[f0 + u], recb[u] = fr[f0 + u];
#pragma unroll
      for (int u = 0; u < kMsgWalkBatch; ++u) {
        const uint64_t f = f0 + u;
        if (f >= stop) break;
        const uint32_t k = kb[u];
        if (!(k & kClsData)) continue;
        if (k & kClsBegin) open = k & kClsText ? 1u : 2u;
        if ((k & kClsBegin) || !in_batch) ++nmsg, in_batch = true;
        comp = (k & kClsComp) != 0;
        if ((k & kClsText) && !comp) {
          const uint64_t L = (uint64_t)recb[u].hdr.length;
          text_bytes += L;
          bool ok = L == 0 || utf8_stitch(payload + recb[u].payload_off, L, ptb[u], pend, pn);
          if (ok && (k & kClsEnd) && pn) ok = false;  // the message ends inside a sequence
          if (!ok) {
            w.err = GEVWS_MSG_ERR_UTF8;
            w.err_frame = f;
            done = true;
            break;
          }
        }
        if (k & kClsEnd) open = 0, in_batch = false, pn = 0;
      }
    }
    memset(&w.st, 0, sizeof(w.st));
    if (w.err) {
      w.st.failed = (uint8_t)w.err;
      failed = 1;
    } else {
      w.st.opcode = (uint8_t)open;
      w.st.utf8_n = (uint8_t)(open == 1 && !comp ? pn : 0u);
      w.st.reserved[0] = (uint8_t)(open && comp ? 1 : 0);
      for (uint32_t i = 0; i < w.st.utf8_n; ++i) w.st.utf8[i] = pend[i];
    }
    w.nmsg = (uint32_t)nmsg;
    work[c] = w;
  }
  // the workgroup's partial: [messages, 0, text bytes, failed connections]
  __shared__ uint64_t s_part[3][kWalkBlock / 64];
  const uint64_t vals[3] = {nmsg, text_bytes, failed};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t sm = wave_sum(vals[k]);
    if (lane == 0) s_part[k][wv] = sm;
  }
  __syncthreads();
  if (threadIdx.x < kBlkFields) {
    uint64_t sm = 0;
    const int fld = threadIdx.x == 0 ? 0 : (threadIdx.x == 1 ? -1 : (int)threadIdx.x - 1);
    if (fld >= 0)
      for (int j = 0; j < kWalkBlock / 64; ++j) sm += s_part[fld][j];
    blk[(uint64_t)blockIdx.x * kBlkFields + threadIdx.x] = sm;
  }
}

// ------------------------------------------------------------------ 4. emit
__global__ __launch_bounds__(kWalkBlock) void k_msg_emit(const gevws_frame* __restrict__ fr,
                                                         const gevws_conn_out* __restrict__ cout, uint32_t n_conns,
                                                         uint64_t max_frames, const gevws_summary* __restrict__ gate,
                                                         const uint8_t* __restrict__ cls,
                                                         const MsgConn* __restrict__ work,
                                                         const uint64_t* __restrict__ blk,
                                                         const gevws_summary* __restrict__ sum,
                                                         gevws_msg_state* __restrict__ state,
                                                         gevws_message* __restrict__ msgs,
                                                         int64_t* __restrict__ msg_of,
                                                         gevws_conn_msg* __restrict__ conn_msg) {
  if (sum->status != GEVWS_OK) return;  // capacity: nothing written, the state kept for the retry
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  MsgConn w;
  memset(&w, 0, sizeof(w));
  if (c < n_conns) w = work[c];
  const uint64_t v[1] = {w.nmsg};
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (c >= n_conns) return;
  const uint64_t base = blk[(uint64_t)blockIdx.x * kBlkFields] + ex[0];
  gevws_conn_msg cm;
  memset(&cm, 0, sizeof(cm));
  cm.first_message = base;
  cm.error_frame = w.err_frame;
  cm.nmessages = w.nmsg;
  cm.error = w.err;
  conn_msg[c] = cm;
  if (!w.active) return;
  const uint64_t n = gated_count(max_frames, gate);
  const gevws_conn_out co = cout[c];
  const uint64_t first = co.first_frame, end = co.nframes < n - first ? first + co.nframes : n;
  const bool utf8 = w.err == GEVWS_MSG_ERR_UTF8;
  // errors 1-5 stop before their frame, a UTF-8 error after it
  const uint64_t stop = w.err_frame < end ? w.err_frame + (utf8 ? 1 : 0) : end;
  gevws_message m;
  memset(&m, 0, sizeof(m));
  m.conn = c;
  uint64_t idx = base;
  bool in_batch = false;
  bool done = false;
  for (uint64_t f0 = first; f0 < stop && !done; f0 += kMsgWalkBatch) {
    uint32_t kb[kMsgWalkBatch];
    uint64_t lenb[kMsgWalkBatch];
#pragma unroll
    for (int u = 0; u < kMsgWalkBatch; ++u)
      if (f0 + u < stop) kb[u] = cls[f0 + u], lenb[u] = (uint64_t)fr[f0 + u].hdr.length;
#pragma unroll
    for (int u = 0; u < kMsgWalkBatch; ++u) {
      const uint64_t f = f0 + u;
      if (f >= stop) break;
      const uint32_t k = kb[u];
      if (!(k & kClsData)) continue;
      if ((k & kClsBegin) || !in_batch) {
        m.first_frame = f;
        m.length = 0;
        m.nframes = 0;
        m.opcode = k & kClsText ? 1 : 2;
        m.flags = (uint8_t)((k & kClsBegin ? GEVWS_MSG_BEGIN : 0u) | (k & kClsComp ? GEVWS_MSG_COMPRESSED : 0u));
        m.status = GEVWS_MSG_OK;
        in_batch = true;
      }
      m.length += lenb[u];
      m.nframes += 1;
      msg_of[f] = (int64_t)idx;
      if (utf8 && f == w.err_frame) {
        m.status = GEVWS_MSG_ERR_UTF8;
        done = true;
        break;
      }
      if (k & kClsEnd) {
        m.flags |= GEVWS_MSG_END;
        msgs[idx++] = m;
        in_batch = false;
      }
    }
  }
  if (in_batch) msgs[idx++] = m;
  if (state) state[c] = w.st;
}

}  // namespace

using namespace gevws_impl;

extern "C" {

int gevws_utf8_valid(const uint8_t* p, uint64_t n) {
  if (n && !p) return 0;
  uint32_t p1 = 0, p2 = 0, p3 = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t c = p[i];
    if (utf8_byte_bad(c, p1, p2, p3)) return 0;
    p3 = p2, p2 = p1, p1 = c;
  }
  return !(p1 >= 0xC0 || p2 >= 0xE0 || p3 >= 0xF0);  // not inside a sequence
}

int gevws_messages_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames, uint64_t max_frames,
                         const gevws_conn_out* d_conn_out, uint32_t n_conns, const gevws_summary* d_decoded,
                         const uint8_t* d_payload, gevws_msg_state* d_state, gevws_message* d_messages,
                         uint64_t max_messages, int64_t* d_msg_of, gevws_conn_msg* d_conn_msg,
                         gevws_summary* d_summary) {
  return gevws_messages_ext_async(ctx, stream, d_frames, max_frames, d_conn_out, n_conns, d_decoded, d_payload,
                                  d_state, d_messages, max_messages, d_msg_of, d_conn_msg, d_summary, nullptr);
}

int gevws_messages_ext_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames, uint64_t max_frames,
                             const gevws_conn_out* d_conn_out, uint32_t n_conns, const gevws_summary* d_decoded,
                             const uint8_t* d_payload, gevws_msg_state* d_state, gevws_message* d_messages,
                             uint64_t max_messages, int64_t* d_msg_of, gevws_conn_msg* d_conn_msg,
                             gevws_summary* d_summary, const uint8_t* d_conn_ext) {
  if (!ctx || !d_summary || max_frames > 0xFFFFFFFFull) return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (n_conns == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_conn_msg || (max_messages && !d_messages) ||
      (max_frames && (!d_frames || !d_conn_out || !d_decoded || !d_payload || !d_msg_of)))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (n_conns + kWalkBlock - 1) / kWalkBlock;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, msg_scratch(nullptr, max_frames, n_conns, nblk).total);
  if (r != GEVWS_OK) return r;
  const MsgScratch s = msg_scratch(ctx->scratch, max_frames, n_conns, nblk);
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  if (max_frames) GEVWS_HIP(hipMemsetAsync(d_msg_of, 0xFF, max_frames * sizeof(int64_t), st));  // -1: no message
  k_msg_classify<<<nblk, kWalkBlock, 0, st>>>(d_frames, max_frames, d_conn_out, n_conns, d_decoded, d_state, d_conn_ext,
                                              s.cls, s.conn);
  const uint32_t fblk = (uint32_t)((max_frames + kWalkBlock / 64 - 1) / (kWalkBlock / 64));
  if (fblk)
    k_msg_utf8_frames<<<fblk, kWalkBlock, 0, st>>>(d_frames, max_frames, d_decoded, d_payload, s.cls, s.part, s.ctl,
                                                   s.big);
  k_msg_utf8_big<<<(uint32_t)ctx->num_cus * kMsgWgPerCU, kWalkBlock, 0, st>>>(d_frames, d_payload, s.part, s.ctl,
                                                                              s.big);
  k_msg_stitch<<<nblk, kWalkBlock, 0, st>>>(d_frames, d_conn_out, n_conns, max_frames, d_decoded, d_payload, s.cls,
                                            s.part, s.conn, s.blk);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk, max_messages, UINT64_MAX, d_summary);
  k_msg_emit<<<nblk, kWalkBlock, 0, st>>>(d_frames, d_conn_out, n_conns, max_frames, d_decoded, s.cls, s.conn, s.blk,
                                          d_summary, d_state, d_messages, d_msg_of, d_conn_msg);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

}  // extern "C"
