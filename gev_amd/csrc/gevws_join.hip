// gevws_join.hip -- the two steps behind the message pass and the inflate
// (gevws_join_async, gevws_reply_bodies_async, include/gevws.h): every whole
// message gets one contiguous body, and the bodies become the deflate step's
// message list and the encoder's frame list on the device.  The reference has
// no code for either: HandlerWrap.OnMessage (plugins/websocket/wrap.go:71)
// hands every data frame to the user, fragment by fragment.
//
// The join: four launches behind one memset, no host round trip:
//   k_join_size    one lane per message: delivered or not, copied or not, its
//                  16-rounded size; block partials (the first partial is `base`)
//   k_scan_blocks  block bases, the summary
//   k_join_place   one lane per message: d_bodies, and for a copied message
//                  its place (mdst), its frames' span, each frame's running
//                  offset inside the message (foff), the output-tile -> message map
//   k_join_copy    the gather: the segmented copy k_send_gather runs too
//                  (gevws_segcopy.hpp), a fragment a segment; every workgroup a
//                  contiguous run of 4 KiB output tiles, a quarter of it a wave
// Only k_join_copy touches payload bytes: L read, L rounded up to 16 written a
// copied body.
//
// The carry (gevws_join_carry_async, gevws_join_carry_ext_async): the same four launches once more over
// the connections instead of the messages -- k_carry_size / k_scan_blocks /
// k_carry_place, then k_join_copy over the carry's tables into d_carry_dst --
// and k_carry_verdict between the scans and the place passes.  The kernels of
// the body side are templates on CARRY: <false> is the code of the NULL call,
// <true> gives a continued message the connection's carried bytes as one more
// fragment in front of its first frame.
//
// The reply step: k_reply_count / k_scan_blocks / k_reply_verdict /
// k_reply_emit, an order-preserving compaction of the delivered bodies into the
// two lists (fields 0 and 1 of the block partials are the two lists' counts).
#include "gevws_internal.hpp"
#include "gevws_segcopy.hpp"

namespace {

static_assert(sizeof(gevws_body) == 32 && offsetof(gevws_body, length) == 8 && offsetof(gevws_body, conn) == 16 &&
                  offsetof(gevws_body, opcode) == 20 && offsetof(gevws_body, flags) == 21 &&
                  offsetof(gevws_body, status) == 22, "gevws_body layout");
static_assert(sizeof(gevws_inflated) == 32 && sizeof(gevws_deflate_msg) == 24 && sizeof(gevws_out_frame) == 32,
              "record layouts");

constexpr int kJoinWalk = 4;  // fragments a wave steps forward to reach a tile's first byte before it bisects

// ------------------------------------------------------------------ scratch
// What a copied body has beside its frames: the first `pre` bytes come from
// carry_src[psrc, psrc + pre); its frames are those of message `msg`.
struct JoinExt {
  uint64_t pre, psrc, msg, reserved;
};
struct JoinScratch {
  uint64_t* ctl;        // [0] base, [1] the gated message count
  uint64_t* blk;        // [nblk + 1][kBlkFields]; partial 0 holds `base` in field 1
  uint64_t* mdst;       // [m] where message m's body starts in d_out (a message that is not copied: where the
                        //     next copied one starts), so the array never decreases
  uint2* span;          // [m] a copied message's first and last data frame
  uint64_t* foff;       // [f] bytes of the message before frame f, for every frame inside a copied message's span
  uint32_t* tile_msg;   // [t] the message that holds the first byte of output tile t (tiles count from `base`)
  // the carry's tables (n_conns != 0), the connection in the message's place
  uint64_t* cctl;       // [0] 0, [1] the gated connection count
  uint64_t* cblk;       // [nblkc][kCarryFields]
  JoinExt* ext;         // [m] a copied message's carried prefix
  JoinExt* cext;        // [c] an OPEN carry's prefix and the message its frames belong to
  gevws_body* cbody;    // [c] an OPEN carry's place in d_carry_dst as a JOINED body record
  uint64_t* cdst;       // [c] as mdst
  uint2* cspan;         // [c] as span
  uint32_t* ctile;      // [t] as tile_msg
  size_t zero_bytes, total;
};
constexpr int kCarryFields = 5;  // OPEN records, arena bytes, lengths, ERR_TOO_BIG, malformed records
inline JoinScratch join_scratch(void* base, uint64_t max_frames, uint64_t max_messages, uint32_t nblk,
                                uint64_t out_cap, uint32_t n_conns = 0, uint32_t nblkc = 0, uint64_t carry_cap = 0) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  JoinScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)(nblk + 1) * kBlkFields * sizeof(uint64_t));
  if (n_conns) {
    s.cctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
    s.cblk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblkc * kCarryFields * sizeof(uint64_t));
  }
  s.zero_bytes = o;
  s.mdst = reinterpret_cast<uint64_t*>(p + o), o += up(max_messages * 8);
  s.span = reinterpret_cast<uint2*>(p + o), o += up(max_messages * 8);
  s.foff = reinterpret_cast<uint64_t*>(p + o), o += up(max_frames * 8);
  s.tile_msg = reinterpret_cast<uint32_t*>(p + o), o += up((out_cap / kTile + 2) * 4);
  if (n_conns) {
    s.ext = reinterpret_cast<JoinExt*>(p + o), o += up(max_messages * 32);
    s.cext = reinterpret_cast<JoinExt*>(p + o), o += up((size_t)n_conns * 32);
    s.cbody = reinterpret_cast<gevws_body*>(p + o), o += up((size_t)n_conns * 32);
    s.cdst = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)n_conns * 8);
    s.cspan = reinterpret_cast<uint2*>(p + o), o += up((size_t)n_conns * 8);
    s.ctile = reinterpret_cast<uint32_t*>(p + o), o += up((carry_cap / kTile + 2) * 4);
  }
  s.total = o;
  return s;
}

// ------------------------------------------------------------------ what becomes of message m
struct JoinDec {
  uint64_t length;   // delivered bytes
  uint64_t inf_off;  // INFLATED: the inflate record's place
  uint32_t flags;    // GEVWS_BODY_*
  uint32_t status;
  bool copy;         // its bytes go to d_out in this call
};
__device__ __forceinline__ JoinDec join_decide(const gevws_message& m, const gevws_inflated* __restrict__ inflated,
                                               uint64_t idx, uint32_t call_flags) {
  JoinDec d;
  d.length = 0, d.inf_off = 0, d.flags = 0, d.status = m.status, d.copy = false;
  const bool whole = (m.flags & GEVWS_MSG_BEGIN) && (m.flags & GEVWS_MSG_END) && m.status == GEVWS_MSG_OK;
  if (m.flags & GEVWS_MSG_COMPRESSED) {
    if (!inflated) return d;
    const gevws_inflated r = inflated[idx];
    d.status = r.status;
    if (whole && (r.flags & GEVWS_INF_DONE) && r.status == GEVWS_MSG_OK) {
      d.flags = GEVWS_BODY_WHOLE | GEVWS_BODY_INFLATED;
      d.length = r.length, d.inf_off = r.out_off;
    }
    return d;
  }
  if (!whole) return d;
  d.length = m.length;
  d.copy = m.nframes >= 2 || (call_flags & GEVWS_JOIN_ALL);
  d.flags = GEVWS_BODY_WHOLE | (d.copy ? GEVWS_BODY_JOINED : 0u);
  return d;
}

// The carry arguments of the body side's <true> kernels.
struct JoinCarryIn {
  const gevws_carry* __restrict__ carry_in;  // may be null
  uint32_t n_conns;
  uint64_t max_bytes;
  uint32_t carry_flags;  // GEVWS_CARRY_KEEP_COMPRESSED (gevws_join_carry_ext_async), or 0
};
// join_decide with the connection's carry: a continued message that ends here
// is delivered behind its carried bytes (pre / psrc: where they are).  With
// KEEP_COMPRESSED a continued compressed message that ends here is the
// inflate's: delivered where its record says, nothing of it copied.
__device__ __forceinline__ JoinDec join_decide_carry(const gevws_message& m,
                                                     const gevws_inflated* __restrict__ inflated, uint64_t idx,
                                                     uint32_t call_flags, const JoinCarryIn& ca, uint64_t& pre,
                                                     uint64_t& psrc) {
  JoinDec d = join_decide(m, inflated, idx, call_flags);
  pre = psrc = 0;
  const bool keep = ca.carry_flags & GEVWS_CARRY_KEEP_COMPRESSED;
  if (keep && inflated && (m.flags & (GEVWS_MSG_BEGIN | GEVWS_MSG_COMPRESSED | GEVWS_MSG_END)) ==
                              (GEVWS_MSG_COMPRESSED | GEVWS_MSG_END)) {
    const gevws_inflated r = inflated[idx];  // (d.status is r.status already)
    if ((r.flags & GEVWS_INF_DONE) && r.status == GEVWS_MSG_OK) {
      d.flags = GEVWS_BODY_WHOLE | GEVWS_BODY_INFLATED;
      d.length = r.length, d.inf_off = r.out_off;
    }
    return d;
  }
  if ((m.flags & (GEVWS_MSG_BEGIN | GEVWS_MSG_COMPRESSED)) || !ca.carry_in || m.conn >= ca.n_conns) return d;
  const gevws_carry ci = ca.carry_in[m.conn];
  if (keep && (ci.flags & GEVWS_CARRY_OPEN) && (ci.flags & GEVWS_CARRY_COMPRESSED)) return d;  // not this message's
  if (ci.flags & GEVWS_CARRY_OPEN) {
    if ((m.flags & GEVWS_MSG_END) && m.status == GEVWS_MSG_OK) {
      const uint64_t total = ci.length + m.length;
      if (total >= ci.length && total <= ca.max_bytes) {
        d.length = total, d.copy = true;
        d.flags = GEVWS_BODY_WHOLE | GEVWS_BODY_JOINED;
        pre = ci.length, psrc = ci.off;
      } else {
        d.status = GEVWS_MSG_ERR_TOO_BIG;
      }
    }
  } else if ((ci.flags & GEVWS_CARRY_LOST) && ci.status) {
    d.status = ci.status;
  }
  return d;
}

// The messages of the call: the message pass's count, none when it or a given inflate failed.
__device__ __forceinline__ uint64_t join_count(uint64_t max_messages, const gevws_summary* __restrict__ msg_sum,
                                               const gevws_summary* __restrict__ inf_sum) {
  if (inf_sum && inf_sum->status != GEVWS_OK) return 0;
  return gated_count(max_messages, msg_sum);
}

// ------------------------------------------------------------------ 1. sizes
template <bool CARRY>
__global__ __launch_bounds__(kWalkBlock) void k_join_size(const gevws_message* __restrict__ msgs,
                                                          uint64_t max_messages,
                                                          const gevws_summary* __restrict__ msg_sum,
                                                          const gevws_inflated* __restrict__ inflated,
                                                          const gevws_summary* __restrict__ inf_sum,
                                                          uint32_t call_flags, uint64_t* __restrict__ ctl,
                                                          uint64_t* __restrict__ blk, JoinCarryIn ca) {
  const uint64_t n = join_count(max_messages, msg_sum, inf_sum);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[CARRY ? 4 : 3] = {};  // delivered, bytes taken in d_out, delivered length; CARRY: malformed records
  if (m < n) {
    JoinDec d;
    if constexpr (CARRY) {
      const gevws_message msg = msgs[m];
      uint64_t pre, psrc;
      d = join_decide_carry(msg, inflated, m, call_flags, ca, pre, psrc);
      vals[3] = msg.conn >= ca.n_conns;  // (the verdict pass moves the count out of `errors`)
    } else {
      d = join_decide(msgs[m], inflated, m, call_flags);
    }
    vals[0] = d.flags ? 1 : 0;
    vals[1] = d.copy ? round16(d.length) : 0;
    vals[2] = d.length;
  }
  block_partial<CARRY ? 4 : 3>(vals, blk, (uint64_t)blockIdx.x + 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // joined bodies start behind the inflate's bytes (a call without messages reads none of its inputs)
    const uint64_t base = n && inf_sum ? round16(inf_sum->payload_bytes) : 0;
    ctl[0] = base;
    ctl[1] = n;
    blk[1] = base;  // partial 0, field 1: every block's base and the summary's payload_bytes include it
  }
}

// ------------------------------------------------------------------ 2. records and maps
template <bool CARRY>
__global__ __launch_bounds__(kWalkBlock) void k_join_place(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                                           const gevws_message* __restrict__ msgs,
                                                           const int64_t* __restrict__ msg_of,
                                                           const gevws_inflated* __restrict__ inflated,
                                                           uint32_t call_flags, const uint64_t* __restrict__ ctl,
                                                           const uint64_t* __restrict__ blk,
                                                           const gevws_summary* __restrict__ sum,
                                                           gevws_body* __restrict__ bodies,
                                                           uint64_t* __restrict__ mdst, uint2* __restrict__ span,
                                                           uint64_t* __restrict__ foff,
                                                           uint32_t* __restrict__ tile_msg, JoinCarryIn ca,
                                                           const gevws_summary* __restrict__ carry_sum,
                                                           JoinExt* __restrict__ ext) {
  if (sum->status != GEVWS_OK) return;  // capacity: nothing written
  if constexpr (CARRY)
    if (carry_sum->status != GEVWS_OK) return;  // either side failing suppresses both
  const uint64_t n = ctl[1], base = ctl[0];
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  gevws_message msg;
  memset(&msg, 0, sizeof(msg));
  JoinDec d;
  memset(&d, 0, sizeof(d));
  uint64_t pre = 0, psrc = 0;
  if (m < n) {
    msg = msgs[m];
    if constexpr (CARRY) d = join_decide_carry(msg, inflated, m, call_flags, ca, pre, psrc);
    else d = join_decide(msg, inflated, m, call_flags);
  }
  const uint64_t padded = d.copy ? round16(d.length) : 0;
  const uint64_t v[1] = {padded};
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (m >= n) return;
  const uint64_t dst = blk[((uint64_t)blockIdx.x + 1) * kBlkFields + 1] + ex[0];  // (exclusive after the scan)
  mdst[m] = dst;
  gevws_body b;
  memset(&b, 0, sizeof(b));
  b.conn = msg.conn;
  b.opcode = msg.opcode;
  b.flags = (uint8_t)d.flags;
  b.status = (uint8_t)d.status;
  if (d.flags) {
    b.length = d.length;
    if (d.flags & GEVWS_BODY_INFLATED) b.off = d.inf_off;
    else if (d.copy) b.off = dst;
    else b.off = msg.first_frame < max_frames ? fr[msg.first_frame].payload_off : 0;  // its one frame's slot
  }
  bodies[m] = b;
  if constexpr (CARRY) ext[m] = JoinExt{pre, psrc, m, 0};
  if (!padded) return;
  // the frames' running offsets; control frames in between get theirs too, so
  // the array never decreases over the span and a bisection finds a byte's frame
  // (CARRY: the carried bytes are one more fragment in front of first_frame)
  uint64_t run = CARRY ? pre : 0, last = msg.first_frame;
  uint32_t seen = 0;
  for (uint64_t f0 = msg.first_frame; f0 < max_frames && seen < msg.nframes; f0 += 4) {
    int64_t ofb[4];
    uint64_t lenb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (f0 + u < max_frames) ofb[u] = msg_of[f0 + u], lenb[u] = (uint64_t)fr[f0 + u].hdr.length;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t f = f0 + u;
      if (f >= max_frames || seen >= msg.nframes) break;
      foff[f] = run;
      if (ofb[u] == (int64_t)m) run += lenb[u], ++seen, last = f;
    }
  }
  span[m] = make_uint2((uint32_t)msg.first_frame, (uint32_t)last);
  const uint64_t r0 = dst - base;
  for (uint64_t t = (r0 + kTile - 1) / kTile; t * kTile < r0 + padded; ++t) tile_msg[t] = (uint32_t)m;
}

// ------------------------------------------------------------------ 3. the gather
// One fragment's counted bytes: d_out[ds, de) come from src[0, de - ds).
struct JoinFrag {
  uint64_t ds, de;
  const uint8_t* src;
  uint64_t m, f, last, body_end;  // its message and frame, the message's last frame, the end of its body in d_out
};
// The map of the segmented copy (gevws_segcopy.hpp): a fragment a segment,
// the tile map's entries messages, no gap inside a body.
template <bool CARRY>
struct JoinMaps {
  using Seg = JoinFrag;
  const gevws_frame* __restrict__ fr;
  const int64_t* __restrict__ msg_of;
  const gevws_body* __restrict__ bodies;
  const uint64_t* __restrict__ mdst;
  const uint2* __restrict__ span;
  const uint64_t* __restrict__ foff;
  const uint8_t* __restrict__ payload;
  uint64_t nframes;
  // CARRY: the bodies' carried prefixes
  const JoinExt* __restrict__ ext;
  const uint8_t* __restrict__ carry_src;
  uint64_t carry_src_bytes;

  // The fragment that holds byte x of d_out, x inside a copied body of a
  // message in [mlo, mhi]; false: x is a pad byte.
  __device__ __forceinline__ bool find(uint64_t x, uint64_t mlo, uint64_t mhi, Seg& g) const {
    uint64_t lo = mlo, hi = mhi;
    while (lo < hi) {  // the last message that starts at or before x: the later ones at its place take no space
      const uint64_t mid = (lo + hi + 1) >> 1;
      if (mdst[mid] <= x) lo = mid;
      else hi = mid - 1;
    }
    const gevws_body b = bodies[lo];
    if (!(b.flags & GEVWS_BODY_JOINED) || x < b.off || x - b.off >= b.length) return false;
    const uint64_t pos = x - b.off;
    const uint2 sp = span[lo];
    uint64_t flo = sp.x, fhi = sp.y;
    uint64_t owner = lo;  // the message its frames map to in msg_of
    if constexpr (CARRY) {
      const JoinExt e = ext[lo];
      owner = e.msg;
      if (pos < e.pre) {  // below foff[first_frame]: the prefix, a fragment whose successor is first_frame
        if (e.psrc > carry_src_bytes || e.pre > carry_src_bytes - e.psrc) return false;
        const bool frames = flo <= fhi && fhi < nframes;
        g.ds = b.off, g.de = b.off + e.pre;
        g.src = carry_src + e.psrc;
        g.m = owner, g.f = frames ? flo - 1 : 1, g.last = frames ? fhi : 0, g.body_end = b.off + b.length;
        return true;
      }
    }
    if (fhi >= nframes || flo > fhi) return false;
    const uint64_t last = fhi;
    while (flo < fhi) {  // the last frame that starts at or before pos: it holds the byte
      const uint64_t mid = (flo + fhi + 1) >> 1;
      if (foff[mid] <= pos) flo = mid;
      else fhi = mid - 1;
    }
    const gevws_frame rec = fr[flo];
    const uint64_t fo = foff[flo], len = (uint64_t)rec.hdr.length;
    if (pos < fo || pos - fo >= len) return false;
    g.ds = b.off + fo;
    g.de = g.ds + len;
    g.src = payload + rec.payload_off;
    g.m = owner, g.f = flo, g.last = last, g.body_end = b.off + b.length;
    return true;
  }
  // g -> the message's next fragment with bytes, which follows it in d_out; false: g was the last.
  // (Not a table the place kernel writes: control frames and empty fragments are skipped here.)
  __device__ __forceinline__ bool next(Seg& g) const {
    if (g.de >= g.body_end) return false;
    for (uint64_t f = g.f + 1; f <= g.last; ++f) {
      const gevws_frame rec = fr[f];
      const uint64_t len = (uint64_t)rec.hdr.length;
      if (len && msg_of[f] == (int64_t)g.m) {
        g.f = f;
        g.ds = g.de, g.de = g.ds + len;
        g.src = payload + rec.payload_off;
        return true;
      }
    }
    return false;
  }
  // A tile's first byte: a few long fragments on in the same body, then the bisections.
  __device__ __forceinline__ bool seek(uint64_t T, uint64_t mlo, uint64_t mhi, bool have, Seg& g) const {
    if (have && T >= g.de && T < g.body_end && g.de - g.ds >= kSegRowBytes)
      for (int k = 0; k < kJoinWalk && next(g); ++k)
        if (T < g.de) return true;
    return find(T, mlo, mhi, g);
  }
  // A fragment's fields in SGPRs (every lane computed the same ones).
  static __device__ __forceinline__ void uniform(Seg& g) {
    g.ds = uniform64(g.ds), g.de = uniform64(g.de);
    g.src = reinterpret_cast<const uint8_t*>(uniform64(reinterpret_cast<uintptr_t>(g.src)));
    g.m = uniform64(g.m), g.f = uniform64(g.f), g.last = uniform64(g.last), g.body_end = uniform64(g.body_end);
  }
};

template <bool CARRY>
__global__ __launch_bounds__(kSegBlock) void k_join_copy(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                                         const int64_t* __restrict__ msg_of,
                                                         const uint8_t* __restrict__ payload,
                                                         const gevws_body* __restrict__ bodies,
                                                         const uint64_t* __restrict__ mdst,
                                                         const uint2* __restrict__ span,
                                                         const uint64_t* __restrict__ foff,
                                                         const uint32_t* __restrict__ tile_msg,
                                                         const uint64_t* __restrict__ ctl,
                                                         const gevws_summary* __restrict__ sum,
                                                         uint8_t* __restrict__ out,
                                                         const gevws_summary* __restrict__ other_sum,
                                                         const JoinExt* __restrict__ ext,
                                                         const uint8_t* __restrict__ carry_src,
                                                         uint64_t carry_src_bytes) {
  if (sum->status != GEVWS_OK) return;
  if constexpr (CARRY)
    if (other_sum->status != GEVWS_OK) return;  // either side failing suppresses both
  const uint64_t base = ctl[0], n = ctl[1], end = sum->payload_bytes;  // the joined region is d_out[base, end)
  if (end <= base || n == 0) return;
  const JoinMaps<CARRY> M{fr, msg_of, bodies, mdst, span, foff, payload, max_frames, ext, carry_src, carry_src_bytes};
  const uint64_t ntiles = (end - base + kTile - 1) / kTile;
  // a workgroup's run of tiles is its four waves' runs, one behind the other
  const uint64_t nw = (uint64_t)gridDim.x * kSegWaves, gw = (uint64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
  const uint64_t per = (ntiles + nw - 1) / nw;
  const uint64_t t0 = gw * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  seg_copy_tiles(M, tile_msg, n, base, end, t0, t1, 1, out);
}

// ------------------------------------------------------------------ the carry side
static_assert(sizeof(gevws_carry) == 32 && offsetof(gevws_carry, length) == 8 && offsetof(gevws_carry, opcode) == 16 &&
                  offsetof(gevws_carry, flags) == 17 && offsetof(gevws_carry, status) == 18 &&
                  offsetof(gevws_carry, reserved) == 19 && sizeof(JoinExt) == 32, "gevws_carry layout");

// What becomes of connection c's carry.
struct CarryDec {
  uint64_t length, pre, psrc;  // OPEN: the bytes kept, of which the first `pre` are carried in from psrc
  int64_t msg;                 // the open message whose frames follow the prefix, or -1
  uint32_t too_big;            // bodies and carries of the connection that became ERR_TOO_BIG
  uint8_t opcode, flags, status;
  bool invalid;
};
struct CarryIn {
  const gevws_message* __restrict__ msgs;
  const gevws_conn_msg* __restrict__ conn_msg;
  const gevws_carry* __restrict__ carry_in;  // may be null
  uint64_t carry_src_bytes, max_bytes;
  uint32_t n_conns;
  uint32_t carry_flags;  // GEVWS_CARRY_KEEP_COMPRESSED, or 0
};
// n: the gated message count.  Nothing is indexed by a field before it is checked.
// With KEEP_COMPRESSED an open compressed message is kept like a plain one,
// its record marked COMPRESSED; a record and a message that disagree in that
// bit (the caller mixed up its states) end LOST.
__device__ __forceinline__ CarryDec carry_decide(const CarryIn& in, uint32_t c, uint64_t n) {
  CarryDec d;
  memset(&d, 0, sizeof(d));
  d.msg = -1;
  const gevws_conn_msg cm = in.conn_msg[c];
  gevws_carry ci;
  memset(&ci, 0, sizeof(ci));
  if (in.carry_in) ci = in.carry_in[c];
  if ((ci.flags & GEVWS_CARRY_OPEN) &&
      ((ci.off & 15) || ci.off > in.carry_src_bytes || ci.length > in.carry_src_bytes - ci.off))
    d.invalid = true;
  else if (cm.first_message > n || cm.nmessages > n - cm.first_message)
    d.invalid = true;
  if (d.invalid) return d;
  const bool keep = in.carry_flags & GEVWS_CARRY_KEEP_COMPRESSED;
  const uint8_t ci_comp = keep ? (ci.flags & GEVWS_CARRY_COMPRESSED) : 0;  // (without the flag the bit is not looked at)
  if (cm.nmessages) {  // the body side's verdict on a continued message that ends here
    const gevws_message f = in.msgs[cm.first_message];
    if (!(f.flags & (GEVWS_MSG_BEGIN | GEVWS_MSG_COMPRESSED)) && (f.flags & GEVWS_MSG_END) &&
        f.status == GEVWS_MSG_OK && (ci.flags & GEVWS_CARRY_OPEN) && !ci_comp &&
        (ci.length + f.length < ci.length || ci.length + f.length > in.max_bytes))
      d.too_big = 1;
  }
  if (cm.error != 0) return d;  // the carry is dropped
  if (cm.nmessages == 0) {      // the record moves forward
    if (ci.flags & GEVWS_CARRY_OPEN) {
      d.flags = GEVWS_CARRY_OPEN | ci_comp, d.opcode = ci.opcode;
      d.length = d.pre = ci.length, d.psrc = ci.off;
    } else if (ci.flags & GEVWS_CARRY_LOST) {
      d.flags = GEVWS_CARRY_LOST, d.opcode = ci.opcode, d.status = ci.status;
    }
  } else {
    const uint64_t li = cm.first_message + cm.nmessages - 1;
    const gevws_message l = in.msgs[li];
    if (l.flags & GEVWS_MSG_END) return d;
    d.opcode = l.opcode;
    const bool begin = l.flags & GEVWS_MSG_BEGIN;
    const uint8_t comp = keep && (l.flags & GEVWS_MSG_COMPRESSED) ? GEVWS_CARRY_COMPRESSED : 0;
    if ((l.flags & GEVWS_MSG_COMPRESSED) && !keep) {
      d.flags = GEVWS_CARRY_LOST;
      d.status = !begin && (ci.flags & GEVWS_CARRY_LOST) ? ci.status : 0;
    } else if (begin) {
      d.flags = GEVWS_CARRY_OPEN | comp, d.length = l.length, d.msg = (int64_t)li;
    } else if ((ci.flags & GEVWS_CARRY_OPEN) && comp != ci_comp) {
      d.flags = GEVWS_CARRY_LOST;  // status 0
    } else if (ci.flags & GEVWS_CARRY_OPEN) {
      d.flags = GEVWS_CARRY_OPEN | comp, d.pre = ci.length, d.psrc = ci.off, d.msg = (int64_t)li;
      d.length = ci.length + l.length;
      if (d.length < ci.length) d.length = UINT64_MAX;  // (over any limit)
    } else {
      d.flags = GEVWS_CARRY_LOST;
      d.status = (ci.flags & GEVWS_CARRY_LOST) ? ci.status : 0;
    }
  }
  if ((d.flags & GEVWS_CARRY_OPEN) && d.length > in.max_bytes) {
    d.flags = GEVWS_CARRY_LOST, d.status = GEVWS_MSG_ERR_TOO_BIG;
    d.length = d.pre = d.psrc = 0, d.msg = -1;
    d.too_big += 1;
  }
  return d;
}
// The connections of the call: all of them, none when the message pass or a given inflate failed.
__device__ __forceinline__ bool carry_gate(const gevws_summary* __restrict__ msg_sum,
                                           const gevws_summary* __restrict__ inf_sum) {
  return !(msg_sum && msg_sum->status != GEVWS_OK) && !(inf_sum && inf_sum->status != GEVWS_OK);
}

__global__ __launch_bounds__(kWalkBlock) void k_carry_size(CarryIn in, uint64_t max_messages,
                                                           const gevws_summary* __restrict__ msg_sum,
                                                           const gevws_summary* __restrict__ inf_sum,
                                                           uint64_t* __restrict__ cctl, uint64_t* __restrict__ cblk) {
  const bool open = carry_gate(msg_sum, inf_sum);
  const uint64_t n = open ? gated_count(max_messages, msg_sum) : 0;
  const uint64_t c = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[kCarryFields] = {};
  if (open && c < in.n_conns) {
    const CarryDec d = carry_decide(in, (uint32_t)c, n);
    const bool keep = d.flags & GEVWS_CARRY_OPEN;
    vals[0] = keep, vals[1] = keep ? round16(d.length) : 0, vals[2] = keep ? d.length : 0;
    vals[3] = d.too_big, vals[4] = d.invalid;
  }
  block_partial<kCarryFields, kCarryFields>(vals, cblk, blockIdx.x);
  if (blockIdx.x == 0 && threadIdx.x == 0) cctl[0] = 0, cctl[1] = open ? in.n_conns : 0;
}

// Behind both scans, one lane: the gates' status or ERR_INVALID into both
// summaries, before a place pass could write.  The scans left the malformed
// messages in body->errors and the malformed connections in carry->run_frames.
__global__ void k_carry_verdict(const gevws_summary* __restrict__ msg_sum, const gevws_summary* __restrict__ inf_sum,
                                gevws_summary* __restrict__ body, gevws_summary* __restrict__ carry) {
  gevws_summary a = *body, b = *carry, z;
  memset(&z, 0, sizeof(z));
  const uint64_t bad = a.errors + b.run_frames;
  a.errors = 0, b.run_frames = 0;
  if (msg_sum && msg_sum->status != GEVWS_OK) z.status = msg_sum->status, a = b = z;
  else if (inf_sum && inf_sum->status != GEVWS_OK) z.status = inf_sum->status, a = b = z;
  else if (bad) z.errors = bad, z.status = GEVWS_ERR_INVALID, a = b = z;
  *body = a;
  *carry = b;
}

__global__ __launch_bounds__(kWalkBlock) void k_carry_place(
    const gevws_frame* __restrict__ fr, uint64_t max_frames, const int64_t* __restrict__ msg_of, CarryIn in,
    uint64_t max_messages, const gevws_summary* __restrict__ msg_sum, const uint64_t* __restrict__ cblk,
    const gevws_summary* __restrict__ sum, const gevws_summary* __restrict__ body_sum,
    gevws_carry* __restrict__ carry_out, gevws_body* __restrict__ cbody, uint64_t* __restrict__ cdst,
    uint2* __restrict__ cspan, JoinExt* __restrict__ cext, uint64_t* __restrict__ foff,
    uint32_t* __restrict__ ctile) {
  if (sum->status != GEVWS_OK || body_sum->status != GEVWS_OK) return;  // either side failing suppresses both
  const uint64_t n = gated_count(max_messages, msg_sum);
  const uint64_t c = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  CarryDec d;
  memset(&d, 0, sizeof(d));
  if (c < in.n_conns) d = carry_decide(in, (uint32_t)c, n);
  const bool keep = d.flags & GEVWS_CARRY_OPEN;
  const uint64_t padded = keep ? round16(d.length) : 0;
  const uint64_t v[1] = {padded};
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (c >= in.n_conns) return;
  const uint64_t dst = cblk[(uint64_t)blockIdx.x * kCarryFields + 1] + ex[0];
  cdst[c] = dst;
  gevws_carry o;
  memset(&o, 0, sizeof(o));
  gevws_body b;
  memset(&b, 0, sizeof(b));
  if (d.flags) o.opcode = d.opcode, o.flags = d.flags, o.status = d.status;
  if (keep) {
    o.off = b.off = dst, o.length = b.length = d.length;
    b.conn = (uint32_t)c, b.opcode = d.opcode, b.flags = GEVWS_BODY_WHOLE | GEVWS_BODY_JOINED;
  }
  carry_out[c] = o;
  cbody[c] = b;
  cext[c] = JoinExt{d.pre, d.psrc, (uint64_t)d.msg, 0};
  if (!padded) return;
  uint2 sp = make_uint2(1, 0);  // no frames: the carried bytes alone
  if (d.msg >= 0) {
    const gevws_message msg = in.msgs[d.msg];
    uint64_t run = d.pre, last = msg.first_frame;
    uint32_t seen = 0;
    for (uint64_t f = msg.first_frame; f < max_frames && seen < msg.nframes; ++f) {
      foff[f] = run;
      if (msg_of[f] == d.msg) run += (uint64_t)fr[f].hdr.length, ++seen, last = f;
    }
    sp = make_uint2((uint32_t)msg.first_frame, (uint32_t)last);
  }
  cspan[c] = sp;
  for (uint64_t t = (dst + kTile - 1) / kTile; t * kTile < dst + padded; ++t) ctile[t] = (uint32_t)c;
}

// ------------------------------------------------------------------ the reply step
struct ReplyDec {
  bool reply, bad, deflate;
};
__device__ __forceinline__ ReplyDec reply_decide(const gevws_body& b, int policy,
                                                 const uint8_t* __restrict__ conn_ext, uint32_t n_conns) {
  ReplyDec r{false, false, false};
  if (policy == GEVWS_HANDLER_NONE || !(b.flags & GEVWS_BODY_WHOLE)) return r;
  // both lists address one arena: a body left in its frame's slot has no place in them
  if (!(b.flags & (GEVWS_BODY_JOINED | GEVWS_BODY_INFLATED)) || b.conn >= n_conns) {
    r.bad = true;
    return r;
  }
  r.reply = true;
  r.deflate = conn_ext && (conn_ext[b.conn] & GEVWS_EXT_DEFLATE);
  return r;
}
__device__ __forceinline__ uint64_t reply_count(uint64_t max_messages, const gevws_summary* __restrict__ msg_sum,
                                                const gevws_summary* __restrict__ join_sum) {
  if (join_sum->status != GEVWS_OK) return 0;
  return gated_count(max_messages, msg_sum);
}

__global__ __launch_bounds__(kWalkBlock) void k_reply_count(const gevws_body* __restrict__ bodies,
                                                            uint64_t max_messages,
                                                            const gevws_summary* __restrict__ msg_sum,
                                                            const gevws_summary* __restrict__ join_sum, int policy,
                                                            const uint8_t* __restrict__ conn_ext, uint32_t n_conns,
                                                            uint64_t* __restrict__ blk) {
  const uint64_t n = reply_count(max_messages, msg_sum, join_sum);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[3] = {0, 0, 0};  // deflate-list entries, plain-list entries, malformed records
  if (m < n) {
    const ReplyDec r = reply_decide(bodies[m], policy, conn_ext, n_conns);
    vals[0] = r.reply && r.deflate, vals[1] = r.reply && !r.deflate, vals[2] = r.bad;
  }
  block_partial<3>(vals, blk, blockIdx.x);
}

// The scan left {deflate entries, plain entries, malformed} in *def_sum's
// frames / payload_bytes / payload_len: the two summaries from them.
__global__ void k_reply_verdict(gevws_summary* __restrict__ def_sum, gevws_summary* __restrict__ plain_sum) {
  const gevws_summary s = *def_sum;
  gevws_summary a, b;
  memset(&a, 0, sizeof(a));
  memset(&b, 0, sizeof(b));
  if (s.payload_len) {
    a.errors = b.errors = s.payload_len;
    a.status = b.status = GEVWS_ERR_INVALID;
  } else {
    a.frames = s.frames;
    b.frames = s.payload_bytes;
  }
  *def_sum = a;
  *plain_sum = b;
}

__global__ __launch_bounds__(kWalkBlock) void k_reply_emit(const gevws_body* __restrict__ bodies,
                                                           uint64_t max_messages,
                                                           const gevws_summary* __restrict__ msg_sum,
                                                           const gevws_summary* __restrict__ join_sum, int policy,
                                                           const uint8_t* __restrict__ conn_ext,
                                                           const uint8_t* __restrict__ conn_wbits, uint32_t n_conns,
                                                           const uint64_t* __restrict__ blk,
                                                           const gevws_summary* __restrict__ def_sum,
                                                           gevws_deflate_msg* __restrict__ def_msgs,
                                                           uint32_t* __restrict__ def_conn,
                                                           gevws_out_frame* __restrict__ plain,
                                                           uint32_t* __restrict__ plain_conn,
                                                           int64_t* __restrict__ reply_of) {
  if (def_sum->status != GEVWS_OK) return;  // a malformed record: nothing written
  const uint64_t n = reply_count(max_messages, msg_sum, join_sum);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  gevws_body b;
  memset(&b, 0, sizeof(b));
  ReplyDec r{false, false, false};
  if (m < n) {
    b = bodies[m];
    r = reply_decide(b, policy, conn_ext, n_conns);
  }
  const uint64_t v[2] = {(uint64_t)(r.reply && r.deflate), (uint64_t)(r.reply && !r.deflate)};
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (m >= n) return;
  const uint8_t op = policy == GEVWS_HANDLER_ECHO_TEXT ? 1 : 2;
  int64_t idx = -1;
  if (r.reply && r.deflate) {
    const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
    gevws_deflate_msg d;
    memset(&d, 0, sizeof(d));
    d.payload_off = b.off;
    d.length = b.length;
    d.opcode = op;
    d.window_bits = conn_wbits ? conn_wbits[b.conn] : 0;
    def_msgs[k] = d;
    def_conn[k] = b.conn;
    idx = (int64_t)k;
  } else if (r.reply) {
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
    idx = (int64_t)k;
  }
  reply_of[m] = idx;
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_join_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames, uint64_t max_frames,
                                const gevws_message* d_messages, uint64_t max_messages, const int64_t* d_msg_of,
                                const gevws_summary* d_msg_summary, const uint8_t* d_payload,
                                const gevws_inflated* d_inflated, const gevws_summary* d_inflate_summary,
                                uint32_t flags, gevws_body* d_bodies, uint8_t* d_out, uint64_t out_cap,
                                gevws_summary* d_summary) {
  return gevws_join_carry_async(ctx, stream, d_frames, max_frames, d_messages, max_messages, d_msg_of, d_msg_summary,
                                d_payload, d_inflated, d_inflate_summary, flags, d_bodies, d_out, out_cap, d_summary,
                                nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr);
}

// The call with a carry: both sides' size / scan, the verdict, both sides' place, both gathers.
static int join_with_carry(gevws_ctx* ctx, hipStream_t st, const gevws_frame* d_frames, uint64_t max_frames,
                           const gevws_message* d_messages, uint64_t max_messages, const int64_t* d_msg_of,
                           const gevws_summary* d_msg_summary, const uint8_t* d_payload,
                           const gevws_inflated* d_inflated, const gevws_summary* d_inflate_summary, uint32_t flags,
                           gevws_body* d_bodies, uint8_t* d_out, uint64_t out_cap, gevws_summary* d_summary,
                           const gevws_conn_msg* d_conn_msg, uint32_t n_conns, uint64_t max_message_bytes,
                           const gevws_carry* d_carry_in, const uint8_t* d_carry_src, uint64_t carry_src_bytes,
                           gevws_carry* d_carry_out, uint8_t* d_carry_dst, uint64_t carry_cap,
                           gevws_summary* d_carry_summary, uint32_t carry_flags) {
  if (max_message_bytes == 0 || max_message_bytes > 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(d_carry_dst) & 15) ||
      (reinterpret_cast<uintptr_t>(d_carry_src) & 15) || (d_carry_in && carry_src_bytes && !d_carry_src))
    return GEVWS_ERR_INVALID;
  if (n_conns == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    GEVWS_HIP(hipMemsetAsync(d_carry_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (max_messages &&
      (!d_frames || !d_messages || !d_msg_of || !d_msg_summary || !d_payload || !d_bodies || !d_out ||
       (reinterpret_cast<uintptr_t>(d_payload) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15)))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_messages + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkc = (n_conns + kWalkBlock - 1) / kWalkBlock;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, join_scratch(nullptr, max_frames, max_messages, nblk, out_cap, n_conns, nblkc, carry_cap).total);
  if (r != GEVWS_OK) return r;
  const JoinScratch s = join_scratch(ctx->scratch, max_frames, max_messages, nblk, out_cap, n_conns, nblkc, carry_cap);
  const JoinCarryIn ca{d_carry_in, n_conns, max_message_bytes, carry_flags};
  const CarryIn in{d_messages, d_conn_msg, d_carry_in, carry_src_bytes, max_message_bytes, n_conns, carry_flags};
  const uint32_t grid = (uint32_t)ctx->num_cus * kSegWgPerCU;
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  if (max_messages) {
    k_join_size<true><<<nblk, kWalkBlock, 0, st>>>(d_messages, max_messages, d_msg_summary, d_inflated,
                                                   d_inflate_summary, flags, s.ctl, s.blk, ca);
    k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk + 1, UINT64_MAX, out_cap, d_summary);
  } else {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
  }
  k_carry_size<<<nblkc, kWalkBlock, 0, st>>>(in, max_messages, d_msg_summary, d_inflate_summary, s.cctl, s.cblk);
  k_scan_blocks<false, kCarryFields, kWalkBlock><<<1, kWalkBlock, 0, st>>>(s.cblk, nblkc, UINT64_MAX, carry_cap, d_carry_summary);
  k_carry_verdict<<<1, 1, 0, st>>>(d_msg_summary, d_inflate_summary, d_summary, d_carry_summary);
  if (max_messages)
    k_join_place<true><<<nblk, kWalkBlock, 0, st>>>(d_frames, max_frames, d_messages, d_msg_of, d_inflated, flags,
                                                    s.ctl, s.blk, d_summary, d_bodies, s.mdst, s.span, s.foff,
                                                    s.tile_msg, ca, d_carry_summary, s.ext);
  k_carry_place<<<nblkc, kWalkBlock, 0, st>>>(d_frames, max_frames, d_msg_of, in, max_messages, d_msg_summary, s.cblk,
                                              d_carry_summary, d_summary, d_carry_out, s.cbody, s.cdst, s.cspan,
                                              s.cext, s.foff, s.ctile);
  if (max_messages)
    k_join_copy<true><<<grid, kSegBlock, 0, st>>>(d_frames, max_frames, d_msg_of, d_payload, d_bodies, s.mdst, s.span,
                                                  s.foff, s.tile_msg, s.ctl, d_summary, d_out, d_carry_summary,
                                                  s.ext, d_carry_src, carry_src_bytes);
  k_join_copy<true><<<grid, kSegBlock, 0, st>>>(d_frames, max_frames, d_msg_of, d_payload, s.cbody, s.cdst, s.cspan,
                                                s.foff, s.ctile, s.cctl, d_carry_summary, d_carry_dst, d_summary,
                                                s.cext, d_carry_src, carry_src_bytes);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_join_carry_ext_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames,
                                          uint64_t max_frames, const gevws_message* d_messages, uint64_t max_messages,
                                          const int64_t* d_msg_of, const gevws_summary* d_msg_summary,
                                          const uint8_t* d_payload, const gevws_inflated* d_inflated,
                                          const gevws_summary* d_inflate_summary, uint32_t flags,
                                          gevws_body* d_bodies, uint8_t* d_out, uint64_t out_cap,
                                          gevws_summary* d_summary, const gevws_conn_msg* d_conn_msg,
                                          uint32_t n_conns, uint64_t max_message_bytes,
                                          const gevws_carry* d_carry_in, const uint8_t* d_carry_src,
                                          uint64_t carry_src_bytes, gevws_carry* d_carry_out, uint8_t* d_carry_dst,
                                          uint64_t carry_cap, gevws_summary* d_carry_summary, uint32_t carry_flags) {
  if (!ctx || !d_summary || (flags & ~GEVWS_JOIN_ALL) || (carry_flags & ~GEVWS_CARRY_KEEP_COMPRESSED) ||
      max_frames > 0xFFFFFFFFull ||
      max_messages > 0x7FFFFFFFull * kWalkBlock)
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (d_conn_msg && d_carry_out && d_carry_dst && d_carry_summary)
    return join_with_carry(ctx, st, d_frames, max_frames, d_messages, max_messages, d_msg_of, d_msg_summary, d_payload,
                           d_inflated, d_inflate_summary, flags, d_bodies, d_out, out_cap, d_summary, d_conn_msg,
                           n_conns, max_message_bytes, d_carry_in, d_carry_src, carry_src_bytes, d_carry_out,
                           d_carry_dst, carry_cap, d_carry_summary, carry_flags);
  // the NULL call: gevws_join_async
  if (max_messages == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  // vectors are loaded and stored whole and aligned: both arenas start on a 16-byte boundary
  if (!d_frames || !d_messages || !d_msg_of || !d_msg_summary || !d_payload || !d_bodies || !d_out ||
      (reinterpret_cast<uintptr_t>(d_payload) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_messages + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, join_scratch(nullptr, max_frames, max_messages, nblk, out_cap).total);
  if (r != GEVWS_OK) return r;
  const JoinScratch s = join_scratch(ctx->scratch, max_frames, max_messages, nblk, out_cap);
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  const JoinCarryIn none{nullptr, 0, 0, 0};
  k_join_size<false><<<nblk, kWalkBlock, 0, st>>>(d_messages, max_messages, d_msg_summary, d_inflated,
                                                  d_inflate_summary, flags, s.ctl, s.blk, none);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk + 1, UINT64_MAX, out_cap, d_summary);
  k_join_place<false><<<nblk, kWalkBlock, 0, st>>>(d_frames, max_frames, d_messages, d_msg_of, d_inflated, flags,
                                                   s.ctl, s.blk, d_summary, d_bodies, s.mdst, s.span, s.foff,
                                                   s.tile_msg, none, nullptr, nullptr);
  k_join_copy<false><<<(uint32_t)ctx->num_cus * kSegWgPerCU, kSegBlock, 0, st>>>(
      d_frames, max_frames, d_msg_of, d_payload, d_bodies, s.mdst, s.span, s.foff, s.tile_msg, s.ctl, d_summary,
      d_out, nullptr, nullptr, nullptr, 0);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_join_carry_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames, uint64_t max_frames,
                                      const gevws_message* d_messages, uint64_t max_messages, const int64_t* d_msg_of,
                                      const gevws_summary* d_msg_summary, const uint8_t* d_payload,
                                      const gevws_inflated* d_inflated, const gevws_summary* d_inflate_summary,
                                      uint32_t flags, gevws_body* d_bodies, uint8_t* d_out, uint64_t out_cap,
                                      gevws_summary* d_summary, const gevws_conn_msg* d_conn_msg, uint32_t n_conns,
                                      uint64_t max_message_bytes, const gevws_carry* d_carry_in,
                                      const uint8_t* d_carry_src, uint64_t carry_src_bytes, gevws_carry* d_carry_out,
                                      uint8_t* d_carry_dst, uint64_t carry_cap, gevws_summary* d_carry_summary) {
  return gevws_join_carry_ext_async(ctx, stream, d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                    d_msg_summary, d_payload, d_inflated, d_inflate_summary, flags, d_bodies, d_out,
                                    out_cap, d_summary, d_conn_msg, n_conns, max_message_bytes, d_carry_in,
                                    d_carry_src, carry_src_bytes, d_carry_out, d_carry_dst, carry_cap, d_carry_summary,
                                    0);
}

extern "C" int gevws_reply_bodies_async(gevws_ctx* ctx, void* stream, const gevws_body* d_bodies,
                                        uint64_t max_messages, const gevws_summary* d_msg_summary,
                                        const gevws_summary* d_join_summary, int policy, const uint8_t* d_conn_ext,
                                        const uint8_t* d_conn_window_bits, uint32_t n_conns,
                                        gevws_deflate_msg* d_def_msgs, uint32_t* d_def_conn,
                                        gevws_summary* d_def_summary, gevws_out_frame* d_plain,
                                        uint32_t* d_plain_conn, gevws_summary* d_plain_summary,
                                        int64_t* d_reply_of) {
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
      !d_reply_of)
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_messages + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  const size_t blk_bytes = (size_t)nblk * kBlkFields * sizeof(uint64_t);
  r = ensure_scratch(ctx, blk_bytes);
  if (r != GEVWS_OK) return r;
  uint64_t* blk = reinterpret_cast<uint64_t*>(ctx->scratch);
  GEVWS_HIP(hipMemsetAsync(blk, 0, blk_bytes, st));
  k_reply_count<<<nblk, kWalkBlock, 0, st>>>(d_bodies, max_messages, d_msg_summary, d_join_summary, policy,
                                             d_conn_ext, n_conns, blk);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(blk, nblk, UINT64_MAX, UINT64_MAX, d_def_summary);
  k_reply_verdict<<<1, 1, 0, st>>>(d_def_summary, d_plain_summary);
  k_reply_emit<<<nblk, kWalkBlock, 0, st>>>(d_bodies, max_messages, d_msg_summary, d_join_summary, policy, d_conn_ext,
                                            d_conn_window_bits, n_conns, blk, d_def_summary, d_def_msgs, d_def_conn,
                                            d_plain, d_plain_conn, d_reply_of);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
