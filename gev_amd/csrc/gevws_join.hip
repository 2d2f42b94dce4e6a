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
//   k_join_copy    the gather: every workgroup a contiguous run of 4 KiB output
//                  tiles, a quarter of it a wave, a tile a wave step; aligned
//                  16-byte non-temporal stores, two aligned loads + funnel16
//                  inside a fragment, vectors that straddle fragments assembled
//                  from each fragment's bytes
// Only k_join_copy touches payload bytes: L read, L rounded up to 16 written a
// copied body.
//
// The reply step: k_reply_count / k_scan_blocks / k_reply_verdict /
// k_reply_emit, an order-preserving compaction of the delivered bodies into the
// two lists (fields 0 and 1 of the block partials are the two lists' counts).
#include "gevws_internal.hpp"

namespace {

static_assert(sizeof(gevws_body) == 32 && offsetof(gevws_body, length) == 8 && offsetof(gevws_body, conn) == 16 &&
                  offsetof(gevws_body, opcode) == 20 && offsetof(gevws_body, flags) == 21 &&
                  offsetof(gevws_body, status) == 22, "gevws_body layout");
static_assert(sizeof(gevws_inflated) == 32 && sizeof(gevws_deflate_msg) == 24 && sizeof(gevws_out_frame) == 32,
              "record layouts");

constexpr int kJoinBlock = 256;    // k_join_copy: four waves
constexpr int kJoinWaves = kJoinBlock / 64;
constexpr int kJoinVecs = (int)(kTile / (64 * 16));  // vectors a lane and tile: a wave takes a whole tile
constexpr int kJoinWgPerCU = 4;   // 98 VGPRs: four waves a SIMD, the whole grid resident
static_assert(kJoinVecs == 4, "one tile = four 1 KiB rows of a wave");
constexpr int kJoinWalk = 4;      // fragments a wave steps forward to reach a tile's first byte before it bisects
constexpr int kJoinRounds = 4;    // fragments of one tile a wave takes as whole rows ...
constexpr uint64_t kJoinRowBytes = 1024;  // ... while they are at least this long; shorter ones lane by lane

// ------------------------------------------------------------------ scratch
struct JoinScratch {
  uint64_t* ctl;        // [0] base, [1] the gated message count
  uint64_t* blk;        // [nblk + 1][kBlkFields]; partial 0 holds `base` in field 1
  uint64_t* mdst;       // [m] where message m's body starts in d_out (a message that is not copied: where the
                        //     next copied one starts), so the array never decreases
  uint2* span;          // [m] a copied message's first and last data frame
  uint64_t* foff;       // [f] bytes of the message before frame f, for every frame inside a copied message's span
  uint32_t* tile_msg;   // [t] the message that holds the first byte of output tile t (tiles count from `base`)
  size_t zero_bytes, total;
};
inline JoinScratch join_scratch(void* base, uint64_t max_frames, uint64_t max_messages, uint32_t nblk,
                                uint64_t out_cap) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  JoinScratch s;
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)(nblk + 1) * kBlkFields * sizeof(uint64_t));
  s.zero_bytes = o;
  s.mdst = reinterpret_cast<uint64_t*>(p + o), o += up(max_messages * 8);
  s.span = reinterpret_cast<uint2*>(p + o), o += up(max_messages * 8);
  s.foff = reinterpret_cast<uint64_t*>(p + o), o += up(max_frames * 8);
  s.tile_msg = reinterpret_cast<uint32_t*>(p + o), o += up((out_cap / kTile + 2) * 4);
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

// The messages of the call: the message pass's count, none when it or a given inflate failed.
__device__ __forceinline__ uint64_t join_count(uint64_t max_messages, const gevws_summary* __restrict__ msg_sum,
                                               const gevws_summary* __restrict__ inf_sum) {
  if (inf_sum && inf_sum->status != GEVWS_OK) return 0;
  return gated_count(max_messages, msg_sum);
}

// The workgroup's partial {vals[0], vals[1], vals[2], 0} -> blk[row].
__device__ __forceinline__ void block_partial(const uint64_t (&vals)[3], uint64_t* __restrict__ blk, uint64_t row) {
  __shared__ uint64_t s_part[3][kWalkBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t sm = wave_sum(vals[k]);
    if (lane == 0) s_part[k][wv] = sm;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint64_t sm = 0;
    for (int j = 0; j < kWalkBlock / 64; ++j) sm += s_part[threadIdx.x][j];
    blk[row * kBlkFields + threadIdx.x] = sm;
  }
}

// ------------------------------------------------------------------ 1. sizes
__global__ __launch_bounds__(kWalkBlock) void k_join_size(const gevws_message* __restrict__ msgs,
                                                          uint64_t max_messages,
                                                          const gevws_summary* __restrict__ msg_sum,
                                                          const gevws_inflated* __restrict__ inflated,
                                                          const gevws_summary* __restrict__ inf_sum,
                                                          uint32_t call_flags, uint64_t* __restrict__ ctl,
                                                          uint64_t* __restrict__ blk) {
  const uint64_t n = join_count(max_messages, msg_sum, inf_sum);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[3] = {0, 0, 0};  // delivered, bytes taken in d_out, delivered length
  if (m < n) {
    const JoinDec d = join_decide(msgs[m], inflated, m, call_flags);
    vals[0] = d.flags ? 1 : 0;
    vals[1] = d.copy ? round16(d.length) : 0;
    vals[2] = d.length;
  }
  block_partial(vals, blk, (uint64_t)blockIdx.x + 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // joined bodies start behind the inflate's bytes (a call without messages reads none of its inputs)
    const uint64_t base = n && inf_sum ? round16(inf_sum->payload_bytes) : 0;
    ctl[0] = base;
    ctl[1] = n;
    blk[1] = base;  // partial 0, field 1: every block's base and the summary's payload_bytes include it
  }
}

// ------------------------------------------------------------------ 2. records and maps
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
                                                           uint32_t* __restrict__ tile_msg) {
  if (sum->status != GEVWS_OK) return;  // capacity: nothing written
  const uint64_t n = ctl[1], base = ctl[0];
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  gevws_message msg;
  memset(&msg, 0, sizeof(msg));
  JoinDec d;
  memset(&d, 0, sizeof(d));
  if (m < n) {
    msg = msgs[m];
    d = join_decide(msg, inflated, m, call_flags);
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
  if (!padded) return;
  // the frames' running offsets; control frames in between get theirs too, so
  // the array never decreases over the span and a bisection finds a byte's frame
  uint64_t run = 0, last = msg.first_frame;
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
struct JoinMaps {
  const gevws_frame* __restrict__ fr;
  const int64_t* __restrict__ msg_of;
  const gevws_body* __restrict__ bodies;
  const uint64_t* __restrict__ mdst;
  const uint2* __restrict__ span;
  const uint64_t* __restrict__ foff;
  const uint8_t* __restrict__ payload;
  uint64_t nframes;
};
// One fragment's counted bytes: d_out[ds, de) come from src[0, de - ds).
struct JoinFrag {
  uint64_t ds, de;
  const uint8_t* src;
  uint64_t m, f, last, body_end;  // its message and frame, the message's last frame, the end of its body in d_out
};

// The fragment that holds byte x of d_out, x inside a copied body of a
// message in [mlo, mhi]; false: x is a pad byte.
__device__ __forceinline__ bool join_lookup(const JoinMaps& M, uint64_t x, uint64_t mlo, uint64_t mhi, JoinFrag& g) {
  uint64_t lo = mlo, hi = mhi;
  while (lo < hi) {  // the last message that starts at or before x: the later ones at its place take no space
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (M.mdst[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  const gevws_body b = M.bodies[lo];
  if (!(b.flags & GEVWS_BODY_JOINED) || x < b.off || x - b.off >= b.length) return false;
  const uint64_t pos = x - b.off;
  const uint2 sp = M.span[lo];
  uint64_t flo = sp.x, fhi = sp.y;
  if (fhi >= M.nframes || flo > fhi) return false;
  const uint64_t last = fhi;
  while (flo < fhi) {  // the last frame that starts at or before pos: it holds the byte
    const uint64_t mid = (flo + fhi + 1) >> 1;
    if (M.foff[mid] <= pos) flo = mid;
    else fhi = mid - 1;
  }
  const gevws_frame rec = M.fr[flo];
  const uint64_t fo = M.foff[flo], len = (uint64_t)rec.hdr.length;
  if (pos < fo || pos - fo >= len) return false;
  g.ds = b.off + fo;
  g.de = g.ds + len;
  g.src = M.payload + rec.payload_off;
  g.m = lo, g.f = flo, g.last = last, g.body_end = b.off + b.length;
  return true;
}

__device__ __forceinline__ u32x4 ld16_nt(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// The destination vector at x assembled byte range by byte range: each
// fragment's part from the one or two aligned source vectors that hold it
// (vectors with a counted byte only), bytes past the body zero.
// g -> the message's next fragment with bytes, which follows it in d_out; false: g was the last.
__device__ __forceinline__ bool join_next(const JoinMaps& M, JoinFrag& g) {
  for (uint64_t f = g.f + 1; f <= g.last; ++f) {
    const gevws_frame rec = M.fr[f];
    const uint64_t len = (uint64_t)rec.hdr.length;
    if (len && M.msg_of[f] == (int64_t)g.m) {
      g.f = f;
      g.ds = g.de, g.de = g.ds + len;
      g.src = M.payload + rec.payload_off;
      return true;
    }
  }
  return false;
}

// seed: a fragment that may hold x (the wave's current one), or null.
__device__ __forceinline__ u32x4 join_vector(const JoinMaps& M, uint64_t x, uint64_t mlo, uint64_t mhi,
                                             const JoinFrag* seed) {
  JoinFrag g;
  if (seed && x >= seed->ds && x < seed->de) g = *seed;
  else if (!join_lookup(M, x, mlo, mhi, g)) return u32x4{0, 0, 0, 0};  // a whole vector of pad
  u128 acc = 0;
  uint64_t p = x;
  for (;;) {
    const uint64_t stop = g.de < x + 16 ? g.de : x + 16;
    const uint32_t cnt = (uint32_t)(stop - p);  // 1..16 bytes of this fragment
    const uint8_t* sa = g.src + (p - g.ds);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(sa) & 15);
    const uint8_t* a0 = sa - mis;
    u128 w = u128_of(ld16_nt(a0)) >> (8 * mis);
    if (mis + cnt > 16) w |= u128_of(ld16_nt(a0 + 16)) << (8 * (16 - mis));
    if (cnt < 16) w &= (((u128)1) << (8 * cnt)) - 1;
    acc |= w << (8 * (uint32_t)(p - x));
    p = stop;
    if (p >= x + 16 || p >= g.body_end) break;
    if (!join_next(M, g)) break;  // (not a table the place kernel writes)
  }
  return u32x4_of(acc);
}

// A fragment's fields in SGPRs (every lane computed the same ones).
__device__ __forceinline__ void uniform_frag(JoinFrag& g) {
  g.ds = uniform64(g.ds), g.de = uniform64(g.de);
  g.src = reinterpret_cast<const uint8_t*>(uniform64(reinterpret_cast<uintptr_t>(g.src)));
  g.m = uniform64(g.m), g.f = uniform64(g.f), g.last = uniform64(g.last), g.body_end = uniform64(g.body_end);
}

__global__ __launch_bounds__(kJoinBlock) void k_join_copy(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                                          const int64_t* __restrict__ msg_of,
                                                          const uint8_t* __restrict__ payload,
                                                          const gevws_body* __restrict__ bodies,
                                                          const uint64_t* __restrict__ mdst,
                                                          const uint2* __restrict__ span,
                                                          const uint64_t* __restrict__ foff,
                                                          const uint32_t* __restrict__ tile_msg,
                                                          const uint64_t* __restrict__ ctl,
                                                          const gevws_summary* __restrict__ sum,
                                                          uint8_t* __restrict__ out) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t base = ctl[0], n = ctl[1], end = sum->payload_bytes;  // the joined region is d_out[base, end)
  if (end <= base || n == 0) return;
  const JoinMaps M{fr, msg_of, bodies, mdst, span, foff, payload, max_frames};
  const uint64_t ntiles = (end - base + kTile - 1) / kTile;
  // a workgroup's run of tiles is its four waves' runs, one behind the other
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * kJoinWaves, gw = (uint64_t)blockIdx.x * kJoinWaves + wv;
  const uint64_t per = (ntiles + nw - 1) / nw;
  const uint64_t t0 = gw * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  JoinFrag g;  // the wave's current fragment, kept from tile to tile (wave-uniform)
  memset(&g, 0, sizeof(g));
  bool have = false;
  for (uint64_t t = t0; t < t1; ++t) {
    const uint64_t T = base + t * kTile;
    uint64_t mlo = tile_msg[t], mhi = t + 1 < ntiles ? (uint64_t)tile_msg[t + 1] : n - 1;
    mlo = mlo < n ? mlo : n - 1;
    mhi = mhi < n ? (mhi > mlo ? mhi : mlo) : n - 1;
    if (!(have && T >= g.ds && T < g.de)) {  // the fragment at the tile's first byte
      bool found = false;
      // a few long fragments on in the same body: no bisection
      if (have && T >= g.de && T < g.body_end && g.de - g.ds >= kJoinRowBytes)
        for (int k = 0; k < kJoinWalk && !found && join_next(M, g); ++k) found = T < g.de;
      if (!found) found = join_lookup(M, T, mlo, mhi, g);
      have = found;
      uniform_frag(g);
    }
    uint32_t done = 0;  // bit u: this lane's vector u is stored
    for (int round = 0; have && g.de - g.ds >= kJoinRowBytes && round < kJoinRounds; ++round) {
      // inside one fragment the source is a constant byte shift off alignment
      const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(g.src) + (T - g.ds)) & 15);
      uint64_t x[kJoinVecs];
      bool fast[kJoinVecs];
      u32x4 v0[kJoinVecs], v1[kJoinVecs];
#pragma unroll
      for (int u = 0; u < kJoinVecs; ++u) {
        x[u] = T + (uint64_t)u * 1024 + (uint64_t)lane * 16;
        // (end is on 16: a vector that starts below it is inside)
        fast[u] = !((done >> u) & 1) && x[u] >= g.ds && x[u] + 16 <= g.de && x[u] < end;
        if (fast[u]) {
          const uint8_t* a0 = g.src + (x[u] - g.ds) - mis;
          v0[u] = ld16_nt(a0);
          if (mis) v1[u] = ld16_nt(a0 + 16);
        }
      }
#pragma unroll
      for (int u = 0; u < kJoinVecs; ++u)
        if (fast[u]) st16_nt(out + x[u], mis ? funnel16(v0[u], v1[u], mis) : v0[u]), done |= 1u << u;
      if (g.de >= T + kTile) break;
      // the vector the fragment's end cuts starts inside it: no lookup for that one
#pragma unroll 1
      for (int u = 0; u < kJoinVecs; ++u) {
        const uint64_t xu = T + (uint64_t)u * 1024 + (uint64_t)lane * 16;
        if (!((done >> u) & 1) && xu < end && xu >= g.ds && xu < g.de)
          st16_nt(out + xu, join_vector(M, xu, mlo, mhi, &g)), done |= 1u << u;
      }
      // on to the body's next fragment while fragments are long enough for whole rows of the wave
      if (!join_next(M, g)) {
        have = false;
        break;
      }
      uniform_frag(g);
    }
    // what no round covered: short fragments, a body's pad, the next body's start
#pragma unroll 1
    for (int u = 0; u < kJoinVecs; ++u) {
      const uint64_t xu = T + (uint64_t)u * 1024 + (uint64_t)lane * 16;
      if (!((done >> u) & 1) && xu < end) st16_nt(out + xu, join_vector(M, xu, mlo, mhi, nullptr));
    }
  }
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
  block_partial(vals, blk, blockIdx.x);
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
  if (!ctx || !d_summary || (flags & ~GEVWS_JOIN_ALL) || max_frames > 0xFFFFFFFFull ||
      max_messages > 0x7FFFFFFFull * kWalkBlock)
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
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
  k_join_size<<<nblk, kWalkBlock, 0, st>>>(d_messages, max_messages, d_msg_summary, d_inflated, d_inflate_summary,
                                           flags, s.ctl, s.blk);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk + 1, UINT64_MAX, out_cap, d_summary);
  k_join_place<<<nblk, kWalkBlock, 0, st>>>(d_frames, max_frames, d_messages, d_msg_of, d_inflated, flags, s.ctl,
                                            s.blk, d_summary, d_bodies, s.mdst, s.span, s.foff, s.tile_msg);
  k_join_copy<<<(uint32_t)ctx->num_cus * kJoinWgPerCU, kJoinBlock, 0, st>>>(
      d_frames, max_frames, d_msg_of, d_payload, d_bodies, s.mdst, s.span, s.foff, s.tile_msg, s.ctl, d_summary,
      d_out);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
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
