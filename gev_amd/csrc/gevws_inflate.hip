// gevws_inflate.hip -- permessage-deflate (RFC 7692) behind the message pass:
// gevws_inflate_async (include/gevws.h) inflates the compressed messages of a
// batch, one wave per message, with the block decoder of
// gevws_inflate_core.hpp.  The reference has no code for it.
//
// Five launches behind one memset, no host round trip:
//   k_inf_size     one wave per message: decodes without storing -- every
//                  verdict but UTF-8, and the inflated length
//   k_scan_blocks  lays the messages out in d_out, the summary, CAPACITY
//   k_inf_emit     one wave per message: decodes again through a 32 KiB LDS
//                  window that is flushed to d_out as 16-byte vectors; writes
//                  d_inflated
//   k_inf_utf8     one wave per inflated text message: the 16-byte-vector rule
//                  of gevws_utf8.hpp over the finished output
//   k_inf_state    one lane per connection's first message: d_state.failed
//
// gevws_inflate_ctx_async (client context takeover) launches k_inf_size<true>
// and k_inf_emit<true>, and k_inf_verdict between the scan and the emit.  They
// serve both kinds of connection with a wave-uniform branch: a connection
// without the takeover bit runs the code above; a takeover connection's
// messages are a chain that one wave decodes in order, the window carried in
// the connection's slot of d_inf_ctx (see "context takeover" below).  The
// <false> instances are the kernels of gevws_inflate_async, unchanged.
//
// gevws_inflate_carry_async (compressed messages that span passes) launches the
// <true, true> instances: a continued message whose connection's carry record
// is OPEN | COMPRESSED is whole -- the carried bytes are one more fragment of
// its source, in front of first_frame.  The instances above do not change.
//
// A wave's decode state -- bit buffer, counters, each Huffman code's limits --
// is the same in every lane; the lanes differ only where bytes move: the 1 KiB
// refills of the input (hopping from fragment to fragment), match copies,
// stored blocks, the window flush, and placing a block's symbols.  One wave is one workgroup, so four messages a CU hold
// 4 x (32 KiB window + 1 KiB input + 1 KiB tables) of its 160 KiB LDS.  A
// wave's LDS accesses complete in order, so the lanes hand bytes to each other
// through LDS without a barrier.
#include "gevws_inflate_core.hpp"
#include "gevws_internal.hpp"
#include "gevws_utf8.hpp"

namespace {

constexpr uint32_t kInfWin = 32768, kInfIn = 1024, kInfBlock = 64;
static_assert(kInfIn == kInfBlock * 16, "a refill / a flush = one 16-byte vector a lane");

// Keeps the compiler from moving one lane's LDS access across another's.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct InfRec {  // per message, between the passes
  uint32_t len;
  uint8_t status, flags;
  uint16_t pad;
};
static_assert(sizeof(InfRec) == 8 && sizeof(gevws_inflated) == 32, "inflate layouts");

struct InfScratch {
  uint64_t* blk;  // per message: [1 if OK, bytes of d_out, length, 1 if failed]
  InfRec* rec;
  size_t total;
};
inline InfScratch inf_scratch(void* base, uint64_t max_messages) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  InfScratch s;
  size_t o = 0;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up(max_messages * kBlkFields * sizeof(uint64_t));
  s.rec = reinterpret_cast<InfRec*>(p + o), o += up(max_messages * sizeof(InfRec));
  s.total = o;
  return s;
}

// ------------------------------------------------------------------ the source
// S of message m: the payloads of its data frames, then 00 00 ff ff, through a
// 1 KiB LDS buffer.  Reads hdr.length bytes of a frame and not one more.  With
// a carry, a continued message's carried bytes come first (prefix()): a run of
// the carry arena that starts on 16, read up to its length and not one more.
struct InfSource {
  const gevws_frame* __restrict__ fr;
  const int64_t* __restrict__ msg_of;
  const uint8_t* __restrict__ payload;
  uint8_t* inbuf;
  uint64_t m, f, max_frames;
  uint32_t frames_left;          // data frames of the message not opened yet
  const uint8_t* p = nullptr;    // the open fragment: L bytes, foff of them taken
  uint64_t L = 0, foff = 0;
  uint32_t rd = 0, n = 0;        // the buffer holds n bytes, rd of them taken
  uint64_t cache = 0;            // ... the last up to eight of those not handed out yet: a byte costs
  uint32_t cache_n = 0;          //     a shift, not an LDS round trip
  uint32_t tail_done = 0;
  uint32_t lane;

  __device__ InfSource(const gevws_frame* fr_, const int64_t* msg_of_, const uint8_t* payload_, uint8_t* inbuf_,
                       uint64_t m_, const gevws_message& msg, uint64_t max_frames_)
      : fr(fr_), msg_of(msg_of_), payload(payload_), inbuf(inbuf_), m(m_), f(msg.first_frame),
        max_frames(max_frames_), frames_left(msg.nframes), lane(threadIdx.x & 63) {}

  // The carried bytes of a continued message: the open fragment before
  // advance() first looks at first_frame (none of them: advance() at once).
  __device__ __forceinline__ void prefix(const uint8_t* p_, uint64_t L_) { p = p_, L = L_, foff = 0; }

  // The buffer is empty and the fragment used up: opens the next fragment
  // with bytes, or puts the tail into the buffer; false at the end of S.
  __device__ __forceinline__ bool advance() {
    while (frames_left && f < max_frames) {
      const uint64_t cur = f++;
      if (uniform64((uint64_t)msg_of[cur]) != m) continue;  // a control frame in between
      --frames_left;
      const gevws_frame rec = fr[cur];
      const int64_t len = (int64_t)uniform64((uint64_t)rec.hdr.length);
      if (len <= 0) continue;
      p = payload + uniform64(rec.payload_off);
      L = (uint64_t)len;
      foff = 0;
      return true;
    }
    frames_left = 0;
    if (tail_done) return false;
    tail_done = 1;
    if (lane < 4) inbuf[lane] = lane < 2 ? 0x00 : 0xff;
    wave_lds_order();
    rd = 0, n = 4;
    return true;
  }
  __device__ __forceinline__ bool fill() {
    if (foff == L) {
      if (!advance()) return false;
      if (rd < n) return true;  // the tail
    }
    const uint64_t left = L - foff;
    const uint32_t k = left < kInfIn ? (uint32_t)left : kInfIn;
    const uint32_t o = 16 * lane;
    if (o + 16 <= k) {
      *reinterpret_cast<u32x4*>(inbuf + o) = ld16u(p + foff + o);
    } else {
      for (uint32_t i = o; i < k; ++i) inbuf[i] = p[foff + i];
    }
    wave_lds_order();
    foff += k;
    rd = 0, n = k;
    return true;
  }
  __device__ __forceinline__ bool get(uint32_t& b) {
    if (cache_n == 0) {
      if (rd == n && !fill()) return false;
      if ((rd & 7) == 0 && n - rd >= 8) {
        cache = uniform64(*reinterpret_cast<const uint64_t*>(inbuf + rd));
        cache_n = 8, rd += 8;
      } else {
        cache = uniform32(inbuf[rd]);
        cache_n = 1, rd += 1;
      }
    }
    b = (uint32_t)(cache & 0xff);
    cache >>= 8;
    --cache_n;
    return true;
  }
  // Up to `want` bytes passed over unread (the sizing pass's stored blocks).
  __device__ __forceinline__ uint64_t skip(uint64_t want) {
    uint64_t got = 0;
    while (got < want && cache_n) cache >>= 8, --cache_n, ++got;
    while (got < want) {
      if (rd < n) {
        const uint64_t k = want - got < n - rd ? want - got : n - rd;
        rd += (uint32_t)k, got += k;
      } else if (foff < L) {
        const uint64_t k = want - got < L - foff ? want - got : L - foff;
        foff += k, got += k;
      } else if (!advance()) {
        break;
      }
    }
    return got;
  }
};

// ------------------------------------------------------------------ the two sinks
struct InfSizeIo : InfSource {  // counts only: the core keeps the count
  using InfSource::InfSource;
  __device__ __forceinline__ void put(uint32_t) {}
  __device__ __forceinline__ void copy(uint32_t, uint32_t) {}
  __device__ __forceinline__ uint64_t stored(uint64_t want) { return skip(want); }
};

// CTX: a message of a context-takeover chain.  The window is the connection's
// ring -- stream byte i at win[i % kInfWin] -- and the message starts in it at
// `start`, the connection's stream position, which is not 16-aligned in
// general; pos and flushed are stream positions too, so a distance reaches
// back over the message boundary without a seam.  The message's byte j still
// goes to out[j], on a 16-byte boundary: the flush realigns.
template <bool CTX>
struct InfEmitIo : InfSource {
  uint8_t* win;  // LDS, kInfWin bytes: byte i of the output at win[i % kInfWin]
  uint8_t* out;  // the message's bytes in d_out (16-byte aligned)
  uint64_t pos = 0, flushed = 0;
  uint64_t start = 0;

  __device__ InfEmitIo(const gevws_frame* fr_, const int64_t* msg_of_, const uint8_t* payload_, uint8_t* inbuf_,
                       uint64_t m_, const gevws_message& msg, uint64_t max_frames_, uint8_t* win_, uint8_t* out_,
                       uint64_t start_ = 0)
      : InfSource(fr_, msg_of_, payload_, inbuf_, m_, msg, max_frames_), win(win_), out(out_) {
    if constexpr (CTX) pos = flushed = start = start_;
  }

  // The 16 bytes of the window from stream position x on.  CTX: x = start mod
  // 16 for every vector of the message, so two aligned reads and a byte shift.
  __device__ __forceinline__ u32x4 window16(uint64_t x) const {
    if constexpr (CTX) {
      const uint32_t a = (uint32_t)x & ~15u;
      return funnel16(*reinterpret_cast<const u32x4*>(win + (a & (kInfWin - 1))),
                      *reinterpret_cast<const u32x4*>(win + ((a + 16) & (kInfWin - 1))), uniform32((uint32_t)start & 15));
    } else {
      return *reinterpret_cast<const u32x4*>(win + (x & (kInfWin - 1)));
    }
  }
  __device__ __forceinline__ uint64_t rel() const {  // `flushed` as an offset into the message
    if constexpr (CTX) return flushed - start;
    else return flushed;
  }
  // Whole KiB of the window to d_out.  At most 1 023 + 1 024 bytes are ever
  // unflushed, so nothing unflushed is overwritten 32 KiB later.
  __device__ __forceinline__ void flush() {
    while (pos - flushed >= kInfIn) {
      const u32x4 v = window16(flushed + 16 * lane);
      *reinterpret_cast<u32x4*>(out + rel() + 16 * lane) = v;
      flushed += kInfIn;
    }
  }
  // The rest, the last vector's pad zeroed.
  __device__ __forceinline__ void finish() {
    flush();
    const uint64_t r = pos - flushed, o = 16 * (uint64_t)lane;
    if (o < r) {
      u32x4 v = window16(flushed + o);
      if (r - o < 16) v = keep_bytes(v, (int64_t)(r - o));
      *reinterpret_cast<u32x4*>(out + rel() + o) = v;
    }
  }
  __device__ __forceinline__ void put(uint32_t b) {
    if (lane == 0) win[pos & (kInfWin - 1)] = (uint8_t)b;
    wave_lds_order();
    ++pos;
    flush();
  }
  // n <= 258 bytes from d <= 32 768 back, as a byte-serial copy: byte i comes
  // from byte i mod d of the d bytes before pos, all written before this call.
  // A slot that byte i takes over (d + i - j = 32 768) held source byte
  // j <= i, read in the same or an earlier round.
  __device__ __forceinline__ void copy(uint32_t d, uint32_t len) {
    for (uint32_t i0 = 0; i0 < len; i0 += kInfBlock) {
      const uint32_t i = i0 + lane;
      if (i < len) {
        const uint32_t j = i < d ? i : i % d;
        const uint8_t c = win[(pos - d + j) & (kInfWin - 1)];
        win[(pos + i) & (kInfWin - 1)] = c;
      }
      wave_lds_order();
    }
    pos += len;
    flush();
  }
  __device__ __forceinline__ uint64_t stored(uint64_t want) {
    uint64_t got = 0;
    while (got < want && cache_n) {
      uint32_t b;
      get(b), put(b), ++got;
    }
    while (got < want) {
      if (rd == n && !fill()) break;
      const uint32_t k = want - got < n - rd ? (uint32_t)(want - got) : n - rd;
      for (uint32_t i = lane; i < k; i += kInfBlock) win[(pos + i) & (kInfWin - 1)] = inbuf[rd + i];
      wave_lds_order();
      rd += k, got += k, pos += k;
      flush();
    }
    return got;
  }
};

__device__ __forceinline__ bool inf_wanted(const gevws_message& msg) {
  const uint32_t all = GEVWS_MSG_COMPRESSED | GEVWS_MSG_BEGIN | GEVWS_MSG_END;
  return (msg.flags & all) == all;
}

// The carry of gevws_inflate_carry_async: the `in` side the pass's join reads
// afterwards.  Only read here.
struct InfCarry {
  const gevws_carry* __restrict__ in;
  const uint8_t* __restrict__ src;
  uint64_t src_bytes;
};
// What the carry makes of a compressed message: both passes ask here, so they
// decide alike.
enum : uint32_t {
  kInfPending = 0,  // not whole: GEVWS_INF_PENDING
  kInfWhole = 1,    // BEGIN and END in the batch
  kInfCarried = 2,  // continued, END here, the record OPEN | COMPRESSED: whole behind pre bytes at psrc
  kInfLost = 3,     // continued, END here, the record LOST with a status: DONE with that status
};
struct InfWhole {
  uint32_t kind, status;
  uint64_t pre, psrc;
};
// An OPEN record the caller did not get from a join: never an address.
__device__ __forceinline__ bool inf_carry_bad(const InfCarry& ca, uint32_t c) {
  const gevws_carry ci = ca.in[c];
  const uint64_t off = uniform64(ci.off), len = uniform64(ci.length);
  return (uniform32(ci.flags) & GEVWS_CARRY_OPEN) && ((off & 15) || off > ca.src_bytes || len > ca.src_bytes - off);
}
// (msg.conn is below n_conns and its record passed inf_carry_bad)
template <bool CARRY>
__device__ __forceinline__ InfWhole inf_whole(const gevws_message& msg, const InfCarry& ca) {
  InfWhole w;
  w.kind = inf_wanted(msg) ? kInfWhole : kInfPending, w.status = 0, w.pre = w.psrc = 0;
  if constexpr (CARRY) {
    const uint32_t want = GEVWS_MSG_COMPRESSED | GEVWS_MSG_END;
    if (w.kind == kInfWhole || (uniform32(msg.flags) & (want | GEVWS_MSG_BEGIN)) != want ||
        uniform32(msg.status) != GEVWS_MSG_OK)
      return w;
    const gevws_carry ci = ca.in[uniform32(msg.conn)];
    const uint32_t cf = uniform32(ci.flags);
    const uint32_t open = GEVWS_CARRY_OPEN | GEVWS_CARRY_COMPRESSED;
    if ((cf & open) == open) {
      w.kind = kInfCarried, w.pre = uniform64(ci.length), w.psrc = uniform64(ci.off);
    } else if (!(cf & GEVWS_CARRY_OPEN) && (cf & GEVWS_CARRY_LOST) && uniform32(ci.status)) {
      w.kind = kInfLost, w.status = uniform32(ci.status);
    }
  }
  return w;
}

// ------------------------------------------------------------------ context takeover
// A takeover connection's compressed messages depend on each other in order
// (message k's window is the output of the messages before it), so the wave of
// the connection's first message in the batch walks all of them, one after
// another, and the waves of its other messages exit: the data dependency of
// context takeover, in both passes.  The slot (include/gevws.h): a 64-byte
// head, then the ring image.
constexpr uint32_t kCtxHead = GEVWS_INF_CTX_BYTES - kInfWin;
constexpr uint64_t kInfInvalid = 1ull << 32;  // in blk field 3: a record with conn >= n_conns
static_assert(kCtxHead == 64 && GEVWS_INF_CTX_BYTES % 16 == 0, "slots and their rings lie on 16-byte boundaries");

// The message of a workgroup.  Workgroups are dealt round-robin over the 8
// XCDs (and within one over its CUs), and a chain's work sits in its first
// message's workgroup: with a regular number of messages a connection (8,
// say) the identity puts every chain on the same XCD -- measured, DESIGN
// section 5.6.  So with contexts the grid is kInfSpread x q workgroups and
// workgroup b takes message (b % kInfSpread) q + b / kInfSpread: consecutive
// workgroups take messages q apart, and q is a multiple of 16 (inf_grid_q),
// so chains of a period that divides 16 have their heads in runs of
// kInfSpread consecutive workgroups, which fill the device evenly, and any
// other period has no common factor with the hardware's powers of two.
constexpr uint32_t kInfSpread = 1024;
inline uint32_t inf_grid_q(uint32_t nm) {
  const uint32_t q = (nm + kInfSpread - 1) / kInfSpread;
  return q <= 8 ? q : (q + 15) / 16 * 16;  // (up to 8 192 messages the grid is nearly resident anyway)
}
template <bool CTX>
__device__ __forceinline__ uint64_t inf_block_message() {
  if constexpr (CTX) return (uint64_t)(blockIdx.x % kInfSpread) * (gridDim.x / kInfSpread) + blockIdx.x / kInfSpread;
  else return blockIdx.x;
}

__device__ __forceinline__ void inf_size_record(uint64_t k, const InfRec& r, uint64_t* __restrict__ blk,
                                                InfRec* __restrict__ rec) {
  rec[k] = r;
  if (r.flags == GEVWS_INF_DONE) {
    const bool ok = r.status == GEVWS_MSG_OK;
    blk[k * kBlkFields + 0] = ok ? 1 : 0;
    blk[k * kBlkFields + 1] = round16(r.len);
    blk[k * kBlkFields + 2] = r.len;
    blk[k * kBlkFields + 3] = ok ? 0 : 1;
  }
}

// The sizing pass over connection c's messages from m on: needs no window
// bytes, only the slot's head; the history length runs through the chain in
// registers.  Writes the records, nothing to the slot.
template <bool CARRY>
__device__ __forceinline__ void inf_size_chain(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                               const gevws_message* __restrict__ msgs, uint64_t n, uint64_t m,
                                               uint32_t c, const int64_t* __restrict__ msg_of,
                                               const uint8_t* __restrict__ payload, uint64_t limit,
                                               const uint8_t* __restrict__ slot, uint8_t* s_in,
                                               gevws_inflate::Tables& s_tab, uint64_t* __restrict__ blk,
                                               InfRec* __restrict__ rec, const InfCarry& ca) {
  const uint64_t total = uniform64(*reinterpret_cast<const uint64_t*>(slot));
  uint32_t hist = total < kInfWin ? (uint32_t)total : kInfWin;
  uint32_t broken = uniform32(slot[8]);
  bool stopped = false;
  for (uint64_t k = m; k < n; ++k) {  // (at most the connection's messages in the batch)
    const gevws_message msg = msgs[k];
    if (uniform32(msg.conn) != c) break;
    if (!(uniform32(msg.flags) & GEVWS_MSG_COMPRESSED)) continue;  // not in the window
    InfRec r;
    r.len = 0, r.status = GEVWS_MSG_OK, r.flags = GEVWS_INF_PENDING, r.pad = 0;
    if (broken) {  // the context is lost: the first failure's status, nothing decoded
      r.status = (uint8_t)broken, r.flags = GEVWS_INF_DONE;
    } else if (InfWhole w; stopped || (w = inf_whole<CARRY>(msg, ca)).kind == kInfPending) {
      stopped = true;  // not whole in the batch: the chain stops here
    } else if (CARRY && w.kind == kInfLost) {  // its bytes were dropped on the way: the context goes with them
      r.status = (uint8_t)w.status, r.flags = GEVWS_INF_DONE;
      broken = w.status;
    } else {
      uint64_t len = 0;
      InfSizeIo io(fr, msg_of, payload, s_in, k, msg, max_frames);
      if constexpr (CARRY)
        if (w.kind == kInfCarried) io.prefix(ca.src + w.psrc, w.pre);  // the chain's first link
      r.status = (uint8_t)gevws_inflate::inflate(io, s_tab, limit, &len, hist);
      r.flags = GEVWS_INF_DONE;
      if (r.status != GEVWS_MSG_OK) {
        broken = r.status;
      } else {
        r.len = (uint32_t)len;
        hist = len + hist < kInfWin ? (uint32_t)len + hist : kInfWin;
      }
    }
    if (threadIdx.x == 0) inf_size_record(k, r, blk, rec);
  }
}

// ------------------------------------------------------------------ 1. sizes and verdicts
// CTX: contexts are given (gevws_inflate_ctx_async); <false> is the kernel of
// gevws_inflate_async.  CARRY (with CTX): a carry is given
// (gevws_inflate_carry_async), and conn_ext / inf_ctx may be null.
template <bool CTX, bool CARRY = false>
__global__ __launch_bounds__(kInfBlock) void k_inf_size(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                                        const gevws_message* __restrict__ msgs,
                                                        uint64_t max_messages, const int64_t* __restrict__ msg_of,
                                                        const gevws_summary* __restrict__ gate,
                                                        const uint8_t* __restrict__ payload, uint64_t limit,
                                                        uint64_t* __restrict__ blk, InfRec* __restrict__ rec,
                                                        const uint8_t* __restrict__ conn_ext,
                                                        const uint8_t* __restrict__ inf_ctx, uint32_t n_conns,
                                                        InfCarry ca) {
  static_assert(CTX || !CARRY, "the carry's kernels check conn like the contexts'");
  __shared__ __attribute__((aligned(16))) uint8_t s_in[kInfIn];
  __shared__ gevws_inflate::Tables s_tab;
  const uint64_t m = inf_block_message<CTX>();
  const uint64_t n = gated_count(max_messages, gate);
  if (m >= n) return;  // (blk and rec are zeroed)
  const gevws_message msg = msgs[m];
  if constexpr (CTX) {
    const uint32_t c = uniform32(msg.conn);
    if (c >= n_conns) {  // never an index: the call is GEVWS_ERR_INVALID (k_inf_verdict)
      if (threadIdx.x == 0) blk[m * kBlkFields + 3] = kInfInvalid;
      return;
    }
    if constexpr (CARRY) {
      if (inf_carry_bad(ca, c)) {  // never an address: GEVWS_ERR_INVALID too, the connection counted once
        if (threadIdx.x == 0 && !(m && msgs[m - 1].conn == c)) blk[m * kBlkFields + 3] = kInfInvalid;
        return;
      }
    }
    if ((!CARRY || conn_ext) && (uniform32(conn_ext[c]) & GEVWS_EXT_CLIENT_TAKEOVER)) {  // wave-uniform
      if (m && uniform32(msgs[m - 1].conn) == c) return;  // the connection's first message walks its messages
      inf_size_chain<CARRY>(fr, max_frames, msgs, n, m, c, msg_of, payload, limit,
                            inf_ctx + (uint64_t)c * GEVWS_INF_CTX_BYTES, s_in, s_tab, blk, rec, ca);
      return;
    }
  }
  if (!(msg.flags & GEVWS_MSG_COMPRESSED)) return;
  InfRec r;
  r.len = 0, r.status = GEVWS_MSG_OK, r.flags = GEVWS_INF_PENDING, r.pad = 0;
  uint64_t len = 0;
  const InfWhole w = inf_whole<CARRY>(msg, ca);
  if (CARRY && w.kind == kInfLost) {
    r.status = (uint8_t)w.status, r.flags = GEVWS_INF_DONE;
  } else if (w.kind != kInfPending) {
    InfSizeIo io(fr, msg_of, payload, s_in, m, msg, max_frames);
    if constexpr (CARRY)
      if (w.kind == kInfCarried) io.prefix(ca.src + w.psrc, w.pre);
    r.status = (uint8_t)gevws_inflate::inflate(io, s_tab, limit, &len);
    r.flags = GEVWS_INF_DONE;
    if (r.status != GEVWS_MSG_OK) len = 0;
    r.len = (uint32_t)len;
  }
  if (threadIdx.x == 0) {
    rec[m] = r;
    if (r.flags == GEVWS_INF_DONE) {
      const bool ok = r.status == GEVWS_MSG_OK;
      blk[m * kBlkFields + 0] = ok ? 1 : 0;
      blk[m * kBlkFields + 1] = round16(len);
      blk[m * kBlkFields + 2] = len;
      blk[m * kBlkFields + 3] = ok ? 0 : 1;
    }
  }
}

// ------------------------------------------------------------------ 1b. a malformed record fails the call
__global__ void k_inf_verdict(gevws_summary* __restrict__ sum) {
  const uint64_t bad = sum->errors >> 32;
  if (bad == 0) return;
  gevws_summary s;
  memset(&s, 0, sizeof(s));
  s.errors = bad;
  s.status = GEVWS_ERR_INVALID;
  *sum = s;
}

// The emit pass over connection c's messages from m on, the only code that
// writes a slot.  The slot's valid part goes into the LDS ring at its own
// indices, the chain is decoded with the ring position running on across the
// messages, and at the end the ring bytes this pass produced go back to the
// slot with the head: the ring image in HBM already holds the older bytes.
template <bool CARRY>
__device__ __forceinline__ void inf_emit_chain(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                               const gevws_message* __restrict__ msgs, uint64_t n, uint64_t m,
                                               uint32_t c, const int64_t* __restrict__ msg_of,
                                               const uint8_t* __restrict__ payload,
                                               const uint64_t* __restrict__ blk, const InfRec* __restrict__ rec,
                                               uint8_t* slot, uint8_t* s_win, uint8_t* s_in,
                                               gevws_inflate::Tables& s_tab, uint8_t* __restrict__ d_out,
                                               const InfCarry& ca) {
  const uint32_t lane = threadIdx.x & 63;
  // what the sizing pass decided for the chain
  bool any = false;
  uint32_t fail = 0;
  for (uint64_t k = m; k < n && uniform32(msgs[k].conn) == c; ++k) {
    const InfRec rk = rec[k];
    if (uniform32(rk.flags) != GEVWS_INF_DONE) continue;
    if (uniform32(rk.status) == GEVWS_MSG_OK) any = any || uniform32(rk.len) != 0;
    else if (!fail) fail = uniform32(rk.status);
  }
  const uint32_t broken = uniform32(slot[8]);
  if (!any && (fail == 0 || broken)) return;  // the slot stays as it is
  const uint64_t total0 = uniform64(*reinterpret_cast<const uint64_t*>(slot));
  uint64_t total = total0;
  uint8_t* ring = slot + kCtxHead;
  if (any) {
    const uint32_t valid = total0 < kInfWin ? (uint32_t)round16(total0) : kInfWin;
    for (uint32_t o = 16 * lane; o < valid; o += kInfIn)
      *reinterpret_cast<u32x4*>(s_win + o) = *reinterpret_cast<const u32x4*>(ring + o);
    wave_lds_order();
    for (uint64_t k = m; k < n && uniform32(msgs[k].conn) == c; ++k) {
      const InfRec rk = rec[k];
      const uint32_t len_k = uniform32(rk.len);
      // (after a failure or a stop nothing is DONE and OK any more)
      if (uniform32(rk.flags) != GEVWS_INF_DONE || uniform32(rk.status) != GEVWS_MSG_OK || len_k == 0) continue;
      const gevws_message msg = msgs[k];
      InfEmitIo<true> io(fr, msg_of, payload, s_in, k, msg, max_frames, s_win,
                         d_out + uniform64(blk[k * kBlkFields + 1]), total);
      if constexpr (CARRY) {  // (a continued message the sizing pass inflated: its record was OPEN | COMPRESSED)
        const InfWhole w = inf_whole<CARRY>(msg, ca);
        if (w.kind == kInfCarried) io.prefix(ca.src + w.psrc, w.pre);
      }
      uint64_t len = 0;
      // the sized length is the limit: the wave never writes past the message's allotted bytes
      (void)gevws_inflate::inflate(io, s_tab, (uint64_t)len_k, &len, total < kInfWin ? (uint32_t)total : kInfWin);
      io.finish();
      total += len_k;
    }
    wave_lds_order();
    // stream bytes [total0, total), at most the last 32 KiB of them, as whole
    // vectors: their other bytes are the slot's own (loaded above), or zeros
    // where the stream has not reached yet
    uint64_t x = total - total0 >= kInfWin ? total - kInfWin : total0;
    for (x = (x & ~15ull) + 16 * lane; x < total; x += kInfIn) {
      const uint32_t o = (uint32_t)x & (kInfWin - 1);
      u32x4 v = *reinterpret_cast<const u32x4*>(s_win + o);
      if (total < kInfWin && total - x < 16) v = keep_bytes(v, (int64_t)(total - x));
      *reinterpret_cast<u32x4*>(ring + o) = v;
    }
  }
  if (lane == 0) {
    *reinterpret_cast<uint64_t*>(slot) = total;
    if (fail && !broken) slot[8] = (uint8_t)fail;
  }
}

// ------------------------------------------------------------------ 2. the bytes
template <bool CTX, bool CARRY = false>
__global__ __launch_bounds__(kInfBlock) void k_inf_emit(const gevws_frame* __restrict__ fr, uint64_t max_frames,
                                                        const gevws_message* __restrict__ msgs,
                                                        uint64_t max_messages, const int64_t* __restrict__ msg_of,
                                                        const gevws_summary* __restrict__ gate,
                                                        const uint8_t* __restrict__ payload,
                                                        const uint64_t* __restrict__ blk,
                                                        const InfRec* __restrict__ rec,
                                                        const gevws_summary* __restrict__ sum,
                                                        gevws_inflated* __restrict__ inflated,
                                                        uint8_t* __restrict__ d_out,
                                                        const uint8_t* __restrict__ conn_ext, uint8_t* inf_ctx,
                                                        InfCarry ca) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kInfWin];
  __shared__ __attribute__((aligned(16))) uint8_t s_in[kInfIn];
  __shared__ gevws_inflate::Tables s_tab;
  if (sum->status != GEVWS_OK) return;  // capacity: nothing written, the slots untouched
  const uint64_t m = inf_block_message<CTX>();
  const uint64_t n = gated_count(max_messages, gate);
  if (m >= n) return;
  const InfRec r = rec[m];
  const uint64_t base = blk[m * kBlkFields + 1];  // (exclusive after the scan)
  if (threadIdx.x == 0) {
    gevws_inflated o;
    memset(&o, 0, sizeof(o));
    if (r.flags) {
      o.out_off = r.flags == GEVWS_INF_DONE ? base : 0;
      o.length = r.len;
      o.status = r.status;
      o.flags = r.flags;
    }
    inflated[m] = o;
  }
  if constexpr (CTX) {
    const uint32_t c = uniform32(msgs[m].conn);  // (below n_conns, or the summary were INVALID)
    if ((!CARRY || conn_ext) && (uniform32(conn_ext[c]) & GEVWS_EXT_CLIENT_TAKEOVER)) {  // wave-uniform
      if (m && uniform32(msgs[m - 1].conn) == c) return;  // the connection's first message walks its messages
      inf_emit_chain<CARRY>(fr, max_frames, msgs, n, m, c, msg_of, payload, blk, rec,
                            inf_ctx + (uint64_t)c * GEVWS_INF_CTX_BYTES, s_win, s_in, s_tab, d_out, ca);
      return;
    }
  }
  if (r.flags != GEVWS_INF_DONE || r.status != GEVWS_MSG_OK || r.len == 0) return;
  const gevws_message msg = msgs[m];
  InfEmitIo<false> io(fr, msg_of, payload, s_in, m, msg, max_frames, s_win, d_out + base);
  if constexpr (CARRY) {  // (a continued message the sizing pass inflated: its record was OPEN | COMPRESSED)
    const InfWhole w = inf_whole<CARRY>(msg, ca);
    if (w.kind == kInfCarried) io.prefix(ca.src + w.psrc, w.pre);
  }
  uint64_t len = 0;
  // the sized length is the limit: the wave never writes past its allotted bytes
  (void)gevws_inflate::inflate(io, s_tab, (uint64_t)r.len, &len);
  io.finish();
}

// ------------------------------------------------------------------ 3. inflated text is UTF-8
__global__ __launch_bounds__(kWalkBlock) void k_inf_utf8(const gevws_message* __restrict__ msgs, uint64_t max_messages,
                                                         const gevws_summary* __restrict__ gate,
                                                         gevws_summary* __restrict__ sum,
                                                         gevws_inflated* __restrict__ inflated,
                                                         const uint8_t* __restrict__ d_out) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t m = (uint64_t)blockIdx.x * (kWalkBlock / 64) + (threadIdx.x >> 6);  // one wave per message
  if (m >= gated_count(max_messages, gate)) return;
  const gevws_inflated o = inflated[m];
  if (o.flags != GEVWS_INF_DONE || o.status != GEVWS_MSG_OK || o.length == 0 || msgs[m].opcode != 1) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint8_t* __restrict__ p = d_out + o.out_off;
  const uint64_t L = o.length, nvec = (L + 15) >> 4;
  uint32_t bad = 0;
  for (uint64_t j = lane; j < nvec; j += 64) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * j);
    const uint32_t pw = j ? *reinterpret_cast<const uint32_t*>(p + 16 * j - 4) : 0u;
    bad |= utf8_vec_bad(v, pw, j, L, 0);
  }
  // ... and the text does not end inside a sequence
  const uint32_t l1 = p[L - 1], l2 = L >= 2 ? p[L - 2] : 0u, l3 = L >= 3 ? p[L - 3] : 0u;
  bad |= (uint32_t)(l1 >= 0xC0 || l2 >= 0xE0 || l3 >= 0xF0);
  if (__ballot(bad != 0) != 0 && lane == 0) {
    inflated[m].status = GEVWS_MSG_ERR_UTF8;
    atomicAdd(reinterpret_cast<unsigned long long*>(&sum->frames), ~0ull);  // one OK message fewer
    atomicAdd(reinterpret_cast<unsigned long long*>(&sum->errors), 1ull);
  }
}

// ------------------------------------------------------------------ 4. the carry state
__global__ __launch_bounds__(kWalkBlock) void k_inf_state(const gevws_message* __restrict__ msgs,
                                                          uint64_t max_messages,
                                                          const gevws_summary* __restrict__ gate,
                                                          const gevws_summary* __restrict__ sum,
                                                          const gevws_inflated* __restrict__ inflated,
                                                          gevws_msg_state* __restrict__ state) {
  if (sum->status != GEVWS_OK) return;  // capacity: the state kept for the retry
  const uint64_t n = gated_count(max_messages, gate);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (m >= n) return;
  const uint32_t c = msgs[m].conn;
  if (m && msgs[m - 1].conn == c) return;  // the connection's first message walks its messages
  for (uint64_t k = m; k < n && msgs[k].conn == c; ++k) {
    const gevws_inflated o = inflated[k];
    if (o.flags == GEVWS_INF_DONE && o.status != GEVWS_MSG_OK) {
      if (state[c].failed == 0) state[c].failed = o.status;
      break;
    }
  }
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_inflate_carry_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames,
                                         uint64_t max_frames, const gevws_message* d_messages, uint64_t max_messages,
                                         const int64_t* d_msg_of, const gevws_summary* d_msg_summary,
                                         const uint8_t* d_payload, uint64_t max_message_bytes,
                                         gevws_msg_state* d_state, gevws_inflated* d_inflated, uint8_t* d_out,
                                         uint64_t out_cap, gevws_summary* d_summary, const uint8_t* d_conn_ext,
                                         uint8_t* d_inf_ctx, uint32_t n_conns, const gevws_carry* d_carry_in,
                                         const uint8_t* d_carry_src, uint64_t carry_src_bytes) {
  const bool with_ctx = d_conn_ext && d_inf_ctx;  // either NULL: gevws_inflate_async, bit for bit
  const bool with_carry = d_carry_in && d_carry_src;  // either NULL: gevws_inflate_ctx_async, bit for bit
  if (with_ctx && ((reinterpret_cast<uintptr_t>(d_inf_ctx) & 15) || max_messages > 0x7FF00000ull))
    return GEVWS_ERR_INVALID;
  if (with_carry && ((reinterpret_cast<uintptr_t>(d_carry_src) & 15) || max_messages > 0x7FF00000ull))
    return GEVWS_ERR_INVALID;
  if (!ctx || !d_summary || max_messages > 0x7FFFFFFFull || max_message_bytes < 1 ||
      max_message_bytes > 0xFFFFFFFFull)
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (max_messages == 0 || max_frames == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_frames || !d_messages || !d_msg_of || !d_msg_summary || !d_payload || !d_inflated || (out_cap && !d_out))
    return GEVWS_ERR_INVALID;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, inf_scratch(nullptr, max_messages).total);
  if (r != GEVWS_OK) return r;
  const InfScratch s = inf_scratch(ctx->scratch, max_messages);
  GEVWS_HIP(hipMemsetAsync(ctx->scratch, 0, s.total, st));
  const uint32_t nm = (uint32_t)max_messages;
  const uint32_t ng = kInfSpread * inf_grid_q(nm);  // the grid with contexts (inf_block_message)
  const InfCarry none{nullptr, nullptr, 0};
  const InfCarry ca{d_carry_in, d_carry_src, carry_src_bytes};
  const uint8_t* ext = with_ctx ? d_conn_ext : nullptr;  // (the carry's kernels take the contexts or none)
  uint8_t* slots = with_ctx ? d_inf_ctx : nullptr;
  if (with_carry)
    k_inf_size<true, true><<<ng, kInfBlock, 0, st>>>(d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                                     d_msg_summary, d_payload, max_message_bytes, s.blk, s.rec, ext,
                                                     slots, n_conns, ca);
  else if (with_ctx)
    k_inf_size<true><<<ng, kInfBlock, 0, st>>>(d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                               d_msg_summary, d_payload, max_message_bytes, s.blk, s.rec, d_conn_ext,
                                               d_inf_ctx, n_conns, none);
  else
    k_inf_size<false><<<nm, kInfBlock, 0, st>>>(d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                                d_msg_summary, d_payload, max_message_bytes, s.blk, s.rec, nullptr,
                                                nullptr, 0, none);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nm, UINT64_MAX, out_cap, d_summary);
  if (with_carry) {
    k_inf_verdict<<<1, 1, 0, st>>>(d_summary);
    k_inf_emit<true, true><<<ng, kInfBlock, 0, st>>>(d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                                     d_msg_summary, d_payload, s.blk, s.rec, d_summary, d_inflated,
                                                     d_out, ext, slots, ca);
  } else if (with_ctx) {
    k_inf_verdict<<<1, 1, 0, st>>>(d_summary);
    k_inf_emit<true><<<ng, kInfBlock, 0, st>>>(d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                               d_msg_summary, d_payload, s.blk, s.rec, d_summary, d_inflated, d_out,
                                               d_conn_ext, d_inf_ctx, none);
  } else {
    k_inf_emit<false><<<nm, kInfBlock, 0, st>>>(d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                                d_msg_summary, d_payload, s.blk, s.rec, d_summary, d_inflated, d_out,
                                                nullptr, nullptr, none);
  }
  k_inf_utf8<<<(nm + kWalkBlock / 64 - 1) / (kWalkBlock / 64), kWalkBlock, 0, st>>>(d_messages, max_messages,
                                                                                   d_msg_summary, d_summary,
                                                                                   d_inflated, d_out);
  if (d_state)
    k_inf_state<<<(nm + kWalkBlock - 1) / kWalkBlock, kWalkBlock, 0, st>>>(d_messages, max_messages, d_msg_summary,
                                                                           d_summary, d_inflated, d_state);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_inflate_ctx_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames,
                                       uint64_t max_frames, const gevws_message* d_messages, uint64_t max_messages,
                                       const int64_t* d_msg_of, const gevws_summary* d_msg_summary,
                                       const uint8_t* d_payload, uint64_t max_message_bytes, gevws_msg_state* d_state,
                                       gevws_inflated* d_inflated, uint8_t* d_out, uint64_t out_cap,
                                       gevws_summary* d_summary, const uint8_t* d_conn_ext, uint8_t* d_inf_ctx,
                                       uint32_t n_conns) {
  return gevws_inflate_carry_async(ctx, stream, d_frames, max_frames, d_messages, max_messages, d_msg_of,
                                   d_msg_summary, d_payload, max_message_bytes, d_state, d_inflated, d_out, out_cap,
                                   d_summary, d_conn_ext, d_inf_ctx, n_conns, nullptr, nullptr, 0);
}

extern "C" int gevws_inflate_async(gevws_ctx* ctx, void* stream, const gevws_frame* d_frames, uint64_t max_frames,
                                   const gevws_message* d_messages, uint64_t max_messages, const int64_t* d_msg_of,
                                   const gevws_summary* d_msg_summary, const uint8_t* d_payload,
                                   uint64_t max_message_bytes, gevws_msg_state* d_state,
                                   gevws_inflated* d_inflated, uint8_t* d_out, uint64_t out_cap,
                                   gevws_summary* d_summary) {
  return gevws_inflate_ctx_async(ctx, stream, d_frames, max_frames, d_messages, max_messages, d_msg_of, d_msg_summary,
                                 d_payload, max_message_bytes, d_state, d_inflated, d_out, out_cap, d_summary, nullptr,
                                 nullptr, 0);
}
