// gevws_deflate.hip -- outbound permessage-deflate (RFC 7692 section 7.2.1):
// gevws_deflate_async (include/gevws.h) compresses a batch's messages, one
// wave per message, with the compressor of gevws_deflate_core.hpp, and writes
// the gevws_out_frame records the encoder frames them from.  The reference
// has no code for it.
//
// Four launches behind one memset, no host round trip:
//   k_def_size     one wave per message: checks the record and compresses
//                  without storing -- the payload's length, plain or not
//   k_scan_blocks  lays the payloads out in d_out, the summary, CAPACITY
//   k_def_verdict  one lane: a malformed record turns the summary into INVALID
//   k_def_emit     one wave per message: compresses again, the bits ORed into
//                  an LDS staging buffer that is flushed to d_out as 16-byte
//                  vectors run by run; writes d_out_frames
// The message is compressed twice rather than once into bound-sized slots and
// compacted: the lengths are device data, so the host could only size such
// slots from src_bytes x max_msgs (messages may share source bytes), and the
// compaction would move every byte once more; the sizing pass here writes
// nothing and, unlike the inflate's, runs lane-parallel.
//
// A wave's scalars -- positions, the bit offset, the masks of the token choice
// -- are the same in every lane; the lanes differ in the position they look
// up, extend and encode.  One wave is one workgroup.  LDS per wave: the 32 KiB
// input window + the 8 KiB hash table (4 096 slots of 16 bits) = 40 KiB when
// sizing, + the 4 736-byte staging buffer = 44.6 KiB when emitting: 4 and 3
// waves a CU of its 160 KiB.  A wave's LDS accesses complete in order, so the
// lanes hand bytes to each other through LDS without a barrier.
//
// With GEVWS_DEFLATE_DYNAMIC the two kernels run as k_def_size<true> /
// k_def_emit<true>: a run may become a dynamic-Huffman block (DefWaveDyn
// below).  46 032 B of LDS when sizing, 53 496 B when emitting: 3 waves a CU.
//
// gevws_deflate_ctx_async (server context takeover) launches the <DYN, true>
// instances, which serve both kinds of connection with a wave-uniform branch:
// a connection without the takeover bit runs the code above; a takeover
// connection's messages are a chain that the wave of the run's first message
// compresses in order, in both passes, the window and the hash table carried
// in the connection's slot of d_def_ctx (see "context takeover" below).  The
// slot's ring and table ARE the LDS window and table, so the <DYN, true>
// instances hold the LDS of their twins.  The <DYN, false> instances are the
// kernels of gevws_deflate_async, unchanged.
#include "gevws_deflate_core.hpp"
#include "gevws_internal.hpp"

namespace {

using namespace gevws_deflate;

constexpr uint32_t kDefBlock = 64;
constexpr uint32_t kRingWords = kWin / 4;
// a run's bits before they are final: the <= 16 bytes not flushed yet, a fixed
// block of kRun 9-bit literals, the widest token's overhang
constexpr uint32_t kOutWords = 1184;
static_assert(kOutWords % 4 == 0 && kOutWords * 32 >= 128 + 3 + 9 * kRun + 7 + 64, "the staging buffer holds a run");
static_assert(kStage == kDefBlock * 16, "a refill = one 16-byte vector a lane");
static_assert(sizeof(gevws_deflate_msg) == 24 && sizeof(gevws_out_frame) == 32, "deflate layouts");

// Keeps the compiler from moving one lane's LDS access across another's.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct DefRec {  // per message, between the passes
  uint32_t wire;   // payload bytes on the wire
  uint32_t plain;  // 1: sent as it is (GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER)
};

struct DefScratch {
  uint64_t* blk;  // per message: [1, bytes of d_out, wire length, 1 if malformed]
  DefRec* rec;
  uint32_t* heads;  // with contexts, per connection: the runs of a takeover connection in the list
  size_t total;
};
inline DefScratch def_scratch(void* base, uint64_t max_msgs, uint32_t n_conns = 0) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  DefScratch s;
  size_t o = 0;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up(max_msgs * kBlkFields * sizeof(uint64_t));
  s.rec = reinterpret_cast<DefRec*>(p + o), o += up(max_msgs * sizeof(DefRec));
  s.heads = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_conns * sizeof(uint32_t));
  s.total = o;
  return s;
}

// 4 input bytes at any position of the window (stream byte i -- byte i of the
// message without a context -- is at ring byte i mod 32 768).
struct DefReader {
  const uint32_t* ring;
  __device__ __forceinline__ uint32_t u32(uint64_t pos) const {
    const uint32_t i = (uint32_t)pos;
    const uint32_t w0 = ring[(i >> 2) & (kRingWords - 1)], w1 = ring[((i >> 2) + 1) & (kRingWords - 1)];
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * (i & 3)));
  }
  // ... and 8: three aligned words, independent reads
  __device__ __forceinline__ uint64_t u64(uint64_t pos) const {
    const uint32_t i = (uint32_t)pos, w = i >> 2, s = 8 * (i & 3);
    const uint32_t w0 = ring[w & (kRingWords - 1)], w1 = ring[(w + 1) & (kRingWords - 1)],
                   w2 = ring[(w + 2) & (kRingWords - 1)];
    const uint64_t lo = (((uint64_t)w1 << 32) | w0) >> s, hi = (((uint64_t)w2 << 32) | w1) >> s;
    return (lo & 0xffffffffull) | (hi << 32);
  }
};

// Bytes [lo, hi) of a vector (0 <= lo, hi <= 16).
__device__ __forceinline__ u32x4 byte_range16(int64_t lo, int64_t hi) {
  const u32x4 ones{~0u, ~0u, ~0u, ~0u};
  const u32x4 a = keep_bytes(ones, hi), b = keep_bytes(ones, lo);
  return u32x4{a[0] & ~b[0], a[1] & ~b[1], a[2] & ~b[2], a[3] & ~b[3]};
}

// CTX: a message of a context-takeover chain.  The ring and the table are the
// connection's, the message starts at stream position `base`, which is not
// 16-aligned in general, and every position is a stream position.
template <bool EMIT, bool CTX = false>
struct DefWave {
  DefReader rd;
  uint32_t* ring;
  uint16_t* tab;
  uint32_t* obuf;             // EMIT: the bits from byte `flushed` of the payload on
  const uint8_t* src;         // the message's bytes (16-byte aligned)
  uint8_t* out;               // EMIT: its payload in d_out (16-byte aligned)
  uint64_t slot;              // EMIT: the bytes of d_out it owns
  uint64_t hi = 0;            // input bytes staged (whole KiB; CTX: the stream position staged up to)
  uint64_t base = 0;          // CTX: the message's first byte in the stream
  uint64_t flushed = 0;       // payload bytes in d_out (whole vectors)
  uint32_t lane;
  uint32_t len = 0, dist = 0, byte = 0;  // the lane's position in this step
  uint32_t carry = 0;         // lanes 0..3: the staging buffer's first words at the run's start

  __device__ DefWave(uint32_t* ring_, uint16_t* tab_, uint32_t* obuf_, const uint8_t* src_, uint8_t* out_,
                     uint64_t slot_, uint64_t base_ = 0)
      : rd{ring_}, ring(ring_), tab(tab_), obuf(obuf_), src(src_), out(out_), slot(slot_), lane(threadIdx.x & 63) {
    if constexpr (CTX) base = base_, hi = base_ & ~15ull;
  }

  // The next KiB of the message into the window while the step's reach
  // (p0 + 64 + 258 + 8) may pass what is there.  At most 2 KiB are ever ahead
  // of p0, so the 30 KiB behind every position of the step stay.
  //
  // CTX: the ring vectors are the stream's, so the message's bytes are shifted
  // into them from two aligned source vectors (never one before the message's
  // first or wholly behind its last byte), and the vectors that hold its first
  // and its last byte are merged: the bytes before the message are the nearest
  // history, the bytes behind it the oldest -- or, while the stream is shorter
  // than the ring, zeros -- whatever lies behind the message in d_src.
  __device__ __forceinline__ void stage(uint64_t p0, uint64_t n) {
    if constexpr (CTX) {
      const uint32_t s = (uint32_t)base & 15;
      const uint64_t len = n - base;  // (n: the message's end in the stream)
      while (hi < n && hi < p0 + kStage) {
        const uint64_t x = hi + 16 * lane;  // a whole vector of the stream
        if (x < n) {
          const uint64_t j = (x + s - base) >> 4;  // source vector j holds message bytes [16 j, 16 j + 16)
          const u32x4 zero{0, 0, 0, 0};
          const u32x4 b = 16 * j < len ? *reinterpret_cast<const u32x4*>(src + 16 * j) : zero;
          u32x4 v = b;
          if (s) {
            const u32x4 a = j ? *reinterpret_cast<const u32x4*>(src + 16 * (j - 1)) : zero;
            v = funnel16(a, b, 16 - s);
          }
          u32x4* at = reinterpret_cast<u32x4*>(ring + (((uint32_t)x & (kWin - 1)) >> 2));
          const int64_t lo = x < base ? (int64_t)(base - x) : 0, hi16 = n - x < 16 ? (int64_t)(n - x) : 16;
          if (lo > 0 || hi16 < 16) {
            u32x4 old = *at;
            if (x < kWin) old = keep_bytes(old, lo);  // nothing was ever written behind the message
            const u32x4 m = byte_range16(lo, hi16);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (v[i] & m[i]) | (old[i] & ~m[i]);
          }
          *at = v;
        }
        wave_lds_order();
        hi += kStage;
      }
    } else {
      while (hi < n && hi < p0 + kStage) {
        const uint64_t o = hi + 16 * lane;
        if (o < n)
          *reinterpret_cast<u32x4*>(ring + (((uint32_t)o & (kWin - 1)) >> 2)) = *reinterpret_cast<const u32x4*>(src + o);
        wave_lds_order();
        hi += kStage;
      }
    }
  }

  // Every pending lane stores its position; a lane that reads back a position
  // that should have lost to its own stores again.  Each round settles at
  // least one lane of every contested slot, so at most 64 rounds; what the
  // slot holds in the end is fixed by the positions alone.
  template <bool LOWEST>
  __device__ __forceinline__ void insert(bool can, uint32_t h, uint32_t p16) {
    bool pend = can;
    while (__ballot(pend) != 0) {
      if (pend) tab[h] = (uint16_t)p16;
      wave_lds_order();
      if (pend) {
        const uint32_t r = tab[h];
        const uint32_t ahead = LOWEST ? (r - p16) & 0xffffu : (p16 - r) & 0xffffu;  // 1..63: the wrong lane won
        pend = ahead - 1u < 63u;
      }
      wave_lds_order();
    }
  }

  __device__ __forceinline__ void find(uint64_t p0, uint32_t cnt, uint64_t run_end, uint64_t n, uint32_t maxd) {
    const uint64_t p = p0 + lane;
    const bool can = lane < cnt && p + 4 <= n;
    const uint32_t v = rd.u32(p);
    byte = v & 0xffu;
    const uint32_t h = hash4(v), p16 = (uint32_t)p & 0xffffu;
    len = 0, dist = 0;
    const uint32_t c1 = can ? tab[h] : 0u;  // the table as the step found it
    wave_lds_order();
    if (can) match_one(rd, p, c1, run_end, maxd, len, dist);
    insert<true>(can, h, p16);
    const uint32_t c2 = can ? tab[h] : 0u;  // the step's lowest position with the slot
    wave_lds_order();
    if (can) second_one(rd, p, c2, run_end, maxd, len, dist);
    insert<false>(can, h, p16);
  }
  __device__ __forceinline__ uint64_t match_mask() const { return __ballot(len != 0); }
  __device__ __forceinline__ uint32_t len_at(uint32_t i) const {
    return (uint32_t)__builtin_amdgcn_readlane((int)len, (int)GEVWS_DEF_UNI(i));
  }

  // v (n <= 32 bits, the rest zero) ORed in at payload bit `bit`: other lanes
  // may hold bits of the same words.
  __device__ __forceinline__ void or_bits(uint64_t bit, uint32_t v) {
    const uint32_t o = (uint32_t)(bit - 8 * flushed), w = o >> 5;
    const uint64_t x = (uint64_t)v << (o & 31);
    if (w + 1 >= kOutWords) return;  // (never: the buffer holds a run)
    __hip_atomic_fetch_or(obuf + w, (uint32_t)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (x >> 32) __hip_atomic_fetch_or(obuf + w + 1, (uint32_t)(x >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }

  template <bool E>
  __device__ __forceinline__ uint32_t tokens(uint64_t lits, uint64_t take, uint64_t bit) {
    uint32_t nb = 0, code = 0;
    if ((lits >> lane) & 1) code = lit_code(byte, nb);
    else if ((take >> lane) & 1) code = match_code(len, dist, nb);
    const uint32_t incl = wave_incl_scan32_dpp(nb);
    if (E) {
      if (nb) or_bits(bit + (incl - nb), code);
      wave_lds_order();
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }

  __device__ __forceinline__ void zero_obuf(uint32_t words) {  // [0, words rounded up to a vector)
    for (uint32_t j = lane; 4 * j < words && 4 * j < kOutWords; j += kDefBlock)
      *reinterpret_cast<u32x4*>(obuf + 4 * j) = u32x4{0, 0, 0, 0};
    wave_lds_order();
  }
  // The run starts less than a vector past `flushed`: words 0..3 hold all there is.
  __device__ __forceinline__ void begin_run(uint64_t) {
    carry = lane < 4 ? obuf[lane] : 0u;
    wave_lds_order();
  }
  __device__ __forceinline__ void rewind(uint64_t) {
    zero_obuf(kOutWords);
    if (lane < 4) obuf[lane] = carry;
    wave_lds_order();
  }
  __device__ __forceinline__ void put_bits(uint64_t bit, uint32_t v, uint32_t) {
    if (lane == 0) or_bits(bit, v);
    wave_lds_order();
  }
  // A run starts on a 4 KiB boundary: whole words of the window.  (CTX: anywhere.)
  __device__ __forceinline__ void stored(uint64_t from, uint32_t n, uint64_t byte_at) {
    const uint32_t nw = (n + 3) >> 2, w0 = (uint32_t)from >> 2;
    for (uint32_t i = lane; i < nw; i += kDefBlock) {
      uint32_t v = CTX ? rd.u32(from + 4 * (uint64_t)i) : ring[(w0 + i) & (kRingWords - 1)];
      const uint32_t rem = n - 4 * i;
      if (rem < 4) v &= (1u << (8 * rem)) - 1u;
      or_bits(8 * (byte_at + 4 * (uint64_t)i), v);
    }
    wave_lds_order();
  }
  // `vecs` vectors of the buffer to d_out, never past the slot sized for the message.
  __device__ __forceinline__ void store_vecs(uint32_t vecs) {
    for (uint32_t j = lane; j < vecs; j += kDefBlock)
      if (flushed + 16 * (uint64_t)j + 16 <= slot)
        *reinterpret_cast<u32x4*>(out + flushed + 16 * (uint64_t)j) = *reinterpret_cast<const u32x4*>(obuf + 4 * j);
  }
  __device__ __forceinline__ void end_run(uint64_t bit) {
    const uint32_t local = (uint32_t)(bit - 8 * flushed), vecs = local >> 7;
    if (vecs == 0 || vecs >= kOutWords / 4) return;  // (the second never: a run's bits fit)
    store_vecs(vecs);
    const uint32_t keep = lane < 4 ? obuf[4 * vecs + lane] : 0u;  // (4 vecs + 3 < kOutWords: a run's bits fit)
    wave_lds_order();
    zero_obuf((local >> 5) + 2);
    if (lane < 4) obuf[lane] = keep;
    wave_lds_order();
    flushed += 16 * (uint64_t)vecs;
  }
  __device__ __forceinline__ void finish(uint64_t bytes) {  // the rest; the bits past the end are zero: the pad
    store_vecs((uint32_t)((bytes - flushed + 15) >> 4));
  }
};

// GEVWS_DEFLATE_DYNAMIC: the histogram and the code table T in LDS, and when
// emitting the run's tokens until its code is known -- a literal mask and a
// match mask over the run's positions and the matches in order (literals are
// read again from the window).  The construction's scratch is the staging
// buffer's tail when emitting (nothing of the run is written before the code is
// known, and the header ends below it), an array of its own when sizing.
constexpr uint32_t kMaskWords = kRun / 64 + 1;
constexpr uint32_t kScrAt = kOutWords - kScrWords;  // (when emitting)
static_assert(kScrWords <= kOutWords && kScrAt % 4 == 0 && kScrAt * 32 >= 128 + 3 + kMaxHeaderBits + 64,
              "the dynamic header ends below the scratch in the staging buffer");

template <bool EMIT, bool CTX = false>
struct DefWaveDyn : DefWave<EMIT, CTX> {
  using B = DefWave<EMIT, CTX>;
  uint32_t* T;       // kTab
  uint32_t* scr;     // kScrWords
  uint64_t* lm;      // EMIT: kMaskWords, the literal positions of the run
  uint64_t* tm;      // EMIT: kMaskWords, the positions where a match starts
  uint32_t* match;   // EMIT: kMaxMatches, (len - 3) | dist << 8 in order
  uint32_t nmatch = 0;

  __device__ DefWaveDyn(uint32_t* ring_, uint16_t* tab_, uint32_t* obuf_, const uint8_t* src_, uint8_t* out_,
                        uint64_t slot_, uint32_t* T_, uint32_t* scr_, uint64_t* lm_, uint64_t* tm_, uint32_t* match_,
                        uint64_t base_ = 0)
      : B(ring_, tab_, obuf_, src_, out_, slot_, base_), T(T_), scr(scr_), lm(lm_), tm(tm_), match(match_) {}

  __device__ __forceinline__ uint32_t* table() { return T; }
  __device__ __forceinline__ uint32_t* scratch() { return scr; }
  __device__ __forceinline__ void sync() { wave_lds_order(); }
  template <class F>
  __device__ __forceinline__ uint32_t sum_n(uint32_t cnt, F f) {
    uint32_t a = 0;
    for (uint32_t i = B::lane; i < cnt; i += kDefBlock) a += f(i);
    wave_lds_order();
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan32_dpp(a), 63);
  }
  // Every lane holds the keys (count, index) of up to five symbols and counts
  // the smaller keys as they come by, lane after lane: no sorting network, no
  // LDS traffic but the stores of the result.
  __device__ __forceinline__ uint32_t rank(const uint32_t* T_, uint32_t N, uint32_t* A, uint32_t* S) {
    constexpr uint32_t K = kTab / kDefBlock;
    uint32_t key[K], r[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t s = kDefBlock * k + B::lane, c = s < N ? tab_cnt(T_[s]) : 0u;
      key[k] = c ? (c << 16) | s : ~0u;
      r[k] = 0;
    }
    uint32_t n = 0;
#pragma unroll
    for (uint32_t kk = 0; kk < K; ++kk) {
      if (kDefBlock * kk >= N) break;
      n += (uint32_t)__popcll(__ballot(key[kk] != ~0u));
      for (uint32_t j = 0; j < kDefBlock; ++j) {
        const uint32_t kt = (uint32_t)__builtin_amdgcn_readlane((int)key[kk], (int)j);
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) r[k] += kt < key[k] ? 1u : 0u;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < K; ++k)
      if (key[k] != ~0u) A[r[k]] = key[k] >> 16, S[r[k]] = key[k] & 0xffffu;  // (r < the used symbols <= N)
    wave_lds_order();
    return n;
  }
  template <bool E, class F>
  __device__ __forceinline__ uint32_t emit_n(uint32_t cnt, uint64_t bit, F f) {
    uint32_t total = 0;
    for (uint32_t i0 = 0; i0 < cnt; i0 += kDefBlock) {
      uint32_t nb = 0, code = 0;
      if (i0 + B::lane < cnt) code = f(i0 + B::lane, nb);
      const uint32_t incl = wave_incl_scan32_dpp(nb);
      if (E && nb) B::or_bits(bit + total + (incl - nb), code);
      total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    wave_lds_order();
    return total;
  }
  __device__ __forceinline__ void begin_dyn() {
    for (uint32_t j = B::lane; j < kTab; j += kDefBlock) T[j] = 0;
    if (EMIT)
      for (uint32_t j = B::lane; j < kMaskWords; j += kDefBlock) lm[j] = 0, tm[j] = 0;
    nmatch = 0;
    wave_lds_order();
  }
  template <bool E>
  __device__ __forceinline__ void note(uint64_t lits, uint64_t take, uint32_t q) {
    const uint32_t lane = B::lane;
    if ((lits >> lane) & 1) {
      __hip_atomic_fetch_add(T + B::byte, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if ((take >> lane) & 1) {
      uint32_t eb, ev;
      __hip_atomic_fetch_add(T + 257 + len_sym(B::len, eb, ev), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(T + kLL + dist_sym(B::dist, eb, ev), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (E) {
        const uint32_t k = nmatch + (uint32_t)__popcll(take & ((1ull << lane) - 1));
        if (k < kMaxMatches) match[k] = (B::len - 3) | (B::dist << 8);  // (always: a match covers three positions)
      }
    }
    if (E) {
      const uint32_t w = q >> 6, sh = q & 63;  // (q < kRun: w + 1 < kMaskWords)
      if (lane == 0) {
        lm[w] |= lits << sh, tm[w] |= take << sh;
        if (sh) lm[w + 1] |= lits >> (64 - sh), tm[w + 1] |= take >> (64 - sh);
      }
      nmatch += (uint32_t)__popcll(take);
    }
    wave_lds_order();
  }
  // The scratch lies in the staging buffer: zero again before the run's bits reach it.
  __device__ __forceinline__ void scratch_done() {
    if (!EMIT) return;
    for (uint32_t j = B::lane; 4 * j < kScrWords; j += kDefBlock)
      *reinterpret_cast<u32x4*>(scr + 4 * j) = u32x4{0, 0, 0, 0};
    wave_lds_order();
  }
  __device__ __forceinline__ uint32_t replay(uint64_t rs, uint32_t rl, uint64_t bit) {
    const uint32_t lane = B::lane;
    uint32_t total = 0, k0 = 0;
    for (uint32_t c = 0; 64 * c < rl; ++c) {
      const uint64_t L = lm[c], M = tm[c];
      uint32_t c1 = 0, n1 = 0, c2 = 0, n2 = 0;
      if ((L >> lane) & 1) {
        c1 = dyn_lit(T, B::rd.u32(rs + 64 * c + lane) & 0xffu, n1);
      } else if ((M >> lane) & 1) {
        const uint32_t k = k0 + (uint32_t)__popcll(M & ((1ull << lane) - 1));
        const uint32_t m = k < kMaxMatches ? match[k] : 0u;
        dyn_match(T, (m & 0xffu) + 3, (m >> 8) | (m >> 8 == 0), c1, n1, c2, n2);
      }
      const uint32_t incl = wave_incl_scan32_dpp(n1 + n2);
      const uint64_t at = bit + total + (incl - n1 - n2);
      if (n1) B::or_bits(at, c1);
      if (n2) B::or_bits(at + n1, c2);
      total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      k0 += (uint32_t)__popcll(M);
    }
    wave_lds_order();
    return total;
  }
};

// ------------------------------------------------------------------ context takeover
// A takeover connection's messages depend on each other in order (message k's
// window is the messages before it), so the wave of the run's first message
// walks the run, one message after another, and the waves of its other
// messages exit -- in both passes, because the sizing needs the matches and so
// the window too.  Both passes load the slot (include/gevws.h: a 64-byte head,
// the ring image, the hash table) into the LDS ring and table at its own
// indices and carry the stream position in registers; the sizing pass writes
// nothing to the slot, the emit pass stores what it produced at the chain's end.
constexpr uint32_t kCtxHead = 64;
static_assert(GEVWS_DEF_CTX_BYTES == kCtxHead + kWin + 2 * kHashSlots && GEVWS_DEF_CTX_BYTES % 16 == 0,
              "slots, their rings and their tables lie on 16-byte boundaries");

// The message of a workgroup: with contexts the grid is kDefSpread x q
// workgroups and workgroup b takes message (b % kDefSpread) q + b / kDefSpread,
// the inflate step's mapping (gevws_inflate.hip): a chain's
// work sits in its first message's workgroup, and with a regular number of
// messages a connection the identity would put every chain head on one XCD.
constexpr uint32_t kDefSpread = 1024;
inline uint32_t def_grid_q(uint32_t nm) {
  const uint32_t q = (nm + kDefSpread - 1) / kDefSpread;
  return q <= 8 ? q : (q + 15) / 16 * 16;
}
template <bool CTX>
__device__ __forceinline__ uint64_t def_block_message() {
  if constexpr (CTX) return (uint64_t)(blockIdx.x % kDefSpread) * (gridDim.x / kDefSpread) + blockIdx.x / kDefSpread;
  else return blockIdx.x;
}

// The slot's valid part into the LDS ring and table; the connection's stream position.
__device__ __forceinline__ uint64_t def_load_slot(const uint8_t* __restrict__ slot, uint32_t* s_ring, uint16_t* s_tab) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total = uniform64(*reinterpret_cast<const uint64_t*>(slot));
  const uint32_t valid = total < kWin ? (uint32_t)round16(total) : kWin;
  for (uint32_t o = 16 * lane; o < valid; o += 16 * kDefBlock)
    *reinterpret_cast<u32x4*>(s_ring + (o >> 2)) = *reinterpret_cast<const u32x4*>(slot + kCtxHead + o);
  for (uint32_t j = lane; j < kHashSlots / 8; j += kDefBlock)
    reinterpret_cast<u32x4*>(s_tab)[j] = reinterpret_cast<const u32x4*>(slot + kCtxHead + kWin)[j];
  wave_lds_order();
  return total;
}

// ------------------------------------------------------------------ 1. checks and sizes
// Message k: its record checked, its payload sized.  CHAIN: it continues a
// takeover connection's stream at `total` (the LDS ring and table are the
// connection's); returns the stream position behind it.
template <bool DYN, bool CHAIN>
__device__ __forceinline__ uint64_t def_size_one(uint64_t k, const gevws_deflate_msg* __restrict__ msgs,
                                                 const uint8_t* __restrict__ src, uint64_t src_bytes, uint32_t flags,
                                                 uint64_t* __restrict__ blk, DefRec* __restrict__ rec,
                                                 uint32_t* s_ring, uint16_t* s_tab, uint32_t* s_T, uint32_t* s_scr,
                                                 uint64_t total, bool& bad) {
  const gevws_deflate_msg msg = msgs[k];
  const uint64_t off = uniform64(msg.payload_off), n = uniform64(msg.length);
  const uint32_t wb = uniform32(msg.window_bits), op = uniform32(msg.opcode);
  // (`bad` is handed out although no caller reads it: with it the <DYN, false>
  // kernels keep the instructions they had before there were contexts, and one
  // more scalar instruction in this prologue measured 0.5 % -- DESIGN section 5.7)
  bad = (op != 1 && op != 2) || (wb != 0 && (wb < 8 || wb > 15)) || (off & (GEVWS_PAYLOAD_ALIGN - 1)) ||
        n > 0xFFFFFFFFull || n > src_bytes || off > src_bytes - n;
  if (bad) {  // (the call is GEVWS_ERR_INVALID; a chain goes on without the message)
    if (threadIdx.x == 0) blk[k * kBlkFields + 3] = 1;
    return total;
  }
  if constexpr (!CHAIN) {
    for (uint32_t j = threadIdx.x; j < kHashSlots / 8; j += kDefBlock)
      reinterpret_cast<u32x4*>(s_tab)[j] = u32x4{0, 0, 0, 0};
    wave_lds_order();
  }
  uint64_t c;
  if constexpr (DYN) {
    DefWaveDyn<false, CHAIN> w(s_ring, s_tab, nullptr, src + off, nullptr, 0, s_T, s_scr, nullptr, nullptr, nullptr,
                               total);
    c = deflate_dyn<false>(w, n, max_dist(wb), total);
  } else {
    DefWave<false, CHAIN> w(s_ring, s_tab, nullptr, src + off, nullptr, 0, total);
    c = deflate<false>(w, n, max_dist(wb), total);
  }
  // (a takeover connection's message is never sent plain: it would have to stay out of the peer's window)
  const bool plain = !CHAIN && (flags & GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER) && c >= n;
  const uint64_t wire = plain ? n : c;
  if (threadIdx.x == 0) {
    rec[k] = DefRec{(uint32_t)wire, plain ? 1u : 0u};
    blk[k * kBlkFields + 0] = 1;
    blk[k * kBlkFields + 1] = round16(wire);
    blk[k * kBlkFields + 2] = wire;
  }
  return total + n;
}

// CTX: contexts are given (gevws_deflate_ctx_async); <DYN, false> is the kernel
// of gevws_deflate_async.
template <bool DYN, bool CTX>
__global__ __launch_bounds__(kDefBlock) void k_def_size(const gevws_deflate_msg* __restrict__ msgs, uint64_t max_msgs,
                                                        const gevws_summary* __restrict__ gate,
                                                        const uint8_t* __restrict__ src, uint64_t src_bytes,
                                                        uint32_t flags, uint64_t* __restrict__ blk,
                                                        DefRec* __restrict__ rec,
                                                        const uint32_t* __restrict__ msg_conn,
                                                        const uint8_t* __restrict__ conn_ext,
                                                        const uint8_t* __restrict__ def_ctx, uint32_t n_conns,
                                                        uint32_t* __restrict__ heads) {
  __shared__ __attribute__((aligned(16))) uint32_t s_ring[kRingWords];
  __shared__ __attribute__((aligned(16))) uint16_t s_tab[kHashSlots];
  uint32_t *s_T = nullptr, *s_scr = nullptr;
  if constexpr (DYN) {
    __shared__ __attribute__((aligned(16))) uint32_t s_Tm[kTab];
    __shared__ __attribute__((aligned(16))) uint32_t s_scrm[kScrWords];
    s_T = s_Tm, s_scr = s_scrm;
  }
  const uint64_t m = def_block_message<CTX>();
  const uint64_t cnt = gated_count(max_msgs, gate);
  if (m >= cnt) return;  // (blk and rec are zeroed)
  if constexpr (CTX) {
    const uint32_t c = uniform32(msg_conn[m]);
    if (c >= n_conns) {  // never an index: the call is GEVWS_ERR_INVALID (k_def_verdict)
      if (threadIdx.x == 0) blk[m * kBlkFields + 3] = 1;
      return;
    }
    if (uniform32(conn_ext[c]) & GEVWS_EXT_SERVER_TAKEOVER) {  // wave-uniform
      if (m && uniform32(msg_conn[m - 1]) == c) return;  // the run's first message walks the run
      // a second run of the connection: two waves would race on its slot
      uint32_t runs = 0;
      if (threadIdx.x == 0) runs = atomicAdd(heads + c, 1u);
      if (uniform32(runs) != 0) {
        if (threadIdx.x == 0) blk[m * kBlkFields + 3] = 1;
        return;
      }
      uint64_t total = def_load_slot(def_ctx + (uint64_t)c * GEVWS_DEF_CTX_BYTES, s_ring, s_tab);
      for (uint64_t k = m; k < cnt; ++k) {  // (at most the run's messages)
        if (k != m && uniform32(msg_conn[k]) != c) break;
        bool bad;
        total = def_size_one<DYN, true>(k, msgs, src, src_bytes, flags, blk, rec, s_ring, s_tab, s_T, s_scr, total,
                                        bad);
      }
      return;
    }
  }
  bool bad;
  (void)def_size_one<DYN, false>(m, msgs, src, src_bytes, flags, blk, rec, s_ring, s_tab, s_T, s_scr, 0, bad);
}

// ------------------------------------------------------------------ 2. a malformed record fails the call
__global__ void k_def_verdict(gevws_summary* __restrict__ sum) {
  const uint64_t e = sum->errors;
  if (e == 0) return;
  gevws_summary s;
  memset(&s, 0, sizeof(s));
  s.errors = e;
  s.status = GEVWS_ERR_INVALID;
  *sum = s;
}

// ------------------------------------------------------------------ 3. the bytes and the records
struct DefEmitLds {
  uint32_t *ring, *out, *T, *match;
  uint16_t* tab;
  uint64_t *lm, *tm;
};

// Message k's payload.  CHAIN: as in def_size_one.
template <bool DYN, bool CHAIN>
__device__ __forceinline__ uint64_t def_emit_one(const gevws_deflate_msg& msg, const DefRec& r, uint64_t base,
                                                 const uint8_t* __restrict__ src, uint8_t* __restrict__ d_out,
                                                 const DefEmitLds& s, uint64_t total) {
  const uint64_t off = uniform64(msg.payload_off), n = uniform64(msg.length);
  const uint32_t wire = uniform32(r.wire), plain = uniform32(r.plain);
  const uint8_t* __restrict__ p = src + off;
  uint8_t* __restrict__ q = d_out + base;
  if (!CHAIN && plain) {  // verbatim, the last vector's pad zeroed
    for (uint64_t o = 16 * (uint64_t)threadIdx.x; o < n; o += 16 * kDefBlock) {
      u32x4 v = *reinterpret_cast<const u32x4*>(p + o);
      if (n - o < 16) v = keep_bytes(v, (int64_t)(n - o));
      *reinterpret_cast<u32x4*>(q + o) = v;
    }
    return total;
  }
  if constexpr (!CHAIN) {
    for (uint32_t j = threadIdx.x; j < kHashSlots / 8; j += kDefBlock)
      reinterpret_cast<u32x4*>(s.tab)[j] = u32x4{0, 0, 0, 0};
  }
  for (uint32_t j = threadIdx.x; j < kOutWords / 4; j += kDefBlock)
    reinterpret_cast<u32x4*>(s.out)[j] = u32x4{0, 0, 0, 0};
  wave_lds_order();
  // the sized length bounds the slot: the wave never writes past its allotted bytes
  if constexpr (DYN) {
    DefWaveDyn<true, CHAIN> w(s.ring, s.tab, s.out, p, q, round16(wire), s.T, s.out + kScrAt, s.lm, s.tm, s.match,
                              total);
    (void)deflate_dyn<true>(w, n, max_dist(uniform32(msg.window_bits)), total);
  } else {
    DefWave<true, CHAIN> w(s.ring, s.tab, s.out, p, q, round16(wire), total);
    (void)deflate<true>(w, n, max_dist(uniform32(msg.window_bits)), total);
  }
  return total + n;
}

template <bool DYN, bool CTX>
__global__ __launch_bounds__(kDefBlock) void k_def_emit(const gevws_deflate_msg* __restrict__ msgs, uint64_t max_msgs,
                                                        const gevws_summary* __restrict__ gate,
                                                        const uint8_t* __restrict__ src,
                                                        const uint64_t* __restrict__ blk,
                                                        const DefRec* __restrict__ rec,
                                                        const gevws_summary* __restrict__ sum,
                                                        gevws_out_frame* __restrict__ frames,
                                                        uint8_t* __restrict__ d_out,
                                                        const uint32_t* __restrict__ msg_conn,
                                                        const uint8_t* __restrict__ conn_ext, uint8_t* def_ctx) {
  __shared__ __attribute__((aligned(16))) uint32_t s_ring[kRingWords];
  __shared__ __attribute__((aligned(16))) uint16_t s_tab[kHashSlots];
  __shared__ __attribute__((aligned(16))) uint32_t s_out[kOutWords];
  DefEmitLds s{s_ring, s_out, nullptr, nullptr, s_tab, nullptr, nullptr};
  if constexpr (DYN) {
    __shared__ __attribute__((aligned(16))) uint32_t s_T[kTab];
    __shared__ __attribute__((aligned(16))) uint64_t s_lm[kMaskWords];
    __shared__ __attribute__((aligned(16))) uint64_t s_tm[kMaskWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_match[kMaxMatches];
    s.T = s_T, s.lm = s_lm, s.tm = s_tm, s.match = s_match;
  }
  if (sum->status != GEVWS_OK) return;  // capacity or a malformed record: nothing written, the slots untouched
  const uint64_t m = def_block_message<CTX>();
  const uint64_t cnt = gated_count(max_msgs, gate);
  if (m >= cnt) return;
  const gevws_deflate_msg msg = msgs[m];
  const DefRec r = rec[m];
  const uint64_t base = uniform64(blk[m * kBlkFields + 1]);  // (exclusive after the scan)
  if (threadIdx.x == 0) {
    const uint32_t wire = uniform32(r.wire), plain = uniform32(r.plain);
    gevws_out_frame o;
    memset(&o, 0, sizeof(o));
    o.hdr.fin = 1;
    o.hdr.rsv = plain ? 0 : 4;
    o.hdr.opcode = msg.opcode;
    o.hdr.length = (int64_t)wire;
    o.payload_off = base;
    o.payload_len = wire;
    frames[m] = o;
  }
  if constexpr (CTX) {
    const uint32_t c = uniform32(msg_conn[m]);  // (below n_conns, or the summary were INVALID)
    if (uniform32(conn_ext[c]) & GEVWS_EXT_SERVER_TAKEOVER) {  // wave-uniform
      if (m && uniform32(msg_conn[m - 1]) == c) return;  // the run's first message walks the run
      uint8_t* slot = def_ctx + (uint64_t)c * GEVWS_DEF_CTX_BYTES;
      const uint64_t total0 = def_load_slot(slot, s_ring, s_tab);
      uint64_t total = total0;
      for (uint64_t k = m; k < cnt; ++k) {  // (at most the run's messages)
        if (k != m && uniform32(msg_conn[k]) != c) break;
        total = def_emit_one<DYN, true>(msgs[k], rec[k], uniform64(blk[k * kBlkFields + 1]), src, d_out, s, total);
      }
      if (total == total0) return;  // only empty messages: the slot stays as it is
      wave_lds_order();
      // stream bytes [total0, total), at most the last 32 KiB of them, as whole
      // vectors (the stage merged their other bytes: the slot's own, or zeros
      // where the stream has not reached yet), the table and the head
      const uint32_t lane = threadIdx.x & 63;
      uint64_t x = total - total0 >= kWin ? total - kWin : total0;
      for (x = (x & ~15ull) + 16 * lane; x < total; x += 16 * kDefBlock) {
        const uint32_t o = (uint32_t)x & (kWin - 1);
        *reinterpret_cast<u32x4*>(slot + kCtxHead + o) = *reinterpret_cast<const u32x4*>(s_ring + (o >> 2));
      }
      for (uint32_t j = lane; j < kHashSlots / 8; j += kDefBlock)
        reinterpret_cast<u32x4*>(slot + kCtxHead + kWin)[j] = reinterpret_cast<const u32x4*>(s_tab)[j];
      if (lane == 0) *reinterpret_cast<uint64_t*>(slot) = total;
      return;
    }
  }
  (void)def_emit_one<DYN, false>(msg, r, base, src, d_out, s, 0);
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_deflate_ctx_async(gevws_ctx* ctx, void* stream, const gevws_deflate_msg* d_msgs,
                                       uint64_t max_msgs, const gevws_summary* d_prev, const uint8_t* d_src,
                                       uint64_t src_bytes, uint32_t flags, gevws_out_frame* d_out_frames,
                                       uint8_t* d_out, uint64_t out_cap, gevws_summary* d_summary,
                                       const uint32_t* d_msg_conn, const uint8_t* d_conn_ext, uint8_t* d_def_ctx,
                                       uint32_t n_conns) {
  const bool with_ctx = d_msg_conn && d_conn_ext && d_def_ctx;  // any NULL: gevws_deflate_async, bit for bit
  if (with_ctx && ((reinterpret_cast<uintptr_t>(d_def_ctx) & 15) || max_msgs > 0x7FF00000ull))
    return GEVWS_ERR_INVALID;
  if (!ctx || !d_summary || max_msgs > 0x7FFFFFFFull ||
      (flags & ~(GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER | GEVWS_DEFLATE_DYNAMIC)))
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (max_msgs == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_msgs || !d_src || !d_out_frames || !d_out) return GEVWS_ERR_INVALID;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  const uint32_t nc = with_ctx ? n_conns : 0;
  r = ensure_scratch(ctx, def_scratch(nullptr, max_msgs, nc).total);
  if (r != GEVWS_OK) return r;
  const DefScratch s = def_scratch(ctx->scratch, max_msgs, nc);
  GEVWS_HIP(hipMemsetAsync(ctx->scratch, 0, s.total, st));
  const uint32_t nm = (uint32_t)max_msgs;
  const uint32_t ng = kDefSpread * def_grid_q(nm);  // the grid with contexts (def_block_message)
  const bool dyn = flags & GEVWS_DEFLATE_DYNAMIC;
  if (with_ctx) {
    if (dyn)
      k_def_size<true, true><<<ng, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, s.blk, s.rec,
                                                       d_msg_conn, d_conn_ext, d_def_ctx, n_conns, s.heads);
    else
      k_def_size<false, true><<<ng, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, s.blk,
                                                        s.rec, d_msg_conn, d_conn_ext, d_def_ctx, n_conns, s.heads);
  } else if (dyn) {
    k_def_size<true, false><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, s.blk, s.rec,
                                                      nullptr, nullptr, nullptr, 0, nullptr);
  } else {
    k_def_size<false, false><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, s.blk, s.rec,
                                                       nullptr, nullptr, nullptr, 0, nullptr);
  }
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nm, UINT64_MAX, out_cap, d_summary);
  k_def_verdict<<<1, 1, 0, st>>>(d_summary);
  if (with_ctx) {
    if (dyn)
      k_def_emit<true, true><<<ng, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, s.blk, s.rec, d_summary,
                                                       d_out_frames, d_out, d_msg_conn, d_conn_ext, d_def_ctx);
    else
      k_def_emit<false, true><<<ng, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, s.blk, s.rec, d_summary,
                                                        d_out_frames, d_out, d_msg_conn, d_conn_ext, d_def_ctx);
  } else if (dyn) {
    k_def_emit<true, false><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, s.blk, s.rec, d_summary,
                                                      d_out_frames, d_out, nullptr, nullptr, nullptr);
  } else {
    k_def_emit<false, false><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, s.blk, s.rec, d_summary,
                                                       d_out_frames, d_out, nullptr, nullptr, nullptr);
  }
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_deflate_async(gevws_ctx* ctx, void* stream, const gevws_deflate_msg* d_msgs, uint64_t max_msgs,
                                   const gevws_summary* d_prev, const uint8_t* d_src, uint64_t src_bytes,
                                   uint32_t flags, gevws_out_frame* d_out_frames, uint8_t* d_out, uint64_t out_cap,
                                   gevws_summary* d_summary) {
  return gevws_deflate_ctx_async(ctx, stream, d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, d_out_frames, d_out,
                                 out_cap, d_summary, nullptr, nullptr, nullptr, 0);
}
