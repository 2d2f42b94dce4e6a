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
  size_t total;
};
inline DefScratch def_scratch(void* base, uint64_t max_msgs) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  DefScratch s;
  size_t o = 0;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up(max_msgs * kBlkFields * sizeof(uint64_t));
  s.rec = reinterpret_cast<DefRec*>(p + o), o += up(max_msgs * sizeof(DefRec));
  s.total = o;
  return s;
}

// 4 input bytes at any position of the window (byte i of the message is at
// ring byte i mod 32 768).
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

template <bool EMIT>
struct DefWave {
  DefReader rd;
  uint32_t* ring;
  uint16_t* tab;
  uint32_t* obuf;             // EMIT: the bits from byte `flushed` of the payload on
  const uint8_t* src;         // the message's bytes (16-byte aligned)
  uint8_t* out;               // EMIT: its payload in d_out (16-byte aligned)
  uint64_t slot;              // EMIT: the bytes of d_out it owns
  uint64_t hi = 0;            // input bytes staged (whole KiB)
  uint64_t flushed = 0;       // payload bytes in d_out (whole vectors)
  uint32_t lane;
  uint32_t len = 0, dist = 0, byte = 0;  // the lane's position in this step
  uint32_t carry = 0;         // lanes 0..3: the staging buffer's first words at the run's start

  __device__ DefWave(uint32_t* ring_, uint16_t* tab_, uint32_t* obuf_, const uint8_t* src_, uint8_t* out_,
                     uint64_t slot_)
      : rd{ring_}, ring(ring_), tab(tab_), obuf(obuf_), src(src_), out(out_), slot(slot_), lane(threadIdx.x & 63) {}

  // The next KiB of the message into the window while the step's reach
  // (p0 + 64 + 258 + 8) may pass what is there.  At most 2 KiB are ever ahead
  // of p0, so the 30 KiB behind every position of the step stay.
  __device__ __forceinline__ void stage(uint64_t p0, uint64_t n) {
    while (hi < n && hi < p0 + kStage) {
      const uint64_t o = hi + 16 * lane;
      if (o < n)
        *reinterpret_cast<u32x4*>(ring + (((uint32_t)o & (kWin - 1)) >> 2)) = *reinterpret_cast<const u32x4*>(src + o);
      wave_lds_order();
      hi += kStage;
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
  // A run starts on a 4 KiB boundary: whole words of the window.
  __device__ __forceinline__ void stored(uint64_t from, uint32_t n, uint64_t byte_at) {
    const uint32_t nw = (n + 3) >> 2, w0 = (uint32_t)from >> 2;
    for (uint32_t i = lane; i < nw; i += kDefBlock) {
      uint32_t v = ring[(w0 + i) & (kRingWords - 1)];
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

template <bool EMIT>
struct DefWaveDyn : DefWave<EMIT> {
  using B = DefWave<EMIT>;
  uint32_t* T;       // kTab
  uint32_t* scr;     // kScrWords
  uint64_t* lm;      // EMIT: kMaskWords, the literal positions of the run
  uint64_t* tm;      // EMIT: kMaskWords, the positions where a match starts
  uint32_t* match;   // EMIT: kMaxMatches, (len - 3) | dist << 8 in order
  uint32_t nmatch = 0;

  __device__ DefWaveDyn(uint32_t* ring_, uint16_t* tab_, uint32_t* obuf_, const uint8_t* src_, uint8_t* out_,
                        uint64_t slot_, uint32_t* T_, uint32_t* scr_, uint64_t* lm_, uint64_t* tm_, uint32_t* match_)
      : B(ring_, tab_, obuf_, src_, out_, slot_), T(T_), scr(scr_), lm(lm_), tm(tm_), match(match_) {}

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

// ------------------------------------------------------------------ 1. checks and sizes
template <bool DYN>
__global__ __launch_bounds__(kDefBlock) void k_def_size(const gevws_deflate_msg* __restrict__ msgs, uint64_t max_msgs,
                                                        const gevws_summary* __restrict__ gate,
                                                        const uint8_t* __restrict__ src, uint64_t src_bytes,
                                                        uint32_t flags, uint64_t* __restrict__ blk,
                                                        DefRec* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) uint32_t s_ring[kRingWords];
  __shared__ __attribute__((aligned(16))) uint16_t s_tab[kHashSlots];
  const uint64_t m = blockIdx.x;
  if (m >= gated_count(max_msgs, gate)) return;  // (blk and rec are zeroed)
  const gevws_deflate_msg msg = msgs[m];
  const uint64_t off = uniform64(msg.payload_off), n = uniform64(msg.length);
  const uint32_t wb = uniform32(msg.window_bits), op = uniform32(msg.opcode);
  const bool bad = (op != 1 && op != 2) || (wb != 0 && (wb < 8 || wb > 15)) || (off & (GEVWS_PAYLOAD_ALIGN - 1)) ||
                   n > 0xFFFFFFFFull || n > src_bytes || off > src_bytes - n;
  if (bad) {
    if (threadIdx.x == 0) blk[m * kBlkFields + 3] = 1;
    return;
  }
  for (uint32_t j = threadIdx.x; j < kHashSlots / 8; j += kDefBlock)
    reinterpret_cast<u32x4*>(s_tab)[j] = u32x4{0, 0, 0, 0};
  wave_lds_order();
  uint64_t c;
  if constexpr (DYN) {
    __shared__ __attribute__((aligned(16))) uint32_t s_T[kTab];
    __shared__ __attribute__((aligned(16))) uint32_t s_scr[kScrWords];
    DefWaveDyn<false> w(s_ring, s_tab, nullptr, src + off, nullptr, 0, s_T, s_scr, nullptr, nullptr, nullptr);
    c = deflate_dyn<false>(w, n, max_dist(wb));
  } else {
    DefWave<false> w(s_ring, s_tab, nullptr, src + off, nullptr, 0);
    c = deflate<false>(w, n, max_dist(wb));
  }
  const bool plain = (flags & GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER) && c >= n;
  const uint64_t wire = plain ? n : c;
  if (threadIdx.x == 0) {
    rec[m] = DefRec{(uint32_t)wire, plain ? 1u : 0u};
    blk[m * kBlkFields + 0] = 1;
    blk[m * kBlkFields + 1] = round16(wire);
    blk[m * kBlkFields + 2] = wire;
  }
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
template <bool DYN>
__global__ __launch_bounds__(kDefBlock) void k_def_emit(const gevws_deflate_msg* __restrict__ msgs, uint64_t max_msgs,
                                                        const gevws_summary* __restrict__ gate,
                                                        const uint8_t* __restrict__ src,
                                                        const uint64_t* __restrict__ blk,
                                                        const DefRec* __restrict__ rec,
                                                        const gevws_summary* __restrict__ sum,
                                                        gevws_out_frame* __restrict__ frames,
                                                        uint8_t* __restrict__ d_out) {
  __shared__ __attribute__((aligned(16))) uint32_t s_ring[kRingWords];
  __shared__ __attribute__((aligned(16))) uint16_t s_tab[kHashSlots];
  __shared__ __attribute__((aligned(16))) uint32_t s_out[kOutWords];
  if (sum->status != GEVWS_OK) return;  // capacity or a malformed record: nothing written
  const uint64_t m = blockIdx.x;
  if (m >= gated_count(max_msgs, gate)) return;
  const gevws_deflate_msg msg = msgs[m];
  const DefRec r = rec[m];
  const uint64_t base = uniform64(blk[m * kBlkFields + 1]);  // (exclusive after the scan)
  const uint64_t off = uniform64(msg.payload_off), n = uniform64(msg.length);
  const uint32_t wire = uniform32(r.wire), plain = uniform32(r.plain);
  if (threadIdx.x == 0) {
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
  const uint8_t* __restrict__ p = src + off;
  uint8_t* __restrict__ q = d_out + base;
  if (plain) {  // verbatim, the last vector's pad zeroed
    for (uint64_t o = 16 * (uint64_t)threadIdx.x; o < n; o += 16 * kDefBlock) {
      u32x4 v = *reinterpret_cast<const u32x4*>(p + o);
      if (n - o < 16) v = keep_bytes(v, (int64_t)(n - o));
      *reinterpret_cast<u32x4*>(q + o) = v;
    }
    return;
  }
  for (uint32_t j = threadIdx.x; j < kHashSlots / 8; j += kDefBlock)
    reinterpret_cast<u32x4*>(s_tab)[j] = u32x4{0, 0, 0, 0};
  for (uint32_t j = threadIdx.x; j < kOutWords / 4; j += kDefBlock)
    reinterpret_cast<u32x4*>(s_out)[j] = u32x4{0, 0, 0, 0};
  wave_lds_order();
  // the sized length bounds the slot: the wave never writes past its allotted bytes
  if constexpr (DYN) {
    __shared__ __attribute__((aligned(16))) uint32_t s_T[kTab];
    __shared__ __attribute__((aligned(16))) uint64_t s_lm[kMaskWords];
    __shared__ __attribute__((aligned(16))) uint64_t s_tm[kMaskWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_match[kMaxMatches];
    DefWaveDyn<true> w(s_ring, s_tab, s_out, p, q, round16(wire), s_T, s_out + kScrAt, s_lm, s_tm, s_match);
    (void)deflate_dyn<true>(w, n, max_dist(uniform32(msg.window_bits)));
  } else {
    DefWave<true> w(s_ring, s_tab, s_out, p, q, round16(wire));
    (void)deflate<true>(w, n, max_dist(uniform32(msg.window_bits)));
  }
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_deflate_async(gevws_ctx* ctx, void* stream, const gevws_deflate_msg* d_msgs, uint64_t max_msgs,
                                   const gevws_summary* d_prev, const uint8_t* d_src, uint64_t src_bytes,
                                   uint32_t flags, gevws_out_frame* d_out_frames, uint8_t* d_out, uint64_t out_cap,
                                   gevws_summary* d_summary) {
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
  r = ensure_scratch(ctx, def_scratch(nullptr, max_msgs).total);
  if (r != GEVWS_OK) return r;
  const DefScratch s = def_scratch(ctx->scratch, max_msgs);
  GEVWS_HIP(hipMemsetAsync(ctx->scratch, 0, s.total, st));
  const uint32_t nm = (uint32_t)max_msgs;
  const bool dyn = flags & GEVWS_DEFLATE_DYNAMIC;
  if (dyn) k_def_size<true><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, s.blk, s.rec);
  else k_def_size<false><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, src_bytes, flags, s.blk, s.rec);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nm, UINT64_MAX, out_cap, d_summary);
  k_def_verdict<<<1, 1, 0, st>>>(d_summary);
  if (dyn)
    k_def_emit<true><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, s.blk, s.rec, d_summary, d_out_frames,
                                               d_out);
  else
    k_def_emit<false><<<nm, kDefBlock, 0, st>>>(d_msgs, max_msgs, d_prev, d_src, s.blk, s.rec, d_summary, d_out_frames,
                                                d_out);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
