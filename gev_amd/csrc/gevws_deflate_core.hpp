// gevws_deflate_core.hpp -- the raw DEFLATE (RFC 1951) compressor behind
// outbound permessage-deflate (RFC 7692 section 7.2.1), written once for the
// device (one wave per message, gevws_deflate.hip) and the host
// (gevws_deflate_raw, the fuzz programs).  Fixed-Huffman and stored blocks,
// dynamic-Huffman blocks too with GEVWS_DEFLATE_DYNAMIC (the second half of
// this file), greedy LZ77 with one candidate per hash slot.
//
// Context takeover.  A message may continue a connection's stream: it starts
// at stream position B (0 without a context), and every position below is a
// STREAM position -- message byte p is stream byte B + p, it sits at ring byte
// (B + p) mod 32 768 and its hash slot holds (B + p) mod 65 536.  The ring and
// the hash table are then the connection's, carried from message to message
// (gevws_deflate_ctx_async, gevws_deflate_raw_ctx): the table is not cleared,
// and a match may reach back across the message's first byte into history.
// Runs and steps still count from the message's first byte, and the last three
// positions of a message are not hashed (the next message is not known).
// B = 0 over an all-zero table is the compressor without a context, bit for bit.
//
// The algorithm is defined in steps of 64 consecutive positions so that a wave
// and a host loop make the same choices, byte for byte:
//
//   runs    The input is cut into runs of kRun bytes; a run becomes one block,
//           fixed or stored, whichever ends at the lower bit (both ends are
//           known before the choice).  No match crosses a run's end.
//   step    At p0 the positions p0 .. p0 + cnt - 1 (cnt <= 64, inside the
//           run) each hash the 4 bytes at p (when the message has them), read
//           the slot's candidate as it was BEFORE the step, and take
//           d = (p - candidate) mod 65 536 when 1 <= d <= min(p, maxd) (p the
//           stream position: history counts); the
//           match length is the common prefix of p and p - d, at most 258 and
//           at most the rest of the run; below 3 it is no match.  A second
//           candidate is the step's LOWEST position with the same slot (a run
//           or a short period that begins inside the step); it is taken when
//           its match is no shorter.  Then every hashed position is inserted; of
//           positions with the same slot the HIGHEST keeps it.  Which lane
//           holds a slot is thus fixed by the positions, never by the order
//           the hardware retires the lanes' stores in.  A stale or aliased
//           candidate only costs a comparison: the bytes decide.
//   choice  Greedy over the step from its first position: a match where there
//           is one (the positions it covers are passed over), else a literal.
//           The next step starts behind the step or behind its last match,
//           whichever is later: positions inside a long match are neither
//           searched nor inserted.
//   codes   Every token's bit string follows from the fixed code; a prefix
//           sum over the step gives the bit offsets, and the strings are ORed
//           into zeroed output.
//
// The driver below is generic over a W that holds the lanes:
//   void stage(p0, end)                     the input up to p0 + 64 + 258 + 8 is at hand (end: the message's)
//   void find(p0, cnt, run_end, end, maxd)  the step's lookups, extensions and inserts
//   uint64_t match_mask()                   positions (bit i: p0 + i) with a match
//   uint32_t len_at(i)                      its length
//   uint32_t tokens<EMIT>(lits, take, bit)  the bits of the step's tokens; writes them at `bit`
//   void begin_run(bit) / rewind(bit)       remember / forget everything written from `bit` on
//   void put_bits(bit, v, n)                n <= 32 bits
//   void stored(src, len, byte)             len input bytes from `src` to output byte `byte`
//   void end_run(bit)                       everything below `bit` is final
//   void finish(bytes)                      the message is `bytes` long
// Every loop here consumes input positions, so the work is bounded by n.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEVWS_DEF_HD __host__ __device__ __forceinline__
#else
#define GEVWS_DEF_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GEVWS_DEF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define GEVWS_DEF_UNI(x) ((uint32_t)(x))
#endif

namespace gevws_deflate {

constexpr uint32_t kLanes = 64, kRun = 4096, kMinMatch = 3, kMaxMatch = 258;
constexpr uint32_t kWin = 32768, kStage = 1024;
// The device keeps the last 32 KiB staged, up to 2 KiB of them ahead of the
// step, so a candidate is at hand up to this far back -- on the host too.
constexpr uint32_t kMaxDist = kWin - 2 * kStage;
constexpr uint32_t kHashBits = 12, kHashSlots = 1u << kHashBits;

// A run adds at most its bytes + 5 (a stored block from any bit position); the
// closing empty stored block, its 00 00 ff ff taken off, one more byte.
GEVWS_DEF_HD uint64_t bound(uint64_t n) { return n + 5 * ((n + kRun - 1) / kRun) + 1; }

GEVWS_DEF_HD uint32_t max_dist(uint32_t window_bits) {
  const uint32_t d = 1u << (window_bits ? window_bits : 15);
  return d < kMaxDist ? d : kMaxDist;
}

GEVWS_DEF_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

GEVWS_DEF_HD uint32_t rev(uint32_t v, uint32_t n) {  // the low n bits of v, reversed
#if defined(__clang__)
  return __builtin_bitreverse32(v) >> (32 - n);
#else
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1) << (n - 1 - i);
  return r;
#endif
}
GEVWS_DEF_HD uint32_t log2u(uint32_t x) {  // x >= 1
  return 31 - (uint32_t)__builtin_clz(x);
}

// A literal's fixed code (RFC 1951 3.2.6) as the bits to write, first bit lowest.
GEVWS_DEF_HD uint32_t lit_code(uint32_t b, uint32_t& nbits) {
  if (b < 144) {
    nbits = 8;
    return rev(0x30 + b, 8);
  }
  nbits = 9;
  return rev(0x190 + (b - 144), 9);
}

// A match (len 3..258, dist 1..32 768): length code, its extra bits, the
// 5-bit distance code, its extra bits; 12 to 31 bits.
GEVWS_DEF_HD uint32_t match_code(uint32_t len, uint32_t dist, uint32_t& nbits) {
  const uint32_t x = len - 3;
  uint32_t s, le = 0, lx = 0;
  if (x < 8) {
    s = x;
  } else if (len == 258) {
    s = 28;
  } else {
    le = log2u(x) - 2;
    s = 4 * le + 4 + ((x >> le) & 3);
    lx = x & ((1u << le) - 1);
  }
  uint32_t bits, n;
  if (s < 23) bits = rev(s + 1, 7), n = 7;
  else bits = rev(0xC0 + (s - 23), 8), n = 8;
  bits |= lx << n, n += le;
  const uint32_t y = dist - 1;
  uint32_t ds, de = 0, dx = 0;
  if (y < 4) {
    ds = y;
  } else {
    de = log2u(y) - 1;
    ds = 2 * de + 2 + ((y >> de) & 1);
    dx = y & ((1u << de) - 1);
  }
  bits |= rev(ds, 5) << n, n += 5;
  bits |= dx << n, n += de;
  nbits = n;
  return bits;
}

// One position's match against the candidate c16 (the slot's 16 bits): R reads
// 4 (u32, the hash) or 8 (u64, the comparison) input bytes at any position at
// hand (bytes past the message may be anything: the length is clamped before
// they count).
template <class R>
GEVWS_DEF_HD void match_one(const R& r, uint64_t p, uint32_t c16, uint64_t run_end, uint32_t maxd, uint32_t& len,
                            uint32_t& dist) {
  len = 0, dist = 0;
  const uint32_t d = ((uint32_t)p - c16) & 0xffffu;
  const uint64_t room = run_end - p;
  const uint32_t maxlen = room < kMaxMatch ? (uint32_t)room : kMaxMatch;
  if (d < 1 || d > maxd || d > p || maxlen < kMinMatch) return;
  uint32_t k = 0;
  while (k < maxlen) {
    const uint64_t x = r.u64(p + k) ^ r.u64(p + k - d);
    if (x) {
      k += (uint32_t)__builtin_ctzll(x) >> 3;
      break;
    }
    k += 8;
  }
  if (k > maxlen) k = maxlen;
  if (k >= kMinMatch) len = k, dist = d;
}

// The second candidate, the step's lowest position with the slot: taken when
// it is no shorter (it is the nearer one).  Not tried by that position itself
// or when the first match already reaches as far as a match may.
template <class R>
GEVWS_DEF_HD void second_one(const R& r, uint64_t p, uint32_t c16, uint64_t run_end, uint32_t maxd, uint32_t& len,
                             uint32_t& dist) {
  const uint64_t room = run_end - p;
  if (c16 == ((uint32_t)p & 0xffffu) || len == kMaxMatch || len == room) return;
  uint32_t len2, dist2;
  match_one(r, p, c16, run_end, maxd, len2, dist2);
  if (len2 && len2 >= len) len = len2, dist = dist2;
}

// The greedy choice over a step whose lookups are done: the literal positions,
// the positions where a match is taken, and how far the step got (>= cnt).
template <class W>
GEVWS_DEF_HD uint32_t choose(W& w, uint32_t cnt, uint64_t& lits, uint64_t& take) {
  const uint64_t m = w.match_mask();
  const uint64_t all = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
  lits = 0, take = 0;
  uint32_t pos = 0;
  while (pos < cnt) {
    const uint64_t rest = m >> pos;
    if (!rest) {
      lits |= all & ~((1ull << pos) - 1);
      pos = cnt;
      break;
    }
    const uint32_t skip = (uint32_t)__builtin_ctzll(rest);
    lits |= ((1ull << skip) - 1) << pos;
    pos += skip;
    take |= 1ull << pos;
    pos += w.len_at(pos);
  }
  return pos;
}

// The whole message: its compressed length in bytes; with EMIT the bytes too.
template <bool EMIT, class W>
GEVWS_DEF_HD uint64_t deflate(W& w, uint64_t n, uint32_t maxd, uint64_t B = 0) {
  uint64_t bit = 0;
  const uint64_t end = B + n;
  for (uint64_t rs = B; rs < end; rs += kRun) {
    const uint32_t rl = end - rs < kRun ? (uint32_t)(end - rs) : kRun;
    const uint64_t run_end = rs + rl, bit0 = bit;
    if (EMIT) {
      w.begin_run(bit0);
      w.put_bits(bit0, 2u, 3);  // BFINAL 0, BTYPE 01
    }
    bit += 3;
    uint64_t p0 = rs;
    while (p0 < run_end) {
      const uint32_t cnt = run_end - p0 < kLanes ? (uint32_t)(run_end - p0) : kLanes;
      w.stage(p0, end);
      w.find(p0, cnt, run_end, end, maxd);
      uint64_t lits, take;
      const uint32_t pos = choose(w, cnt, lits, take);
      bit += w.template tokens<EMIT>(lits, take, bit);
      p0 += pos;  // (>= cnt)
    }
    bit += 7;  // end of block: seven zero bits
    const uint64_t data = ((bit0 + 3 + 7) >> 3) + 4;  // the stored block's first data byte
    const uint64_t stored_end = 8 * (data + rl);
    if (stored_end < bit) {
      if (EMIT) {
        w.rewind(bit0);  // (BFINAL 0, BTYPE 00 and the pad: zero bits)
        w.put_bits(8 * (data - 4), rl | ((~rl & 0xffffu) << 16), 32);
        w.stored(rs, rl, data);
      }
      bit = stored_end;
    }
    if (EMIT) w.end_run(bit);
  }
  bit += 3;  // the empty stored block's header; its pad and 00 00 ff ff are not sent
  const uint64_t bytes = (bit + 7) >> 3;
  if (EMIT) w.finish(bytes);
  return bytes;
}

// ------------------------------------------------------------------ dynamic codes
// GEVWS_DEFLATE_DYNAMIC: the same runs and the same tokens, but a run may also
// become a dynamic-Huffman block (BTYPE 10).  A run's tokens are counted and
// (with EMIT) kept first; the code and its header are one integer function of
// the counts, so the three ends -- stored, fixed, dynamic -- are known before a
// bit is written, and the lowest wins (a tie: stored, then fixed).
//
// The table T[kTab] holds the 286 literal / length symbols at 0 and the 30
// distance symbols at kLL: the count in the low 16 bits while the code is built
// (a run has at most 4 097 symbols), the code's length in bits 16..20, and once
// the codes are assigned the code itself, reversed, in the low 16 bits.
//
// On top of the W above, a dynamic W has
//   void sync()                             what the lanes stored is visible to all
//   uint32_t sum_n(cnt, f)                  the sum of f(i), i < cnt, any order
//   uint32_t rank(T, N, A, S)               the used symbols sorted by (count, index): RankF below
//   uint32_t emit_n<EMIT>(cnt, bit, f)      the bits f(i, nbits) one after the other from `bit`
//   uint32_t* table() / scratch()           T[kTab]; kScrWords words for the construction
//   void begin_dyn()                        T, the kept tokens: empty
//   void note<EMIT>(lits, take, q)          counts the step's tokens (its first position: q in the run); EMIT keeps them
//   void scratch_done()                     the scratch is not used again in this run
//   uint32_t replay(rs, rl, bit)            the bits of the run's kept tokens by T
// The serial parts (the tree, the length limit, the header's run lengths, the
// canonical codes) run in every lane alike: each lane stores what all the
// others store, and reads back what it stored itself.
constexpr uint32_t kLL = 286, kND = 30, kCL = 19, kTab = 320;
constexpr uint32_t kMaxMatches = kRun / kMinMatch + 1;
constexpr uint32_t kScrA = 0, kScrS = 288, kScrBl = 576, kScrNx = 592, kScrCl = 608, kScrItems = 628;
constexpr uint32_t kScrWords = kScrItems + kTab;
// the dynamic header at its longest: HLIT, HDIST, HCLEN, 19 x 3, 316 lengths of 7 + 7 bits
constexpr uint32_t kMaxHeaderBits = 14 + 3 * kCL + (kLL + kND) * 14;

GEVWS_DEF_HD uint32_t len_sym(uint32_t len, uint32_t& eb, uint32_t& ev) {  // 0..28: symbol 257 + it
  const uint32_t x = len - 3;
  eb = 0, ev = 0;
  if (x < 8) return x;
  if (len == 258) return 28;
  eb = log2u(x) - 2, ev = x & ((1u << eb) - 1);
  return 4 * eb + 4 + ((x >> eb) & 3);
}
GEVWS_DEF_HD uint32_t dist_sym(uint32_t dist, uint32_t& eb, uint32_t& ev) {  // 0..29
  const uint32_t y = dist - 1;
  eb = 0, ev = 0;
  if (y < 4) return y;
  eb = log2u(y) - 1, ev = y & ((1u << eb) - 1);
  return 2 * eb + 2 + ((y >> eb) & 1);
}
// The extra bits behind symbol s of T, and its length in the fixed code.
GEVWS_DEF_HD uint32_t extra_bits(uint32_t s) {
  if (s < 265 || s == 285) return 0;
  if (s < kLL) return (s - 261) >> 2;
  return s < kLL + 4 ? 0 : (s - kLL - 2) >> 1;
}
GEVWS_DEF_HD uint32_t fixed_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < kLL ? 8 : 5; }
GEVWS_DEF_HD uint32_t fixed_entry(uint32_t s) {
  const uint32_t c = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : s < kLL ? 0xC0 + (s - 280) : s - kLL;
  return rev(c, fixed_len(s)) | (fixed_len(s) << 16);
}
GEVWS_DEF_HD uint32_t tab_len(uint32_t e) { return e >> 16; }
GEVWS_DEF_HD uint32_t tab_cnt(uint32_t e) { return e & 0xffffu; }

// A literal's and a match's bits by T: the match in two parts (length, distance), each below 32 bits.
GEVWS_DEF_HD uint32_t dyn_lit(const uint32_t* T, uint32_t b, uint32_t& nbits) {
  const uint32_t e = T[b];
  nbits = tab_len(e);
  return tab_cnt(e);
}
GEVWS_DEF_HD void dyn_match(const uint32_t* T, uint32_t len, uint32_t dist, uint32_t& c1, uint32_t& n1, uint32_t& c2,
                            uint32_t& n2) {
  uint32_t eb, ev;
  uint32_t e = T[257 + len_sym(len, eb, ev)];
  c1 = tab_cnt(e) | (ev << tab_len(e)), n1 = tab_len(e) + eb;
  e = T[kLL + dist_sym(dist, eb, ev)];
  c2 = tab_cnt(e) | (ev << tab_len(e)), n2 = tab_len(e) + eb;
}

// The code-length symbols in the order the header sends their lengths (RFC 1951 3.2.7).
GEVWS_DEF_HD uint32_t cl_order(uint32_t i) {
  // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                          6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)(i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u;
}
GEVWS_DEF_HD uint32_t cl_extra(uint32_t s) { return s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0; }

// rank(T, N, A, S): the used symbols of T[0, N) in rising (count, index)
// order, A their counts and S the symbols; how many there are.  One symbol's
// share, as the host takes them:
struct RankF {
  const uint32_t* T;
  uint32_t N;
  uint32_t *A, *S;
  GEVWS_DEF_HD uint32_t operator()(uint32_t s) const {
    const uint32_t c = tab_cnt(T[s]);
    if (!c) return 0;
    uint32_t r = 0;
    for (uint32_t t = 0; t < N; ++t) {
      const uint32_t ct = tab_cnt(T[t]);
      r += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1u : 0u;
    }
    A[r] = c, S[r] = s;
    return 1;
  }
};

struct LenF {  // the rarest symbols take the longest codes: sorted symbol i's length by the counts per length
  uint32_t* T;
  const uint32_t *S, *bl;
  uint32_t limit;
  GEVWS_DEF_HD uint32_t operator()(uint32_t i) const {
    uint32_t end = 0, len = limit;
    for (uint32_t l = limit; l > 0; --l) {
      end += bl[l];
      if (i < end) {
        len = l;
        break;
      }
    }
    T[S[i]] |= len << 16;
    return 0;
  }
};

// The lengths of a Huffman code for the counts in T[0, N), none above `limit`,
// into bits 16.. of T.  Two or more used symbols: a complete code (Kraft sum 1),
// no symbol with a larger count has a longer code.  One: length 1 (with
// `complete` a second symbol gets the other code of one bit, as a code-length
// code has to be complete).  None: symbol 0 gets length 1.
// The tree is Moffat and Katajainen's in-place construction over the sorted
// counts; lengths above the limit are cut to it and the Kraft sum is brought
// back to 1 on the counts per length: one code off the limit, the deepest
// shorter code one bit longer with a new sibling beside it, the sum one unit
// (2^-limit) less each time.
template <class W>
GEVWS_DEF_HD void code_lengths(W& w, uint32_t* T, uint32_t N, uint32_t limit, bool complete, uint32_t* scr) {
  uint32_t *A = scr + kScrA, *S = scr + kScrS, *bl = scr + kScrBl;
  const uint32_t n = w.rank(T, N, A, S);
  w.sync();
  if (n < 2) {
    const uint32_t s = n ? S[0] : 0;
    T[s] |= 1u << 16;
    if (complete) T[s ? 0 : 1] |= 1u << 16;
    w.sync();
    return;
  }
  // parents: A[i] becomes the index of internal node i's parent
  A[0] += A[1];
  uint32_t root = 0, leaf = 2;
  for (uint32_t next = 1; next + 1 < n; ++next) {
    uint32_t v;
    if (leaf >= n || A[root] < A[leaf]) {
      v = A[root];
      A[root] = next;
      ++root;
    } else {
      v = A[leaf++];
    }
    if (leaf >= n || (root < next && A[root] < A[leaf])) {
      v += A[root];
      A[root] = next;
      ++root;
    } else {
      v += A[leaf++];
    }
    A[next] = v;
  }
  // depths of the internal nodes
  A[n - 2] = 0;
  for (int32_t next = (int32_t)n - 3; next >= 0; --next) {
    A[next] = A[A[next]] + 1;
  }
  // leaves per depth, cut at the limit
  for (uint32_t i = 0; i <= 15; ++i) bl[i] = 0;
  {
    uint32_t avbl = 1, used = 0, depth = 0;
    int32_t r = (int32_t)n - 2;
    while (avbl > 0) {
      while (r >= 0 && A[r] == depth) ++used, --r;
      if (avbl > used) {
        bl[depth < limit ? depth : limit] += avbl - used;
      }
      avbl = 2 * used, ++depth, used = 0;
    }
  }
  uint32_t total = 0;
  for (uint32_t i = 1; i <= limit; ++i) total += bl[i] << (limit - i);
  while (total > (1u << limit)) {
    --bl[limit];
    for (uint32_t i = limit - 1; i > 0; --i)
      if (bl[i]) {
        --bl[i], bl[i + 1] += 2;
        break;
      }
    --total;
  }
  (void)w.sum_n(n, LenF{T, S, bl, limit});
  w.sync();
}

// Canonical codes (RFC 1951 3.2.2) for the lengths in T[0, N): each entry
// becomes its code, reversed, and its length.
template <class W>
GEVWS_DEF_HD void assign_codes(W& w, uint32_t* T, uint32_t N, uint32_t* scr) {
  uint32_t *bl = scr + kScrBl, *nx = scr + kScrNx;
  for (uint32_t i = 0; i <= 15; ++i) bl[i] = 0;
  for (uint32_t s = 0; s < N; ++s) {
    const uint32_t l = tab_len(T[s]);
    if (l) ++bl[l];
  }
  uint32_t code = 0;
  for (uint32_t l = 1; l <= 15; ++l) {
    code = (code + bl[l - 1]) << 1;
    nx[l] = code;
  }
  for (uint32_t s = 0; s < N; ++s) {
    const uint32_t l = tab_len(T[s]);
    if (l) {
      T[s] = rev(nx[l]++, l) | (l << 16);
    } else {
      T[s] = 0;
    }
  }
  w.sync();
}

struct BodyBitsF {  // a symbol's share of the block: its count x (code length + extra bits)
  const uint32_t* T;
  bool fixed;
  GEVWS_DEF_HD uint32_t operator()(uint32_t s) const {
    const uint32_t e = T[s];
    return tab_cnt(e) * ((fixed ? fixed_len(s) : tab_len(e)) + extra_bits(s));
  }
};
struct FixedTabF {
  uint32_t* T;
  GEVWS_DEF_HD uint32_t operator()(uint32_t s) const {
    T[s] = fixed_entry(s);
    return 0;
  }
};
struct ClLenF {  // the header's HCLEN x 3 bits
  const uint32_t* C;
  GEVWS_DEF_HD uint32_t operator()(uint32_t i, uint32_t& nbits) const {
    nbits = 3;
    return tab_len(C[cl_order(i)]);
  }
};
struct HdrItemF {  // a code-length symbol (low 8 bits of the item) and its extra bits (above)
  const uint32_t *items, *C;
  GEVWS_DEF_HD uint32_t operator()(uint32_t i, uint32_t& nbits) const {
    const uint32_t it = items[i], s = it & 0xffu, e = C[s];
    nbits = tab_len(e) + cl_extra(s);
    return tab_cnt(e) | ((it >> 8) << tab_len(e));
  }
};

// The lengths L[0, cnt) as code-length symbols from items[k] on: a run of
// zeros as 18 (11..138) and 17 (3..10), a repeated length as itself and 16
// (3..6 more); what is left over one by one.  Counts the symbols in C.
GEVWS_DEF_HD uint32_t rle_lengths(const uint32_t* L, uint32_t cnt, uint32_t* items, uint32_t k, uint32_t* C) {
  auto item = [&](uint32_t s, uint32_t extra) {
    items[k++] = s | (extra << 8), ++C[s];
  };
  uint32_t i = 0;
  while (i < cnt) {
    const uint32_t v = tab_len(L[i]);
    uint32_t run = 1;
    while (i + run < cnt && tab_len(L[i + run]) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const uint32_t r = run < 138 ? run : 138;
        item(18, r - 11), run -= r;
      }
      if (run >= 3) item(17, run - 3), run = 0;
    } else {
      item(v, 0), --run;
      while (run >= 3) {
        const uint32_t r = run < 6 ? run : 6;
        item(16, r - 3), run -= r;
      }
    }
    for (; run; --run) item(v, 0);
  }
  return k;
}

struct DynHeader {
  uint32_t hlit, hdist, hclen, items, bits;  // bits: everything behind the block's first three
};

// The code of a run from its counts in T, and the header that describes it.
template <class W>
GEVWS_DEF_HD DynHeader dyn_code(W& w, uint32_t* T, uint32_t* scr) {
  code_lengths(w, T, kLL, 15, false, scr);
  code_lengths(w, T + kLL, kND, 15, false, scr);
  DynHeader h;
  h.hlit = kLL, h.hdist = kND;
  while (h.hlit > 257 && tab_len(T[h.hlit - 1]) == 0) --h.hlit;
  while (h.hdist > 1 && tab_len(T[kLL + h.hdist - 1]) == 0) --h.hdist;
  uint32_t *C = scr + kScrCl, *items = scr + kScrItems;
  for (uint32_t i = 0; i < kCL; ++i) C[i] = 0;
  h.items = rle_lengths(T, h.hlit, items, 0, C);
  h.items = rle_lengths(T + kLL, h.hdist, items, h.items, C);
  w.sync();
  code_lengths(w, C, kCL, 7, true, scr);
  h.hclen = kCL;
  while (h.hclen > 4 && tab_len(C[cl_order(h.hclen - 1)]) == 0) --h.hclen;
  h.bits = 14 + 3 * h.hclen;
  for (uint32_t s = 0; s < kCL; ++s) h.bits += tab_cnt(C[s]) * (tab_len(C[s]) + cl_extra(s));
  return h;
}

// The whole message with GEVWS_DEFLATE_DYNAMIC.
template <bool EMIT, class W>
GEVWS_DEF_HD uint64_t deflate_dyn(W& w, uint64_t n, uint32_t maxd, uint64_t B = 0) {
  uint64_t bit = 0;
  const uint64_t end = B + n;
  uint32_t* T = w.table();
  uint32_t* scr = w.scratch();
  for (uint64_t rs = B; rs < end; rs += kRun) {
    const uint32_t rl = end - rs < kRun ? (uint32_t)(end - rs) : kRun;
    const uint64_t run_end = rs + rl, bit0 = bit;
    w.begin_dyn();
    uint64_t p0 = rs;
    while (p0 < run_end) {
      const uint32_t cnt = run_end - p0 < kLanes ? (uint32_t)(run_end - p0) : kLanes;
      w.stage(p0, end);
      w.find(p0, cnt, run_end, end, maxd);
      uint64_t lits, take;
      const uint32_t pos = choose(w, cnt, lits, take);
      w.template note<EMIT>(lits, take, (uint32_t)(p0 - rs));
      p0 += pos;
    }
    T[256] = 1;  // end of block
    w.sync();
    const uint64_t fixed_end = bit0 + 3 + w.sum_n(kLL + kND, BodyBitsF{T, true});
    const DynHeader h = dyn_code(w, T, scr);
    const uint64_t dyn_end = bit0 + 3 + h.bits + w.sum_n(kLL + kND, BodyBitsF{T, false});
    const uint64_t data = ((bit0 + 3 + 7) >> 3) + 4;  // the stored block's first data byte
    const uint64_t stored_end = 8 * (data + rl);
    if (stored_end <= fixed_end && stored_end <= dyn_end) {
      if (EMIT) {
        w.scratch_done();  // (BFINAL 0, BTYPE 00 and the pad: zero bits)
        w.put_bits(8 * (data - 4), rl | ((~rl & 0xffffu) << 16), 32);
        w.stored(rs, rl, data);
      }
      bit = stored_end;
    } else if (fixed_end <= dyn_end) {
      if (EMIT) {
        w.scratch_done();
        (void)w.sum_n(kLL + kND, FixedTabF{T});
        w.sync();
        w.put_bits(bit0, 2u, 3);  // BFINAL 0, BTYPE 01
        const uint64_t b = bit0 + 3 + w.replay(rs, rl, bit0 + 3);
        w.put_bits(b, tab_cnt(T[256]), 7);
      }
      bit = fixed_end;
    } else {
      if (EMIT) {
        uint32_t* C = scr + kScrCl;
        assign_codes(w, C, kCL, scr);
        assign_codes(w, T, kLL, scr);
        assign_codes(w, T + kLL, kND, scr);
        w.put_bits(bit0, 4u | ((h.hlit - 257) << 3) | ((h.hdist - 1) << 8) | ((h.hclen - 4) << 13), 17);  // BTYPE 10
        uint64_t b = bit0 + 17;
        b += w.template emit_n<true>(h.hclen, b, ClLenF{C});
        b += w.template emit_n<true>(h.items, b, HdrItemF{scr + kScrItems, C});
        w.scratch_done();
        b += w.replay(rs, rl, b);
        w.put_bits(b, tab_cnt(T[256]), tab_len(T[256]));
      }
      bit = dyn_end;
    }
    if (EMIT) w.end_run(bit);
  }
  bit += 3;  // the empty stored block's header; its pad and 00 00 ff ff are not sent
  const uint64_t bytes = (bit + 7) >> 3;
  if (EMIT) w.finish(bytes);
  return bytes;
}

// The steps above taken one after the other: the base of a host W.
struct SerialSteps {
  void sync() {}
  template <class F>
  uint32_t sum_n(uint32_t cnt, F f) {
    uint32_t a = 0;
    for (uint32_t i = 0; i < cnt; ++i) a += f(i);
    return a;
  }
  uint32_t rank(const uint32_t* T, uint32_t N, uint32_t* A, uint32_t* S) { return sum_n(N, RankF{T, N, A, S}); }
};

}  // namespace gevws_deflate
