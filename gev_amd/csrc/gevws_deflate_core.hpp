// gevws_deflate_core.hpp -- the raw DEFLATE (RFC 1951) compressor behind
// outbound permessage-deflate (RFC 7692 section 7.2.1), written once for the
// device (one wave per message, gevws_deflate.hip) and the host
// (gevws_deflate_raw, the fuzz program).  Fixed-Huffman and stored blocks
// only, greedy LZ77 with one candidate per hash slot, no context takeover.
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
//           d = (p - candidate) mod 65 536 when 1 <= d <= min(p, maxd); the
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
//   void stage(p0, n)                       the input up to p0 + 64 + 258 + 8 is at hand
//   void find(p0, cnt, run_end, n, maxd)    the step's lookups, extensions and inserts
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

// The whole message: its compressed length in bytes; with EMIT the bytes too.
template <bool EMIT, class W>
GEVWS_DEF_HD uint64_t deflate(W& w, uint64_t n, uint32_t maxd) {
  uint64_t bit = 0;
  for (uint64_t rs = 0; rs < n; rs += kRun) {
    const uint32_t rl = n - rs < kRun ? (uint32_t)(n - rs) : kRun;
    const uint64_t run_end = rs + rl, bit0 = bit;
    if (EMIT) {
      w.begin_run(bit0);
      w.put_bits(bit0, 2u, 3);  // BFINAL 0, BTYPE 01
    }
    bit += 3;
    uint64_t p0 = rs;
    while (p0 < run_end) {
      const uint32_t cnt = run_end - p0 < kLanes ? (uint32_t)(run_end - p0) : kLanes;
      w.stage(p0, n);
      w.find(p0, cnt, run_end, n, maxd);
      const uint64_t m = w.match_mask();
      const uint64_t all = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
      uint64_t lits = 0, take = 0;
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

}  // namespace gevws_deflate
