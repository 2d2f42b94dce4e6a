// gevws_inflate_core.hpp -- the raw DEFLATE (RFC 1951) block decoder behind
// permessage-deflate (RFC 7692), written once for the device (one wave per
// message, gevws_inflate.hip) and the host (gevws_inflate_raw, the fuzz
// program).  No allocation and no recursion; the symbol tables live in the
// Tables the caller hands in (LDS on the device), and the few small arrays
// beside them are only indexed by unrolled loops, so the device build keeps
// them in registers (none spills to scratch).
//
// The decoder is generic over an Io that joins the byte source and the sink:
//   bool get(uint32_t& b)            the next byte of the stream S, false at its end
//   void put(uint32_t b)             one output byte
//   void copy(uint32_t d, uint32_t n)  n >= 1 bytes from d back, as a byte-serial copy
//                                    (with a history, d may reach behind the message's first byte)
//   uint64_t stored(uint64_t n)      up to n bytes from the source to the sink;
//                                    returns how many there were
// On the device every lane of the wave runs this code on the same values
// (bit buffer, counters and table reads are wave-uniform); only the Io's
// methods work per lane.  GEVWS_INF_UNI tells the compiler so.
//
// Verdicts (include/gevws.h, gevws_inflate_async): a block that ends with
// BFINAL set ends the stream, one that ends with less than a whole byte of S
// unread ends it too (unless the bits left already spell block type 3);
// running out of S anywhere else, a distance beyond the bytes produced (plus
// the history the caller vouches for) and everything zlib's inflate rejects
// are kErrDeflate; an output byte beyond
// `limit` is kErrTooBig.  Errors come in stream order, as from a byte-serial
// decoder.  Every loop consumes at least one bit of S or produces at least one
// byte, so the work is bounded by the length of S and by `limit`.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEVWS_INF_HD __host__ __device__ __forceinline__
#else
#define GEVWS_INF_HD inline
#endif
#if defined(__clang__)
#define GEVWS_INF_UNROLL _Pragma("unroll")
#else
#define GEVWS_INF_UNROLL
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GEVWS_INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define GEVWS_INF_UNI(x) ((uint32_t)(x))
#endif

namespace gevws_inflate {

constexpr int kOk = 0, kErrDeflate = 7, kErrTooBig = 8;  // GEVWS_MSG_OK / _ERR_DEFLATE / _ERR_TOO_BIG
constexpr uint32_t kMaxBits = 15, kMaxLit = 288, kMaxDist = 32, kMaxCodes = 19;

// A canonical Huffman code: count[l] codes of l bits, their symbols in
// symbol[] ordered by length, then by value.  The arrays are in the Tables
// (memory); what a symbol's decode compares against is in a Code (registers:
// every loop over it has a constant trip count and is unrolled).
struct Code {
  uint32_t lim[kMaxBits + 1];   // l-bit codes are below lim[l], as 15-bit values (the code's bits first)
  uint32_t base[kMaxBits + 1];  // symbol[base[l] + code] is the symbol of the l-bit code `code`
};
struct Tables {
  uint16_t lsym[kMaxLit], dsym[kMaxDist], csym[kMaxCodes + 1];
  uint8_t lens[kMaxLit + kMaxDist];
};

struct Bits {
  uint64_t buf = 0;
  uint32_t cnt = 0;
};

// Bits of S into the buffer while a byte fits and S has one.
template <class Io>
GEVWS_INF_HD void refill(Bits& b, Io& io) {
  while (b.cnt <= 56) {
    uint32_t c;
    if (!io.get(c)) break;
    b.buf |= (uint64_t)c << b.cnt;
    b.cnt += 8;
  }
}
// n <= 32 bits, or false when S ends first.
template <class Io>
GEVWS_INF_HD bool take(Bits& b, Io& io, uint32_t n, uint32_t& v) {
  if (b.cnt < n) {
    refill(b, io);
    if (b.cnt < n) return false;
  }
  v = (uint32_t)(b.buf & ((1ull << n) - 1));
  b.buf >>= n;
  b.cnt -= n;
  return true;
}

// zlib's inflate_table verdict on n code lengths, the Code and the symbol
// order; false when the set is over-subscribed, or incomplete where zlib does
// not allow it (allowed: no code at all, or a single code of one bit, and
// neither for the code-length code).  On the device the wave counts and
// places 64 symbols at a time: a lane's symbol goes behind the symbols of its
// length in lower lanes (a ballot per length) and in earlier rounds.
GEVWS_INF_HD bool build(Code& code, uint16_t* symbol, const uint8_t* lens, uint32_t n, bool strict) {
  uint32_t cnt[kMaxBits + 1], run[kMaxBits + 1];
  GEVWS_INF_UNROLL
  for (uint32_t l = 0; l <= kMaxBits; ++l) cnt[l] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  for (uint32_t s0 = 0; s0 < n; s0 += 64) {
    const uint32_t mine = s0 + lane < n ? lens[s0 + lane] : 0u;
    GEVWS_INF_UNROLL
    for (uint32_t l = 1; l <= kMaxBits; ++l) cnt[l] += (uint32_t)__popcll(__ballot(mine == l));
  }
#else
  for (uint32_t s = 0; s < n; ++s) ++cnt[lens[s]];
#endif
  uint32_t max = 0, first = 0, index = 0;
  int32_t left = 1;
  bool over = false;
  GEVWS_INF_UNROLL
  for (uint32_t l = 1; l <= kMaxBits; ++l) {
    const uint32_t c = cnt[l];
    if (c) max = l;
    left = 2 * left - (int32_t)c;
    over = over || left < 0;
    code.lim[l] = over ? 0u : (first + c) << (kMaxBits - l);
    code.base[l] = index - first;
    run[l] = index;
    index += c;
    first = (first + c) << 1;
  }
  if (max == 0) return !strict;  // (no code: every lim is 0, nothing decodes)
  if (over) return false;
  if (left > 0 && (strict || max != 1)) return false;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t below = (1ull << lane) - 1;
  for (uint32_t s0 = 0; s0 < n; s0 += 64) {
    const uint32_t mine = s0 + lane < n ? lens[s0 + lane] : 0u;
    uint32_t at = 0;
    GEVWS_INF_UNROLL
    for (uint32_t l = 1; l <= kMaxBits; ++l) {
      const uint64_t same = __ballot(mine == l);
      if (mine == l) at = run[l] + (uint32_t)__popcll(same & below);
      run[l] += (uint32_t)__popcll(same);
    }
    if (mine) symbol[at] = (uint16_t)(s0 + lane);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the decode reads what other lanes placed)
  __builtin_amdgcn_wave_barrier();
#else
  for (uint32_t s = 0; s < n; ++s)
    if (lens[s]) symbol[run[lens[s]]++] = (uint16_t)s;
#endif
  return true;
}

// One symbol, or -1: S ended inside the code, or the bits are no code of an
// incomplete set.
// The next 15 bits of the buffer (zeros past its fill) with the first bit on
// top: the value a Huffman code, packed from its most significant bit, has.
GEVWS_INF_HD uint32_t peek15(const Bits& b) {
  uint32_t v = (uint32_t)b.buf;
#if defined(__clang__)
  v = __builtin_bitreverse32(v);
#else
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
  v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
  v = (v >> 16) | (v << 16);
#endif
  return v >> (32 - kMaxBits);
}

template <class Io>
GEVWS_INF_HD int32_t decode(Bits& b, Io& io, const Code& code, const uint16_t* symbol) {
  if (b.cnt < kMaxBits) refill(b, io);
  const uint32_t v = GEVWS_INF_UNI(peek15(b));
  uint32_t len = 0, base = 0;
  GEVWS_INF_UNROLL
  for (uint32_t l = kMaxBits; l >= 1; --l)  // the shortest length whose codes reach past v (lim[] never falls)
    if (v < code.lim[l]) len = l, base = code.base[l];
  if (len == 0 || len > b.cnt) return -1;
  b.buf >>= len;
  b.cnt -= len;
  return (int32_t)GEVWS_INF_UNI(symbol[base + (v >> (kMaxBits - len))]);
}

GEVWS_INF_HD uint32_t len_base(uint32_t s) {  // s = symbol - 257, 0..28
  return s < 8 ? 3 + s : (s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1)));
}
GEVWS_INF_HD uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
GEVWS_INF_HD uint32_t dist_base(uint32_t s) {  // 0..29
  return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1));
}
GEVWS_INF_HD uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

GEVWS_INF_HD void fixed_tables(Tables& t, Code& lit, Code& dist) {
  for (uint32_t s = 0; s < 144; ++s) t.lens[s] = 8;
  for (uint32_t s = 144; s < 256; ++s) t.lens[s] = 9;
  for (uint32_t s = 256; s < 280; ++s) t.lens[s] = 7;
  for (uint32_t s = 280; s < 288; ++s) t.lens[s] = 8;
  for (uint32_t s = 0; s < 32; ++s) t.lens[288 + s] = 5;
  build(lit, t.lsym, t.lens, 288, false);
  build(dist, t.dsym, t.lens + 288, 32, false);
}

// The header of a dynamic block into the tables.
template <class Io>
GEVWS_INF_HD bool dynamic_tables(Bits& b, Io& io, Tables& t, Code& lit, Code& dist) {
  uint32_t v;
  if (!take(b, io, 14, v)) return false;
  const uint32_t nlen = (v & 31) + 257, ndist = ((v >> 5) & 31) + 1, ncode = (v >> 10) + 4;
  if (nlen > 286 || ndist > 30) return false;
  for (uint32_t i = 0; i < kMaxCodes; ++i) t.lens[i] = 0;
  for (uint32_t i = 0; i < ncode; ++i) {
    if (!take(b, io, 3, v)) return false;
    // the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const uint32_t j = i - 3;  // (i >= 3: 0, then 8 7 9 6 10 ... outwards from 8)
    const uint32_t pos = i < 3 ? 16 + i : (j == 0 ? 0 : ((j & 1) ? 8 + (j >> 1) : 8 - (j >> 1)));
    t.lens[pos] = (uint8_t)v;
  }
  Code cl;
  if (!build(cl, t.csym, t.lens, kMaxCodes, true)) return false;
  uint32_t have = 0, prev = 0;
  while (have < nlen + ndist) {
    const int32_t s = decode(b, io, cl, t.csym);
    if (s < 0) return false;
    if (s < 16) {
      t.lens[have++] = (uint8_t)s;
      prev = (uint32_t)s;
      continue;
    }
    uint32_t rep, val = 0;
    if (s == 16) {
      if (have == 0) return false;
      if (!take(b, io, 2, v)) return false;
      rep = 3 + v;
      val = prev;
    } else if (s == 17) {
      if (!take(b, io, 3, v)) return false;
      rep = 3 + v;
    } else {
      if (!take(b, io, 7, v)) return false;
      rep = 11 + v;
    }
    if (have + rep > nlen + ndist) return false;
    for (uint32_t i = 0; i < rep; ++i) t.lens[have++] = (uint8_t)val;
    prev = val;
  }
  if (GEVWS_INF_UNI(t.lens[256]) == 0) return false;  // no end-of-block code
  if (!build(lit, t.lsym, t.lens, nlen, false)) return false;
  return build(dist, t.dsym, t.lens + nlen, ndist, false);
}

// The whole stream.  *produced = bytes handed to the sink (at most limit).
// `history` (at most 32 768) = the bytes of the connection's earlier messages
// that lie before this one's first byte (context takeover): a distance may
// reach that far behind the message, and the sink's copy() serves it.  zlib
// counts the same way, so the check stays exact; 0 is a message on its own.
template <class Io>
GEVWS_INF_HD int inflate(Io& io, Tables& t, uint64_t limit, uint64_t* produced, uint32_t history = 0) {
  Bits b;
  Code lcode, dcode;
  uint64_t out = 0;
  int status = kOk;
  for (;;) {
    uint32_t v;
    if (!take(b, io, 3, v)) {
      status = kErrDeflate;
      break;
    }
    const uint32_t last = v & 1, type = v >> 1;
    if (type == 3) {
      status = kErrDeflate;
      break;
    }
    if (type == 0) {
      const uint32_t drop = b.cnt & 7;  // (the buffer holds whole bytes of S: its fill is S's alignment)
      b.buf >>= drop;
      b.cnt -= drop;
      if (!take(b, io, 32, v) || (v & 0xffff) != ((v >> 16) ^ 0xffff)) {
        status = kErrDeflate;
        break;
      }
      uint64_t n = v & 0xffff;
      while (n && b.cnt >= 8 && status == kOk) {  // the bytes already in the bit buffer
        if (out == limit) {
          status = kErrTooBig;
        } else {
          io.put((uint32_t)(b.buf & 0xff));
          b.buf >>= 8, b.cnt -= 8, ++out, --n;
        }
      }
      if (status != kOk) break;
      if (n) {
        const uint64_t want = n < limit - out ? n : limit - out;
        const uint64_t got = want ? io.stored(want) : 0;
        out += got;
        if (got < want) {
          status = kErrDeflate;
          break;
        }
        if (want < n) {  // the byte past the limit, if S has it
          uint32_t c;
          status = io.get(c) ? kErrTooBig : kErrDeflate;
          break;
        }
      }
    } else {
      if (type == 1) {
        fixed_tables(t, lcode, dcode);
      } else if (!dynamic_tables(b, io, t, lcode, dcode)) {
        status = kErrDeflate;
        break;
      }
      for (;;) {
        int32_t s = decode(b, io, lcode, t.lsym);
        if (s < 0) {
          status = kErrDeflate;
          break;
        }
        if (s < 256) {
          if (out == limit) {
            status = kErrTooBig;
            break;
          }
          io.put((uint32_t)s);
          ++out;
          continue;
        }
        if (s == 256) break;
        s -= 257;
        if (s >= 29) {
          status = kErrDeflate;
          break;
        }
        uint32_t len = len_base((uint32_t)s), dist, x;
        if (!take(b, io, len_extra((uint32_t)s), x)) {
          status = kErrDeflate;
          break;
        }
        len += x;
        const int32_t d = decode(b, io, dcode, t.dsym);
        if (d < 0 || d >= 30 || !take(b, io, dist_extra((uint32_t)d), x)) {
          status = kErrDeflate;
          break;
        }
        dist = dist_base((uint32_t)d) + x;
        if (dist > out + history) {
          status = kErrDeflate;
          break;
        }
        if (len > limit - out) {
          if (limit - out) io.copy(dist, (uint32_t)(limit - out));
          out = limit;
          status = kErrTooBig;
          break;
        }
        io.copy(dist, len);
        out += len;
      }
      if (status != kOk) break;
    }
    if (last) break;
    refill(b, io);
    if (b.cnt < 8) {  // no whole byte left: the message ends here
      if (b.cnt >= 3 && ((b.buf >> 1) & 3) == 3) status = kErrDeflate;  // (zlib already reads the next block type)
      break;
    }
  }
  *produced = out;
  return status;
}

}  // namespace gevws_inflate
