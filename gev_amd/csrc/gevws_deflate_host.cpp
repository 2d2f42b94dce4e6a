// gevws_deflate_host.cpp -- gevws_deflate_raw, gevws_deflate_raw_flags and gevws_deflate_bound
// (include/gevws.h): the compressor of gevws_deflate_core.hpp on host memory,
// the 64 positions of a step taken one after the other, and gevws_deflate_raw_ctx,
// the same over one connection's context slot (server context takeover).  Plain
// C++: it also builds outside the library, under sanitizers
// (tests/cpp/deflate_fuzz.cpp, tests/cpp/deflate_ctx_fuzz.cpp).
#include <cstring>

#include "gevws.h"
#include "gevws_deflate_core.hpp"

namespace {

using namespace gevws_deflate;

// A run's bits before they are final: a fixed block of kRun 9-bit literals,
// the partial byte before it and the step's slack.
constexpr uint32_t kOutBytes = kRun + kRun / 8 + 128;
// the slot (include/gevws.h): a 64-byte head, the ring image, the hash table
constexpr uint32_t kCtxHead = 64;
static_assert(GEVWS_DEF_CTX_BYTES == kCtxHead + kWin + kHashSlots * 2, "the deflate slot");

struct HostW {
  // Positions are stream positions: the message is stream bytes [B, B + n), and
  // what lies before B is read from the slot's ring as the call found it.
  struct Reader {
    const uint8_t* in;
    uint64_t n, B;
    const uint8_t* ring;  // with B > 0: stream byte i at ring[i & 32767]
    uint8_t at(uint64_t pos) const {  // zeros past the message (the core clamps before they count)
      if (pos < B) return ring[pos & (kWin - 1)];
      return pos - B < n ? in[pos - B] : 0;
    }
    uint32_t u32(uint64_t pos) const {
      uint32_t v = 0;
      for (uint32_t i = 0; i < 4; ++i) v |= (uint32_t)at(pos + i) << (8 * i);
      return v;
    }
    uint64_t u64(uint64_t pos) const { return (uint64_t)u32(pos) | ((uint64_t)u32(pos + 4) << 32); }
  } rd;
  uint8_t* out;          // NULL: sizing
  uint64_t flushed = 0;  // bytes of out that are final; obuf[0] is byte `flushed`
  uint64_t p0 = 0;
  uint32_t cnt = 0;
  uint16_t tab[kHashSlots];
  uint32_t len[kLanes], dist[kLanes];
  uint8_t obuf[kOutBytes];

  // slot: the connection's context (its table is copied: the slot is written by the caller alone)
  HostW(const uint8_t* in, uint64_t n, uint8_t* out_, const uint8_t* slot = nullptr, uint64_t B = 0)
      : rd{in, n, B, slot ? slot + kCtxHead : nullptr}, out(out_) {
    if (slot) memcpy(tab, slot + kCtxHead + kWin, sizeof(tab));
    else memset(tab, 0, sizeof(tab));
    memset(obuf, 0, sizeof(obuf));
  }
  void stage(uint64_t, uint64_t) {}
  void find(uint64_t p0_, uint32_t cnt_, uint64_t run_end, uint64_t n, uint32_t maxd) {
    p0 = p0_, cnt = cnt_;
    uint32_t h[kLanes];
    for (uint32_t l = 0; l < cnt; ++l) {  // every lookup sees the table as the step found it
      const uint64_t p = p0 + l;
      len[l] = dist[l] = 0;
      h[l] = kHashSlots;
      if (p + 4 > n) continue;
      h[l] = hash4(rd.u32(p));
      match_one(rd, p, tab[h[l]], run_end, maxd, len[l], dist[l]);
    }
    for (uint32_t l = cnt; l-- > 0;)  // in falling order: the step's lowest position takes the slot ...
      if (h[l] < kHashSlots) tab[h[l]] = (uint16_t)(p0 + l);
    for (uint32_t l = 0; l < cnt; ++l)  // ... as every position's second candidate
      if (h[l] < kHashSlots) second_one(rd, p0 + l, tab[h[l]], run_end, maxd, len[l], dist[l]);
    for (uint32_t l = 0; l < cnt; ++l)  // in rising order: the highest position keeps the slot
      if (h[l] < kHashSlots) tab[h[l]] = (uint16_t)(p0 + l);
  }
  uint64_t match_mask() const {
    uint64_t m = 0;
    for (uint32_t l = 0; l < cnt; ++l) m |= (uint64_t)(len[l] != 0) << l;
    return m;
  }
  uint32_t len_at(uint32_t i) const { return len[i]; }
  void or_bits(uint64_t bit, uint32_t v) {
    const uint64_t o = bit - 8 * flushed;
    uint64_t x = (uint64_t)v << (o & 7);
    for (uint64_t i = o >> 3; x; ++i, x >>= 8) obuf[i] |= (uint8_t)x;
  }
  template <bool EMIT>
  uint32_t tokens(uint64_t lits, uint64_t take, uint64_t bit) {
    uint32_t total = 0;
    for (uint32_t l = 0; l < cnt; ++l) {
      uint32_t nb = 0, code = 0;
      if ((lits >> l) & 1) code = lit_code(rd.at(p0 + l), nb);
      else if ((take >> l) & 1) code = match_code(len[l], dist[l], nb);
      if (EMIT && nb) or_bits(bit + total, code);
      total += nb;
    }
    return total;
  }
  void begin_run(uint64_t) {}
  void rewind(uint64_t bit0) {
    const uint64_t o = bit0 - 8 * flushed;  // (< 8: end_run left a partial byte at most)
    obuf[o >> 3] &= (uint8_t)((1u << (o & 7)) - 1);
    memset(obuf + (o >> 3) + 1, 0, sizeof(obuf) - (o >> 3) - 1);
  }
  void put_bits(uint64_t bit, uint32_t v, uint32_t) { or_bits(bit, v); }
  void stored(uint64_t src, uint32_t n, uint64_t byte) { memcpy(obuf + (byte - flushed), rd.in + (src - rd.B), n); }
  void end_run(uint64_t bit) {
    const uint64_t whole = (bit >> 3) - flushed;
    memcpy(out + flushed, obuf, whole);
    const uint8_t part = obuf[whole];
    memset(obuf, 0, sizeof(obuf));
    obuf[0] = part;
    flushed += whole;
  }
  void finish(uint64_t bytes) {
    if (bytes > flushed) memcpy(out + flushed, obuf, bytes - flushed);
  }
};

// GEVWS_DEFLATE_DYNAMIC: the run's tokens are kept as the device keeps them --
// a literal mask, a match mask and the matches in order -- and replayed once
// the run's code is known.
struct HostDynW : HostW, SerialSteps {
  uint32_t tab32[kTab];
  uint32_t scr[kScrWords];
  uint64_t lm[kRun / 64 + 1], tm[kRun / 64 + 1];
  uint32_t match[kMaxMatches];
  uint32_t nmatch = 0;

  HostDynW(const uint8_t* in, uint64_t n, uint8_t* out_, const uint8_t* slot = nullptr, uint64_t B = 0)
      : HostW(in, n, out_, slot, B) {}
  uint32_t* table() { return tab32; }
  uint32_t* scratch() { return scr; }
  void begin_dyn() {
    memset(tab32, 0, sizeof(tab32));
    memset(lm, 0, sizeof(lm));
    memset(tm, 0, sizeof(tm));
    nmatch = 0;
  }
  template <bool EMIT>
  void note(uint64_t lits, uint64_t take, uint32_t q) {
    for (uint32_t l = 0; l < cnt; ++l) {
      if ((lits >> l) & 1) {
        ++tab32[rd.at(p0 + l)];
      } else if ((take >> l) & 1) {
        uint32_t eb, ev;
        ++tab32[257 + len_sym(len[l], eb, ev)];
        ++tab32[kLL + dist_sym(dist[l], eb, ev)];
        if (EMIT) match[nmatch++] = (len[l] - 3) | (dist[l] << 8);
      }
    }
    if (EMIT) {
      const uint32_t w = q >> 6, sh = q & 63;
      lm[w] |= lits << sh, tm[w] |= take << sh;
      if (sh) lm[w + 1] |= lits >> (64 - sh), tm[w + 1] |= take >> (64 - sh);
    }
  }
  template <bool EMIT, class F>
  uint32_t emit_n(uint32_t n, uint64_t bit, F f) {
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t nb = 0;
      const uint32_t code = f(i, nb);
      if (EMIT && nb) or_bits(bit + total, code);
      total += nb;
    }
    return total;
  }
  void scratch_done() {}
  uint32_t replay(uint64_t rs, uint32_t rl, uint64_t bit) {
    uint32_t total = 0, k = 0;
    for (uint32_t i = 0; i < rl; ++i) {
      if ((lm[i >> 6] >> (i & 63)) & 1) {
        uint32_t nb;
        const uint32_t code = dyn_lit(tab32, rd.at(rs + i), nb);
        or_bits(bit + total, code);
        total += nb;
      } else if ((tm[i >> 6] >> (i & 63)) & 1) {
        const uint32_t m = match[k++];
        uint32_t c1, n1, c2, n2;
        dyn_match(tab32, (m & 0xffu) + 3, m >> 8, c1, n1, c2, n2);
        or_bits(bit + total, c1);
        or_bits(bit + total + n1, c2);
        total += n1 + n2;
      }
    }
    return total;
  }
};

// slot: NULL, or the connection's context: both passes start from it as it
// stands (each on a copy of its table), and only a message that fits is
// appended to it -- the ring, the table as the emitting pass left it, the head.
template <class W, bool DYN>
int run(const uint8_t* in, uint64_t n, uint32_t maxd, uint8_t* out, uint64_t cap, uint64_t* out_len,
        uint8_t* slot = nullptr) {
  uint64_t B = 0;
  if (slot) memcpy(&B, slot, sizeof(B));
  uint64_t need;
  {
    W w(in, n, nullptr, slot, B);
    if constexpr (DYN) need = deflate_dyn<false>(w, n, maxd, B);
    else need = deflate<false>(w, n, maxd, B);
  }
  if (out_len) *out_len = need;
  if (need > cap) return GEVWS_ERR_CAPACITY;
  W w(in, n, out, slot, B);
  uint64_t got;
  if constexpr (DYN) got = deflate_dyn<true>(w, n, maxd, B);
  else got = deflate<true>(w, n, maxd, B);
  if (got != need) return GEVWS_ERR_INVALID;  // (the two passes are one algorithm)
  if (slot && n) {
    for (uint64_t i = n > kWin ? n - kWin : 0; i < n; ++i) slot[kCtxHead + ((B + i) & (kWin - 1))] = in[i];
    memcpy(slot + kCtxHead + kWin, w.tab, sizeof(w.tab));
    B += n;
    memcpy(slot, &B, sizeof(B));
  }
  return GEVWS_OK;
}

}  // namespace

extern "C" uint64_t gevws_deflate_bound(uint64_t n) { return gevws_deflate::bound(n); }

extern "C" int gevws_deflate_raw_flags(const uint8_t* in, uint64_t n, int window_bits, uint32_t flags, uint8_t* out,
                                       uint64_t cap, uint64_t* out_len) {
  if (out_len) *out_len = 0;
  if ((n && !in) || (cap && !out) || n > 0xFFFFFFFFull || (window_bits != 0 && (window_bits < 8 || window_bits > 15)) ||
      (flags & ~GEVWS_DEFLATE_DYNAMIC))
    return GEVWS_ERR_INVALID;
  const uint32_t maxd = max_dist((uint32_t)window_bits);
  if (flags & GEVWS_DEFLATE_DYNAMIC) return run<HostDynW, true>(in, n, maxd, out, cap, out_len);
  return run<HostW, false>(in, n, maxd, out, cap, out_len);
}

extern "C" int gevws_deflate_raw_ctx(const uint8_t* in, uint64_t n, int window_bits, uint32_t flags, uint8_t* out,
                                     uint64_t cap, uint64_t* out_len, uint8_t* ctx) {
  if (out_len) *out_len = 0;
  if (!ctx || (n && !in) || (cap && !out) || n > 0xFFFFFFFFull ||
      (window_bits != 0 && (window_bits < 8 || window_bits > 15)) || (flags & ~GEVWS_DEFLATE_DYNAMIC))
    return GEVWS_ERR_INVALID;
  const uint32_t maxd = max_dist((uint32_t)window_bits);
  if (flags & GEVWS_DEFLATE_DYNAMIC) return run<HostDynW, true>(in, n, maxd, out, cap, out_len, ctx);
  return run<HostW, false>(in, n, maxd, out, cap, out_len, ctx);
}

extern "C" int gevws_deflate_raw(const uint8_t* in, uint64_t n, int window_bits, uint8_t* out, uint64_t cap,
                                 uint64_t* out_len) {
  return gevws_deflate_raw_flags(in, n, window_bits, 0, out, cap, out_len);
}
