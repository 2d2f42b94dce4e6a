// inflate_fuzz.cpp -- the DEFLATE decode core (gev_amd/csrc/gevws_inflate_core.hpp)
// and gevws_inflate_raw (gevws_inflate_host.cpp) on hostile input, built with
// -fsanitize=address,undefined (tests/test_inflate_host.py): hand-made streams
// of every block type, their bit flips, byte overwrites and truncations, and
// random bytes, each under several output limits.  Checked here: the output
// buffer is sized exactly to the limit (ASan sees one byte too many), the
// verdict is one of the three, the produced length never passes the limit, a
// smaller limit yields a prefix of a larger one's bytes, and the core driven
// through a second Io (one that counts, as the device's sizing pass does)
// agrees with the exported function.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gev_amd/csrc/gevws_inflate_core.hpp"
#include "gevws.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

struct BitWriter {
  std::vector<uint8_t> out;
  uint32_t nbits = 0;
  void bits(uint32_t v, uint32_t n) {  // LSB first (header fields, extra bits)
    for (uint32_t i = 0; i < n; ++i) {
      if ((nbits & 7) == 0) out.push_back(0);
      out.back() |= (uint8_t)(((v >> i) & 1) << (nbits & 7));
      ++nbits;
    }
  }
  void code(uint32_t v, uint32_t n) {  // a Huffman code: MSB first
    for (uint32_t i = n; i-- > 0;) bits((v >> i) & 1, 1);
  }
  void align() { nbits = (nbits + 7) & ~7u; }
  void fixed_lit(uint32_t s) {
    if (s < 144) code(0x30 + s, 8);
    else if (s < 256) code(0x190 + s - 144, 9);
    else if (s < 280) code(s - 256, 7);
    else code(0xC0 + s - 280, 8);
  }
};

// A counting Io over host memory: what the device's sizing pass is.
struct CountIo {
  const uint8_t* in;
  uint64_t n, rd = 0, wr = 0;
  bool get(uint32_t& b) {
    if (rd >= n + 4) return false;
    b = rd < n ? in[rd] : (rd - n < 2 ? 0x00u : 0xffu);
    ++rd;
    return true;
  }
  void put(uint32_t) { ++wr; }
  void copy(uint32_t d, uint32_t len) {
    if (d > wr || len == 0) abort();  // the core checks the distance first
    wr += len;
  }
  uint64_t stored(uint64_t want) {
    const uint64_t k = want < n + 4 - rd ? want : n + 4 - rd;
    rd += k, wr += k;
    return k;
  }
};

uint64_t g_cases = 0, g_ok = 0;

void check(const std::vector<uint8_t>& s) {
  const uint64_t limits[] = {1, 7, 300, 70000};
  std::vector<uint8_t> prev;
  int prev_st = -1;
  for (uint64_t limit : limits) {
    std::vector<uint8_t> out(limit);  // exactly the limit: one byte more is an ASan report
    uint64_t len = ~0ull;
    const int st = gevws_inflate_raw(s.data(), s.size(), out.data(), limit, &len);
    if (st != GEVWS_MSG_OK && st != GEVWS_MSG_ERR_DEFLATE && st != GEVWS_MSG_ERR_TOO_BIG) abort();
    if (len > limit) abort();
    if (st == GEVWS_MSG_ERR_TOO_BIG && len != limit) abort();
    if (prev_st >= 0) {  // a smaller limit saw a prefix, and failed if this one did
      if (prev.size() > len || (!prev.empty() && memcmp(prev.data(), out.data(), prev.size()) != 0)) abort();
      if (prev_st == GEVWS_MSG_OK && (st != GEVWS_MSG_OK || len != prev.size())) abort();
    }
    gevws_inflate::Tables t;
    CountIo io{s.data(), s.size()};
    uint64_t produced = 0;
    if (gevws_inflate::inflate(io, t, limit, &produced) != st || produced != len || io.wr != len) abort();
    prev.assign(out.begin(), out.begin() + (long)len);
    prev_st = st;
    ++g_cases;
    g_ok += st == GEVWS_MSG_OK;
  }
}

std::vector<std::vector<uint8_t>> seeds() {
  std::vector<std::vector<uint8_t>> v;
  {  // fixed block: literals, a run (distance 1), a far match, end of block, not final
    BitWriter w;
    w.bits(0, 1), w.bits(1, 2);
    for (const char* p = "websocket frame "; *p; ++p) w.fixed_lit((uint8_t)*p);
    w.fixed_lit(285), w.code(0, 5);            // length 258, distance 1
    w.fixed_lit(257 + 8), w.bits(1, 1), w.code(6, 5), w.bits(3, 2);  // length 12, distance 12
    w.fixed_lit(256);
    w.bits(0, 1), w.bits(0, 2), w.align();     // the sync flush's empty stored block, minus its tail
    v.push_back(w.out);
  }
  {  // stored blocks
    BitWriter w;
    for (int k = 0; k < 3; ++k) {
      const uint32_t n = k == 0 ? 0 : 37 * (uint32_t)k;
      w.bits(0, 3), w.align(), w.bits(n, 16), w.bits(~n & 0xffff, 16);
      for (uint32_t i = 0; i < n; ++i) w.bits(rnd() & 0xff, 8);
    }
    w.bits(0, 3), w.align();
    v.push_back(w.out);
  }
  {  // dynamic block: code lengths 2 for 'a', 'b', 256 and length symbol 257; one distance code
    BitWriter w;
    w.bits(0, 1), w.bits(2, 2);
    w.bits(1, 5), w.bits(0, 5), w.bits(15, 4);  // 258 lengths, 1 distance, 19 code-length codes
    // code-length code: symbols 0, 1, 2, 18 with 2 bits each
    const uint32_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (uint32_t i = 0; i < 19; ++i) w.bits(order[i] <= 2 || order[i] == 18 ? 2 : 0, 3);
    // canonical: 0 -> 00, 1 -> 01, 2 -> 10, 18 -> 11
    auto zeros = [&](uint32_t n) {
      while (n >= 11) {
        const uint32_t k = n > 138 ? 138 : n;
        w.code(3, 2), w.bits(k - 11, 7), n -= k;
      }
      while (n--) w.code(0, 2);
    };
    zeros(97), w.code(2, 2), w.code(2, 2), zeros(256 - 99), w.code(2, 2), w.code(2, 2);  // a b ... 256 257
    w.code(1, 2);                                                                     // the distance code: 1 bit
    // a: 00  b: 01  256: 10  257: 11 ; distance 0: 0
    w.code(0, 2), w.code(1, 2), w.code(0, 2), w.code(3, 2), w.code(0, 1), w.code(2, 2);
    w.bits(0, 3), w.align();
    v.push_back(w.out);
  }
  return v;
}

}  // namespace

int main() {
  const auto base = seeds();
  for (const auto& s : base) {  // the seeds themselves are valid streams
    std::vector<uint8_t> out(70000);
    uint64_t len = 0;
    if (gevws_inflate_raw(s.data(), s.size(), out.data(), out.size(), &len) != GEVWS_MSG_OK || len == 0) {
      fprintf(stderr, "a seed stream does not inflate\n");
      return 1;
    }
    check(s);
  }
  for (int it = 0; it < 60000; ++it) {
    std::vector<uint8_t> s = base[rnd() % base.size()];
    switch (rnd() % 5) {
      case 0:
        s[rnd() % s.size()] ^= (uint8_t)(1u << (rnd() & 7));
        break;
      case 1:
        for (uint32_t k = 1 + rnd() % 6; k; --k) {
          const uint32_t span = s.size() < 24 ? (uint32_t)s.size() : 24;
          s[rnd() % span] ^= (uint8_t)(1u << (rnd() & 7));
        }
        break;
      case 2:
        s.resize(rnd() % s.size());
        break;
      case 3:
        s[rnd() % s.size()] = (uint8_t)rnd();
        break;
      default:
        s.resize(1 + rnd() % 48);
        for (auto& c : s) c = (uint8_t)rnd();
    }
    check(s);
  }
  uint64_t zero = 0;  // NULL buffers are refused; no payload at all is a stored block cut short
  if (gevws_inflate_raw(nullptr, 3, nullptr, 0, &zero) != GEVWS_ERR_INVALID) return 1;
  if (gevws_inflate_raw(nullptr, 0, nullptr, 0, &zero) != GEVWS_MSG_ERR_DEFLATE || zero != 0) return 1;
  printf("inflate_fuzz ok: %llu runs, %llu inflated\n", (unsigned long long)g_cases, (unsigned long long)g_ok);
  return 0;
}
