// deflate_dynamic_fuzz.cpp -- the dynamic-Huffman mode of the compressor
// (GEVWS_DEFLATE_DYNAMIC; gev_amd/csrc/gevws_deflate_core.hpp and
// gevws_deflate_host.cpp) built with -fsanitize=address,undefined
// (tests/test_deflate_dynamic_host.py).
//
// The code builder, called directly from the core header with the serial
// steps of the host: for Fibonacci, all-equal, single-symbol, two-symbol and
// random counts at the limits 15 and 7, every length is within the limit, the
// Kraft sum is exactly 1 for two or more symbols, no symbol with a larger
// count has a longer code, and the canonical codes are prefix-free.
//
// The compressor: random and structured messages of 0 .. 20 000 bytes with
// the flag, into a buffer sized exactly to the need with canary bytes behind
// it; the sizing length is the emitted length, cap = need - 1 writes nothing,
// gevws_inflate_raw gives the input back, the payload is never longer than
// without the flag, and flags 0 is gevws_deflate_raw byte for byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gev_amd/csrc/gevws_deflate_core.hpp"
#include "gevws.h"

namespace {

using namespace gevws_deflate;

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

constexpr uint8_t kCanary = 0xA5;
constexpr size_t kCanaries = 64;

#define REQUIRE(c)                                                                   \
  do {                                                                               \
    if (!(c)) {                                                                      \
      fprintf(stderr, "deflate_dynamic_fuzz: %s failed at line %d\n", #c, __LINE__); \
      abort();                                                                       \
    }                                                                                \
  } while (0)

uint64_t g_codes = 0;

// counts[0, N) -> lengths and codes, checked
void check_code(const std::vector<uint32_t>& counts, uint32_t limit, bool complete) {
  const uint32_t N = (uint32_t)counts.size();
  std::vector<uint32_t> T(counts), scr(kScrWords, 0xDEADBEEFu);
  SerialSteps w;
  code_lengths(w, T.data(), N, limit, complete, scr.data());
  uint32_t used = 0;
  uint64_t kraft = 0;  // in units of 2^-limit
  for (uint32_t s = 0; s < N; ++s) {
    const uint32_t l = tab_len(T[s]);
    REQUIRE(tab_cnt(T[s]) == counts[s]);
    REQUIRE(l <= limit);
    if (counts[s]) {
      REQUIRE(l >= 1);
      ++used;
    }
    if (l) kraft += 1ull << (limit - l);
  }
  if (used >= 2) {
    REQUIRE(kraft == 1ull << limit);
    for (uint32_t s = 0; s < N; ++s) REQUIRE((tab_len(T[s]) != 0) == (counts[s] != 0));
  } else {  // one code of one bit; a complete code has the other one too
    REQUIRE(kraft == (complete ? 2ull : 1ull) << (limit - 1));
    if (used == 1)
      for (uint32_t s = 0; s < N; ++s)
        if (counts[s]) REQUIRE(tab_len(T[s]) == 1);
  }
  for (uint32_t a = 0; a < N; ++a)
    for (uint32_t b = 0; b < N; ++b)
      if (counts[a] && counts[b] && counts[a] > counts[b]) REQUIRE(tab_len(T[a]) <= tab_len(T[b]));
  assign_codes(w, T.data(), N, scr.data());
  for (uint32_t a = 0; a < N; ++a)
    for (uint32_t b = 0; b < N; ++b) {
      const uint32_t la = tab_len(T[a]), lb = tab_len(T[b]);
      if (a == b || !la || !lb || la > lb) continue;
      // the codes are stored reversed: a is a prefix of b when b's first la bits are a
      REQUIRE((tab_cnt(T[b]) & ((1u << la) - 1)) != tab_cnt(T[a]));
    }
  ++g_codes;
}

void code_cases(uint32_t N, uint32_t limit, bool complete) {
  std::vector<uint32_t> c(N, 0);
  // Fibonacci counts: the deepest tree a given total allows (the counts stay below 2^16)
  for (uint32_t terms : {2u, 3u, 8u, 16u, 17u, 19u, 23u}) {
    if (terms > N) continue;
    for (int shuffled = 0; shuffled < 2; ++shuffled) {
      std::fill(c.begin(), c.end(), 0);
      uint32_t a = 1, b = 1;
      for (uint32_t i = 0; i < terms; ++i) {
        c[shuffled ? (i * 7 + 3) % N : i] = a;
        const uint32_t t = a + b;
        a = b, b = t;
      }
      check_code(c, limit, complete);
    }
  }
  for (uint32_t v : {1u, 2u, 4097u}) {  // all equal: every count, and a prefix of them
    std::fill(c.begin(), c.end(), v);
    check_code(c, limit, complete);
    for (uint32_t k : {3u, 5u, 17u})
      if (k < N) {
        std::fill(c.begin(), c.end(), 0);
        std::fill(c.begin(), c.begin() + k, v);
        check_code(c, limit, complete);
      }
  }
  std::fill(c.begin(), c.end(), 0);
  check_code(c, limit, complete);  // none
  for (uint32_t s : {0u, 1u, N - 1}) {  // one symbol
    std::fill(c.begin(), c.end(), 0);
    c[s] = 1 + rnd() % 4097;
    check_code(c, limit, complete);
  }
  for (int it = 0; it < 8; ++it) {  // two symbols
    std::fill(c.begin(), c.end(), 0);
    const uint32_t a = rnd() % N, b = (a + 1 + rnd() % (N - 1)) % N;
    c[a] = 1 + rnd() % 4097, c[b] = it & 1 ? c[a] : 1 + rnd() % 4097;
    check_code(c, limit, complete);
  }
  for (int it = 0; it < 300; ++it) {  // random: sparse, dense, skewed
    std::fill(c.begin(), c.end(), 0);
    const uint32_t fill = 1 + rnd() % N, shape = rnd() % 3;
    for (uint32_t k = 0; k < fill; ++k) {
      const uint32_t s = rnd() % N;
      c[s] = shape == 0 ? 1 + rnd() % 8 : shape == 1 ? 1 + rnd() % 4097 : 1u << (rnd() % 13);
    }
    check_code(c, limit, complete);
  }
}

std::vector<uint8_t> make(uint32_t n, uint32_t kind) {
  std::vector<uint8_t> v(n);
  switch (kind) {
    case 0:  // words
      for (uint32_t i = 0; i < n;) {
        static const char* w[] = {"frame", "socket", "deflate", "window", " ", "\n", "ping", "\xe2\x82\xacuro"};
        const char* s = w[rnd() % 8];
        for (; *s && i < n; ++s) v[i++] = (uint8_t)*s;
      }
      break;
    case 1:  // random
      for (auto& c : v) c = (uint8_t)rnd();
      break;
    case 2:  // runs of one byte
      for (uint32_t i = 0; i < n;) {
        const uint8_t c = (uint8_t)('a' + rnd() % 26);
        for (uint32_t k = 1 + rnd() % 400; k && i < n; --k) v[i++] = c;
      }
      break;
    case 3: {  // a short period
      const uint32_t per = 1 + rnd() % 8;
      uint8_t pat[8];
      for (auto& c : pat) c = (uint8_t)rnd();
      for (uint32_t i = 0; i < n; ++i) v[i] = pat[i % per];
      break;
    }
    case 4: {  // skewed literals without matches to speak of: few values, geometric weights
      for (auto& c : v) c = (uint8_t)(__builtin_ctz(rnd() | 0x80000000u) * 37);
      break;
    }
    case 5:  // one value
      std::fill(v.begin(), v.end(), (uint8_t)rnd());
      break;
    case 6: {  // random with copies from far back
      for (auto& c : v) c = (uint8_t)rnd();
      for (uint32_t k = 0; n > 8 && k < n / 64 + 1; ++k) {
        const uint32_t len = 3 + rnd() % 300, dst = rnd() % n, src = rnd() % (dst + 1);
        for (uint32_t i = 0; i < len && dst + i < n; ++i) v[dst + i] = v[src + i];
      }
      break;
    }
    default:  // compressible and incompressible stretches side by side
      for (uint32_t i = 0; i < n; ++i) v[i] = ((i >> 11) & 1) ? (uint8_t)rnd() : (uint8_t)('a' + (i % 7));
  }
  return v;
}

uint64_t g_cases = 0, g_bytes = 0, g_smaller = 0;

void check(const std::vector<uint8_t>& in, int wb) {
  const uint64_t n = in.size();
  const uint32_t fl = GEVWS_DEFLATE_DYNAMIC;
  uint64_t need = ~0ull;
  REQUIRE(gevws_deflate_raw_flags(in.data(), n, wb, fl, nullptr, 0, &need) == GEVWS_ERR_CAPACITY);
  REQUIRE(need >= 1 && need <= gevws_deflate_bound(n));
  {
    std::vector<uint8_t> out(need - 1 + kCanaries, kCanary);
    uint64_t len = 0;
    REQUIRE(gevws_deflate_raw_flags(in.data(), n, wb, fl, out.data(), need - 1, &len) == GEVWS_ERR_CAPACITY);
    REQUIRE(len == need);
    for (uint8_t c : out) REQUIRE(c == kCanary);
  }
  std::vector<uint8_t> out(need + kCanaries, kCanary);
  uint64_t len = 0;
  REQUIRE(gevws_deflate_raw_flags(in.data(), n, wb, fl, out.data(), need, &len) == GEVWS_OK && len == need);
  for (size_t i = need; i < out.size(); ++i) REQUIRE(out[i] == kCanary);
  std::vector<uint8_t> back(n + 1);
  uint64_t blen = ~0ull;
  REQUIRE(gevws_inflate_raw(out.data(), need, back.data(), n + 1, &blen) == GEVWS_MSG_OK);
  REQUIRE(blen == n && (n == 0 || memcmp(back.data(), in.data(), n) == 0));
  // never longer than without the flag; flags 0 is gevws_deflate_raw
  std::vector<uint8_t> f0(gevws_deflate_bound(n)), f1(gevws_deflate_bound(n));
  uint64_t l0 = 0, l1 = 0;
  REQUIRE(gevws_deflate_raw_flags(in.data(), n, wb, 0, f0.data(), f0.size(), &l0) == GEVWS_OK);
  REQUIRE(gevws_deflate_raw(in.data(), n, wb, f1.data(), f1.size(), &l1) == GEVWS_OK);
  REQUIRE(l0 == l1 && memcmp(f0.data(), f1.data(), l0) == 0);
  REQUIRE(need <= l0);
  g_smaller += need < l0;
  ++g_cases, g_bytes += n;
}

}  // namespace

int main() {
  code_cases(kLL, 15, false);
  code_cases(kND, 15, false);
  code_cases(kCL, 7, true);
  code_cases(kCL, 7, false);
  const uint32_t sizes[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 1024, 4095, 4096, 4097, 4099, 8191, 8192,
                            8193, 12289, 20000};
  const int wbs[] = {0, 8, 9, 10, 11, 12, 13, 14, 15};
  for (uint32_t n : sizes)
    for (uint32_t kind = 0; kind < 8; ++kind) {
      const auto in = make(n, kind);
      check(in, 0);
      check(in, wbs[rnd() % 9]);
    }
  for (int it = 0; it < 1500; ++it) {
    const uint32_t n = rnd() % 3 == 0 ? rnd() % 20001 : rnd() % 700;
    check(make(n, rnd() % 8), wbs[rnd() % 9]);
  }
  uint64_t len = 7;
  uint8_t b[8];
  REQUIRE(gevws_deflate_raw_flags(b, 3, 0, 4, b, 8, &len) == GEVWS_ERR_INVALID && len == 0);
  REQUIRE(gevws_deflate_raw_flags(b, 3, 0, GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER, b, 8, &len) == GEVWS_ERR_INVALID);
  REQUIRE(gevws_deflate_raw_flags(b, 3, 7, GEVWS_DEFLATE_DYNAMIC, b, 8, &len) == GEVWS_ERR_INVALID);
  REQUIRE(gevws_deflate_raw_flags(nullptr, 0, 0, GEVWS_DEFLATE_DYNAMIC, b, 8, &len) == GEVWS_OK && len == 1 && b[0] == 0);
  REQUIRE(g_smaller > 0);
  printf("deflate_dynamic_fuzz ok: %llu codes, %llu runs, %llu bytes, %llu smaller than fixed\n",
         (unsigned long long)g_codes, (unsigned long long)g_cases, (unsigned long long)g_bytes,
         (unsigned long long)g_smaller);
  return 0;
}
