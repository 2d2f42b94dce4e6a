// deflate_fuzz.cpp -- gevws_deflate_raw (gev_amd/csrc/gevws_deflate_host.cpp,
// the compressor of gevws_deflate_core.hpp) built with
// -fsanitize=address,undefined (tests/test_deflate_host.py): random and
// structured inputs of the sizes where the code changes path, compressed under
// every window_bits and inflated back by gevws_inflate_raw.  Checked here: the
// output buffer is sized exactly to the need with canary bytes behind it (ASan
// guards the end of the allocation, the canaries the bytes inside it), the
// need never passes gevws_deflate_bound, cap = need - 1 and cap = 0 answer
// GEVWS_ERR_CAPACITY with the need and write nothing, the payload inflates to
// the input, and the same input gives the same bytes twice.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gevws.h"

namespace {

uint64_t g_rng = 0xD1B54A32D192ED03ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

constexpr uint8_t kCanary = 0xA5;
constexpr size_t kCanaries = 64;

#define REQUIRE(c)                                                             \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "deflate_fuzz: %s failed at line %d\n", #c, __LINE__);   \
      abort();                                                                 \
    }                                                                          \
  } while (0)

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
    case 4: {  // random with copies from far back (distances up to the whole message)
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

uint64_t g_cases = 0, g_bytes = 0;

void check(const std::vector<uint8_t>& in, int wb) {
  const uint64_t n = in.size();
  uint64_t need = ~0ull;
  // cap = 0: the need, nothing written (there is nothing to write to)
  REQUIRE(gevws_deflate_raw(in.data(), n, wb, nullptr, 0, &need) == GEVWS_ERR_CAPACITY);
  REQUIRE(need >= 1 && need <= gevws_deflate_bound(n));
  REQUIRE(gevws_deflate_bound(n) <= n + n / 512 + 16);
  // cap = need - 1: the same answer, and not a byte touched
  {
    std::vector<uint8_t> out(need - 1 + kCanaries, kCanary);
    uint64_t len = 0;
    REQUIRE(gevws_deflate_raw(in.data(), n, wb, out.data(), need - 1, &len) == GEVWS_ERR_CAPACITY && len == need);
    for (uint8_t c : out) REQUIRE(c == kCanary);
  }
  std::vector<uint8_t> out(need + kCanaries, kCanary);
  uint64_t len = 0;
  REQUIRE(gevws_deflate_raw(in.data(), n, wb, out.data(), need, &len) == GEVWS_OK && len == need);
  for (size_t i = need; i < out.size(); ++i) REQUIRE(out[i] == kCanary);
  {
    std::vector<uint8_t> again(need);  // exactly the need: one byte more is an ASan report
    REQUIRE(gevws_deflate_raw(in.data(), n, wb, again.data(), need, &len) == GEVWS_OK && len == need);
    REQUIRE(memcmp(again.data(), out.data(), need) == 0);
  }
  std::vector<uint8_t> back(n + 1);
  uint64_t blen = ~0ull;
  REQUIRE(gevws_inflate_raw(out.data(), need, back.data(), n + 1, &blen) == GEVWS_MSG_OK);
  REQUIRE(blen == n && (n == 0 || memcmp(back.data(), in.data(), n) == 0));
  ++g_cases, g_bytes += n;
}

}  // namespace

int main() {
  const uint32_t sizes[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 127, 257, 258, 259, 322, 1023, 1024, 1025,
                            4095, 4096, 4097, 4099, 8191, 8192, 8193, 30719, 30720, 30721, 32767, 32768, 32769,
                            65535, 65536, 65537, 70000};
  const int wbs[] = {0, 8, 9, 10, 11, 12, 13, 14, 15};
  for (uint32_t n : sizes)
    for (uint32_t kind = 0; kind < 6; ++kind) {
      const auto in = make(n, kind);
      if (n <= 4099) {
        for (int wb : wbs) check(in, wb);
      } else {
        check(in, wbs[rnd() % 9]);
        check(in, 0);
      }
    }
  for (int it = 0; it < 3000; ++it) {
    const uint32_t n = rnd() % 3 == 0 ? rnd() % 20000 : rnd() % 700;
    check(make(n, rnd() % 6), wbs[rnd() % 9]);
  }
  uint64_t len = 7;
  uint8_t b[8];
  REQUIRE(gevws_deflate_raw(nullptr, 3, 0, b, 8, &len) == GEVWS_ERR_INVALID && len == 0);
  REQUIRE(gevws_deflate_raw(b, 3, 7, b, 8, &len) == GEVWS_ERR_INVALID);
  REQUIRE(gevws_deflate_raw(b, 3, 16, b, 8, &len) == GEVWS_ERR_INVALID);
  REQUIRE(gevws_deflate_raw(b, 1ull << 32, 0, b, 8, &len) == GEVWS_ERR_INVALID);
  REQUIRE(gevws_deflate_raw(nullptr, 0, 0, b, 8, &len) == GEVWS_OK && len == 1 && b[0] == 0);
  printf("deflate_fuzz ok: %llu runs, %llu bytes\n", (unsigned long long)g_cases, (unsigned long long)g_bytes);
  return 0;
}
