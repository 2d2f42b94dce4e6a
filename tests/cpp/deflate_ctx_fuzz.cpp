// deflate_ctx_fuzz.cpp -- gevws_deflate_raw_ctx (gevws_deflate_host.cpp): the
// compressor over one connection's context slot, built with
// -fsanitize=address,undefined (tests/test_deflate_takeover_host.py).  Random
// chains of random and structured messages, in both flag modes and with random
// window_bits, run through one slot beside a plain model of the stream.  The
// input, the output and the slot are heap blocks of exactly the size the call
// is given (ASan sees one byte too many), the output and the slot with canary
// bytes around them as well.  Checked: the sizing length is the emitted
// length, cap = need - 1 leaves out and the slot untouched, every chain
// inflates back through gevws_inflate_raw_ctx over one inflate slot, the
// payload is within gevws_deflate_bound, the slot's head and ring follow the
// model, and a zeroed slot gives gevws_deflate_raw_flags's bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gevws.h"

namespace {

uint64_t g_rng = 0xA0761D6478BD642Full;
uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

constexpr uint8_t kCanary = 0xA5;
constexpr size_t kCanaries = 64;
constexpr uint64_t kWin = 32768, kHead = 64;

#define REQUIRE(c)                                                               \
  do {                                                                           \
    if (!(c)) {                                                                  \
      fprintf(stderr, "deflate_ctx_fuzz: %s failed at line %d\n", #c, __LINE__); \
      abort();                                                                   \
    }                                                                            \
  } while (0)

// `n` usable bytes with canaries on both sides, on the heap.
struct Guarded {
  uint8_t* base;
  size_t n;
  explicit Guarded(size_t n_, uint8_t fill = 0) : base((uint8_t*)malloc(n_ + 2 * kCanaries)), n(n_) {
    memset(base, kCanary, n + 2 * kCanaries);
    memset(base + kCanaries, fill, n);
  }
  ~Guarded() { free(base); }
  uint8_t* p() { return base + kCanaries; }
  bool intact() const {
    for (size_t i = 0; i < kCanaries; ++i)
      if (base[i] != kCanary || base[kCanaries + n + i] != kCanary) return false;
    return true;
  }
};

std::vector<uint8_t> message(uint32_t n, const std::vector<uint8_t>& stream) {
  std::vector<uint8_t> m(n);
  switch (rnd() % 5) {
    case 0:
      for (auto& b : m) b = (uint8_t)rnd();
      break;
    case 1:  // few symbols
      for (auto& b : m) b = (uint8_t)("abcdefgh \n"[rnd() % 10]);
      break;
    case 2: {  // runs
      uint32_t i = 0;
      while (i < n) {
        const uint8_t v = (uint8_t)rnd();
        for (uint32_t r = 1 + rnd() % 600; r && i < n; --r) m[i++] = v;
      }
      break;
    }
    case 3: {  // a short period
      const uint32_t per = 1 + rnd() % 300;
      for (uint32_t i = 0; i < n; ++i) m[i] = i < per ? (uint8_t)rnd() : m[i - per];
      break;
    }
    default:  // pieces of the connection's own history, near and far
      for (uint32_t i = 0; i < n;) {
        if (stream.empty() || rnd() % 4 == 0) {
          m[i++] = (uint8_t)rnd();
          continue;
        }
        const uint64_t back = 1 + rnd() % (stream.size() < 40000 ? stream.size() : 40000);
        uint64_t from = stream.size() - back;
        for (uint32_t r = 3 + rnd() % 400; r && i < n && from < stream.size(); --r) m[i++] = stream[from++];
      }
      break;
  }
  return m;
}

uint64_t g_msgs = 0, g_bytes = 0;

void chain(uint32_t flags) {
  Guarded slot(GEVWS_DEF_CTX_BYTES), islot(GEVWS_INF_CTX_BYTES);
  std::vector<uint8_t> stream;
  const int wb_fixed = rnd() % 2 ? 0 : 8 + (int)(rnd() % 8);  // a connection has one window_bits ...
  const uint32_t count = 1 + rnd() % 24;
  for (uint32_t k = 0; k < count; ++k) {
    static const uint32_t kLens[] = {0, 1, 2, 3, 4, 5, 17, 63, 64, 65, 300, 512, 4095, 4096, 4097, 9000, 20000, 40000};
    uint32_t n = kLens[rnd() % (sizeof(kLens) / sizeof(kLens[0]))];
    if (rnd() % 3 == 0) n = rnd() % 1200;
    const std::vector<uint8_t> m = message(n, stream);
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: a read past the message is an error
    if (n) memcpy(in, m.data(), n);
    const int wb = wb_fixed;
    // the need, from a call that cannot fit: nothing is written
    std::vector<uint8_t> before(slot.p(), slot.p() + GEVWS_DEF_CTX_BYTES);
    uint64_t need = 0;
    REQUIRE(gevws_deflate_raw_ctx(in, n, wb, flags, nullptr, 0, &need, slot.p()) == GEVWS_ERR_CAPACITY);
    REQUIRE(need >= 1 && need <= gevws_deflate_bound(n));
    REQUIRE(memcmp(before.data(), slot.p(), GEVWS_DEF_CTX_BYTES) == 0);
    Guarded out(need, 0xEE);
    uint64_t got = 0;
    if (need > 1) {
      REQUIRE(gevws_deflate_raw_ctx(in, n, wb, flags, out.p(), need - 1, &got, slot.p()) == GEVWS_ERR_CAPACITY);
      REQUIRE(got == need && memcmp(before.data(), slot.p(), GEVWS_DEF_CTX_BYTES) == 0);
      for (uint64_t i = 0; i < need; ++i) REQUIRE(out.p()[i] == 0xEE);
    }
    if (stream.empty()) {  // a fresh slot: the compressor without a context
      std::vector<uint8_t> alone(need + 1);
      uint64_t an = 0;
      REQUIRE(gevws_deflate_raw_flags(in, n, wb, flags, alone.data(), need + 1, &an) == GEVWS_OK && an == need);
      REQUIRE(gevws_deflate_raw_ctx(in, n, wb, flags, out.p(), need, &got, slot.p()) == GEVWS_OK);
      REQUIRE(memcmp(alone.data(), out.p(), need) == 0);
    } else {
      REQUIRE(gevws_deflate_raw_ctx(in, n, wb, flags, out.p(), need, &got, slot.p()) == GEVWS_OK);
    }
    REQUIRE(got == need && out.intact() && slot.intact());
    // back through the inflate step's host twin, one slot for the chain
    uint8_t* back = (uint8_t*)malloc(n ? n : 1);
    uint64_t bn = 0;
    REQUIRE(gevws_inflate_raw_ctx(out.p(), need, back, n, &bn, islot.p()) == 0);
    REQUIRE(bn == n && (n == 0 || memcmp(back, in, n) == 0) && islot.intact());
    free(back);
    free(in);
    // the slot against the model of the stream
    stream.insert(stream.end(), m.begin(), m.end());
    uint64_t total = 0;
    memcpy(&total, slot.p(), 8);
    REQUIRE(total == stream.size());
    for (size_t i = 8; i < kHead; ++i) REQUIRE(slot.p()[i] == 0);
    if (n == 0) REQUIRE(memcmp(before.data(), slot.p(), GEVWS_DEF_CTX_BYTES) == 0);
    const uint64_t have = total < kWin ? total : kWin;
    for (uint64_t i = total - have; i < total; ++i) REQUIRE(slot.p()[kHead + (i & (kWin - 1))] == stream[i]);
    for (uint64_t i = total; i < kWin; ++i) REQUIRE(slot.p()[kHead + i] == 0);
    // the two windows hold the same stream
    REQUIRE(memcmp(slot.p() + kHead, islot.p() + kHead, kWin) == 0);
    ++g_msgs, g_bytes += n;
  }
}

}  // namespace

int main() {
  uint64_t n = 0;
  REQUIRE(gevws_deflate_raw_ctx((const uint8_t*)"a", 1, 0, 0, nullptr, 0, &n, nullptr) == GEVWS_ERR_INVALID);
  for (int i = 0; i < 160; ++i) chain(i % 2 ? GEVWS_DEFLATE_DYNAMIC : 0u);
  printf("deflate_ctx_fuzz ok: %llu messages, %llu bytes\n", (unsigned long long)g_msgs, (unsigned long long)g_bytes);
  return 0;
}
