// inflate_ctx_fuzz.cpp -- gevws_inflate_raw_ctx (gevws_inflate_host.cpp): the
// DEFLATE decode core over one connection's context slot, built with
// -fsanitize=address,undefined (tests/test_inflate_takeover_host.py).  Chains
// of hand-assembled messages -- fixed-Huffman blocks whose matches reach up to
// 32 768 bytes back, across message boundaries and the ring's wrap, and stored
// blocks -- run through one slot beside a plain model of the stream; between
// them, mutated messages run on copies of the slot.  The output buffer and the
// slot are heap blocks of exactly the size the call is given (ASan sees one
// byte too many).  Checked: bytes and verdicts of the valid messages, the
// slot's head and ring against the model, that a failure marks the slot and
// leaves its ring, that a broken slot decodes nothing, that a smaller limit
// yields a prefix, and that the core driven through a counting Io with the
// same history (the device's sizing pass) agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gev_amd/csrc/gevws_inflate_core.hpp"
#include "gevws.h"

namespace {

constexpr uint64_t kWin = 32768, kHead = 64;
static_assert(GEVWS_INF_CTX_BYTES == kWin + kHead, "the slot");

uint64_t g_rng = 0xD1B54A32D192ED03ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      abort();                                                    \
    }                                                             \
  } while (0)

struct BitWriter {
  std::vector<uint8_t> out;
  uint32_t nbits = 0;
  void bits(uint32_t v, uint32_t n) {  // LSB first
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
  void match(uint32_t len, uint32_t dist) {
    uint32_t ls = 28;
    if (len < 258) {
      ls = 0;
      while (ls + 1 < 28 && gevws_inflate::len_base(ls + 1) <= len) ++ls;
    }
    fixed_lit(257 + ls);
    bits(len - gevws_inflate::len_base(ls), gevws_inflate::len_extra(ls));
    uint32_t ds = 0;
    while (ds + 1 < 30 && gevws_inflate::dist_base(ds + 1) <= dist) ++ds;
    code(ds, 5);
    bits(dist - gevws_inflate::dist_base(ds), gevws_inflate::dist_extra(ds));
  }
};

// The slot on the heap, exactly GEVWS_INF_CTX_BYTES.
struct Slot {
  uint8_t* p;
  Slot() : p((uint8_t*)calloc(1, GEVWS_INF_CTX_BYTES)) {}
  Slot(const Slot& o) : p((uint8_t*)malloc(GEVWS_INF_CTX_BYTES)) { memcpy(p, o.p, GEVWS_INF_CTX_BYTES); }
  Slot& operator=(const Slot&) = delete;
  ~Slot() { free(p); }
  uint64_t total() const {
    uint64_t t;
    memcpy(&t, p, 8);
    return t;
  }
  uint8_t broken() const { return p[8]; }
};

// A counting Io over host memory: what the device's sizing pass is.
struct CountIo {
  const uint8_t* in;
  uint64_t n, hist, rd = 0, wr = 0;
  bool get(uint32_t& b) {
    if (rd >= n + 4) return false;
    b = rd < n ? in[rd] : (rd - n < 2 ? 0x00u : 0xffu);
    ++rd;
    return true;
  }
  void put(uint32_t) { ++wr; }
  void copy(uint32_t d, uint32_t len) {
    if (d > wr + hist || len == 0) abort();  // the core checks the distance first
    wr += len;
  }
  uint64_t stored(uint64_t want) {
    const uint64_t k = want < n + 4 - rd ? want : n + 4 - rd;
    rd += k, wr += k;
    return k;
  }
};

std::vector<uint8_t> g_stream;  // the model: every byte the chain has inflated to
uint64_t g_valid = 0, g_mutated = 0, g_mut_ok = 0, g_far = 0, g_back = 0;

// The slot's head and ring against the model.
void check_slot(const Slot& s) {
  CHECK(s.total() == g_stream.size() && s.broken() == 0);
  for (uint32_t i = 9; i < kHead; ++i) CHECK(s.p[i] == 0);
  const uint64_t n = g_stream.size();
  for (uint64_t i = n > kWin ? n - kWin : 0; i < n; ++i) CHECK(s.p[kHead + (i & (kWin - 1))] == g_stream[i]);
  for (uint64_t i = n; i < kWin; ++i) CHECK(s.p[kHead + i] == 0);  // never written
}

// One message: its compressed bytes and what it must inflate to behind g_stream.
void make_message(std::vector<uint8_t>& msg, std::vector<uint8_t>& data) {
  BitWriter w;
  data.clear();
  const uint32_t how = rnd() % 8;
  if (how == 0) {  // stored blocks: bulk, to move the ring along
    const uint32_t blocks = 1 + rnd() % 2;
    for (uint32_t k = 0; k < blocks; ++k) {
      const uint32_t n = rnd() % 9000;
      w.bits(0, 3), w.align(), w.bits(n, 16), w.bits(~n & 0xffff, 16);
      for (uint32_t i = 0; i < n; ++i) {
        const uint8_t c = (uint8_t)rnd();
        w.bits(c, 8), data.push_back(c);
      }
    }
  } else if (how == 1) {  // the empty message
  } else {
    w.bits(0, 1), w.bits(1, 2);
    const uint32_t tokens = 1 + rnd() % 40;
    for (uint32_t k = 0; k < tokens; ++k) {
      const uint64_t have = g_stream.size() + data.size();
      const uint64_t reach = have < kWin ? have : kWin;
      if (reach == 0 || rnd() % 3 == 0) {
        const uint8_t c = (uint8_t)rnd();
        w.fixed_lit(c), data.push_back(c);
        continue;
      }
      uint32_t dist;
      switch (rnd() % 4) {
        case 0: dist = (uint32_t)reach; break;                    // the farthest legal byte
        case 1: dist = 1 + rnd() % (reach < 8 ? (uint32_t)reach : 8); break;  // overlapping
        default: dist = 1 + rnd() % (uint32_t)reach;
      }
      const uint32_t len = rnd() % 5 == 0 ? 258 : 3 + rnd() % 256;
      g_far += dist == kWin;
      g_back += dist > data.size();
      w.match(len, dist);
      for (uint32_t i = 0; i < len; ++i) {
        const uint64_t at = g_stream.size() + data.size() - dist;  // (byte-serial: may be a byte just made)
        data.push_back(at < g_stream.size() ? g_stream[at] : data[at - g_stream.size()]);
      }
    }
    w.fixed_lit(256);
  }
  w.bits(0, 3), w.align();  // the sync flush's empty stored block, minus its tail
  msg = w.out;
}

// `msg` on a copy of `base` under several limits.
void run_mutated(const Slot& base, const std::vector<uint8_t>& msg) {
  const uint64_t limits[] = {1, 7, 300, 20000};
  std::vector<uint8_t> prev;
  int prev_st = -1;
  for (uint64_t limit : limits) {
    Slot s(base);
    uint8_t* out = (uint8_t*)malloc(limit);  // exactly the limit
    uint64_t len = ~0ull;
    const int st = gevws_inflate_raw_ctx(msg.data(), msg.size(), out, limit, &len, s.p);
    CHECK(st == GEVWS_MSG_OK || st == GEVWS_MSG_ERR_DEFLATE || st == GEVWS_MSG_ERR_TOO_BIG);
    CHECK(len <= limit && (st != GEVWS_MSG_ERR_TOO_BIG || len == limit));
    if (prev_st >= 0) {
      CHECK(prev.size() <= len && (prev.empty() || memcmp(prev.data(), out, prev.size()) == 0));
      CHECK(prev_st != GEVWS_MSG_OK || (st == GEVWS_MSG_OK && len == prev.size()));
    }
    gevws_inflate::Tables t;
    const uint64_t total = base.total();
    CountIo io{msg.data(), msg.size(), total < kWin ? total : kWin};
    uint64_t produced = 0;
    CHECK(gevws_inflate::inflate(io, t, limit, &produced, (uint32_t)io.hist) == st && produced == len && io.wr == len);
    if (st == GEVWS_MSG_OK) {
      CHECK(s.total() == total + len && s.broken() == 0);
      for (uint64_t i = len > kWin ? len - kWin : 0; i < len; ++i) CHECK(s.p[kHead + ((total + i) & (kWin - 1))] == out[i]);
    } else {  // the mark, and nothing else
      CHECK(s.total() == total && s.broken() == st);
      CHECK(memcmp(s.p + 9, base.p + 9, GEVWS_INF_CTX_BYTES - 9) == 0);
      uint64_t again = ~0ull;  // sticky: a valid message is not decoded any more
      const uint8_t empty_msg[1] = {0x00};
      CHECK(gevws_inflate_raw_ctx(empty_msg, 1, out, limit, &again, s.p) == st && again == 0);
      CHECK(s.total() == total && s.broken() == st);
    }
    prev.assign(out, out + len);
    prev_st = st;
    free(out);
    ++g_mutated;
    g_mut_ok += st == GEVWS_MSG_OK;
  }
}

}  // namespace

int main() {
  for (int chain = 0; chain < 24; ++chain) {
    Slot slot;
    g_stream.clear();
    std::vector<uint8_t> msg, data;
    for (int k = 0; k < 60; ++k) {
      make_message(msg, data);
      for (int it = 0; it < 6; ++it) {  // mutations of it, on copies of the slot
        std::vector<uint8_t> s = msg;
        switch (rnd() % 4) {
          case 0:
            s[rnd() % s.size()] ^= (uint8_t)(1u << (rnd() & 7));
            break;
          case 1:
            s.resize(rnd() % s.size());
            break;
          case 2:
            s[rnd() % s.size()] = (uint8_t)rnd();
            break;
          default:
            s.resize(1 + rnd() % 48);
            for (auto& c : s) c = (uint8_t)rnd();
        }
        run_mutated(slot, s);
      }
      if (!data.empty()) {  // one byte short: TOO_BIG on a copy, the bytes a prefix
        Slot s(slot);
        uint8_t* out = (uint8_t*)malloc(data.size() - 1 ? data.size() - 1 : 1);
        uint64_t len = ~0ull;
        CHECK(gevws_inflate_raw_ctx(msg.data(), msg.size(), out, data.size() - 1, &len, s.p) == GEVWS_MSG_ERR_TOO_BIG);
        CHECK(len == data.size() - 1 && memcmp(out, data.data(), len) == 0 && s.broken() == GEVWS_MSG_ERR_TOO_BIG);
        free(out);
      }
      uint8_t* out = (uint8_t*)malloc(data.size() ? data.size() : 1);  // exactly the message
      uint64_t len = ~0ull;
      CHECK(gevws_inflate_raw_ctx(msg.data(), msg.size(), out, data.size(), &len, slot.p) == GEVWS_MSG_OK);
      CHECK(len == data.size() && (len == 0 || memcmp(out, data.data(), len) == 0));
      free(out);
      g_stream.insert(g_stream.end(), data.begin(), data.end());
      check_slot(slot);
      ++g_valid;
    }
  }
  CHECK(g_far > 50 && g_back > 1000);
  uint64_t zero = 7;  // a NULL slot is refused
  uint8_t byte = 0;
  if (gevws_inflate_raw_ctx(&byte, 1, &byte, 1, &zero, nullptr) != GEVWS_ERR_INVALID || zero != 0) return 1;
  printf("inflate_ctx_fuzz ok: %llu chain messages, %llu mutated runs (%llu inflated), %llu matches at 32768\n",
         (unsigned long long)g_valid, (unsigned long long)g_mutated, (unsigned long long)g_mut_ok,
         (unsigned long long)g_far);
  return 0;
}
