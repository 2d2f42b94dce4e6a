// push_fuzz.cpp -- gevws_push_check (gev_amd/csrc/gevws_push_host.cpp, the rule
// of gevws_push.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
// sorted lists with single-field mutations and random records, each list at
// the end of a heap block of exactly its size, so a read behind records[n) is a
// heap-buffer-overflow; every count against a second reading of the contract
// written here field by field.  Stand-alone: builds with g++ alone, needs no
// GPU (tests/test_push_sanitizers.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gevws.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// The contract, one cause at a time.
static int64_t expect(const std::vector<gevws_push>& v, uint32_t n_conns, uint32_t n_rooms, uint64_t src_bytes) {
  int64_t bad = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    const gevws_push& p = v[i];
    bool b = p.kind > 2;
    b |= p.kind == 0 && p.target != 0;
    b |= p.kind == 1 && p.target >= n_rooms;
    b |= p.kind == 2 && p.target >= n_conns;
    b |= !(p.opcode == 1 || p.opcode == 2 || p.opcode == 9 || p.opcode == 10);
    b |= (p.off & 15) != 0;
    b |= p.length > 0xFFFFFFFFull;
    b |= (unsigned __int128)p.off + p.length > src_bytes;
    b |= (p.opcode == 9 || p.opcode == 10) && p.length > 125;
    for (int k = 0; k < 10; ++k) b |= p.reserved[k] != 0;
    if (i) {
      const uint64_t k0 = ((uint64_t)v[i - 1].kind << 32) | v[i - 1].target, k1 = ((uint64_t)p.kind << 32) | p.target;
      b |= k1 < k0;
    }
    bad += b;
  }
  return bad;
}

static long checked = 0, clean = 0, dirty = 0;

static bool check(const std::vector<gevws_push>& v, uint32_t n_conns, uint32_t n_rooms, uint64_t src_bytes) {
  const size_t bytes = v.size() * sizeof(gevws_push);
  uint8_t* block = static_cast<uint8_t*>(malloc(bytes ? bytes : 1));  // the list ends where its allocation ends
  if (!block) return false;
  if (bytes) memcpy(block, v.data(), bytes);
  const int64_t got = gevws_push_check(reinterpret_cast<const gevws_push*>(block), v.size(), n_conns, n_rooms, src_bytes);
  free(block);
  const int64_t want = expect(v, n_conns, n_rooms, src_bytes);
  if (got != want) {
    fprintf(stderr, "mismatch on %zu records (%u conns, %u rooms, %llu bytes): got %lld, want %lld\n", v.size(), n_conns,
            n_rooms, (unsigned long long)src_bytes, (long long)got, (long long)want);
    return false;
  }
  ++checked, ++(want ? dirty : clean);
  return true;
}

static gevws_push rec(uint8_t kind, uint32_t target, uint8_t opcode, uint64_t off, uint64_t length) {
  gevws_push p;
  memset(&p, 0, sizeof(p));
  p.kind = kind, p.target = target, p.opcode = opcode, p.off = off, p.length = length;
  return p;
}

int main() {
  static_assert(sizeof(gevws_push) == 32, "gevws_push");
  const uint32_t n_conns = 300, n_rooms = 7;
  const uint64_t src = 1 << 20;
  // a well-formed list: every kind, every opcode, the size classes, keys in order
  std::vector<gevws_push> good = {rec(0, 0, 1, 0, 0),        rec(0, 0, 9, 16, 125),      rec(0, 0, 2, 256, 65536),
                                  rec(1, 0, 1, 0, 17),       rec(1, 3, 10, 32, 0),       rec(1, 6, 2, src - 16, 16),
                                  rec(2, 0, 1, 48, 126),     rec(2, 0, 2, 48, 65535),    rec(2, 299, 9, 64, 1)};
  if (!check(good, n_conns, n_rooms, src) || expect(good, n_conns, n_rooms, src) != 0) return 1;
  for (size_t k = 0; k <= good.size(); ++k)  // every prefix, the empty list too
    if (!check(std::vector<gevws_push>(good.begin(), good.begin() + k), n_conns, n_rooms, src)) return 1;
  // every single-byte mutation of every record
  for (size_t i = 0; i < good.size(); ++i) {
    for (size_t b = 0; b < sizeof(gevws_push); ++b) {
      for (int v = 0; v < 256; v += (b < 16 ? 17 : 1)) {
        std::vector<gevws_push> m = good;
        reinterpret_cast<uint8_t*>(&m[i])[b] = (uint8_t)v;
        if (!check(m, n_conns, n_rooms, src)) return 1;
      }
    }
  }
  // the edges of every cause, alone
  const gevws_push edges[] = {
      rec(3, 0, 1, 0, 0),           rec(255, 0, 1, 0, 0),         rec(0, 1, 1, 0, 0),         rec(1, 7, 1, 0, 0),
      rec(1, 6, 1, 0, 0),           rec(2, 300, 1, 0, 0),         rec(2, 299, 1, 0, 0),       rec(0, 0, 0, 0, 0),
      rec(0, 0, 8, 0, 0),           rec(0, 0, 3, 0, 0),           rec(0, 0, 11, 0, 0),        rec(0, 0, 1, 8, 0),
      rec(0, 0, 1, 15, 0),          rec(0, 0, 1, src, 0),         rec(0, 0, 1, src, 1),       rec(0, 0, 1, src + 16, 0),
      rec(0, 0, 1, 0, src),         rec(0, 0, 1, 0, src + 1),     rec(0, 0, 1, 16, ~0ull),    rec(0, 0, 1, ~0ull - 15, 32),
      rec(0, 0, 1, 0, 1ull << 32),  rec(0, 0, 9, 0, 126),         rec(0, 0, 10, 0, 126),      rec(0, 0, 10, 0, 125),
  };
  for (const gevws_push& e : edges) {
    if (!check({e}, n_conns, n_rooms, src)) return 1;
    if (!check({e}, n_conns, n_rooms, ~0ull)) return 1;  // an arena as large as the address space
    if (!check({e}, 0, 0, 0)) return 1;
  }
  // the order: equal keys, a step down inside a kind, a step down across kinds
  if (!check({rec(1, 3, 1, 0, 0), rec(1, 3, 1, 0, 0), rec(1, 2, 1, 0, 0), rec(2, 0, 1, 0, 0), rec(0, 0, 1, 0, 0)},
             n_conns, n_rooms, src))
    return 1;
  if (expect({rec(1, 3, 1, 0, 0), rec(1, 2, 1, 0, 0), rec(0, 0, 1, 0, 0)}, n_conns, n_rooms, src) != 2) return 1;
  // random lists: fields drawn near their limits
  for (int it = 0; it < 60000; ++it) {
    const uint32_t nc = (uint32_t)(rnd() % 5), nr = (uint32_t)(rnd() % 4);
    const uint64_t sb = (rnd() % 4) * 64;
    std::vector<gevws_push> v(rnd() % 9);
    for (gevws_push& p : v) {
      p = rec((uint8_t)(rnd() % 4), (uint32_t)(rnd() % 6), (uint8_t)(rnd() % 12), (rnd() % 20) * (rnd() % 8 ? 16 : 1),
              rnd() % 8 ? rnd() % 200 : rnd());
      if (rnd() % 16 == 0) p.reserved[rnd() % 10] = (uint8_t)rnd();
    }
    if (!check(v, nc, nr, sb)) return 1;
  }
  // invalid calls
  if (gevws_push_check(nullptr, 1, 1, 1, 16) != GEVWS_ERR_INVALID) return 1;
  if (gevws_push_check(good.data(), 1ull << 32, 1, 1, 16) != GEVWS_ERR_INVALID) return 1;
  if (gevws_push_check(nullptr, 0, 1, 1, 16) != 0) return 1;
  if (!clean || !dirty) return 1;
  printf("push_fuzz ok: %ld lists (%ld clean, %ld with malformed records)\n", checked, clean, dirty);
  return 0;
}
